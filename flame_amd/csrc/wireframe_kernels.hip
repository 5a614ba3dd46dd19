// wireframe_kernels.hip -- getDebugImageWireframe from what the pipeline leaves on the device:
//   drawWireframe                flame.cc:2414-2457
//   drawColorMappedWireframe     utils/image_utils.h:693-719
//   applyColorMapLine            utils/visualization.h:235-260
// The reference draws sequentially: triangle by triangle, three lines each, pixel by pixel along cv::LineIterator, and every pixel
// it visits becomes the mean of the line's colour and what the pixel held.  A pixel's final value is a fold over the draws that
// touched it, in draw order.  Here (include/flame_nltgv2.h states the rule in full; tests/wireframe_ref.py restates it):
//   setup     one lane per line: endpoints rounded, validity and the outside rule applied -> a 16-byte draw record (the only
//             reader of pos / x / tri_valid)
//   count     one lane per draw walks its line: cnt[pixel] += 1
//   offsets   every touched pixel takes a range of cnt[pixel] entries from one cursor, 1024 pixels of a wave at a time (placement is
//             not deterministic and need not be: the fold orders by id); k_draw_offsets, draw_offsets.hpp, shared with the matches
//             picture like the line walk (draw_lists.hpp)
//   fill      one lane per draw walks again: (id << 32 | colour) into the pixel's range
//   fold      per OUTPUT pixel, four per thread: the grey value, then the entries in increasing id, (c + v) >> 1 per channel
// The fold takes the entries in order by selection (the smallest id above the last one taken) instead of sorting a copy: no
// scratch memory, any list length, and a list of one or two entries -- nearly all of them -- costs one or four reads.
// Built with -ffp-contract=off like the rest of the library: val = A + ii * slope0 is a product and a sum.
#include <hip/hip_runtime.h>

#include "debug_pixel.hpp"
#include "draw_lists.hpp"
#include "draw_offsets.hpp"
#include "wireframe_kernels.h"

namespace flame_hip {
namespace {

__global__ void __launch_bounds__(256)
k_wire_setup(int n_draws, const int32_t* __restrict__ tris, const float2* __restrict__ vtx, const float* __restrict__ x,
             float value_scale, const uint8_t* __restrict__ tri_valid, int rows, int cols, WireDraw* __restrict__ draws,
             int* __restrict__ counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool valid = false, drawn = false;
  if (i < n_draws) {
    const int t = i / 3, k = i - 3 * t;
    valid = tri_valid ? tri_valid[t] != 0 : true;
    WireDraw d;
    d.x1 = -1, d.y1 = d.x2 = d.y2 = 0, d.a_val = d.b_val = 0.0f;
    if (valid) {
      const int va = tris[3 * t + (k == 1 ? 1 : 0)], vb = tris[3 * t + (k == 0 ? 1 : 2)];  // v0 -> v1, v1 -> v2, v0 -> v2
      const float2 pa = vtx[va], pb = vtx[vb];
      int x1 = 0, y1 = 0, x2 = 0, y2 = 0;
      const bool in_a = round_inside(pa.x, cols - 1, &x1) && round_inside(pa.y, rows - 1, &y1);
      drawn = in_a && round_inside(pb.x, cols - 1, &x2) && round_inside(pb.y, rows - 1, &y2);
      if (drawn) {
        d.x1 = (int16_t)x1, d.y1 = (int16_t)y1, d.x2 = (int16_t)x2, d.y2 = (int16_t)y2;
        d.a_val = x[va] * value_scale, d.b_val = x[vb] * value_scale;
      }
    }
    draws[i] = d;
  }
  const int n_drawn = __popcll(__ballot(drawn)), n_skipped = __popcll(__ballot(valid && !drawn));
  if ((threadIdx.x & 63) == 0) {
    if (n_drawn) atomicAdd(&counts[kWireDrawn], n_drawn);
    if (n_skipped) atomicAdd(&counts[kWireSkipped], n_skipped);
  }
}

__global__ void __launch_bounds__(256)
k_wire_count(int n_draws, const WireDraw* __restrict__ draws, int rows, int cols, uint32_t* __restrict__ cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_draws) return;
  const WireDraw d = draws[i];
  if (d.x1 < 0) return;
  walk_line(d.x1, d.y1, d.x2, d.y2, [&](int, int, int x, int y) {
    if ((unsigned)x < (unsigned)cols && (unsigned)y < (unsigned)rows) atomicAdd(&cnt[(long)y * cols + x], 1u);
  });
}

__global__ void __launch_bounds__(256)
k_wire_fill(int n_draws, const WireDraw* __restrict__ draws, int rows, int cols, float scene_color_scale,
            const uint32_t* __restrict__ offset, uint32_t* __restrict__ fill, uint64_t* __restrict__ entries, uint32_t capacity) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_draws) return;
  const WireDraw d = draws[i];
  if (d.x1 < 0) return;
  const float a_val = d.a_val, b_val = d.b_val;
  walk_line(d.x1, d.y1, d.x2, d.y2, [&](int ii, int count, int x, int y) {
    if (!((unsigned)x < (unsigned)cols && (unsigned)y < (unsigned)rows)) return;
    const float slope0 = (b_val - a_val) / (float)count;
    const float val = a_val + (float)ii * slope0;
    uint8_t c[3];
    jet02(val * scene_color_scale, c);
    const long p = (long)y * cols + x;
    const uint32_t at = offset[p] + atomicAdd(&fill[p], 1u);
    if (at < capacity) entries[at] = ((uint64_t)(uint32_t)i << 32) | (uint64_t)pack3(c);
  });
}

__global__ void __launch_bounds__(256)
k_wire_fold(WireImageArgs a, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ offset,
            const uint64_t* __restrict__ entries, uint32_t capacity, uint8_t* __restrict__ img) {
  const long n = (long)a.rows * a.cols;
  const long o0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * kPixelsPerThread;
  if (o0 >= n) return;
  uint32_t px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < kPixelsPerThread; ++k) {
    const long o = o0 + k;
    if (o >= n) continue;
    const long i = a.flip ? n - 1 - o : o;  // the source pixel of output pixel o
    const int row = (int)(i / a.cols), col = (int)(i % a.cols);
    const uint32_t g = a.gray[(long)row * a.gray_step + col];  // cvtColor(GRAY2RGB): three equal bytes
    uint32_t c0 = g, c1 = g, c2 = g;
    const uint32_t c = cnt[i], off = offset[i];
    // (a list that does not fit the entry buffer is left alone: the total says so and the host repeats fill and fold)
    if (c != 0u && (uint64_t)off + c <= (uint64_t)capacity) {
      const uint64_t* e = entries + off;
      int64_t last = -1;
      for (uint32_t j = 0; j < c; ++j) {
        uint64_t best = ~0ull;
        if (c == 1u) {
          best = e[0];
        } else {
          for (uint32_t m = 0; m < c; ++m) {
            const uint64_t v = e[m];
            if ((int64_t)(v >> 32) > last && v < best) best = v;
          }
        }
        if (best == ~0ull) break;
        last = (int64_t)(best >> 32);
        c0 = (c0 + ((uint32_t)best & 255u)) >> 1;
        c1 = (c1 + ((uint32_t)(best >> 8) & 255u)) >> 1;
        c2 = (c2 + ((uint32_t)(best >> 16) & 255u)) >> 1;
      }
    }
    px[k] = c0 | (c1 << 8) | (c2 << 16);
  }
  store_pixels(img, o0, n, px);
}

}  // namespace

int launch_wireframe_lists(int T, const int32_t* tris, const float2* vtx, const float* x, float value_scale, const uint8_t* tri_valid,
                           const WireBuffers& b, int rows, int cols, hipEvent_t after_setup, hipStream_t s) {
  const long n = (long)rows * cols;
  const int n_draws = 3 * T;
  if (n <= 0) return 0;
  (void)hipMemsetAsync(b.cnt, 0, sizeof(uint32_t) * (size_t)n, s);
  (void)hipMemsetAsync(b.counts, 0, kWireCounts * sizeof(int), s);
  if (n_draws > 0)
    hipLaunchKernelGGL(k_wire_setup, grid1d(n_draws), dim3(256), 0, s, n_draws, tris, vtx, x, value_scale, tri_valid, rows, cols,
                       b.draws, b.counts);
  if (after_setup) {
    const hipError_t e = hipEventRecord(after_setup, s);
    if (e != hipSuccess) return (int)e;
  }
  if (n_draws > 0) hipLaunchKernelGGL(k_wire_count, grid1d(n_draws), dim3(256), 0, s, n_draws, b.draws, rows, cols, b.cnt);
  hipLaunchKernelGGL(k_draw_offsets, grid1d((n + kOffsetsPerLane - 1) / kOffsetsPerLane), dim3(256), 0, s, n, b.cnt, b.offset,
                     (uint32_t*)&b.counts[kWireTotal]);
  return (int)hipGetLastError();
}

int launch_wireframe_paint(int T, const WireBuffers& b, const WireImageArgs& a, uint8_t* img, hipStream_t s) {
  const long n = (long)a.rows * a.cols;
  const int n_draws = 3 * T;
  if (n <= 0) return 0;
  (void)hipMemsetAsync(b.fill, 0, sizeof(uint32_t) * (size_t)n, s);
  if (n_draws > 0)
    hipLaunchKernelGGL(k_wire_fill, grid1d(n_draws), dim3(256), 0, s, n_draws, b.draws, a.rows, a.cols, a.scene_color_scale, b.offset,
                       b.fill, b.entries, b.capacity);
  hipLaunchKernelGGL(k_wire_fold, grid1d((n + kPixelsPerThread - 1) / kPixelsPerThread), dim3(256), 0, s, a, b.cnt, b.offset,
                     b.entries, b.capacity, img);
  return (int)hipGetLastError();
}

}  // namespace flame_hip
