// view_kernels.hip -- the mesh rendered into another camera (include/flame_nltgv2.h, flame_nltgv2_render_view_begin, states every rule;
// tests/view_ref.py restates them in numpy float32 and Python integers and is the checker, bit for bit):
//   clear       the key image and the counters
//   vertices    one lane per vertex: back-projection with its inverse depth, R P + t, projection, 1/16-pixel snapping in both views,
//               1 / z' -- float32, every sum of three products left to right
//   triangles   one lane per triangle counts what rule 2 makes of it (one atomic per workgroup and counter); one wavefront per drawn
//               triangle walks its pixel bounding box clipped to the image -- but a triangle stretched across a depth edge can hold a
//               thousand times the pixels of its neighbours, and one wave walking it alone was the whole kernel's time
//               (profiles/render_view.txt): boxes of more than kViewWavePixels pixels are listed and shared by kViewBigWaves waves each.  The edge functions are affine in (col, row) with integer
//               coefficients: w = e0 + row * dy + col * dx in int64 is the rule's value exactly (|X|, |Y| <= 2^20: |w| < 2^44).  The
//               nearest surface wins through a 64-bit atomicMax on {bits(val), t + 1}: val > 0, so its bits order as the floats do
//   resolve     keys -> map, owner index, coverage (one atomic per workgroup: the lesson of k_raster_resolve)
// The device functions of rules 1 - 5 are in view_device.hpp, shared with fuse_kernels.hip.
// No floating-point atomics: the key image does not depend on scheduling.  Built with -ffp-contract=off (no FMA); division and the
// int64 -> float conversions are correctly rounded.
#include <hip/hip_runtime.h>

#include "view_device.hpp"
#include "view_kernels.h"

namespace flame_hip {
namespace {

using namespace view_device;  // rules 1 - 5, shared with fuse_kernels.hip

constexpr int kPerThread = kViewResolveTile / 256;

__global__ void __launch_bounds__(256)
k_view_clear(long n, unsigned long long* __restrict__ keys, ViewCounts* __restrict__ counts, int* __restrict__ big) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *counts = ViewCounts{0, 0, 0, 0}, big[0] = 0;
  const long base = (long)blockIdx.x * kViewResolveTile + threadIdx.x;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const long i = base + (long)j * 256;
    if (i < n) keys[i] = 0ull;
  }
}

__global__ void __launch_bounds__(256)
k_view_vertices(int V, const float2* __restrict__ pos, const float* __restrict__ values, float value_scale, ViewCamera cam,
                ViewVertex* __restrict__ out) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  out[v] = view_vertex(pos[v], values[v] * value_scale, cam);
}

// One lane per triangle: what rule 2 makes of it, counted with one atomic per workgroup and counter; a drawn triangle whose box holds
// more than kViewWavePixels pixels goes on the list big[1 ..], big[0] counting them (few: a triangle stretched across a depth edge).
__global__ void __launch_bounds__(256)
k_view_count(int T, const int32_t* __restrict__ tris, const uint8_t* __restrict__ tri_valid, const ViewVertex* __restrict__ vtx,
             ViewCounts* __restrict__ counts, int* __restrict__ big, int rows, int cols) {
  __shared__ int s_n[4];
  if (threadIdx.x < 4) s_n[threadIdx.x] = 0;
  __syncthreads();
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  int cls = kInvalid;
  if (t < T) {
    long long A = 0;
    const ViewVertex a = vtx[tris[3 * t]], b = vtx[tris[3 * t + 1]], c = vtx[tris[3 * t + 2]];
    cls = classify(t, tri_valid, a, b, c, &A);
    if (cls == kDraw && bounding_box(a, b, c, rows, cols).n > (unsigned)kViewWavePixels) big[1 + atomicAdd(&big[0], 1)] = t;
  }
  for (int k = kDraw; k <= kCulledFacing; ++k) {
    if (k == kInvalid) continue;
    const int n = __popcll(__ballot(cls == k));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&s_n[k], n);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_n[kDraw]) atomicAdd(&counts->tris_drawn, s_n[kDraw]);
    if (s_n[kCulledVertex]) atomicAdd(&counts->tris_culled_vertex, s_n[kCulledVertex]);
    if (s_n[kCulledFacing]) atomicAdd(&counts->tris_culled_facing, s_n[kCulledFacing]);
  }
}

// One wavefront per triangle whose box holds at most kViewWavePixels pixels: the others are k_view_raster_big's.
__global__ void __launch_bounds__(64)
k_view_raster(int T, const int32_t* __restrict__ tris, const uint8_t* __restrict__ tri_valid, const ViewVertex* __restrict__ vtx,
              unsigned long long* __restrict__ keys, int rows, int cols) {
  const int t = blockIdx.x;
  if (t >= T) return;
  const ViewVertex a = vtx[tris[3 * t]], b = vtx[tris[3 * t + 1]], c = vtx[tris[3 * t + 2]];
  long long A = 0;
  if (classify(t, tri_valid, a, b, c, &A) != kDraw) return;
  const ViewBox box = bounding_box(a, b, c, rows, cols);
  if (box.n > (unsigned)kViewWavePixels) return;
  raster_pixels(t, A, a, b, c, box, threadIdx.x, 64u, keys, cols);
}

// The listed triangles: kViewBigWaves wavefronts share one triangle's box (blockIdx.x: which of them), blockIdx.y walks the list.
__global__ void __launch_bounds__(64)
k_view_raster_big(const int32_t* __restrict__ tris, const ViewVertex* __restrict__ vtx, const int* __restrict__ big,
                  unsigned long long* __restrict__ keys, int rows, int cols) {
  const int n_big = big[0];
  for (int item = blockIdx.y; item < n_big; item += gridDim.y) {
    const int t = big[1 + item];
    const ViewVertex a = vtx[tris[3 * t]], b = vtx[tris[3 * t + 1]], c = vtx[tris[3 * t + 2]];
    long long A = 0;
    (void)classify(t, nullptr, a, b, c, &A);  // (listed: drawn)
    raster_pixels(t, A, a, b, c, bounding_box(a, b, c, rows, cols), blockIdx.x * 64u + threadIdx.x, 64u * kViewBigWaves, keys, cols);
  }
}

__global__ void __launch_bounds__(256)
k_view_resolve(long n, const unsigned long long* __restrict__ keys, float* __restrict__ map, int32_t* __restrict__ tri_index,
               ViewCounts* __restrict__ counts) {
  __shared__ int s_count;
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  int count = 0;
  const long base = (long)blockIdx.x * kViewResolveTile + threadIdx.x;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const long i = base + (long)j * 256;
    bool covered = false;
    if (i < n) {
      const unsigned long long k = keys[i];
      const int owner = (int)(unsigned)k;  // t + 1; 0: nobody
      covered = owner != 0;
      if (map) map[i] = covered ? __uint_as_float((unsigned)(k >> 32)) : __uint_as_float(0x7fc00000u);
      if (tri_index) tri_index[i] = owner - 1;
    }
    count += __popcll(__ballot(covered));
  }
  if ((threadIdx.x & 63) == 0 && count) atomicAdd(&s_count, count);
  __syncthreads();
  if (threadIdx.x == 0 && s_count) atomicAdd(&counts->coverage, s_count);
}

inline dim3 tiles(long n) { return dim3((unsigned)((n + kViewResolveTile - 1) / kViewResolveTile)); }

}  // namespace

int launch_view_clear(long n, unsigned long long* keys, ViewCounts* counts, int* big, hipStream_t s) {
  hipLaunchKernelGGL(k_view_clear, tiles(n > 0 ? n : 1), dim3(256), 0, s, n, keys, counts, big);
  return (int)hipGetLastError();
}

int launch_view_vertices(int V, const float2* pos, const float* values, float value_scale, const ViewCamera& cam, ViewVertex* out, hipStream_t s) {
  if (V <= 0) return 0;
  hipLaunchKernelGGL(k_view_vertices, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, s, V, pos, values, value_scale, cam, out);
  return (int)hipGetLastError();
}

int launch_view_raster(int T, const int32_t* tris, const uint8_t* tri_valid, const ViewVertex* vtx, unsigned long long* keys, ViewCounts* counts,
                       int* big, int rows, int cols, hipStream_t s) {
  if (T <= 0) return 0;
  hipLaunchKernelGGL(k_view_count, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, T, tris, tri_valid, vtx, counts, big, rows, cols);
  hipLaunchKernelGGL(k_view_raster, dim3((unsigned)T), dim3(64), 0, s, T, tris, tri_valid, vtx, keys, rows, cols);
  hipLaunchKernelGGL(k_view_raster_big, dim3(kViewBigWaves, kViewBigRows), dim3(64), 0, s, tris, vtx, big, keys, rows, cols);
  return (int)hipGetLastError();
}

int launch_view_resolve(long n, const unsigned long long* keys, float* map, int32_t* tri_index, ViewCounts* counts, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_view_resolve, tiles(n), dim3(256), 0, s, n, keys, map, tri_index, counts);
  return (int)hipGetLastError();
}

}  // namespace flame_hip
