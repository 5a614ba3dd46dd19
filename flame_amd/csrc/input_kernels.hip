// input_kernels.hip -- the input stage in front of Frame::create: what the reference's front-end does on the host with
// cv::cvtColor and cv::undistort before it calls Flame::update.  include/flame_stereo.h (flame_stereo_add_raw_frame) states the
// rule -- the integer grey, the float32 map in a fixed association, the inside test, the reference's bilinear weights
// (utils/image_utils.h:199-214), the rounding (UNPINNED) --; tests/input_ref.py restates it.  Built with -ffp-contract=off.
//
// A gather with a few dozen float operations per pixel and nothing to reuse: a thread owns four consecutive OUTPUT pixels and
// stores them as one dword (bytes at the image's tail); consecutive lanes write consecutive dwords.  The output is one flat
// run of pixels, so a thread's four may cross a row end: row and column are formed per pixel.  A tap is read byte by byte --
// neither the raw pointer nor the stride has any alignment, and a 3-byte pixel has none either way --, except that a 4-byte
// format whose base and stride are both multiples of 4 reads a tap as one dword (kDwordTaps).  The outside pixels are counted
// per wave (ballot + popcount) and added with one atomic per wave into one of kInputSlots copies of the counter.
#include <hip/hip_runtime.h>

#include "input_kernels.h"
#include "input_params.hpp"

namespace flame_hip {
namespace {

// The grey of the tap at p.  kBgr: the first byte is blue (BGR8, BGRA8), else red (RGB8, RGBA8).
template <int kBpp, bool kBgr, bool kDwordTaps>
__device__ __forceinline__ uint32_t tap_grey(const uint8_t* __restrict__ p) {
  if (kBpp == 1) return p[0];
  uint32_t c0, c1, c2;
  if (kBpp == 4 && kDwordTaps) {
    const uint32_t v = *(const uint32_t*)p;
    c0 = v & 255u, c1 = (v >> 8) & 255u, c2 = (v >> 16) & 255u;
  } else {
    c0 = p[0], c1 = p[1], c2 = p[2];
  }
  const uint32_t r = kBgr ? c2 : c0, b = kBgr ? c0 : c2;
  return (4899u * r + 9617u * c1 + 1868u * b + 8192u) >> 14;
}

template <int kBpp, bool kBgr, bool kDwordTaps, bool kRemap>
__global__ void __launch_bounds__(kInputBlock)
k_input_rectify(const InputMap m, const uint8_t* __restrict__ raw, const long stride, const int width, const int n,
                int* __restrict__ stats, uint8_t* __restrict__ out) {
  const int o0 = (blockIdx.x * kInputBlock + threadIdx.x) * kInputPixelsPerThread;  // (n <= 2^28: input_params.hpp)
  uint32_t px = 0;
  int n_outside = 0;
  int vi = o0 / width, ui = o0 - vi * width;  // one division per thread: the other three pixels step from here
#pragma unroll
  for (int k = 0; k < kInputPixelsPerThread; ++k, ++ui) {
    const int o = o0 + k;
    bool outside = false;
    uint32_t g = 0;
    if (ui == width) ui = 0, ++vi;
    if (o < n) {
      if (!kRemap) {
        g = tap_grey<kBpp, kBgr, kDwordTaps>(raw + (long)vi * stride + (long)ui * kBpp);
      } else {
        const float u = (float)ui, v = (float)vi;
        const float x = (m.kinv[0] * u + m.kinv[1] * v) + m.kinv[2];
        const float y = (m.kinv[3] * u + m.kinv[4] * v) + m.kinv[5];
        const float r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
        const float rad = (((1.0f + m.k1 * r2) + m.k2 * r4) + m.k3 * r6) / (((1.0f + m.k4 * r2) + m.k5 * r4) + m.k6 * r6);
        const float tx = 2.0f * x, ty = 2.0f * y, a1 = tx * y, a2 = r2 + tx * x, a3 = r2 + ty * y;
        const float xd = (x * rad + m.p1 * a1) + m.p2 * a2;
        const float yd = (y * rad + m.p1 * a3) + m.p2 * a1;
        const float xs = (m.fx * xd + m.skew * yd) + m.cx;
        const float ys = m.fy * yd + m.cy;
        // decided on the floats, before any integer or address exists: a NaN or an infinity fails it by itself
        const bool inside = xs >= 0.0f && ys >= 0.0f && xs < (float)(m.raw_width - 1) && ys < (float)(m.raw_height - 1);
        outside = !inside;
        if (inside) {
          const int x0 = (int)xs, y0 = (int)ys;  // 0 <= x0 <= raw_width - 2, 0 <= y0 <= raw_height - 2
          const float dx = xs - (float)x0, dy = ys - (float)y0;
          const float w11 = dx * dy, w01 = dx - w11, w10 = dy - w11, w00 = ((1.0f - dx) - dy) + w11;
          const uint8_t* p = raw + (long)y0 * stride + (long)x0 * kBpp;
          const float g00 = (float)tap_grey<kBpp, kBgr, kDwordTaps>(p);
          const float g01 = (float)tap_grey<kBpp, kBgr, kDwordTaps>(p + kBpp);
          const float g10 = (float)tap_grey<kBpp, kBgr, kDwordTaps>(p + stride);
          const float g11 = (float)tap_grey<kBpp, kBgr, kDwordTaps>(p + stride + kBpp);
          const float value = ((w00 * g00 + w01 * g01) + w10 * g10) + w11 * g11;
          g = (uint32_t)(uint8_t)(int)(value + 0.5f);
        }
      }
    }
    px |= g << (8 * k);
    if (kRemap) n_outside += __popcll(__ballot(outside));  // (every lane of the wave is here: nothing returned early)
  }
  if (o0 + kInputPixelsPerThread <= n) {
    *(uint32_t*)(out + o0) = px;  // (4 j bytes from a 4-byte aligned base)
  } else {
#pragma unroll
    for (int k = 0; k < kInputPixelsPerThread - 1; ++k)
      if (o0 + k < n) out[o0 + k] = (uint8_t)(px >> (8 * k));
  }
  if (kRemap && (threadIdx.x & 63) == 0 && n_outside)
    atomicAdd(&stats[(blockIdx.x % kInputSlots) * kInputSlotStride], n_outside);
}

template <int kBpp, bool kBgr, bool kDwordTaps>
void launch(const InputMap& m, bool remap, const uint8_t* raw, int stride, int width, int n, int* stats, uint8_t* out,
            hipStream_t s) {
  const dim3 grid(input_blocks(n)), block(kInputBlock);
  if (remap)
    hipLaunchKernelGGL((k_input_rectify<kBpp, kBgr, kDwordTaps, true>), grid, block, 0, s, m, raw, (long)stride, width, n, stats, out);
  else
    hipLaunchKernelGGL((k_input_rectify<kBpp, kBgr, kDwordTaps, false>), grid, block, 0, s, m, raw, (long)stride, width, n, stats, out);
}

}  // namespace

int launch_input_rectify(const InputMap& map, int format, bool remap, const uint8_t* raw, int row_stride_bytes, int width,
                         int height, int* stats, uint8_t* out, hipStream_t s) {
  const long n = (long)width * height;
  (void)hipMemsetAsync(stats, 0, kInputWords * sizeof(int), s);
  if (n <= 0) return (int)hipGetLastError();
  const bool dwords = ((uintptr_t)raw % 4 == 0) && (row_stride_bytes % 4 == 0);
  switch (format) {
    case FLAME_STEREO_FMT_GREY8: launch<1, false, false>(map, remap, raw, row_stride_bytes, width, (int)n, stats, out, s); break;
    case FLAME_STEREO_FMT_BGR8: launch<3, true, false>(map, remap, raw, row_stride_bytes, width, (int)n, stats, out, s); break;
    case FLAME_STEREO_FMT_RGB8: launch<3, false, false>(map, remap, raw, row_stride_bytes, width, (int)n, stats, out, s); break;
    case FLAME_STEREO_FMT_BGRA8:
      if (dwords) launch<4, true, true>(map, remap, raw, row_stride_bytes, width, (int)n, stats, out, s);
      else launch<4, true, false>(map, remap, raw, row_stride_bytes, width, (int)n, stats, out, s);
      break;
    case FLAME_STEREO_FMT_RGBA8:
      if (dwords) launch<4, false, true>(map, remap, raw, row_stride_bytes, width, (int)n, stats, out, s);
      else launch<4, false, false>(map, remap, raw, row_stride_bytes, width, (int)n, stats, out, s);
      break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

}  // namespace flame_hip
