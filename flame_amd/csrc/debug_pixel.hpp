// debug_pixel.hpp -- what the kernels of debug_kernels.hip and wireframe_kernels.hip share: the colour map and the way a thread
// stores its four consecutive OUTPUT pixels (12 bytes, three dwords).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace flame_hip {
namespace {

constexpr int kPixelsPerThread = 4;

inline dim3 grid1d(long n, int block = 256) { return dim3((unsigned)((n + block - 1) / block)); }

// static_cast<uint8_t> of a value the callers keep inside [0, 256); a NaN gives 0 (see jet02)
__device__ __forceinline__ uint8_t to_u8(float v) { return (uint8_t)(int)v; }
__device__ __forceinline__ uint8_t to_u8(double v) { return (uint8_t)(int)v; }

// utils::jet(v, vmin, vmax), visualization.h:142-167.  c starts white; the first branch is float arithmetic, the other three go
// through double (their 0.25 * dv, 0.5 * dv, 0.75 * dv literals); `4 * a / dv` is (4 * a) / dv.
// A NaN v fails every comparison and ends in the last branch with a NaN cast to uint8_t, which C++ leaves undefined: the
// library's colour for it is (0, 0, 255), what x86 produces (UNPINNED).
__device__ __forceinline__ void jet(float v, const float vmin, const float vmax, uint8_t c[3]) {
  c[0] = 255, c[1] = 255, c[2] = 255;
  if (v < vmin) v = vmin;
  if (v > vmax) v = vmax;
  const float dv = vmax - vmin;
  const double dvd = (double)dv, vd = (double)v, vmind = (double)vmin;
  if (vd < vmind + 0.25 * dvd) {
    c[2] = 0;
    c[1] = to_u8(255.0f * ((4.0f * (v - vmin)) / dv));
  } else if (vd < vmind + 0.5 * dvd) {
    c[2] = 0;
    c[0] = to_u8(255.0 * (1.0 + (4.0 * ((vmind + 0.25 * dvd) - vd)) / dvd));
  } else if (vd < vmind + 0.75 * dvd) {
    c[2] = to_u8(255.0 * ((4.0 * ((double)(v - vmin) - 0.5 * dvd)) / dvd));
    c[0] = 0;
  } else {
    c[1] = to_u8(255.0 * (1.0 + (4.0 * ((vmind + 0.75 * dvd) - vd)) / dvd));
    c[0] = 0;
  }
}

// jet(v, 0, 2): the map of the inverse-depth colours (drawInverseDepthMap, drawFeatures, drawWireframe, the matches)
__device__ __forceinline__ void jet02(float v, uint8_t c[3]) { jet(v, 0.0f, 2.0f, c); }

// four pixels, each packed as c[0] | c[1] << 8 | c[2] << 16 -> memory: three dwords where all four exist, bytes at the image's tail
__device__ __forceinline__ uint32_t pack3(const uint8_t c[3]) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16); }
__device__ __forceinline__ void store_pixels(uint8_t* __restrict__ img, long o0, long n, const uint32_t px[4]) {
  if (o0 + kPixelsPerThread <= n) {
    uint32_t* p = (uint32_t*)(img + 3 * o0);  // (3 * 4 j bytes from a 4-byte aligned base)
    p[0] = px[0] | (px[1] << 24);
    p[1] = (px[1] >> 8) | (px[2] << 16);
    p[2] = (px[2] >> 16) | (px[3] << 8);
  } else {
#pragma unroll
    for (int k = 0; k < kPixelsPerThread - 1; ++k)
      if (o0 + k < n) {
        uint8_t* q = img + 3 * (o0 + k);
        q[0] = (uint8_t)px[k], q[1] = (uint8_t)(px[k] >> 8), q[2] = (uint8_t)(px[k] >> 16);
      }
  }
}

}  // namespace
}  // namespace flame_hip
