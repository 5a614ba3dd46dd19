// draw_offsets.hpp -- the kernel wireframe_kernels.hip and matches_kernels.hip share between their count and fill passes: every
// touched pixel takes its range of the entry buffer from one cursor.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace flame_hip {
namespace {

// offset[p] = the sum of cnt over the pixels that came before p at the cursor.  A lane sums kOffsetsPerLane consecutive pixels, the
// wave scans its 64 sums with shuffles and takes its range with ONE atomicAdd: atomics on one address follow each other at about
// 11 ns, and a wave per 64 pixels made this kernel the longest of the wireframe's five (370 us at 1080p); a wave per 1024 pixels takes 2025.
// No lane leaves before the shuffles.
constexpr int kOffsetsPerLane = 16;

__global__ void __launch_bounds__(256)
k_draw_offsets(long n, const uint32_t* __restrict__ cnt, uint32_t* __restrict__ offset, uint32_t* __restrict__ cursor) {
  const long i0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * kOffsetsPerLane;
  const int lane = threadIdx.x & 63;
  uint32_t c[kOffsetsPerLane];
  uint32_t sum = 0u;
#pragma unroll
  for (int k = 0; k < kOffsetsPerLane; ++k) {
    c[k] = i0 + k < n ? cnt[i0 + k] : 0u;
    sum += c[k];
  }
  uint32_t incl = sum;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const uint32_t v = __shfl_up(incl, s, 64);
    if (lane >= s) incl += v;
  }
  uint32_t base = 0u;
  if (lane == 63 && incl != 0u) base = atomicAdd(cursor, incl);
  base = __shfl(base, 63, 64);
  uint32_t at = base + (incl - sum);
#pragma unroll
  for (int k = 0; k < kOffsetsPerLane; ++k) {
    if (i0 + k < n) offset[i0 + k] = at;
    at += c[k];
  }
}

}  // namespace
}  // namespace flame_hip
