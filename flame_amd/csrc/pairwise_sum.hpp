// pairwise_sum.hpp -- the one fixed-order sum of this library's double reductions (flame_nltgv2_map_error's `sum`, include/flame_nltgv2.h;
// the 28 sums of flame_stereo_align_linearize, include/flame_stereo.h): p[t] += p[t + s] for s = 512, 256, ..., 1 over the 1024 values of a
// workgroup of 1024 threads.  The result is a function of the 1024 values alone, so it does not depend on the launch geometry.
#pragma once
#include <hip/hip_runtime.h>

namespace flame_hip {

constexpr int kPairwiseChunk = 1024;  // values per sum = threads per workgroup: part of the sum's definition

// N sums at once over p[k * 1024 + t], k < N: the barriers are shared, the additions of each sum are those of the rule.  out[k] is the
// sum for thread 0 (the other threads get values of no meaning).  The steps down to 64 go through LDS; the last six stay inside wave 0:
// lane t adds the value of lane t + s, which for t < s is the very p[t + s] of the rule -- the same additions in the same order, without
// six barriers.
template <int N>
__device__ __forceinline__ void pairwise_sum_n(double* p, int t, double* out) {
  __syncthreads();
  for (int s = kPairwiseChunk / 2; s >= 64; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int k = 0; k < N; ++k) p[k * kPairwiseChunk + t] += p[k * kPairwiseChunk + t + s];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < N; ++k) out[k] = 0.0;
  if (t < 64) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      double v = p[k * kPairwiseChunk + t];
      for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s);
      out[k] = v;
    }
  }
  __syncthreads();  // (p may be rewritten behind this)
}

__device__ __forceinline__ double pairwise_sum(double* p, int t) {
  double v;
  pairwise_sum_n<1>(p, t, &v);
  return v;
}

}  // namespace flame_hip
