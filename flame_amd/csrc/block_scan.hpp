// block_scan.hpp -- the one-workgroup exclusive scan of mesh_kernels.hip (the incidence lists' offsets) and metric_kernels.hip (the
// compactions' workgroup counts): a chunk of the array per thread, the chunk totals through LDS.  Device-only.
#pragma once
#include <hip/hip_runtime.h>

namespace flame_hip {

constexpr int kScanThreads = 1024;

// For a kernel of ONE workgroup of kScanThreads threads.  tail(i, run) is called once for every i of [0, n) with run = the sum of
// data[0 .. i): it stores what becomes of element i (also over data[i], read by then).  Returns the sum of all n to every thread.
template <class Tail>
__device__ __forceinline__ int block_exclusive_scan(int n, const int* data, Tail tail) {
  __shared__ int s_sum[kScanThreads];
  const int chunk = (n + kScanThreads - 1) / kScanThreads;
  const long lo_l = (long)threadIdx.x * chunk;  // (it and lo_l + chunk may pass n: long, so that no n wraps)
  const int lo = (int)(lo_l < n ? lo_l : n), hi = (int)(lo_l + chunk < n ? lo_l + chunk : n);
  int sum = 0;
  for (int i = lo; i < hi; ++i) sum += data[i];
  s_sum[threadIdx.x] = sum;
  __syncthreads();
  for (int d = 1; d < kScanThreads; d <<= 1) {  // inclusive scan of the chunk totals
    const int add = threadIdx.x >= (unsigned)d ? s_sum[threadIdx.x - d] : 0;
    __syncthreads();
    s_sum[threadIdx.x] += add;
    __syncthreads();
  }
  int run = s_sum[threadIdx.x] - sum;
  for (int i = lo; i < hi; ++i) {
    const int c = data[i];
    tail(i, run);
    run += c;
  }
  return s_sum[kScanThreads - 1];
}

}  // namespace flame_hip
