// volume_shift_kernels.hip -- the window of the truncated-signed-distance volume moved over the grid (include/flame_nltgv2.h,
// flame_nltgv2_volume_shift_begin): out of place, from the volume's buffer into a second one of the same size.
//   A lane owns the linear index L of one record (the 8-byte path) or of two records side by side along x (the 16-byte path, taken
// where nx and the linear displacement delta = (s.z * ny + s.y) * nx + s.x are even: then s.x is even too, a pair starts at an even i,
// stays in its row, and both of its records stay or leave together).  The lane
//   reads source L, once;
//   scatters it to L - delta where (i, j, k) - s lies in the volume, else counts it as lost;
//   writes the fresh record {1.0f, 0.0f} to destination L where (i, j, k) + s does not lie in the volume: destination L has no source.
// So every source record is read exactly once and every destination record has exactly one writer; the loads and both kinds of stores
// run along x with the lanes.  No floating-point atomics, no counter raced for a place: two calls give the same bytes, and the two
// paths give the same bytes as each other.  A record travels as 8 (16) bytes in integer registers: NaN payloads, -0 and subnormals survive.
//   A workgroup takes 256 consecutive units per round and walks the volume in strides of the grid (at most kIntegrateGrid workgroups,
// as the integration does and for its reason: volume_kernels.h), keeping (i, j, k) by carries, not by divisions: the kernel has two
// divisions per lane, not per record.  The counters: ballot + popcount per wave as in volume_kernels.hip, one set of integer atomics per
// workgroup into one of the kVolumeCountSlots partial sets.
#include <hip/hip_runtime.h>

#include "volume_kernels.h"

namespace flame_hip {
namespace {

struct ShiftArgs {
  int nxu, ny, nz;  // the volume in units along x (nx, or nx / 2 pairs), rows, slices
  int su, sy, sz;   // the shift in the same units
  int delta_u;      // the linear displacement in units
};

__device__ __forceinline__ int wave_count(bool flag) { return __popcll(__ballot(flag)); }
__device__ __forceinline__ bool within(int v, int n) { return (unsigned)v < (unsigned)n; }

// Unit: uint2 (one record) or uint4 (two).  kMove == false: nothing is written, the counters alone are made.
template <class Unit, bool kMove>
__global__ void __launch_bounds__(kVolumeBlock)
k_volume_shift(const ShiftArgs a, const Unit* __restrict__ src, Unit* __restrict__ dst, int* __restrict__ counts) {
  constexpr bool kPair = sizeof(Unit) == 16;
  __shared__ int s_cnt[kShiftCounters];
  if (threadIdx.x < kShiftCounters) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t n = (uint32_t)a.nxu * (uint32_t)a.ny * (uint32_t)a.nz;  // (<= 2^28)
  const uint32_t stride = gridDim.x * (uint32_t)kVolumeBlock;            // (<= 2^18)
  // the stride as steps along the three axes; the lane's own place
  const uint32_t stride_rows = stride / (uint32_t)a.nxu;
  const int di = (int)(stride - stride_rows * (uint32_t)a.nxu), dk = (int)(stride_rows / (uint32_t)a.ny);
  const int dj = (int)(stride_rows - (uint32_t)dk * (uint32_t)a.ny);
  uint32_t L = blockIdx.x * (uint32_t)kVolumeBlock + threadIdx.x;
  const uint32_t row0 = L / (uint32_t)a.nxu;
  int i = (int)(L - row0 * (uint32_t)a.nxu), k = (int)(row0 / (uint32_t)a.ny);
  int j = (int)(row0 - (uint32_t)k * (uint32_t)a.ny);
  Unit fresh;
  fresh.x = 0x3f800000u, fresh.y = 0u;  // {1.0f, 0.0f}
  if constexpr (kPair) fresh.z = 0x3f800000u, fresh.w = 0u;
  int cnt[kShiftCounters] = {0, 0, 0, 0};
  for (uint32_t first = blockIdx.x * (uint32_t)kVolumeBlock; first < n; first += stride) {  // (uniform in the workgroup)
    bool keep = false, enters = false;
    int seen = 0;
    if (L < n) {
      const Unit r = src[L];
      seen = (__uint_as_float(r.y) > 0.0f) ? 1 : 0;
      if constexpr (kPair) seen += (__uint_as_float(r.w) > 0.0f) ? 1 : 0;
      keep = within(i - a.su, a.nxu) && within(j - a.sy, a.ny) && within(k - a.sz, a.nz);
      enters = !(within(i + a.su, a.nxu) && within(j + a.sy, a.ny) && within(k + a.sz, a.nz));
      if (kMove) {
        if (keep) dst[(int)L - a.delta_u] = r;  // (in range: its three indices are)
        if (enters) dst[L] = fresh;
      }
    }
    const int per = kPair ? 2 : 1;
    cnt[0] += per * wave_count(keep), cnt[3] += per * wave_count(enters);
    // the seen records of the lanes that keep / lose theirs: 0, 1 or 2 per lane
    cnt[1] += wave_count(keep && seen >= 1) + wave_count(keep && seen == 2);
    cnt[2] += wave_count(L < n && !keep && seen >= 1) + wave_count(L < n && !keep && seen == 2);
    L += stride;
    i += di;
    if (i >= a.nxu) i -= a.nxu, ++j;
    j += dj;
    if (j >= a.ny) j -= a.ny, ++k;
    k += dk;
  }
  if ((threadIdx.x & 63) == 0)
    for (int c = 0; c < kShiftCounters; ++c)
      if (cnt[c]) atomicAdd(&s_cnt[c], cnt[c]);
  __syncthreads();
  if (threadIdx.x < kShiftCounters && s_cnt[threadIdx.x])
    atomicAdd(&counts[(blockIdx.x % kVolumeCountSlots) * kVolumeCountSlotWords + threadIdx.x], s_cnt[threadIdx.x]);
}

template <class Unit>
void launch_units(const ShiftArgs& a, const Voxel* src, Voxel* dst, int* counts, hipStream_t s) {
  const long n = (long)a.nxu * a.ny * a.nz;
  const long blocks = volume_blocks(n) < kIntegrateGrid ? volume_blocks(n) : kIntegrateGrid;
  if (dst) hipLaunchKernelGGL((k_volume_shift<Unit, true>), dim3((unsigned)blocks), dim3(kVolumeBlock), 0, s, a, (const Unit*)src, (Unit*)dst, counts);
  else hipLaunchKernelGGL((k_volume_shift<Unit, false>), dim3((unsigned)blocks), dim3(kVolumeBlock), 0, s, a, (const Unit*)src, (Unit*)nullptr, counts);
}

}  // namespace

int launch_volume_shift(const VolumeGrid& g, const int shift[3], const Voxel* src, Voxel* dst, int* counts, int* record_bytes, hipStream_t s) {
  const long delta = ((long)shift[2] * g.ny + shift[1]) * g.nx + shift[0];
  const bool pair = g.nx % 2 == 0 && delta % 2 == 0;  // (then shift[0] is even)
  ShiftArgs a;
  a.nxu = pair ? g.nx / 2 : g.nx, a.ny = g.ny, a.nz = g.nz;
  a.su = pair ? shift[0] / 2 : shift[0], a.sy = shift[1], a.sz = shift[2];
  a.delta_u = (int)(pair ? delta / 2 : delta);
  (void)hipMemsetAsync(counts, 0, kVolumeCountsBytes, s);
  if (pair) launch_units<uint4>(a, src, dst, counts, s);
  else launch_units<uint2>(a, src, dst, counts, s);
  if (record_bytes) *record_bytes = pair ? 16 : 8;
  return (int)hipGetLastError();
}

}  // namespace flame_hip
