// volume_kernels.hip -- the truncated-signed-distance volume (include/flame_nltgv2.h, flame_nltgv2_volume_create):
//   fill        every voxel {1.0f, 0.0f}
//   integrate   one pass over the volume, one lane per voxel and round with x along the lanes: the voxel centre into the camera, the nearest
//               pixel of the inverse-depth map, the projective signed distance, the weighted mean.  The tests of rules 2 - 7 come before
//               the voxel's record is loaded, so a voxel that is not updated costs no memory traffic but the map's pixel, and a wave
//               whose lanes are all behind the camera or outside the image touches no memory at all.
//   raycast     one lane per pixel marches z_near + n * dz, eight 8-byte taps per step, trilinear, to the first valid sample <= 0; a wave
//               leaves when all of its rays have ended.
// The arithmetic is scalar float code with every sum of three products taken left to right (built with -ffp-contract=off: no FMA;
// correctly rounded division), so that the outputs equal the numpy restatement (tests/volume_ref.py) bit for bit.  Every voxel has
// one owner and there are no floating-point atomics: the same calls in the same order give the same bytes.
//   The counters: ballot + popcount per wave, summed in registers over a workgroup's rounds, one LDS word per counter and workgroup, then
// one integer atomic per workgroup and counter into one of kVolumeCountSlots partial sets (volume_kernels.h says why).
#include <hip/hip_runtime.h>

#include "volume_kernels.h"

namespace flame_hip {
namespace {

constexpr uint32_t kQuietNan = 0x7fc00000u;

inline dim3 grid1d(long n) { return dim3((unsigned)volume_blocks(n)); }

// ((m0 * x + m1 * y) + m2 * z) + t for the three rows of a row-major [R | t].
__device__ __forceinline__ void pose_point(const float* T, float x, float y, float z, float& ox, float& oy, float& oz) {
  ox = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
  oy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
  oz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

// The lanes of this wave with `flag`: the same number in every lane.
__device__ __forceinline__ int wave_count(bool flag) { return __popcll(__ballot(flag)); }

// A workgroup's counters (s_cnt, summed over its waves) into its partial set of the stage's counters.
template <int N>
__device__ __forceinline__ void publish_counts(const int* wave_cnt, int* s_cnt, int* __restrict__ counts) {
  if ((threadIdx.x & 63) == 0)
    for (int c = 0; c < N; ++c)
      if (wave_cnt[c]) atomicAdd(&s_cnt[c], wave_cnt[c]);
  __syncthreads();
  if (threadIdx.x < N && s_cnt[threadIdx.x])
    atomicAdd(&counts[(blockIdx.x % kVolumeCountSlots) * kVolumeCountSlotWords + threadIdx.x], s_cnt[threadIdx.x]);
}

__global__ void __launch_bounds__(kVolumeBlock)
k_volume_fill(long n, Voxel* __restrict__ vol) {
  const long i = (long)blockIdx.x * kVolumeBlock + threadIdx.x;
  if (i < n) vol[i] = Voxel{1.0f, 0.0f};
}

// A workgroup takes 256 consecutive voxels per round and walks the volume in strides of the grid (at most kIntegrateGrid workgroups), so
// that its counters cost one set of atomics per workgroup, not per 256 voxels.
__global__ void __launch_bounds__(kVolumeBlock)
k_volume_integrate(const VolumeGrid g, const IntegrateArgs a, const float* __restrict__ map, Voxel* __restrict__ vol, int* __restrict__ counts) {
  __shared__ int s_cnt[kIntegrateCounters];
  if (threadIdx.x < kIntegrateCounters) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t n = (uint32_t)g.nx * (uint32_t)g.ny * (uint32_t)g.nz;  // (<= 2^28: flame_nltgv2_volume_create)
  const float u_end = (float)a.cols - 0.5f, v_end = (float)a.rows - 0.5f;
  int cnt[kIntegrateCounters] = {0, 0, 0, 0, 0, 0};
  for (uint32_t base = blockIdx.x * (uint32_t)kVolumeBlock; base < n; base += gridDim.x * (uint32_t)kVolumeBlock) {  // (uniform in the workgroup)
    const uint32_t idx = base + threadIdx.x;
    bool front = false, in = false, valid = false, behind = false, updated = false, saturated = false;
    float Pz = 0.0f, u = 0.0f, v = 0.0f;
    if (idx < n) {
      const uint32_t row_idx = idx / (uint32_t)g.nx, i = idx - row_idx * (uint32_t)g.nx;
      const uint32_t k = row_idx / (uint32_t)g.ny, j = row_idx - k * (uint32_t)g.ny;
      // (the global index: the sum in integers, then the conversion)
      const float px = g.origin[0] + (float)(g.base[0] + (int)i) * g.voxel_size;
      const float py = g.origin[1] + (float)(g.base[1] + (int)j) * g.voxel_size;
      const float pz = g.origin[2] + (float)(g.base[2] + (int)k) * g.voxel_size;
      float Px, Py;
      pose_point(a.pose, px, py, pz, Px, Py, Pz);
      front = Pz > a.near_depth;
      if (front) {
        const float q0 = (a.K[0] * Px + a.K[1] * Py) + a.K[2] * Pz;
        const float q1 = (a.K[3] * Px + a.K[4] * Py) + a.K[5] * Pz;
        const float q2 = (a.K[6] * Px + a.K[7] * Py) + a.K[8] * Pz;
        u = q0 / q2, v = q1 / q2;
        in = u >= -0.5f && u < u_end && v >= -0.5f && v < v_end;  // (first, so that no NaN or huge value reaches a conversion)
      }
    }
    if (in) {
      int col = (int)floorf(u + 0.5f), row = (int)floorf(v + 0.5f);
      col = col < 0 ? 0 : col > a.cols - 1 ? a.cols - 1 : col;
      row = row < 0 ? 0 : row > a.rows - 1 ? a.rows - 1 : row;
      const float d = map[(size_t)row * (size_t)a.cols + (size_t)col];
      const float zm = 1.0f / d;
      valid = d > 0.0f && zm > a.min_depth && zm < a.max_depth;  // (a NaN fails every one of them)
      if (valid) {
        const float sdf = zm - Pz;
        behind = sdf < -g.trunc;
        if (!behind) {
          const float s = fminf(sdf / g.trunc, 1.0f);
          const Voxel o = vol[idx];
          const float W = o.weight + a.weight;
          Voxel w;
          w.tsdf = ((o.tsdf * o.weight) + (s * a.weight)) / W;
          w.weight = fminf(W, g.max_weight);
          vol[idx] = w;
          updated = true;
          saturated = W > g.max_weight;
        }
      }
    }
    cnt[0] += wave_count(front), cnt[1] += wave_count(in), cnt[2] += wave_count(valid);
    cnt[3] += wave_count(behind), cnt[4] += wave_count(updated), cnt[5] += wave_count(saturated);
  }
  publish_counts<kIntegrateCounters>(cnt, s_cnt, counts);
}

__device__ __forceinline__ float lerp1(float a, float b, float t) { return a + t * (b - a); }

// One axis of a sample: the global coordinate g in [base, base + n_axis - 1] (a NaN is not), the lower voxel's LOCAL index and the
// fraction above the lower GLOBAL voxel.
__device__ __forceinline__ bool axis_cell(float gv, int base, int n_axis, int& i0, float& f) {
  if (!(gv >= (float)base && gv <= (float)(base + n_axis - 1))) return false;
  const int fl = (int)floorf(gv);
  const int ig = fl < base + n_axis - 2 ? fl : base + n_axis - 2;
  i0 = ig - base;
  f = gv - (float)ig;
  return true;
}

__global__ void __launch_bounds__(kVolumeBlock)
k_volume_raycast(const VolumeGrid g, const RaycastArgs a, const Voxel* __restrict__ vol, float* __restrict__ out, int* __restrict__ counts) {
  __shared__ int s_cnt[3];
  if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const long n = (long)a.rows * a.cols;
  const long pix = (long)blockIdx.x * kVolumeBlock + threadIdx.x;
  bool hit = false, back = false, empty = false;
  if (pix < n) {
    const uint32_t row = (uint32_t)pix / (uint32_t)a.cols, col = (uint32_t)pix - row * (uint32_t)a.cols;  // (rows, cols <= 32767)
    const float fc = (float)col, fr = (float)row;
    const float q0 = (a.Kinv[0] * fc + a.Kinv[1] * fr) + a.Kinv[2] * 1.0f;
    const float q1 = (a.Kinv[3] * fc + a.Kinv[4] * fr) + a.Kinv[5] * 1.0f;
    const float q2 = (a.Kinv[6] * fc + a.Kinv[7] * fr) + a.Kinv[8] * 1.0f;
    const bool has_cells = g.nx >= 2 && g.ny >= 2 && g.nz >= 2;  // an axis of one voxel has no valid sample
    const size_t sy = (size_t)g.nx, sz = (size_t)g.nx * (size_t)g.ny;
    bool any_valid = false, prev_ok = false, ended = false;
    float prev_val = 0.0f, result = __uint_as_float(kQuietNan);
    for (int step = 0; step < a.n_steps && !ended; ++step) {
      const float z = a.z_near + (float)step * a.dz;
      float wx, wy, wz;
      pose_point(a.pose, q0 * z, q1 * z, q2 * z, wx, wy, wz);
      const float gx = (wx - g.origin[0]) / g.voxel_size;
      const float gy = (wy - g.origin[1]) / g.voxel_size;
      const float gz = (wz - g.origin[2]) / g.voxel_size;
      int ix = 0, iy = 0, iz = 0;
      float fx = 0.0f, fy = 0.0f, fz = 0.0f;
      bool ok = has_cells && axis_cell(gx, g.base[0], g.nx, ix, fx) && axis_cell(gy, g.base[1], g.ny, iy, fy) &&
                axis_cell(gz, g.base[2], g.nz, iz, fz);
      float val = 0.0f;
      if (ok) {
        const Voxel* b = vol + ((size_t)iz * sz + (size_t)iy * sy + (size_t)ix);
        const Voxel v000 = b[0], v100 = b[1], v010 = b[sy], v110 = b[sy + 1];
        const Voxel v001 = b[sz], v101 = b[sz + 1], v011 = b[sz + sy], v111 = b[sz + sy + 1];
        ok = v000.weight > 0.0f && v100.weight > 0.0f && v010.weight > 0.0f && v110.weight > 0.0f && v001.weight > 0.0f &&
             v101.weight > 0.0f && v011.weight > 0.0f && v111.weight > 0.0f;
        const float c00 = lerp1(v000.tsdf, v100.tsdf, fx), c10 = lerp1(v010.tsdf, v110.tsdf, fx);
        const float c01 = lerp1(v001.tsdf, v101.tsdf, fx), c11 = lerp1(v011.tsdf, v111.tsdf, fx);
        val = lerp1(lerp1(c00, c10, fy), lerp1(c01, c11, fy), fz);
      }
      if (ok) {
        any_valid = true;
        if (val <= 0.0f) {
          ended = true;
          if (prev_ok && prev_val > 0.0f) {
            const float z_prev = a.z_near + (float)(step - 1) * a.dz;
            const float zs = z_prev + a.dz * (prev_val / (prev_val - val));
            result = 1.0f / (zs * q2);
            hit = true;
          } else {
            back = true;  // the surface met from inside or behind
          }
        }
      }
      prev_ok = ok, prev_val = val;
    }
    empty = !any_valid;
    out[pix] = result;
  }
  const int cnt[3] = {wave_count(hit), wave_count(back), wave_count(empty)};
  publish_counts<3>(cnt, s_cnt, counts);
}

}  // namespace

int launch_volume_fill(const VolumeGrid& g, Voxel* vol, hipStream_t s) {
  const long n = (long)g.nx * g.ny * g.nz;
  hipLaunchKernelGGL(k_volume_fill, grid1d(n), dim3(kVolumeBlock), 0, s, n, vol);
  return (int)hipGetLastError();
}

int launch_volume_integrate(const VolumeGrid& g, const IntegrateArgs& a, const float* map, Voxel* vol, int* counts, hipStream_t s) {
  const long n = (long)g.nx * g.ny * g.nz;
  const long blocks = volume_blocks(n) < kIntegrateGrid ? volume_blocks(n) : kIntegrateGrid;
  (void)hipMemsetAsync(counts, 0, kVolumeCountsBytes, s);
  hipLaunchKernelGGL(k_volume_integrate, dim3((unsigned)blocks), dim3(kVolumeBlock), 0, s, g, a, map, vol, counts);
  return (int)hipGetLastError();
}

int launch_volume_raycast(const VolumeGrid& g, const RaycastArgs& a, const Voxel* vol, float* out, int* counts, hipStream_t s) {
  const long n = (long)a.rows * a.cols;
  (void)hipMemsetAsync(counts, 0, kVolumeCountsBytes, s);
  hipLaunchKernelGGL(k_volume_raycast, grid1d(n), dim3(kVolumeBlock), 0, s, g, a, vol, out, counts);
  return (int)hipGetLastError();
}

}  // namespace flame_hip
