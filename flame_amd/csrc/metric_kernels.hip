// metric_kernels.hip -- the metric outputs (include/flame_nltgv2.h, flame_nltgv2_metric_outputs_begin) from a dense inverse-depth map
// and the mesh buffers of flame_nltgv2_mesh_outputs_begin:
//   per pixel   q = Kinv * (col, row, 1);  P = q / v;  valid iff v > 0 && P.z > min_depth && P.z < max_depth;  P_w = R * P + t
//   depth, depth_mm, organized   one pass, one lane per pixel
//   cloud, cloud_pixel           the valid pixels in row-major order: count (that same pass) -> scan -> scatter
//   mesh vertices / normals      the back-projected vertices of mesh_kernels.hip, posed
//   mesh triangles               the triangles with non-zero validity in ascending index: count -> scan -> scatter
// The arithmetic is scalar float code with every sum of three products taken left to right (built with -ffp-contract=off: no FMA;
// correctly rounded division), so that the outputs equal the numpy restatement (tests/metric_ref.py) bit for bit.
//
// The compactions use no counter in memory that lanes race for: a lane's rank is (valid pixels of the workgroups before its own, from
// the scan) + (those of the waves before its own, through LDS) + (those of the lanes before it, from the 64-bit ballot), so the order
// is the pixels' own and two calls give the same bytes.
//
// The 12-byte points: every lane stores its x, y, z itself, three dword stores 12 bytes apart from its neighbours'; a wave's three
// instructions together fill the same 768 consecutive bytes.  Staging the points through LDS, so that every instruction writes 256
// consecutive bytes, was measured and was 4-11 % SLOWER (profiles/metric_outputs.txt): it is not done.
#include <hip/hip_runtime.h>

#include "block_scan.hpp"
#include "metric_kernels.h"

namespace flame_hip {
namespace {

constexpr int kWaves = kMetricBlock / 64;
constexpr uint32_t kQuietNan = 0x7fc00000u;

inline dim3 grid1d(long n) { return dim3((unsigned)metric_blocks(n)); }

struct Point {
  float x, y, z;  // the point that is written (camera or world frame)
  float depth;    // the camera-frame z
  bool valid;
};

__device__ __forceinline__ void pose_point(const MetricArgs& a, float& x, float& y, float& z) {
  const float wx = ((a.pose[0] * x + a.pose[1] * y) + a.pose[2] * z) + a.pose[3];
  const float wy = ((a.pose[4] * x + a.pose[5] * y) + a.pose[6] * z) + a.pose[7];
  const float wz = ((a.pose[8] * x + a.pose[9] * y) + a.pose[10] * z) + a.pose[11];
  x = wx, y = wy, z = wz;
}

__device__ __forceinline__ Point metric_point(const MetricArgs& a, long i, float v) {
  // (rows * cols < 2^31, flame_nltgv2_metric_outputs_begin: one 32-bit division, not an emulated 64-bit one)
  const uint32_t row = (uint32_t)i / (uint32_t)a.cols, col = (uint32_t)i - row * (uint32_t)a.cols;
  const float fc = (float)col, fr = (float)row;
  const float q0 = (a.Kinv[0] * fc + a.Kinv[1] * fr) + a.Kinv[2] * 1.0f;
  const float q1 = (a.Kinv[3] * fc + a.Kinv[4] * fr) + a.Kinv[5] * 1.0f;
  const float q2 = (a.Kinv[6] * fc + a.Kinv[7] * fr) + a.Kinv[8] * 1.0f;
  Point p;
  p.x = q0 / v, p.y = q1 / v, p.z = q2 / v;
  p.depth = p.z;
  p.valid = v > 0.0f && p.z > a.min_depth && p.z < a.max_depth;  // (a NaN fails every one of them)
  if (a.has_pose) pose_point(a, p.x, p.y, p.z);
  return p;
}

// Lanes below this one whose bit is set in the wave's ballot.
__device__ __forceinline__ int lanes_before(unsigned long long ballot) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

__global__ void __launch_bounds__(kMetricBlock)
k_metric_pixels(MetricArgs a, const float* __restrict__ map, float* __restrict__ depth, uint16_t* __restrict__ depth_mm,
                float* __restrict__ organized, int* __restrict__ block_count) {
  __shared__ int s_wave[kWaves];
  const long n = (long)a.rows * a.cols;
  const long i = (long)blockIdx.x * kMetricBlock + threadIdx.x;
  Point p;
  p.valid = false;
  if (i < n) p = metric_point(a, i, map[i]);
  const float nan = __uint_as_float(kQuietNan);
  if (i < n) {
    if (depth) depth[i] = p.valid ? p.depth : nan;
    if (depth_mm) {
      const float mm = rintf(p.depth * 1000.0f);  // ties to even
      depth_mm[i] = (p.valid && mm >= 1.0f && mm <= 65535.0f) ? (uint16_t)mm : (uint16_t)0;
    }
    if (organized) organized[3 * i] = p.valid ? p.x : nan, organized[3 * i + 1] = p.valid ? p.y : nan, organized[3 * i + 2] = p.valid ? p.z : nan;
  }
  if (block_count) {
    const unsigned long long ballot = __ballot(p.valid);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(ballot);
    __syncthreads();
    if (threadIdx.x == 0) {
      int sum = 0;
      for (int w = 0; w < kWaves; ++w) sum += s_wave[w];
      block_count[blockIdx.x] = sum;
    }
  }
}

// Exclusive scan of n counts in place, their sum to *total; one workgroup (block_scan.hpp).
__global__ void __launch_bounds__(kScanThreads)
k_metric_scan(int n, int* __restrict__ count, int* __restrict__ total) {
  const int sum = block_exclusive_scan(n, count, [=](int i, int run) { count[i] = run; });
  if (threadIdx.x == kScanThreads - 1) *total = sum;
}

__global__ void __launch_bounds__(kMetricBlock)
k_metric_cloud(MetricArgs a, const float* __restrict__ map, const int* __restrict__ block_offset, float* __restrict__ cloud,
               uint32_t* __restrict__ cloud_pixel) {
  __shared__ int s_wave[kWaves];
  const long n = (long)a.rows * a.cols;
  const long i = (long)blockIdx.x * kMetricBlock + threadIdx.x;
  Point p;
  p.valid = false;
  if (i < n) p = metric_point(a, i, map[i]);
  const unsigned long long ballot = __ballot(p.valid);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_wave[wave] = __popcll(ballot);
  __syncthreads();
  int local = lanes_before(ballot);
  for (int w = 0; w < wave; ++w) local += s_wave[w];
  if (!p.valid) return;
  const long r = (long)block_offset[blockIdx.x] + local;  // (< the valid pixels of the map <= n: what cloud holds)
  cloud[3 * r] = p.x, cloud[3 * r + 1] = p.y, cloud[3 * r + 2] = p.z;
  cloud_pixel[r] = (uint32_t)i;
}

__global__ void __launch_bounds__(kMetricBlock)
k_metric_vertices(MetricArgs a, int V, const float4* __restrict__ P, const float* __restrict__ normals, float* __restrict__ vertices,
                  float* __restrict__ normals_out) {
  const int v = blockIdx.x * kMetricBlock + threadIdx.x;
  if (v >= V) return;
  const float4 p = P[v];
  float x = p.x, y = p.y, z = p.z;
  float nx = normals[3 * v], ny = normals[3 * v + 1], nz = normals[3 * v + 2];
  if (a.has_pose) {
    pose_point(a, x, y, z);
    const float rx = (a.pose[0] * nx + a.pose[1] * ny) + a.pose[2] * nz;
    const float ry = (a.pose[4] * nx + a.pose[5] * ny) + a.pose[6] * nz;
    const float rz = (a.pose[8] * nx + a.pose[9] * ny) + a.pose[10] * nz;
    nx = rx, ny = ry, nz = rz;
  }
  vertices[3 * v] = x, vertices[3 * v + 1] = y, vertices[3 * v + 2] = z;
  normals_out[3 * v] = nx, normals_out[3 * v + 1] = ny, normals_out[3 * v + 2] = nz;
}

__global__ void __launch_bounds__(kMetricBlock)
k_metric_tri_count(int T, const uint8_t* __restrict__ tri_valid, int* __restrict__ block_count) {
  __shared__ int s_wave[kWaves];
  const int t = blockIdx.x * kMetricBlock + threadIdx.x;
  const unsigned long long ballot = __ballot(t < T && tri_valid[t] != 0);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = __popcll(ballot);
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0;
    for (int w = 0; w < kWaves; ++w) sum += s_wave[w];
    block_count[blockIdx.x] = sum;
  }
}

__global__ void __launch_bounds__(kMetricBlock)
k_metric_tri_scatter(int T, const int32_t* __restrict__ tris, const uint8_t* __restrict__ tri_valid, const int* __restrict__ block_offset,
                     int32_t* __restrict__ out) {
  __shared__ int s_wave[kWaves];
  const int t = blockIdx.x * kMetricBlock + threadIdx.x;
  const bool valid = t < T && tri_valid[t] != 0;
  const unsigned long long ballot = __ballot(valid);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_wave[wave] = __popcll(ballot);
  __syncthreads();
  int local = lanes_before(ballot);
  for (int w = 0; w < wave; ++w) local += s_wave[w];
  if (!valid) return;
  const long r = (long)block_offset[blockIdx.x] + local;  // (< the valid triangles <= T: what `out` holds)
  out[3 * r] = tris[3 * t], out[3 * r + 1] = tris[3 * t + 1], out[3 * r + 2] = tris[3 * t + 2];
}

}  // namespace

int launch_metric_pixels(const MetricArgs& a, const float* map, float* depth, uint16_t* depth_mm, float* organized, int* block_count,
                         hipStream_t s) {
  const long n = (long)a.rows * a.cols;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_metric_pixels, grid1d(n), dim3(kMetricBlock), 0, s, a, map, depth, depth_mm, organized, block_count);
  return (int)hipGetLastError();
}

int launch_metric_cloud(const MetricArgs& a, const float* map, int* block_count, int* n_points, float* cloud, uint32_t* cloud_pixel,
                        hipStream_t s) {
  const long n = (long)a.rows * a.cols;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_metric_scan, dim3(1), dim3(kScanThreads), 0, s, (int)metric_blocks(n), block_count, n_points);
  hipLaunchKernelGGL(k_metric_cloud, grid1d(n), dim3(kMetricBlock), 0, s, a, map, block_count, cloud, cloud_pixel);
  return (int)hipGetLastError();
}

int launch_metric_vertices(const MetricArgs& a, int V, const float4* P, const float* normals, float* vertices, float* normals_out,
                           hipStream_t s) {
  if (V <= 0) return 0;
  hipLaunchKernelGGL(k_metric_vertices, grid1d(V), dim3(kMetricBlock), 0, s, a, V, P, normals, vertices, normals_out);
  return (int)hipGetLastError();
}

int launch_metric_triangles(int T, const int32_t* tris, const uint8_t* tri_valid, int* block_count, int* n_valid, int32_t* out,
                            hipStream_t s) {
  if (T <= 0) return 0;
  hipLaunchKernelGGL(k_metric_tri_count, grid1d(T), dim3(kMetricBlock), 0, s, T, tri_valid, block_count);
  hipLaunchKernelGGL(k_metric_scan, dim3(1), dim3(kScanThreads), 0, s, (int)metric_blocks(T), block_count, n_valid);
  hipLaunchKernelGGL(k_metric_tri_scatter, grid1d(T), dim3(kMetricBlock), 0, s, T, tris, tri_valid, block_count, out);
  return (int)hipGetLastError();
}

}  // namespace flame_hip
