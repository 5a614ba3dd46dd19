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
// clear, vertices and the three triangle kernels are thin instances of the bodies in view_project.hpp, which fuse_kernels.hip
// instantiates too: this file draws ONE source (view_project::OneSource -- no table is searched, the listed boxes are (0, triangle)
// pairs) and publishes all three counted classes of rule 2.  The resolve is this file's own.  Rules 1 - 5: view_device.hpp.
// No floating-point atomics: the key image does not depend on scheduling.  Built with -ffp-contract=off (no FMA); division and the
// int64 -> float conversions are correctly rounded.
#include <hip/hip_runtime.h>

#include "view_kernels.h"
#include "view_project.hpp"

namespace flame_hip {
namespace {

using namespace view_project;  // the five bodies, shared with fuse_kernels.hip; OneSource: this file's model of the sources

__global__ void __launch_bounds__(256)
k_view_clear(long n, unsigned long long* __restrict__ keys, ViewCounts* __restrict__ counts, int* __restrict__ big) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *counts = ViewCounts{0, 0, 0, 0}, big[0] = 0;
  clear_tile(n, keys);
}

__global__ void __launch_bounds__(256)
k_view_vertices(OneSource m, ViewVertex* __restrict__ out) { project_vertices(m, out); }

__global__ void __launch_bounds__(256)
k_view_count(OneSource m, const ViewVertex* __restrict__ vtx, ViewCounts* __restrict__ counts, int* __restrict__ big, int rows, int cols) {
  count_triangles(m, vtx, big, rows, cols, [=](const int* n) {
    if (n[kDraw]) atomicAdd(&counts->tris_drawn, n[kDraw]);
    if (n[kCulledVertex]) atomicAdd(&counts->tris_culled_vertex, n[kCulledVertex]);
    if (n[kCulledFacing]) atomicAdd(&counts->tris_culled_facing, n[kCulledFacing]);
  });
}

__global__ void __launch_bounds__(64)
k_view_raster(OneSource m, const ViewVertex* __restrict__ vtx, unsigned long long* __restrict__ keys, int rows, int cols) {
  raster_triangle(m, vtx, keys, rows, cols);
}

__global__ void __launch_bounds__(64)
k_view_raster_big(OneSource m, const ViewVertex* __restrict__ vtx, const int* __restrict__ big, unsigned long long* __restrict__ keys, int rows,
                  int cols) {
  raster_listed(m, vtx, big, keys, rows, cols);
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

}  // namespace

int launch_view_clear(long n, unsigned long long* keys, ViewCounts* counts, int* big, hipStream_t s) {
  hipLaunchKernelGGL(k_view_clear, tiles(n > 0 ? n : 1), dim3(256), 0, s, n, keys, counts, big);
  return (int)hipGetLastError();
}

int launch_view_vertices(const FuseSource& mesh, int V, ViewVertex* out, hipStream_t s) {
  if (V <= 0) return 0;
  hipLaunchKernelGGL(k_view_vertices, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, s, OneSource{mesh, V, 0}, out);
  return (int)hipGetLastError();
}

int launch_view_raster(const FuseSource& mesh, int T, const ViewVertex* vtx, unsigned long long* keys, ViewCounts* counts, int* big, int rows,
                       int cols, hipStream_t s) {
  if (T <= 0) return 0;
  const OneSource m{mesh, 0, T};
  hipLaunchKernelGGL(k_view_count, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, m, vtx, counts, big, rows, cols);
  hipLaunchKernelGGL(k_view_raster, dim3((unsigned)T), dim3(64), 0, s, m, vtx, keys, rows, cols);
  hipLaunchKernelGGL(k_view_raster_big, dim3(kViewBigWaves, kViewBigRows), dim3(64), 0, s, m, vtx, big, keys, rows, cols);
  return (int)hipGetLastError();
}

int launch_view_resolve(long n, const unsigned long long* keys, float* map, int32_t* tri_index, ViewCounts* counts, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_view_resolve, tiles(n), dim3(256), 0, s, n, keys, map, tri_index, counts);
  return (int)hipGetLastError();
}

}  // namespace flame_hip
