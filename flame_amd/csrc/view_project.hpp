// view_project.hpp -- rules 1 - 5 (view_device.hpp) as the bodies of the clear, vertices, count, raster and raster_big kernels, written once
// for view_kernels.hip (one mesh into one key image) and fuse_kernels.hip (up to eight meshes into eight key layers), whose __global__
// entry points are thin instances.  Device-only.  A body is a template over the SOURCES m it draws, which answer:
//   m.v_end, m.t_end                   how many vertices and triangles there are, over all sources
//   source_of_vertex / _triangle(m, i) the source k that vertex / triangle i of the concatenated numbering belongs to
//   source(m, k)                       its FuseSource: i - v0 / i - t0 is the local index, vtx[v0 + tris[..]] a triangle's three ViewVertex
//   key_layer(m, keys, k, rows, cols)  the key image source k is drawn into
//   kCountsCulled<Sources>             whether the stage publishes rule 2's culled classes beside the drawn one
// The two models: OneSource (the view renderer: k is 0, nothing is searched, the culled classes are counted) and FuseTable.
#pragma once
#include <hip/hip_runtime.h>

#include "fuse_kernels.h"
#include "view_device.hpp"

namespace flame_hip {
namespace view_project {

using namespace view_device;

struct OneSource {
  FuseSource s;  // (v0 = t0 = 0)
  int32_t v_end, t_end;
};
__device__ __forceinline__ int source_of_vertex(const OneSource&, int) { return 0; }
__device__ __forceinline__ int source_of_triangle(const OneSource&, int) { return 0; }
__device__ __forceinline__ const FuseSource& source(const OneSource& m, int) { return m.s; }
__device__ __forceinline__ unsigned long long* key_layer(const OneSource&, unsigned long long* keys, int, int, int) { return keys; }

// The last source whose `start` (v0 or t0) is at or before i: how many of the later ones have begun.  Empty sources share their start
// with the next one and are passed over.  (A popcount of the comparisons, not their sum: the compiler turns a sum's last term into a
// select between two sources' addresses for every member that is loaded, and k_fuse_vertices then loads its camera dword by dword.)
__device__ __forceinline__ int source_at(const FuseTable& tab, int32_t FuseSource::*start, int i) {
  unsigned begun = 0u;
#pragma unroll
  for (int j = 1; j < kFuseSources; ++j) begun |= (j < tab.n && i >= tab.s[j].*start) ? 1u << j : 0u;
  return __popc(begun);
}
__device__ __forceinline__ int source_of_vertex(const FuseTable& tab, int v) { return source_at(tab, &FuseSource::v0, v); }
__device__ __forceinline__ int source_of_triangle(const FuseTable& tab, int t) { return source_at(tab, &FuseSource::t0, t); }
__device__ __forceinline__ const FuseSource& source(const FuseTable& tab, int k) { return tab.s[k]; }
__device__ __forceinline__ unsigned long long* key_layer(const FuseTable&, unsigned long long* keys, int k, int rows, int cols) {
  return keys + (size_t)k * (size_t)rows * (size_t)cols;
}
template <class Sources> inline constexpr bool kCountsCulled = false;
template <> inline constexpr bool kCountsCulled<OneSource> = true;

constexpr int kPerThread = kViewResolveTile / 256;
inline dim3 tiles(long n) { return dim3((unsigned)((n + kViewResolveTile - 1) / kViewResolveTile)); }

// keys[i] = 0 for this workgroup's tile of kViewResolveTile keys (256 threads).
__device__ __forceinline__ void clear_tile(long n, unsigned long long* __restrict__ keys) {
  const long base = (long)blockIdx.x * kViewResolveTile + threadIdx.x;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const long i = base + (long)j * 256;
    if (i < n) keys[i] = 0ull;
  }
}

// vertices: one lane per vertex of any source, rule 1 with that source's camera
template <class Sources>
__device__ __forceinline__ void project_vertices(const Sources& m, ViewVertex* __restrict__ out) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= m.v_end) return;
  const FuseSource& S = source(m, source_of_vertex(m, v));
  const int local = v - S.v0;
  out[v] = view_vertex(S.pos[local], S.values[local] * S.value_scale, S.cam);
}

struct Triangle { ViewVertex a, b, c; };
__device__ __forceinline__ Triangle load_triangle(const FuseSource& S, int local, const ViewVertex* __restrict__ vtx) {
  const int32_t* tri = S.tris + 3 * (size_t)local;
  return Triangle{vtx[S.v0 + tri[0]], vtx[S.v0 + tri[1]], vtx[S.v0 + tri[2]]};
}

// count: one lane per triangle of any source (256 threads).  Rule 2's classes are tallied with one LDS atomic per wave; thread 0 then calls
// publish(n), n[class] the workgroup's totals (n[kDraw] alone unless kCountsCulled).  A drawn triangle whose box holds more than
// kViewWavePixels pixels is listed: big[2 + 2 i] = its source, big[3 + 2 i] = its index there, big[0] counts them (few: depth edges).
template <class Sources, class Publish>
__device__ __forceinline__ void count_triangles(const Sources& m, const ViewVertex* __restrict__ vtx, int* __restrict__ big, int rows, int cols,
                                                Publish publish) {
  constexpr int kClasses = kCountsCulled<Sources> ? kCulledFacing + 1 : kDraw + 1;
  __shared__ int s_n[kClasses];
  if (threadIdx.x < kClasses) s_n[threadIdx.x] = 0;
  __syncthreads();
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  int cls = kInvalid;
  if (t < m.t_end) {
    const int k = source_of_triangle(m, t);
    const FuseSource& S = source(m, k);
    const int local = t - S.t0;
    const Triangle tr = load_triangle(S, local, vtx);
    long long A = 0;
    cls = classify(local, S.tri_valid, tr.a, tr.b, tr.c, &A);
    if (cls == kDraw && bounding_box(tr.a, tr.b, tr.c, rows, cols).n > (unsigned)kViewWavePixels) {
      const int at = atomicAdd(&big[0], 1);
      big[2 + 2 * at] = k, big[3 + 2 * at] = local;
    }
  }
#pragma unroll
  for (int c = kDraw; c < kClasses; ++c) {
    if (c == kInvalid) continue;
    const int n = __popcll(__ballot(cls == c));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&s_n[c], n);
  }
  __syncthreads();
  if (threadIdx.x == 0) publish(s_n);
}

// raster: one wavefront per triangle whose box holds at most kViewWavePixels pixels; the others are raster_big's
template <class Sources>
__device__ __forceinline__ void raster_triangle(const Sources& m, const ViewVertex* __restrict__ vtx, unsigned long long* __restrict__ keys, int rows,
                                                int cols) {
  const int t = blockIdx.x;
  if (t >= m.t_end) return;
  const int k = source_of_triangle(m, t);
  const FuseSource& S = source(m, k);
  const int local = t - S.t0;
  const Triangle tr = load_triangle(S, local, vtx);
  long long A = 0;
  if (classify(local, S.tri_valid, tr.a, tr.b, tr.c, &A) != kDraw) return;
  const ViewBox box = bounding_box(tr.a, tr.b, tr.c, rows, cols);
  if (box.n > (unsigned)kViewWavePixels) return;
  raster_pixels(local, A, tr.a, tr.b, tr.c, box, threadIdx.x, 64u, key_layer(m, keys, k, rows, cols), cols);
}

// raster_big: kViewBigWaves wavefronts share one listed triangle's box (blockIdx.x: which of them), blockIdx.y walks the list
template <class Sources>
__device__ __forceinline__ void raster_listed(const Sources& m, const ViewVertex* __restrict__ vtx, const int* __restrict__ big,
                                              unsigned long long* __restrict__ keys, int rows, int cols) {
  const int n_big = big[0];
  for (int item = blockIdx.y; item < n_big; item += gridDim.y) {
    const int k = big[2 + 2 * item], local = big[3 + 2 * item];
    const Triangle tr = load_triangle(source(m, k), local, vtx);
    long long A = 0;
    (void)classify(local, nullptr, tr.a, tr.b, tr.c, &A);  // (listed: drawn)
    raster_pixels(local, A, tr.a, tr.b, tr.c, bounding_box(tr.a, tr.b, tr.c, rows, cols), blockIdx.x * 64u + threadIdx.x, 64u * kViewBigWaves,
                  key_layer(m, keys, k, rows, cols), cols);
  }
}

}  // namespace view_project
}  // namespace flame_hip
