// mesh_kernels.hip -- the mesh outputs of Flame::update() between the solver and the getters (flame.cc:372-407), from the
// canonical device state:
//   vtx_idepths_ = x * graph_scale                                              flame.cc:377
//   getVertexNormals (the triangle-based overload)                              flame.cc:2554-2641
//   tri_validity_: obliqueTriangleFilter, edgeLengthFilter, idepthTriangleFilter flame.cc:2207-2361, in the order of flame.cc:389-407
// The arithmetic is the reference's scalar float code, operation for operation (built with -ffp-contract=off: no FMA), so that
// the outputs equal the CPU restatement (tests/mesh_ref.py) bit for bit.  Division and square root are the correctly rounded ones
// (hipcc's default without -ffast-math).  Conventions that Eigen leaves to its version are stated in include/flame_nltgv2.h:
// sums of three products left to right, normalize() a no-op unless the squared norm is > 0.
//
// The reference back-projects every vertex three times per triangle and twice over (filter and normals); the operations per
// vertex are the same each time, so it is done once per vertex here: P[v] = (Kinv * (pos, 1)) / idepth, idepth kept in P[v].w.
//
// The vertex normals are a SEQUENTIAL running mean in triangle order (flame.cc:2614-2630) and therefore order dependent: the
// triangles of a vertex are collected with count -> scan -> fill (atomics: the fill order depends on scheduling), then the one
// lane that owns the vertex puts its short list in ascending order before it walks it.  The result depends on the triangle
// list alone.
#include <hip/hip_runtime.h>

#include "block_scan.hpp"
#include "mesh_kernels.h"

namespace flame_hip {
namespace {

inline dim3 grid1d(long n, int block = 256) { return dim3((unsigned)((n + block - 1) / block)); }

struct Vec3 {
  float x, y, z;
};

__device__ __forceinline__ Vec3 sub3(const float4& a, const float4& b) { return Vec3{a.x - b.x, a.y - b.y, a.z - b.z}; }
// Eigen's cross3: (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x)
__device__ __forceinline__ Vec3 cross3(const Vec3& a, const Vec3& b) {
  return Vec3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ float dot3(const Vec3& a, const Vec3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
// MatrixBase::normalize(): z = squaredNorm(); if (z > 0) *this /= sqrt(z)
__device__ __forceinline__ void normalize3(Vec3& v) {
  const float z = dot3(v, v);
  if (z > 0.0f) {
    const float n = sqrtf(z);
    v.x = v.x / n, v.y = v.y / n, v.z = v.z / n;
  }
}
// the skip rule of getVertexNormals, flame.cc:2585 (a NaN idepth does not skip)
__device__ __forceinline__ bool contributes(float id0, float id1, float id2) { return !((id0 <= 0.0f) || (id1 <= 0.0f) || (id2 <= 0.0f)); }

__global__ void __launch_bounds__(256)
k_mesh_vertices(int V, const float2* __restrict__ pos, const float* __restrict__ x, float graph_scale, MeshFilter f,
                float4* __restrict__ P, float* __restrict__ vtx_idepth, int* __restrict__ offset, int* __restrict__ n_valid) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v == 0) offset[V] = 0, *n_valid = 0;
  if (v >= V) return;
  const float2 u = pos[v];
  const float idepth = x[v] * graph_scale;  // flame.cc:377
  // p = Kinv * (u.x, u.y, 1) / idepth   (flame.cc:2226-2229, 2593-2596)
  const float h0 = (f.Kinv[0] * u.x + f.Kinv[1] * u.y) + f.Kinv[2] * 1.0f;
  const float h1 = (f.Kinv[3] * u.x + f.Kinv[4] * u.y) + f.Kinv[5] * 1.0f;
  const float h2 = (f.Kinv[6] * u.x + f.Kinv[7] * u.y) + f.Kinv[8] * 1.0f;
  P[v] = make_float4(h0 / idepth, h1 / idepth, h2 / idepth, idepth);
  vtx_idepth[v] = idepth;
  offset[v] = 0;
}

// One lane per triangle: the three filters (each can only clear validity), the outward normal for the vertex pass, and the
// triangle's entry in the incidence counts of its corners.
__global__ void __launch_bounds__(256)
k_mesh_triangles(int T, const int32_t* __restrict__ tris, const float2* __restrict__ pos, const float4* __restrict__ P,
                 MeshFilter f, uint8_t* __restrict__ tri_valid, float4* __restrict__ tri_normal, int* __restrict__ offset,
                 int* __restrict__ n_valid) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  bool valid = false;
  if (t < T) {
    const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    const float4 p0 = P[a], p1 = P[b], p2 = P[c];
    const float id0 = p0.w, id1 = p1.w, id2 = p2.w;
    const Vec3 delta1 = sub3(p1, p0), delta2 = sub3(p2, p0);
    valid = true;
    if (f.do_oblique) {  // obliqueTriangleFilter, flame.cc:2220-2272
      Vec3 normal = cross3(delta1, delta2);  // inward
      normalize3(normal);
      Vec3 ray{((p0.x + p1.x) + p2.x) / 3.0f, ((p0.y + p1.y) + p2.y) / 3.0f, ((p0.z + p1.z) + p2.z) / 3.0f};
      normalize3(ray);
      const float d = dot3(ray, normal);
      // fabs(acos(d)) > oblique_normal_thresh, as a test on d (flame_nltgv2_oblique_cos_bound)
      if (d >= -1.0f && d <= 1.0f && d < f.cos_bound) valid = false;
      float min_id = (id0 < id1) ? id0 : id1;
      min_id = (min_id < id2) ? min_id : id2;
      float max_id = (id0 > id1) ? id0 : id1;
      max_id = (max_id > id2) ? max_id : id2;
      if ((max_id - min_id) / max_id > f.diff_factor) valid = false;
      if (max_id - min_id > f.diff_abs) valid = false;
    }
    if (f.do_edge_length) {  // edgeLengthFilter, flame.cc:2300-2317
      const float2 v0 = pos[a], v1 = pos[b], v2 = pos[c];
      const float d01x = v0.x - v1.x, d01y = v0.y - v1.y;
      const float d02x = v0.x - v2.x, d02y = v0.y - v2.y;
      const float d12x = v1.x - v2.x, d12y = v1.y - v2.y;
      const float dist01 = d01x * d01x + d01y * d01y;
      const float dist02 = d02x * d02x + d02y * d02y;
      const float dist12 = d12x * d12x + d12y * d12y;
      if ((dist01 > f.edge_thresh2) || (dist02 > f.edge_thresh2) || (dist12 > f.edge_thresh2)) valid = false;
    }
    if (f.do_idepth) {  // idepthTriangleFilter, flame.cc:2341-2350
      const float mean_idepth = ((id0 + id1) + id2) / 3.0f;
      if (mean_idepth < f.min_idepth) valid = false;
    }
    tri_valid[t] = valid ? 1 : 0;
    // getVertexNormals, flame.cc:2608-2612: outward, delta2 x delta1
    Vec3 out = cross3(delta2, delta1);
    normalize3(out);
    tri_normal[t] = make_float4(out.x, out.y, out.z, 0.0f);
    if (contributes(id0, id1, id2)) {
      atomicAdd(&offset[a], 1);
      atomicAdd(&offset[b], 1);
      atomicAdd(&offset[c], 1);
    }
  }
  const int n = __popcll(__ballot(valid));
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(n_valid, n);
}

// Exclusive scan of the V + 1 counts in place, one workgroup (block_scan.hpp).
__global__ void __launch_bounds__(kScanThreads)
k_mesh_scan(int n, int* __restrict__ offset, int* __restrict__ cursor) {
  block_exclusive_scan(n, offset, [=](int i, int run) {
    offset[i] = run;
    if (i < n - 1) cursor[i] = run;  // (entry n - 1 is the total: it has no list)
  });
}

__global__ void __launch_bounds__(256)
k_mesh_fill(int T, const int32_t* __restrict__ tris, const float4* __restrict__ P, int* __restrict__ cursor,
            int32_t* __restrict__ incident) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
  if (!contributes(P[a].w, P[b].w, P[c].w)) return;
  incident[atomicAdd(&cursor[a], 1)] = t;
  incident[atomicAdd(&cursor[b], 1)] = t;
  incident[atomicAdd(&cursor[c], 1)] = t;
}

// One lane per vertex: its triangles in ascending index (a triangle that names the vertex twice is in the list twice, as the
// reference updates the vertex twice), then the running mean of flame.cc:2614-2630.  No cap on the length of a list.
__global__ void __launch_bounds__(256)
k_mesh_vertex_normals(int V, const int* __restrict__ offset, int32_t* __restrict__ incident,
                      const float4* __restrict__ tri_normal, float* __restrict__ normals) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const int lo = offset[v], hi = offset[v + 1];
  for (int i = lo + 1; i < hi; ++i) {  // insertion sort: the lists hold ~6 entries
    const int32_t key = incident[i];
    int j = i - 1;
    while (j >= lo && incident[j] > key) {
      incident[j + 1] = incident[j];
      --j;
    }
    incident[j + 1] = key;
  }
  Vec3 n{0.0f, 0.0f, 0.0f};
  int count = 0;
  for (int i = lo; i < hi; ++i) {
    const float4 tn = tri_normal[incident[i]];
    const float c0 = (float)count, c1 = (float)(count + 1);
    n.x = (c0 * n.x + tn.x) / c1;
    n.y = (c0 * n.y + tn.y) / c1;
    n.z = (c0 * n.z + tn.z) / c1;
    normalize3(n);
    ++count;
  }
  normals[3 * v] = n.x, normals[3 * v + 1] = n.y, normals[3 * v + 2] = n.z;
}

}  // namespace

int launch_mesh_outputs(int V, int T, const float2* pos, const float* x, float graph_scale, const int32_t* tris,
                        const MeshFilter& f, const MeshBuffers& b, hipStream_t s) {
  if (V <= 0) return 0;
  hipLaunchKernelGGL(k_mesh_vertices, grid1d(V), dim3(256), 0, s, V, pos, x, graph_scale, f, b.P, b.vtx_idepth, b.offset, b.n_valid);
  if (T > 0) hipLaunchKernelGGL(k_mesh_triangles, grid1d(T), dim3(256), 0, s, T, tris, pos, b.P, f, b.tri_valid, b.tri_normal, b.offset, b.n_valid);
  hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(kScanThreads), 0, s, V + 1, b.offset, b.cursor);
  if (T > 0) hipLaunchKernelGGL(k_mesh_fill, grid1d(T), dim3(256), 0, s, T, tris, b.P, b.cursor, b.incident);
  hipLaunchKernelGGL(k_mesh_vertex_normals, grid1d(V), dim3(256), 0, s, V, b.offset, b.incident, b.tri_normal, b.normals);
  return (int)hipGetLastError();
}

}  // namespace flame_hip
