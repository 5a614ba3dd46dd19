// volume_mesh_kernels.hip -- the surface of the truncated-signed-distance volume as a triangle mesh (include/flame_nltgv2.h,
// flame_nltgv2_volume_mesh_begin): marching tetrahedra over Kuhn's six tets of every live cube of a box, vertices on the tet edges.
// One lane per voxel of the box, in the box's linear order with x along the lanes, 256 voxels per workgroup, four passes:
//   classify   the voxel's record and, where the cube with its lower corner here lies in the box, the seven other corners' weights ->
//              cls: bit 0 inside (tsdf <= 0), bit 1 the cube is live.  The only pass that reads the whole box of the volume: 8 bytes read
//              (the neighbours' lines are the next rows', met again in cache) and 1 byte written per voxel.
//   count      14 neighbours' cls bytes -> the 7-bit mask of the owned edges that carry a vertex (a sign change along the edge and a live
//              cube of the box around it), the cube's triangles (the six tet masks through the generated table); an exclusive scan of
//              both over the workgroup -> emask, vloc, tloc per voxel (1 + 2 + 2 bytes), the workgroup's totals; the cube counters.
//   scan       two workgroups side by side, one for the vertices and one for the triangles: block_exclusive_scan over the workgroups'
//              totals (up to 2^18), in place; the two counts -> MeshTotals.
//   emit       leaves at once if a count passes its capacity.  A voxel's vertices lie at block_v + vloc + rank within the mask: ascending key
//              order; they are written one lane per VERTEX of the workgroup's voxels (the owner found by a search over the 256 prefixes
//              in LDS), so that no lane walks seven edges while its neighbours idle; a live cube writes its triangles at block_t + tloc in the order tet, triangle, each corner the
//              place of its edge's vertex, looked up at the owner.  Every element is placed by rank: no counter is raced for, no
//              floating-point atomics, the same call gives the same bytes.
// Scratch between the passes: 6 bytes per voxel of the box (cls, emask, vloc, tloc) and 8 per workgroup.
// The arithmetic is scalar float code (built with -ffp-contract=off: no FMA; correctly rounded division and square root), so that the
// outputs equal the numpy restatement (tests/volume_mesh_ref.py) bit for bit.  The volume is read only.
#include <hip/hip_runtime.h>

#include "block_scan.hpp"
#include "volume_mesh_kernels.h"
#include "volume_mesh_table.h"

namespace flame_hip {
namespace {

__constant__ uint8_t kTetCorners[6][4] = {FLAME_VOLUME_MESH_TET_CORNERS};
__constant__ uint8_t kTriCounts[6][16] = {FLAME_VOLUME_MESH_TRI_COUNTS};
__constant__ uint8_t kTriEdges[6][16][6] = {FLAME_VOLUME_MESH_TRI_EDGES};

// E[e] as the corner code dx | dy << 1 | dz << 2.
__device__ __forceinline__ uint32_t edge_offset_code(int e) { return e < 3 ? (1u << e) : e == 3 ? 3u : e == 4 ? 5u : e == 5 ? 6u : 7u; }

// A voxel of the box: its index in the box, its place per axis, and whether the cube above it lies in the box.
struct BoxVoxel {
  uint32_t b, bi, bj, bk;
  bool in_box;
};
__device__ __forceinline__ BoxVoxel box_voxel(const MeshBox& box, uint32_t n_box) {
  BoxVoxel v;
  v.b = blockIdx.x * (uint32_t)kMeshBlock + threadIdx.x;  // (n_box <= 2^26)
  v.in_box = v.b < n_box;
  const uint32_t b = v.in_box ? v.b : 0u;
  const uint32_t row = b / (uint32_t)box.n[0];
  v.bi = b - row * (uint32_t)box.n[0];
  v.bk = row / (uint32_t)box.n[1];
  v.bj = row - v.bk * (uint32_t)box.n[1];
  return v;
}
// Its linear index in the volume (< 2^28).
__device__ __forceinline__ uint32_t volume_index(const VolumeGrid& g, const MeshBox& box, const BoxVoxel& v) {
  return (((uint32_t)box.lo[2] + v.bk) * (uint32_t)g.ny + ((uint32_t)box.lo[1] + v.bj)) * (uint32_t)g.nx + ((uint32_t)box.lo[0] + v.bi);
}

__device__ __forceinline__ int wave_count(bool flag) { return __popcll(__ballot(flag)); }

__global__ void __launch_bounds__(kMeshBlock)
k_mesh_classify(const VolumeGrid g, const MeshBox box, uint32_t n_box, const Voxel* __restrict__ vol, uint8_t* __restrict__ cls) {
  const BoxVoxel v = box_voxel(box, n_box);
  if (!v.in_box) return;
  const uint32_t sy = (uint32_t)g.nx, sz = (uint32_t)g.nx * (uint32_t)g.ny;
  const Voxel* p = vol + volume_index(g, box, v);
  const Voxel own = p[0];
  const bool inside = own.tsdf <= 0.0f;  // (a NaN is outside, -0 inside)
  bool live = v.bi + 1 < (uint32_t)box.n[0] && v.bj + 1 < (uint32_t)box.n[1] && v.bk + 1 < (uint32_t)box.n[2] && own.weight > 0.0f;
  if (live)
    live = p[1].weight > 0.0f && p[sy].weight > 0.0f && p[sy + 1].weight > 0.0f && p[sz].weight > 0.0f && p[sz + 1].weight > 0.0f &&
           p[sz + sy].weight > 0.0f && p[sz + sy + 1].weight > 0.0f;
  cls[v.b] = (uint8_t)((inside ? 1 : 0) | (live ? 2 : 0));
}

__global__ void __launch_bounds__(kMeshBlock)
k_mesh_count(const MeshBox box, uint32_t n_box, const uint8_t* __restrict__ cls, uint8_t* __restrict__ emask, uint16_t* __restrict__ vloc,
             uint16_t* __restrict__ tloc, int* __restrict__ block_v, int* __restrict__ block_t, int* __restrict__ counts) {
  __shared__ uint32_t s_wave[kMeshBlock / 64];
  __shared__ int s_cnt[kMeshCubeCounters];
  if (threadIdx.x < kMeshCubeCounters) s_cnt[threadIdx.x] = 0;
  const BoxVoxel v = box_voxel(box, n_box);
  const uint32_t bx = (uint32_t)box.n[0], by = (uint32_t)box.n[1], bz = (uint32_t)box.n[2];
  const uint32_t sy = bx, sz = bx * by;
  uint32_t em = 0, ntri = 0;
  bool live = false;
  if (v.in_box) {
    const uint32_t own = cls[v.b];
    const bool has[3] = {v.bi + 1 < bx, v.bj + 1 < by, v.bk + 1 < bz};   // the neighbour above lies in the box
    const bool low[3] = {v.bi > 0, v.bj > 0, v.bk > 0};                   // ... the one below
    // the inside bits of the cube's corners (bit = corner code); a corner outside the box reads as this voxel's: no sign change
    uint32_t corners = 0;
#pragma unroll
    for (uint32_t c = 0; c < 8; ++c) {
      const bool there = (!(c & 1) || has[0]) && (!(c & 2) || has[1]) && (!(c & 4) || has[2]);
      const uint32_t at = v.b + (c & 1) + ((c >> 1) & 1) * sy + ((c >> 2) & 1) * sz;
      const uint32_t in = there ? (cls[at] & 1u) : (own & 1u);
      corners |= in << c;
    }
    // the live bits of the cubes below: bit d = the cube with its lower corner at this voxel - d (d a corner code; never 7)
    uint32_t lives = 0;
#pragma unroll
    for (uint32_t d = 0; d < 7; ++d) {
      const bool there = (!(d & 1) || low[0]) && (!(d & 2) || low[1]) && (!(d & 4) || low[2]);
      const uint32_t at = v.b - (d & 1) - ((d >> 1) & 1) * sy - ((d >> 2) & 1) * sz;
      const uint32_t l = there ? ((cls[at] >> 1) & 1u) : 0u;
      lives |= l << d;
    }
    live = (own & 2u) != 0;
    // the cubes around edge e, as a mask over `lives`: an axis edge has four, a face diagonal two, the body diagonal one
    const uint32_t cubes_of[7] = {
        (1u << 0) | (1u << 2) | (1u << 4) | (1u << 6),  // (1,0,0): this voxel - (0, dj, dk)
        (1u << 0) | (1u << 1) | (1u << 4) | (1u << 5),  // (0,1,0): - (di, 0, dk)
        (1u << 0) | (1u << 1) | (1u << 2) | (1u << 3),  // (0,0,1): - (di, dj, 0)
        (1u << 0) | (1u << 4),                          // (1,1,0): - (0, 0, dk)
        (1u << 0) | (1u << 2),                          // (1,0,1): - (0, dj, 0)
        (1u << 0) | (1u << 1),                          // (0,1,1): - (di, 0, 0)
        (1u << 0)};                                     // (1,1,1)
    const uint32_t in0 = corners & 1u;
#pragma unroll
    for (int e = 0; e < 7; ++e) {
      const uint32_t far = (corners >> edge_offset_code(e)) & 1u;  // (outside the box: in0, no change)
      if (far != in0 && (lives & cubes_of[e])) em |= 1u << e;
    }
    if (live) {
#pragma unroll
      for (int p = 0; p < 6; ++p) {
        uint32_t mask = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) mask |= ((corners >> kTetCorners[p][c]) & 1u) << c;
        ntri += kTriCounts[p][mask];
      }
    }
  }
  // exclusive scan over the workgroup of (triangles << 16 | vertices): at most 255 * 7 and 255 * 12 before a voxel
  const uint32_t mine = (ntri << 16) | (uint32_t)__popc(em);
  // (within a wave by shuffles, the four waves' totals through LDS)
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t incl = mine;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t below = __shfl_up(incl, d, 64);
    if (lane >= (uint32_t)d) incl += below;
  }
  if (lane == 63u) s_wave[wave] = incl;
  __syncthreads();
  for (uint32_t w = 0; w < wave; ++w) incl += s_wave[w];
  const uint32_t excl = incl - mine;
  if (v.in_box) {
    emask[v.b] = (uint8_t)em;
    vloc[v.b] = (uint16_t)(excl & 0xffffu);
    tloc[v.b] = (uint16_t)(excl >> 16);
  }
  if (threadIdx.x == kMeshBlock - 1) {
    block_v[blockIdx.x] = (int)(incl & 0xffffu);
    block_t[blockIdx.x] = (int)(incl >> 16);
  }
  const int cnt[kMeshCubeCounters] = {wave_count(live), wave_count(ntri > 0)};
  if ((threadIdx.x & 63) == 0)
    for (int c = 0; c < kMeshCubeCounters; ++c)
      if (cnt[c]) atomicAdd(&s_cnt[c], cnt[c]);
  __syncthreads();
  if (threadIdx.x < kMeshCubeCounters && s_cnt[threadIdx.x])
    atomicAdd(&counts[(blockIdx.x % kVolumeCountSlots) * kVolumeCountSlotWords + threadIdx.x], s_cnt[threadIdx.x]);
}

// Two workgroups: 0 scans the vertices' totals, 1 the triangles', side by side.
__global__ void __launch_bounds__(kScanThreads)
k_mesh_scan(int n_blocks, int* block_v, int* block_t, MeshTotals* totals) {
  int* data = blockIdx.x == 0 ? block_v : block_t;
  const int sum = block_exclusive_scan(n_blocks, data, [&](int i, int run) { data[i] = run; });
  if (threadIdx.x == 0) {
    if (blockIdx.x == 0) totals->n_vertices = sum, totals->reserved[0] = 0;
    else totals->n_triangles = sum, totals->reserved[1] = 0;
  }
}

// The gradient along one axis at a voxel of the volume: over the neighbours inside the volume with weight > 0.
__device__ __forceinline__ float grad_axis(const Voxel* __restrict__ p, uint32_t idx, uint32_t n_axis, uint32_t stride, float f0) {
  bool hp = idx + 1 < n_axis, hm = idx > 0;
  float fp = 0.0f, fm = 0.0f;
  if (hp) {
    const Voxel q = p[stride];
    hp = q.weight > 0.0f, fp = q.tsdf;
  }
  if (hm) {
    const Voxel q = *(p - stride);
    hm = q.weight > 0.0f, fm = q.tsdf;
  }
  return hp && hm ? (fp - fm) * 0.5f : hp ? fp - f0 : hm ? f0 - fm : 0.0f;
}

__global__ void __launch_bounds__(kMeshBlock)
k_mesh_emit(const VolumeGrid g, const MeshBox box, uint32_t n_box, const Voxel* __restrict__ vol, const uint8_t* __restrict__ cls,
            const uint8_t* __restrict__ emask, const uint16_t* __restrict__ vloc, const uint16_t* __restrict__ tloc,
            const int* __restrict__ block_v, const int* __restrict__ block_t, const MeshTotals* __restrict__ totals, int max_vertices,
            int max_triangles, float* __restrict__ vertices, float* __restrict__ normals, int32_t* __restrict__ triangles) {
  if (totals->n_vertices > max_vertices || totals->n_triangles > max_triangles) return;  // (uniform: nothing is written unless both counts fit)
  // The vertices, one lane per VERTEX of the workgroup's voxels: the voxel that owns local vertex lv is the last one whose prefix is
  // <= lv (a search over the 256 prefixes in LDS), its edge the (lv - prefix)-th set bit of the voxel's mask.
  __shared__ uint16_t s_vloc[kMeshBlock];
  __shared__ uint8_t s_em[kMeshBlock];
  __shared__ uint32_t s_nv;
  const BoxVoxel v = box_voxel(box, n_box);
  const uint32_t sy = (uint32_t)g.nx, sz = (uint32_t)g.nx * (uint32_t)g.ny;
  const uint32_t bsy = (uint32_t)box.n[0], bsz = (uint32_t)box.n[0] * (uint32_t)box.n[1];
  {
    const uint32_t em = v.in_box ? (uint32_t)emask[v.b] : 0u;
    const uint32_t pre = v.in_box ? (uint32_t)vloc[v.b] : 0xffffu;  // (past the box: above every lv, so the search never lands there)
    s_em[threadIdx.x] = (uint8_t)em, s_vloc[threadIdx.x] = (uint16_t)pre;
    if (v.in_box && (threadIdx.x == kMeshBlock - 1 || v.b + 1 == n_box)) s_nv = pre + (uint32_t)__popc(em);
  }
  __syncthreads();
  const uint32_t first = blockIdx.x * (uint32_t)kMeshBlock;
  const size_t vbase = (size_t)block_v[blockIdx.x];
  const uint32_t n_axis[3] = {(uint32_t)g.nx, (uint32_t)g.ny, (uint32_t)g.nz};
  const uint32_t stride[3] = {1u, sy, sz};
  for (uint32_t lv = threadIdx.x; lv < s_nv; lv += kMeshBlock) {  // (s_nv <= 7 * 256)
    uint32_t at_voxel = 0;
#pragma unroll
    for (uint32_t step = kMeshBlock / 2; step > 0; step >>= 1)
      if ((uint32_t)s_vloc[at_voxel + step] <= lv) at_voxel += step;
    uint32_t m = s_em[at_voxel];
    for (uint32_t r = lv - s_vloc[at_voxel]; r > 0; --r) m &= m - 1u;  // drop the r lowest set bits
    const int e = __ffs((int)m) - 1;
    const uint32_t b = first + at_voxel, row = b / bsy, bk = row / (uint32_t)box.n[1];
    const uint32_t idx[3] = {(uint32_t)box.lo[0] + (b - row * bsy), (uint32_t)box.lo[1] + (row - bk * (uint32_t)box.n[1]), (uint32_t)box.lo[2] + bk};
    const Voxel* p0 = vol + ((idx[2] * (uint32_t)g.ny + idx[1]) * (uint32_t)g.nx + idx[0]);
    const uint32_t oc = edge_offset_code(e);
    const uint32_t d[3] = {oc & 1u, (oc >> 1) & 1u, (oc >> 2) & 1u};
    const Voxel* p1 = p0 + (d[0] + d[1] * sy + d[2] * sz);
    const float f0 = p0->tsdf, f1 = p1->tsdf;
    const float t = f0 / (f0 - f1);
    const size_t at = 3 * (vbase + lv);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int at0 = g.base[a] + (int)idx[a];  // the global index: integration rule 1
      const float pos0 = g.origin[a] + (float)at0 * g.voxel_size;
      const float pos1 = g.origin[a] + (float)(at0 + (int)d[a]) * g.voxel_size;
      vertices[at + a] = pos0 + t * (pos1 - pos0);
    }
    if (normals) {
      float n[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float g0 = grad_axis(p0, idx[a], n_axis[a], stride[a], f0);
        const float g1 = grad_axis(p1, idx[a] + d[a], n_axis[a], stride[a], f1);
        n[a] = g0 + t * (g1 - g0);
      }
      const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
      const bool ok = len > 0.0f;
#pragma unroll
      for (int a = 0; a < 3; ++a) normals[at + a] = ok ? n[a] / len : 0.0f;
    }
  }
  if (!v.in_box) return;
  if (!(cls[v.b] & 2u)) return;
  // a live cube: all eight corners lie in the box
  uint32_t corners = 0;
#pragma unroll
  for (uint32_t c = 0; c < 8; ++c) corners |= (uint32_t)(cls[v.b + (c & 1) + ((c >> 1) & 1) * bsy + ((c >> 2) & 1) * bsz] & 1u) << c;
  if (corners == 0u || corners == 0xffu) return;
  size_t tat = 3 * ((size_t)block_t[blockIdx.x] + tloc[v.b]);
  for (int p = 0; p < 6; ++p) {
    uint32_t mask = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) mask |= ((corners >> kTetCorners[p][c]) & 1u) << c;
    const int n = kTriCounts[p][mask];
    for (int k = 0; k < 3 * n; ++k) {
      const uint32_t code = kTriEdges[p][mask][k];
      const uint32_t oc = code >> 3, e = code & 7u;
      const uint32_t ob = v.b + (oc & 1u) + ((oc >> 1) & 1u) * bsy + ((oc >> 2) & 1u) * bsz;  // the edge's owner: a corner of this cube
      const int rank = block_v[ob / (uint32_t)kMeshBlock] + (int)vloc[ob] + __popc((uint32_t)emask[ob] & ((1u << e) - 1u));
      triangles[tat + k] = rank;
    }
    tat += 3 * (size_t)n;
  }
}

}  // namespace

int launch_volume_mesh(const VolumeGrid& g, const MeshBox& box, const Voxel* vol, const MeshScratch& sc, int* counts, MeshTotals* totals,
                       int max_vertices, int max_triangles, const MeshOut& out, hipEvent_t* pass_ev, hipStream_t s) {
  const long n_box = (long)box.n[0] * box.n[1] * box.n[2];
  const long blocks = mesh_blocks(n_box);
  const dim3 grid((unsigned)blocks), block(kMeshBlock);
  (void)hipMemsetAsync(counts, 0, kVolumeCountsBytes, s);
  hipLaunchKernelGGL(k_mesh_classify, grid, block, 0, s, g, box, (uint32_t)n_box, vol, sc.cls);
  if (pass_ev) (void)hipEventRecord(pass_ev[0], s);
  hipLaunchKernelGGL(k_mesh_count, grid, block, 0, s, box, (uint32_t)n_box, sc.cls, sc.emask, sc.vloc, sc.tloc, sc.block_v, sc.block_t, counts);
  if (pass_ev) (void)hipEventRecord(pass_ev[1], s);
  hipLaunchKernelGGL(k_mesh_scan, dim3(2), dim3(kScanThreads), 0, s, (int)blocks, sc.block_v, sc.block_t, totals);
  if (pass_ev) (void)hipEventRecord(pass_ev[2], s);
  hipLaunchKernelGGL(k_mesh_emit, grid, block, 0, s, g, box, (uint32_t)n_box, vol, sc.cls, sc.emask, sc.vloc, sc.tloc, sc.block_v, sc.block_t,
                     totals, max_vertices, max_triangles, out.vertices, out.normals, out.triangles);
  return (int)hipGetLastError();
}

}  // namespace flame_hip
