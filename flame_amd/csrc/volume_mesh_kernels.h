// volume_mesh_kernels.h -- launch wrapper of volume_mesh_kernels.hip: the surface of the truncated-signed-distance volume as a triangle
// mesh (include/flame_nltgv2.h, flame_nltgv2_volume_mesh_begin): marching tetrahedra over a box of voxels, count / scan / emit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "volume_kernels.h"

namespace flame_hip {

constexpr int kMeshBlock = kVolumeBlock;  // voxels of the box per workgroup, in the box's linear order with x fastest
constexpr int kMeshPasses = 4;            // classify, count, scan, emit

// The box of a call: voxels lo[a] .. lo[a] + n[a] - 1 of the volume per axis; at most 2^26 of them.
struct MeshBox {
  int lo[3], n[3];
};

// What the scan leaves on the device and what travels to the host first: flame_nltgv2_volume_mesh_counts' n_vertices and n_triangles;
// overflow is either of them above its capacity, to the emit pass and to the host alike (the cube counters come through the partial
// sets of volume_kernels.h: word 0 live_cubes, word 1 surface_cubes).
struct MeshTotals {
  int n_vertices, n_triangles, reserved[2];
};
constexpr int kMeshCubeCounters = 2;

// What the passes keep between them, per voxel of the box (6 bytes) and per workgroup (8 bytes).
struct MeshScratch {
  uint8_t* cls;     // bit 0: the voxel is inside; bit 1: the cube with its lower corner here lies in the box and is live
  uint8_t* emask;   // bit e: the edge to the voxel at E[e] carries a vertex
  uint16_t* vloc;   // the vertices owned by the voxels before this one in its workgroup
  uint16_t* tloc;   // the triangles of the cubes before this one in its workgroup
  int* block_v;     // per workgroup: its vertices, then (after the scan) the vertices before it
  int* block_t;     // ... its triangles
};
inline size_t mesh_scratch_voxel_bytes() { return 6; }
inline long mesh_blocks(long box_voxels) { return (box_voxels + kMeshBlock - 1) / kMeshBlock; }

struct MeshOut {
  float* vertices;   // 3 per vertex; room for min(max_vertices, 7 * box voxels)
  float* normals;    // the same, or NULL
  int32_t* triangles;  // 3 per triangle; room for min(max_triangles, 12 * box voxels)
};

// The four passes on `s`.  counts: kVolumeCountsBytes, cleared first; totals: written by the scan; the arrays are written only if
// n_vertices <= max_vertices and n_triangles <= max_triangles.  pass_ev: kMeshPasses - 1 events recorded between the passes (or NULL).
int launch_volume_mesh(const VolumeGrid& g, const MeshBox& box, const Voxel* vol, const MeshScratch& sc, int* counts, MeshTotals* totals,
                       int max_vertices, int max_triangles, const MeshOut& out, hipEvent_t* pass_ev, hipStream_t s);

}  // namespace flame_hip
