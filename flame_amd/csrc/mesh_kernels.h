// mesh_kernels.h -- launch wrapper of mesh_kernels.hip: the mesh outputs of Flame::update() (flame.cc:372-407) from the
// canonical device state -- vertex inverse depths, triangle filters, vertex normals (include/flame_nltgv2.h,
// flame_nltgv2_mesh_outputs_begin).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace flame_hip {

// What the kernels compare against, prepared once per call on the host.
struct MeshFilter {
  float Kinv[9];        // row-major
  int do_oblique, do_edge_length, do_idepth;
  float cos_bound;      // flame_nltgv2_oblique_cos_bound(oblique_normal_thresh): reject iff d in [-1, 1] and d < cos_bound
  float diff_factor, diff_abs;
  float edge_thresh2;   // (edge_length_thresh * cols)^2, in float (flame.cc:2297-2298)
  float min_idepth;
};

// Scratch and outputs, all device memory.
struct MeshBuffers {
  float4* P;            // [V] back-projected vertex (x, y, z) and its idepth in w
  float* vtx_idepth;    // [V] out
  float* normals;       // [3V] out
  uint8_t* tri_valid;   // [T] out (+ what the filtered rasteriser reads)
  int* n_valid;         // [1] out
  float4* tri_normal;   // [T] outward unit normal of a triangle
  int* offset;          // [V + 1] incidence counts, then their exclusive scan
  int* cursor;          // [V] fill positions
  int32_t* incident;    // [3T] per vertex: its contributing triangles (ascending after the vertex pass ordered them)
};

// k_mesh_vertices -> k_mesh_triangles -> k_mesh_scan -> k_mesh_fill -> k_mesh_vertex_normals on `s`, nothing in between.
int launch_mesh_outputs(int V, int T, const float2* pos, const float* x, float graph_scale, const int32_t* tris,
                        const MeshFilter& f, const MeshBuffers& b, hipStream_t s);

}  // namespace flame_hip
