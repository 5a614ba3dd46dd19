// fuse_kernels.h -- launch wrappers of fuse_kernels.hip: the kept-mesh snapshot, and up to kFuseSources meshes rendered into one target
// camera in one batch of launches (rules 1 - 5 of the view renderer per source, view_device.hpp) with the per-pixel vote behind them
// (include/flame_nltgv2.h, flame_nltgv2_fuse_views_begin, states every rule; tests/fuse_ref.py is the checker).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "view_kernels.h"

namespace flame_hip {

constexpr int kFuseSources = 8;

// == flame_nltgv2_fuse_counts, as the kernels leave it on the device: 32 words.
struct FuseCounts {
  int32_t coverage, support_hist[kFuseSources + 1], present[kFuseSources], inlier[kFuseSources], tris_drawn, reserved[5];
};
constexpr int kFuseCountWords = 32;
static_assert(sizeof(FuseCounts) == kFuseCountWords * sizeof(int32_t), "the counters are 32 words");

// The sources of a batch (FuseSource: view_kernels.h).  The table travels by value in the kernel arguments (under 2 KB).  v_end /
// t_end: the sums of V and T over all sources.
struct FuseTable {
  FuseSource s[kFuseSources];
  int32_t n, v_end, t_end;
};
static_assert(sizeof(FuseTable) < 2048, "the source table must fit the kernel arguments comfortably");

// What the vote writes (each may be NULL) and its two parameters.
struct FuseOutputs {
  float* fused;
  uint8_t* present_mask;
  uint8_t* inlier_mask;
  float* spread;
  float* layers;  // n_sources * n floats
};

// pos_out[v] = pos[v], id_out[v] = x[v] * scale (one float32 multiply) for the V vertices: the snapshot of flame_nltgv2_keep_mesh.  The
// only reader of pos / x.
int launch_keep_vertices(int V, const float2* pos, const float* x, float scale, float2* pos_out, float* id_out, hipStream_t s);
// keys[0 .. n_sources * n) = 0, *counts = 0, big[0] = 0.  big: [2 + 2 * t_end] ints, the list of (source, triangle) with large boxes.
int launch_fuse_clear(long n_keys, unsigned long long* keys, FuseCounts* counts, int* big, hipStream_t s);
// Rule 1 for every vertex of every source in one launch: vtx[tab.s[k].v0 + v].  The only reader of the sources' pos / values.
int launch_fuse_vertices(const FuseTable& tab, ViewVertex* vtx, hipStream_t s);
// Rules 2 - 5 for every triangle of every source: one count launch, one raster launch, one launch for the listed large boxes.  Layer k
// writes keys[k * rows * cols ..]; tris_drawn sums over the sources.
int launch_fuse_raster(const FuseTable& tab, const ViewVertex* vtx, unsigned long long* keys, FuseCounts* counts, int* big, int rows, int cols,
                       hipStream_t s);
// The vote over the n = rows * cols pixels' tab.n keys, the outputs asked for, and the counters (one atomic per workgroup and non-zero
// counter).
int launch_fuse_vote(const FuseTable& tab, long n, const unsigned long long* keys, float rel_tol, int min_support, const FuseOutputs& out,
                     FuseCounts* counts, hipStream_t s);

}  // namespace flame_hip
