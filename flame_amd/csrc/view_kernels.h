// view_kernels.h -- launch wrappers of view_kernels.hip: the mesh rendered into another camera -- every vertex lifted to 3-D, moved and
// projected to 1/16 pixel, every front-facing triangle rasterised with exact integer edge functions, the nearest surface kept per
// pixel (include/flame_nltgv2.h, flame_nltgv2_render_view_begin, states every rule).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace flame_hip {

constexpr float kViewCoordBound = 1048576.0f;  // |16 * pixel coordinate| of a usable vertex: the edge functions stay below 2^44
constexpr int kViewResolveTile = 2048;         // pixels per workgroup of the resolve: 256 threads, 8 pixels each
constexpr int kViewWavePixels = 2048;          // the largest pixel bounding box one wavefront walks alone (32 rounds of its 64 lanes)
constexpr int kViewBigWaves = 64;              // wavefronts that share a larger box ...
constexpr int kViewBigRows = 128;              // ... and how many such triangles are in work at a time

// A vertex in the target view (rule 1): its position there and in the source view in 1/16 pixel, its inverse depth there.
struct ViewVertex {
  int32_t X, Y, Xs, Ys;
  float idepth;
  int32_t usable;
};

// == flame_nltgv2_view_counts, as the kernels leave it on the device.
struct ViewCounts {
  int32_t coverage, tris_drawn, tris_culled_vertex, tris_culled_facing;
};

struct ViewCamera {
  float Kinv_src[9], K_dst[9], R[9], t[3];
  float near_depth;
};

// A mesh on the device and its camera into the target: the view renderer draws one, the fusion (fuse_kernels.h) a table of them, where
// weight is the vote's and v0, t0 the prefix sums of V and T over the sources before this one.  The view renderer leaves the three 0.
struct FuseSource {
  ViewCamera cam;
  const float2* pos;
  const float* values;       // the inverse depth of vertex v: values[v] * value_scale
  const int32_t* tris;
  const uint8_t* tri_valid;  // NULL: every triangle is valid
  float value_scale, weight;
  int32_t v0, t0;
};

// keys[0 .. n) = 0, *counts = 0 and big[0] = 0.  big: [2 + 2 * T] ints of scratch, the list of the triangles with large boxes.
int launch_view_clear(long n, unsigned long long* keys, ViewCounts* counts, int* big, hipStream_t s);
// out[v] for the V vertices of the mesh: one lane per vertex.  The only reader of pos / values.
int launch_view_vertices(const FuseSource& mesh, int V, ViewVertex* out, hipStream_t s);
// Rule 2 per triangle of the mesh into counts (one atomic per workgroup and counter), then rules 3 - 5 into keys of rows x cols: one
// wavefront per triangle, kViewBigWaves of them where its clipped box holds more than kViewWavePixels pixels (big: as launch_view_clear left it).
int launch_view_raster(const FuseSource& mesh, int T, const ViewVertex* vtx, unsigned long long* keys, ViewCounts* counts, int* big, int rows,
                       int cols, hipStream_t s);
// Rule 6: map / tri_index (each may be NULL) from keys, the coverage into counts with one atomic per workgroup.
int launch_view_resolve(long n, const unsigned long long* keys, float* map, int32_t* tri_index, ViewCounts* counts, hipStream_t s);

}  // namespace flame_hip
