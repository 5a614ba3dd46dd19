// flame_hip/nltgv2_l1_graph_regularizer.hpp -- C++11 facade over the C-ABI (flame_nltgv2.h) that
// keeps the reference's call surface:
//
//   reference  /root/reference/src/flame/optimizers/nltgv2_l1_graph_regularizer.h
//     namespace flame::optimizers::nltgv2_l1_graph_regularizer
//       struct Params                                   h:121-129
//       void  step(const Params&, Graph*)               h:134
//       float smoothnessCost / dataCost / cost          h:139-151
//       internal::dualStep / primalStep / extraGradientStep   h:158-168
//
//   here       namespace flame::optimizers::nltgv2_l1_graph_regularizer::hip  -- same names, same
//              argument meaning, same Params fields and defaults.  A maintainer switches a call site
//              by adding `::hip` (or a namespace alias).
//
// Host side stays ordinary C++: the facade is header-only, needs no HIP headers and works with any
// graph container for which flame_hip::GraphAccess<Graph> is specialised:
//   * flame_hip/bgl_adaptor.hpp      the reference's boost::adjacency_list Graph (needs Boost)
//   * flame_hip::FlatGraph (below)   a dependency-free container with the reference's field names
//
// Errors: the reference aborts the process (FLAME_ASSERT -> exit(1), assert.h:111); the facade throws
// flame_hip::Error carrying the C-ABI status instead.  Nothing is ever computed on the CPU here.
#ifndef FLAME_HIP_NLTGV2_L1_GRAPH_REGULARIZER_HPP_
#define FLAME_HIP_NLTGV2_L1_GRAPH_REGULARIZER_HPP_

#include <cstdint>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "flame_nltgv2.h"

namespace flame_hip {

struct Error : std::runtime_error {
  int status;
  Error(int s, const std::string& what)
      : std::runtime_error(what + ": " + flame_nltgv2_status_string(s)), status(s) {}
};

// Flat image of a Graph in boost::vertices()/boost::edges() order; what upload/download move.
struct FlatArrays {
  std::vector<float> pos, x, w1, w2, x_bar, w1_bar, w2_bar, x_prev, w1_prev, w2_prev, data_term, data_weight;
  std::vector<int32_t> src, dst;
  std::vector<float> alpha, beta, q1, q2, q3;
  void resize(size_t V, size_t E) {
    pos.resize(2 * V);
    for (auto* a : {&x, &w1, &w2, &x_bar, &w1_bar, &w2_bar, &x_prev, &w1_prev, &w2_prev, &data_term, &data_weight})
      a->resize(V);
    src.resize(E), dst.resize(E);
    for (auto* a : {&alpha, &beta, &q1, &q2, &q3}) a->resize(E);
  }
  flame_nltgv2_graph view() {
    flame_nltgv2_graph g;
    g.V = static_cast<int32_t>(x.size()), g.E = static_cast<int32_t>(src.size());
    g.pos = pos.data();
    g.x = x.data(), g.w1 = w1.data(), g.w2 = w2.data();
    g.x_bar = x_bar.data(), g.w1_bar = w1_bar.data(), g.w2_bar = w2_bar.data();
    g.x_prev = x_prev.data(), g.w1_prev = w1_prev.data(), g.w2_prev = w2_prev.data();
    g.data_term = data_term.data(), g.data_weight = data_weight.data();
    g.src = src.data(), g.dst = dst.data();
    g.alpha = alpha.data(), g.beta = beta.data();
    g.q1 = q1.data(), g.q2 = q2.data(), g.q3 = q3.data();
    return g;
  }
};

// Specialise for a graph container:
//   static void pack(const Graph&, FlatArrays*)      vertices()/edges() order; (src,dst) = (source,target)
//   static void unpack(const FlatArrays&, Graph*)    writes x,w,x_bar,w_bar,x_prev,w_prev,q back
//   static void size(const Graph&, size_t* V, size_t* E)
//   static uint64_t identity(const Graph&)           a hash of WHICH objects stand at which position of vertices()/edges()
//                                                    (0 where positions are stable by construction): download() refuses a graph
//                                                    whose identity differs from the uploaded one's -- an edit that leaves the
//                                                    counts alone (remove_edge + add_edge) still moves objects to other positions
template <class Graph>
struct GraphAccess;

inline uint64_t mix_identity(uint64_t h, uint64_t v) {  // (splitmix64 step: order-sensitive running hash)
  h += 0x9e3779b97f4a7c15ull + v;
  h = (h ^ (h >> 30)) * 0xbf58476d1ce4e5b9ull;
  h = (h ^ (h >> 27)) * 0x94d049bb133111ebull;
  return h ^ (h >> 31);
}

// Dependency-free graph container with the reference's VertexData/EdgeData field names (h:74-102).
struct VertexData {
  float pos_x = 0.0f, pos_y = 0.0f;  // cv::Point2f pos
  float x = 0.0f, w1 = 0.0f, w2 = 0.0f;
  float x_bar = 0.0f, w1_bar = 0.0f, w2_bar = 0.0f;
  float x_prev = 0.0f, w1_prev = 0.0f, w2_prev = 0.0f;
  float data_term = 0.0f, data_weight = 1.0f;
};
struct EdgeData {
  int32_t source = 0, target = 0;  // boost::source / boost::target
  float alpha = 1.0f, beta = 1.0f;
  float q1 = 0.0f, q2 = 0.0f, q3 = 0.0f;
  bool valid = true;
};
struct FlatGraph {
  std::vector<VertexData> vertices;
  std::vector<EdgeData> edges;
};

template <>
struct GraphAccess<FlatGraph> {
  static void pack(const FlatGraph& g, FlatArrays* f) {
    f->resize(g.vertices.size(), g.edges.size());
    for (size_t v = 0; v < g.vertices.size(); ++v) {
      const VertexData& d = g.vertices[v];
      f->pos[2 * v] = d.pos_x, f->pos[2 * v + 1] = d.pos_y;
      f->x[v] = d.x, f->w1[v] = d.w1, f->w2[v] = d.w2;
      f->x_bar[v] = d.x_bar, f->w1_bar[v] = d.w1_bar, f->w2_bar[v] = d.w2_bar;
      f->x_prev[v] = d.x_prev, f->w1_prev[v] = d.w1_prev, f->w2_prev[v] = d.w2_prev;
      f->data_term[v] = d.data_term, f->data_weight[v] = d.data_weight;
    }
    for (size_t e = 0; e < g.edges.size(); ++e) {
      const EdgeData& d = g.edges[e];
      f->src[e] = d.source, f->dst[e] = d.target;
      f->alpha[e] = d.alpha, f->beta[e] = d.beta;
      f->q1[e] = d.q1, f->q2[e] = d.q2, f->q3[e] = d.q3;
    }
  }
  static void size(const FlatGraph& g, size_t* V, size_t* E) { *V = g.vertices.size(), *E = g.edges.size(); }
  static uint64_t identity(const FlatGraph&) { return 0; }  // (vector positions: stable by construction)
  static void unpack(const FlatArrays& f, FlatGraph* g) {
    for (size_t v = 0; v < g->vertices.size(); ++v) {
      VertexData& d = g->vertices[v];
      d.x = f.x[v], d.w1 = f.w1[v], d.w2 = f.w2[v];
      d.x_bar = f.x_bar[v], d.w1_bar = f.w1_bar[v], d.w2_bar = f.w2_bar[v];
      d.x_prev = f.x_prev[v], d.w1_prev = f.w1_prev[v], d.w2_prev = f.w2_prev[v];
    }
    for (size_t e = 0; e < g->edges.size(); ++e) {
      EdgeData& d = g->edges[e];
      d.q1 = f.q1[e], d.q2 = f.q2[e], d.q3 = f.q3[e];
    }
  }
};

// utils::Delaunay counterpart (src/flame/utils/delaunay.{h,cc}): triangles()/edges() of the Delaunay
// triangulation of `vertices_xy` (x0,y0,x1,y1,...), exact predicates, host code.
inline void delaunayTriangulate(const std::vector<float>& vertices_xy, std::vector<int32_t>* triangles,
                                std::vector<int32_t>* edges) {
  const int32_t n = static_cast<int32_t>(vertices_xy.size() / 2);
  int32_t nt = 0, ne = 0;
  std::vector<int32_t> t(static_cast<size_t>(n > 0 ? 6 * n : 3)), e(static_cast<size_t>(n > 0 ? 6 * n : 2));
  const int rc = flame_delaunay_triangulate(vertices_xy.data(), n, t.data(), static_cast<int32_t>(t.size() / 3), &nt,
                                            e.data(), static_cast<int32_t>(e.size() / 2), &ne);
  if (rc != 0) throw Error(rc, "flame_delaunay_triangulate");
  if (triangles) triangles->assign(t.begin(), t.begin() + 3 * nt);
  if (edges) edges->assign(e.begin(), e.begin() + 2 * ne);
}

}  // namespace flame_hip

namespace flame {
namespace optimizers {
namespace nltgv2_l1_graph_regularizer {
namespace hip {

// == struct Params h:121-129: layout-identical to flame_nltgv2_params, same defaults.
struct Params {
  float data_factor = 0.1f;  // lambda in the TV literature.
  float step_x = 0.001f;     // Primal step size.
  float step_q = 125.0f;     // Dual step size.
  float theta = 0.25f;       // Extra gradient step size.
  float x_min = 0.0f;        // Feasible set.
  float x_max = 10.0f;
};
static_assert(sizeof(Params) == sizeof(flame_nltgv2_params), "Params must mirror the C-ABI struct");

inline flame_nltgv2_params to_c(const Params& p) {
  flame_nltgv2_params c;
  c.data_factor = p.data_factor, c.step_x = p.step_x, c.step_q = p.step_q;
  c.theta = p.theta, c.x_min = p.x_min, c.x_max = p.x_max;
  return c;
}

// == the mesh filter fields of flame::Params (params.h:69-85): layout-identical to flame_nltgv2_mesh_filter_params, same defaults.
struct MeshFilterParams {
  int32_t do_oblique_triangle_filter = 1;
  float oblique_normal_thresh = 1.39626f;       // 80 degrees. Max angle between surface normal and viewing ray.
  float oblique_idepth_diff_factor = 0.35f;     // (max_idepth - min_idepth)/max_idepth
  float oblique_idepth_diff_abs = 0.1f;         // (max_idepth - min_idepth)
  int32_t do_edge_length_filter = 1;
  float edge_length_thresh = 0.333f;            // As fraction of image width.
  int32_t do_idepth_triangle_filter = 1;
  float min_triangle_idepth = 0.01f;
};
static_assert(sizeof(MeshFilterParams) == sizeof(flame_nltgv2_mesh_filter_params), "MeshFilterParams must mirror the C-ABI struct");

// What Flame::update() leaves for its getters (flame.cc:372-407), under the reference's member names.  Pointers into pinned
// memory of the DeviceGraph, valid until its next meshOutputsBegin().
struct MeshOutputs {
  size_t num_vertices = 0, num_triangles = 0;
  const float* vtx_idepths = nullptr;     // [num_vertices]      vtx_idepths_
  const float* vtx_normals = nullptr;     // [3 * num_vertices]  vtx_normals_, (x, y, z) interleaved
  const uint8_t* tri_validity = nullptr;  // [num_triangles]     tri_validity_
  int num_valid_triangles = 0;
  int rows = 0, cols = 0;
  const float* filtered_idepthmap = nullptr;  // [rows * cols] getFilteredInverseDepthMap (flame.h:217-228), or nullptr
  int filtered_coverage = 0;
};

// What the metric outputs read beside the maps (flame_nltgv2_metric_params, same defaults): the depth window in metres (both bounds
// exclusive), which map, which outputs, and whether they travel to the host.  Layout-identical to the C-ABI struct.
struct MetricParams {
  float min_depth = 0.0f;
  float max_depth = std::numeric_limits<float>::infinity();
  int32_t use_filtered_map = 0;  // 0: the resident unfiltered map; 1: the filtered map of meshOutputsBegin(want_filtered_map)
  int32_t want_depth = 1;
  int32_t want_depth_mm = 1;
  int32_t want_organized = 1;
  int32_t want_cloud = 1;
  int32_t want_mesh = 0;         // mesh_vertices + mesh_normals + mesh_triangles (needs a meshOutputsBegin for the resident triangles)
  int32_t copy_out = 1;          // 0: the outputs stay on the device, only the counters travel
  int32_t reserved = 0;
  const void* map_device = nullptr;  // a rows x cols float map in device memory of the caller's, read instead of the resident ones
};
static_assert(sizeof(MetricParams) == sizeof(flame_nltgv2_metric_params), "MetricParams must mirror the C-ABI struct");

// What a consumer reads (flame_nltgv2_metric_outputs_view): depth image in metres, the 16-bit millimetre image, the organised and the
// dense cloud, the posed mesh with the triangles that survived the filters.  Host pointers into pinned memory of the DeviceGraph and,
// beside each, the device pointer of the same array; all valid until its next metricOutputsBegin().  Not asked for: nullptr.
struct MetricOutputs {
  int rows = 0, cols = 0;
  size_t num_vertices = 0, num_triangles = 0;
  size_t num_points = 0;            // points of the dense cloud
  size_t num_valid_triangles = 0;   // triples in mesh_triangles
  const float* depth = nullptr;             const void* depth_device = nullptr;           // [rows * cols], NaN on holes
  const uint16_t* depth_mm = nullptr;       const void* depth_mm_device = nullptr;        // [rows * cols], 0 on holes
  const float* organized = nullptr;         const void* organized_device = nullptr;       // [rows * cols * 3], NaN on holes
  const float* cloud = nullptr;             const void* cloud_device = nullptr;           // [num_points * 3]
  const uint32_t* cloud_pixel = nullptr;    const void* cloud_pixel_device = nullptr;     // [num_points] row * cols + col, ascending
  const float* mesh_vertices = nullptr;     const void* mesh_vertices_device = nullptr;   // [num_vertices * 3]
  const float* mesh_normals = nullptr;      const void* mesh_normals_device = nullptr;    // [num_vertices * 3]
  const int32_t* mesh_triangles = nullptr;  const void* mesh_triangles_device = nullptr;  // [num_valid_triangles * 3]
};

// What the map error reads (flame_nltgv2_map_error_params, constructed with its defaults): the source -- photometric against another
// frame (KRKinv, Kt, border, the two images) or a true inverse-depth map (update()'s idepths_true) --, the box, the histogram's scale
// and rank, the picture, which outputs, and whether they travel to the host.  The C-ABI struct itself: the header states every rule.
struct MapErrorParams : flame_nltgv2_map_error_params {
  MapErrorParams() { flame_nltgv2_default_map_error_params(this); }
};

// What flame.cc:854-984 computed (flame_nltgv2_map_error_view): photo_error_ (the smoothed error image, NaN where undefined), the
// histogram with its median and percentile bins, total_photo_error / avg_photo_error, and the debug_draw_photo_error picture.  Host
// pointers into pinned memory of the DeviceGraph and the device pointers of the same arrays; all valid until its next mapErrorBegin().
struct MapError {
  int rows = 0, cols = 0, source = 0, win_size = 0;
  float hist_scale = 0.0f;
  const flame_nltgv2_map_error_stats* stats = nullptr;  const void* stats_device = nullptr;
  const float* error = nullptr;                         const void* error_device = nullptr;      // [rows * cols]
  const uint8_t* debug_img_photo_error = nullptr;       const void* image_device = nullptr;      // [rows * cols * 3]
};

// The camera the mesh is rendered into and what is wanted of it (flame_nltgv2_view_params, constructed with its defaults): Kinv_src,
// K_dst, R, t with P_dst = R * P_src + t, near_depth, where the triangle validity comes from, which outputs, and whether they travel
// to the host.  The C-ABI struct itself: the header states every rule.
struct ViewParams : flame_nltgv2_view_params {
  ViewParams() { flame_nltgv2_default_view_params(this); }
};

// The mesh seen from another camera (flame_nltgv2_view_outputs_view): the inverse depth of the nearest surface per pixel (NaN on
// holes), the triangle that owns the pixel (-1 on holes) and the counters.  Host pointers into pinned memory of the DeviceGraph and the
// device pointers of the same arrays; all valid until its next renderViewBegin().
struct RenderedView {
  int rows = 0, cols = 0, num_triangles = 0;
  flame_nltgv2_view_counts counts = {0, 0, 0, 0};
  const float* idepthmap = nullptr;    const void* idepthmap_device = nullptr;  // [rows * cols]
  const int32_t* tri_index = nullptr;  const void* tri_index_device = nullptr;  // [rows * cols]
};

// The sources of a fusion, the target camera and the vote (flame_nltgv2_fuse_params, constructed with its defaults): sources[s].slot
// names a kept mesh, or -1 the live one.  The C-ABI struct itself: the header states every rule.
struct FuseParams : flame_nltgv2_fuse_params {
  FuseParams() { flame_nltgv2_default_fuse_params(this); }
};

// Several meshes fused in one view (flame_nltgv2_fuse_outputs_view): the weighted mean of the sources that agree per pixel (NaN where
// too few do), who was present and who agreed (bit s: source s), the spread of the agreeing values, the layers themselves if asked for,
// and the counters.  Host pointers into pinned memory of the DeviceGraph and the device pointers of the same arrays; all valid until
// its next fuseViewsBegin().
struct FusedView {
  int rows = 0, cols = 0, num_sources = 0;
  flame_nltgv2_fuse_counts counts;
  const float* idepthmap = nullptr;       const void* idepthmap_device = nullptr;     // [rows * cols]
  const uint8_t* present_mask = nullptr;  const void* present_mask_device = nullptr;  // [rows * cols]
  const uint8_t* inlier_mask = nullptr;   const void* inlier_mask_device = nullptr;   // [rows * cols]
  const float* spread = nullptr;          const void* spread_device = nullptr;        // [rows * cols]
  const float* layers = nullptr;          const void* layers_device = nullptr;        // [num_sources * rows * cols]
  FusedView() { std::memset(&counts, 0, sizeof(counts)); }
};

// The volumetric map's parameters (flame_nltgv2_volume_params, flame_nltgv2_integrate_params, flame_nltgv2_raycast_params, each
// constructed with its defaults).  The C-ABI structs themselves: the header states every rule.
struct VolumeParams : flame_nltgv2_volume_params {
  VolumeParams() { flame_nltgv2_default_volume_params(this); }
};
struct IntegrateParams : flame_nltgv2_integrate_params {
  IntegrateParams() { flame_nltgv2_default_integrate_params(this); }
};
struct RaycastParams : flame_nltgv2_raycast_params {
  RaycastParams() { flame_nltgv2_default_raycast_params(this); }
};

// What one integration did (flame_nltgv2_integrate_view): the six counters.
struct IntegratedMap {
  int rows = 0, cols = 0;
  flame_nltgv2_integrate_counts counts;
  IntegratedMap() { std::memset(&counts, 0, sizeof(counts)); }
};

// The volume seen from a camera (flame_nltgv2_raycast_view): the inverse depth of the surface per pixel (NaN on holes) and the counters.
// The host pointer into pinned memory of the DeviceGraph (nullptr with copy_out == 0) and the device pointer of the same array; both
// valid until its next volumeRaycastBegin().
struct RaycastView {
  int rows = 0, cols = 0;
  flame_nltgv2_raycast_counts counts = {0, 0, 0, 0};
  const float* idepthmap = nullptr;    const void* idepthmap_device = nullptr;  // [rows * cols]
};

// The surface extraction's parameters (flame_nltgv2_volume_mesh_params with its defaults: the whole volume, capacities 0 -- a count query).
struct VolumeMeshParams : flame_nltgv2_volume_mesh_params {
  VolumeMeshParams() { flame_nltgv2_default_volume_mesh_params(this); }
};

// The volume's surface as a triangle mesh (flame_nltgv2_volume_mesh_view): vertices in the world frame, unit normals into free space,
// triangles counter-clockwise seen from there, and the counters.  Host pointers into pinned memory of the DeviceGraph (nullptr with
// copy_out == 0 and on overflow; the normals also without want_normals) and the device pointers of the same arrays; all valid until its
// next volumeMeshBegin().  On overflow ask again with counts.n_vertices / counts.n_triangles as the capacities.
struct VolumeMesh {
  flame_nltgv2_volume_mesh_counts counts;
  float device_ms = 0.0f;
  const float* vertices = nullptr;     const void* vertices_device = nullptr;   // [3 * counts.n_vertices]
  const float* normals = nullptr;      const void* normals_device = nullptr;    // [3 * counts.n_vertices]
  const int32_t* triangles = nullptr;  const void* triangles_device = nullptr;  // [3 * counts.n_triangles]
  VolumeMesh() { std::memset(&counts, 0, sizeof(counts)); }
};

// The window that follows the camera (flame_nltgv2_volume_shift_begin, flame_nltgv2_volume_follow; the header states every rule).
struct FollowParams : flame_nltgv2_follow_params {
  FollowParams() { flame_nltgv2_default_follow_params(this); }
};
// Where the window should move: the shift, the box that stays and the up to three boxes that leave, in pre-shift local indices, as
// VolumeMeshParams::lo / hi take them.
typedef flame_nltgv2_follow_plan FollowPlan;
// What one shift did (flame_nltgv2_shift_view): the window afterwards, the four counters, and the bytes per access of the kernel's path.
struct ShiftedWindow {
  int32_t shift[3] = {0, 0, 0}, base[3] = {0, 0, 0};
  int record_bytes = 0;
  float device_ms = 0.0f;
  flame_nltgv2_shift_counts counts;
  ShiftedWindow() { std::memset(&counts, 0, sizeof(counts)); }
};

// == the members of flame::Params the debug images read (params.h:109, debug_flip_images, debug_draw_idepthmap, debug_draw_normals):
// layout-identical to flame_nltgv2_debug_image_params, same defaults.  debug_draw_text_overlay is treated as false.
struct DebugImageParams {
  float scene_color_scale = 1.0f;
  int32_t debug_flip_images = 0;
  int32_t debug_draw_idepthmap = 1;
  int32_t debug_draw_normals = 1;
};
static_assert(sizeof(DebugImageParams) == sizeof(flame_nltgv2_debug_image_params), "DebugImageParams must mirror the C-ABI struct");

// What the "Draw stuff" block of Flame::update() (flame.cc:490-511) leaves for getDebugImageInverseDepthMap / getDebugImageNormals
// (flame.h:294-306), under the reference's member names.  Pointers into pinned memory of the DeviceGraph, valid until its next
// debugImagesBegin(); a picture that was not asked for is nullptr.  Pixels are cv::Vec3b: 3 bytes, c[0], c[1], c[2].
struct DebugImages {
  int rows = 0, cols = 0;
  const uint8_t* debug_img_idepthmap = nullptr;  // [rows * cols * 3]
  const uint8_t* debug_img_normals = nullptr;    // [rows * cols * 3]
  const float* w1_map = nullptr;                 // [rows * cols] w1_map_, NaN where uncovered (with the normals only)
  const float* w2_map = nullptr;                 // [rows * cols] w2_map_
};

// == the members of flame::Params drawWireframe reads (params.h:109, debug_flip_images) and where the triangle validity comes from:
// layout-identical to flame_nltgv2_wireframe_params, same defaults.  debug_draw_text_overlay is treated as false.
struct WireframeParams {
  float scene_color_scale = 1.0f;
  int32_t debug_flip_images = 0;
  int32_t validity = 0;  // 0: every triangle valid; 1: tri_validity is a host array; 2: what the last meshOutputsBegin left on the device
};
static_assert(sizeof(WireframeParams) == sizeof(flame_nltgv2_wireframe_params), "WireframeParams must mirror the C-ABI struct");

// What drawWireframe (flame.cc:2414-2457) leaves for getDebugImageWireframe, under the reference's member name.  The pointer goes into
// pinned memory of the DeviceGraph, valid until its next debugWireframeBegin().  Pixels are cv::Vec3b: 3 bytes, c[0], c[1], c[2].
struct Wireframe {
  int rows = 0, cols = 0;
  const uint8_t* debug_img_wireframe = nullptr;  // [rows * cols * 3]
  int lines_drawn = 0, lines_skipped = 0;        // lines of valid triangles: walked / left out (an endpoint outside the image)
  bool refilled = false;                         // the stage's entry buffer had to grow: the second half ran twice
};

// Device image of ONE Graph: what the pipeline keeps next to `Graph graph_` (flame.h:536).  Not
// thread-safe -- hold graph_mtx_ (flame.h:539) around every call exactly as the reference does around
// step() and the graph edits (flame.cc:103, 302, 309, 329, 365).
class DeviceGraph {
 public:
  explicit DeviceGraph(int device = 0) : ctx_(nullptr) {
    const int rc = flame_nltgv2_create(&ctx_, device);
    if (rc != 0) throw flame_hip::Error(rc, "flame_nltgv2_create");
  }
  ~DeviceGraph() { flame_nltgv2_destroy(ctx_); }
  DeviceGraph(const DeviceGraph&) = delete;
  DeviceGraph& operator=(const DeviceGraph&) = delete;

  // After Flame::syncGraph changed vertices / edges / data (flame.cc:1940-2188).
  // `generation`: any caller-side counter of graph edits; download() of another generation is refused.
  template <class Graph>
  void upload(const Graph& graph, uint64_t generation = 0) {
    flame_hip::GraphAccess<Graph>::pack(graph, &flat_);
    flame_nltgv2_graph v = flat_.view();
    check(flame_nltgv2_upload_graph(ctx_, &v), "upload_graph");
    uploaded_v_ = flat_.x.size(), uploaded_e_ = flat_.src.size(), generation_ = generation, uploaded_ = true;
    identity_ = flame_hip::GraphAccess<Graph>::identity(graph);
  }
  // Before Flame::update reads x, w1, w2 (flame.cc:372-380) or edits the graph.  Values go back to the objects they
  // came from BY POSITION in vertices()/edges() order, so the graph must be the one that was uploaded: a graph whose
  // vertex or edge count differs, or (when the caller tracks edits) whose generation differs, is refused
  // (FLAME_NLTGV2_ERR_INVALID_ARG) instead of receiving values that belong to other vertices.
  template <class Graph>
  void download(Graph* graph, uint64_t generation = 0) {
    if (!matches(*graph, generation)) throw flame_hip::Error(FLAME_NLTGV2_ERR_INVALID_ARG, "download: the graph changed since upload()");
    flame_nltgv2_graph v = flat_.view();
    check(flame_nltgv2_download_state(ctx_, &v), "download_state");
    flame_hip::GraphAccess<Graph>::unpack(flat_, graph);
  }
  template <class Graph>
  bool matches(const Graph& graph, uint64_t generation = 0) const {
    size_t V = 0, E = 0;
    flame_hip::GraphAccess<Graph>::size(graph, &V, &E);
    return uploaded_ && V == uploaded_v_ && E == uploaded_e_ && generation == generation_ &&
           flame_hip::GraphAccess<Graph>::identity(graph) == identity_;
  }
  uint64_t generation() const { return generation_; }

  // Per-frame warm-start synchronisation: Flame::syncGraph's graph edits (flame.cc:1985-2121) applied to the
  // device image; see flame_nltgv2_sync_graph.  `edges` = triangulator->edges() as index pairs.
  void sync(const std::vector<int32_t>& feat_id, const std::vector<float>& pos_xy, const std::vector<float>& data_term,
            const std::vector<float>& data_weight, const std::vector<int32_t>& edges, bool check_sticky_obstacles = false,
            const float* init_x = nullptr, float init_graph_scale = 0.0f, bool edges_unique = false) {
    sync(static_cast<int32_t>(feat_id.size()), feat_id.data(), pos_xy.data(), data_term.data(), data_weight.data(), edges,
         check_sticky_obstacles, init_x, init_graph_scale, edges_unique);
  }
  // Pointer + count form: V vertices in arrays that need not be std::vectors -- the arrays of
  // flame_hip::FeatureTracker::selectGraphFeatures (flame_stereo_graph_inputs) go in as they are, without a copy.
  void sync(int32_t V, const int32_t* feat_id, const float* pos_xy, const float* data_term, const float* data_weight,
            const std::vector<int32_t>& edges, bool check_sticky_obstacles = false, const float* init_x = nullptr,
            float init_graph_scale = 0.0f, bool edges_unique = false) {
    flame_nltgv2_sync_input in{};
    in.init_graph_scale = init_graph_scale;  // > 0: NaN entries of init_x -> neighbours' mean (flame.cc:2133-2158)
    in.edges_unique = edges_unique ? 1 : 0;  // the caller vouches (a triangulator's edge list): no search for repeated pairs
    in.V = V;
    in.feat_id = feat_id, in.pos = pos_xy;
    in.data_term = data_term, in.data_weight = data_weight;
    in.init_x = init_x;
    in.E = static_cast<int32_t>(edges.size() / 2);
    in.edges = edges.data();
    in.check_sticky_obstacles = check_sticky_obstacles ? 1 : 0;
    in.sticky_threshold = 0.25f;  // flame.cc:2011
    check(flame_nltgv2_sync_graph(ctx_, &in), "sync_graph");
  }

  // The same sync in two halves (flame_nltgv2_sync_prepare / _commit): prepare under graph_mtx_ right after the triangulation --
  // it only reads the device image, the solver thread goes on stepping --, commit under graph_mtx_ when Flame::update would have
  // left syncGraph.  init_from_map: new vertices start at the prediction of the dense map the last interpolateMesh left on the
  // device (init_with_prediction, flame.cc:2131) instead of a host gather into init_x.
  void syncPrepare(const std::vector<int32_t>& feat_id, const std::vector<float>& pos_xy, const std::vector<float>& data_term,
                   const std::vector<float>& data_weight, const std::vector<int32_t>& edges, bool check_sticky_obstacles = false,
                   const float* init_x = nullptr, float init_graph_scale = 0.0f, bool edges_unique = false, bool init_from_map = false) {
    syncPrepare(static_cast<int32_t>(feat_id.size()), feat_id.data(), pos_xy.data(), data_term.data(), data_weight.data(), edges,
                check_sticky_obstacles, init_x, init_graph_scale, edges_unique, init_from_map);
  }
  // Pointer + count form (see sync): the caller's arrays are free when it returns.
  void syncPrepare(int32_t V, const int32_t* feat_id, const float* pos_xy, const float* data_term, const float* data_weight,
                   const std::vector<int32_t>& edges, bool check_sticky_obstacles = false, const float* init_x = nullptr,
                   float init_graph_scale = 0.0f, bool edges_unique = false, bool init_from_map = false) {
    flame_nltgv2_sync_input in{};
    in.init_graph_scale = init_graph_scale, in.edges_unique = edges_unique ? 1 : 0, in.init_from_map = init_from_map ? 1 : 0;
    in.V = V;
    in.feat_id = feat_id, in.pos = pos_xy;
    in.data_term = data_term, in.data_weight = data_weight;
    in.init_x = init_x;
    in.E = static_cast<int32_t>(edges.size() / 2);
    in.edges = edges.data();
    in.check_sticky_obstacles = check_sticky_obstacles ? 1 : 0;
    in.sticky_threshold = 0.25f;  // flame.cc:2011
    check(flame_nltgv2_sync_prepare(ctx_, &in), "sync_prepare");
  }
  void syncCommit() { check(flame_nltgv2_sync_commit(ctx_), "sync_commit"); }
  // interpolateMesh in two halves: the rasteriser and the copy-out run on a side stream while the solver steps again.
  void interpolateMeshBegin(const std::vector<int32_t>& triangles, int rows, int cols, float graph_scale, const uint8_t* tri_validity = nullptr) {
    check(flame_nltgv2_interpolate_mesh_begin(ctx_, triangles.data(), static_cast<int32_t>(triangles.size() / 3), tri_validity, rows, cols,
                                              graph_scale), "interpolate_mesh_begin");
  }
  int interpolateMeshEnd(const float** idepthmap) {
    int32_t coverage = 0;
    check(flame_nltgv2_interpolate_mesh_end(ctx_, idepthmap, &coverage), "interpolate_mesh_end");
    return coverage;
  }

  // The mesh outputs of Flame::update() (flame.cc:372-407: vtx_idepths_, getVertexNormals, the three triangle filters) and, if
  // asked for, getFilteredInverseDepthMap's map, from the device state on the side stream (flame_nltgv2_mesh_outputs_begin / _end).
  // `triangles` == nullptr: the triangles the last interpolateMesh[Begin] left on the device (num_triangles of them).
  void meshOutputsBegin(const std::vector<int32_t>* triangles, size_t num_triangles, const float Kinv[9], const MeshFilterParams& filter,
                        int rows, int cols, float graph_scale, bool want_filtered_map) {
    flame_nltgv2_mesh_filter_params c;
    std::memcpy(&c, &filter, sizeof(c));
    check(flame_nltgv2_mesh_outputs_begin(ctx_, triangles ? triangles->data() : nullptr,
                                          static_cast<int32_t>(triangles ? triangles->size() / 3 : num_triangles), Kinv, &c, rows, cols,
                                          graph_scale, want_filtered_map ? 1 : 0), "mesh_outputs_begin");
  }
  MeshOutputs meshOutputsEnd() {
    flame_nltgv2_mesh_outputs_view v;
    check(flame_nltgv2_mesh_outputs_end(ctx_, &v), "mesh_outputs_end");
    MeshOutputs m;
    m.num_vertices = static_cast<size_t>(v.V), m.num_triangles = static_cast<size_t>(v.T);
    m.vtx_idepths = v.vtx_idepth, m.vtx_normals = v.normals, m.tri_validity = v.tri_valid;
    m.num_valid_triangles = v.n_valid;
    m.rows = v.rows, m.cols = v.cols, m.filtered_idepthmap = v.filtered_map, m.filtered_coverage = v.filtered_coverage;
    return m;
  }

  // Depth image, millimetre image, point clouds and the posed mesh from the maps and the mesh buffers the last interpolateMesh[Begin] /
  // meshOutputsBegin left on the device, on the side stream (flame_nltgv2_metric_outputs_begin / _end; the semantics are stated
  // there).  T_world_cam: 12 floats, row-major [R | t], or nullptr for the camera frame.
  void metricOutputsBegin(const float Kinv[9], const float* T_world_cam, const MetricParams& params, int rows, int cols) {
    flame_nltgv2_metric_params c;
    std::memcpy(&c, &params, sizeof(c));
    check(flame_nltgv2_metric_outputs_begin(ctx_, Kinv, T_world_cam, &c, rows, cols), "metric_outputs_begin");
  }
  MetricOutputs metricOutputsEnd() {
    flame_nltgv2_metric_outputs_view v;
    check(flame_nltgv2_metric_outputs_end(ctx_, &v), "metric_outputs_end");
    MetricOutputs m;
    m.rows = v.rows, m.cols = v.cols;
    m.num_vertices = static_cast<size_t>(v.V), m.num_triangles = static_cast<size_t>(v.T);
    m.num_points = static_cast<size_t>(v.n_points), m.num_valid_triangles = static_cast<size_t>(v.n_valid);
    m.depth = v.depth, m.depth_device = v.depth_device;
    m.depth_mm = v.depth_mm, m.depth_mm_device = v.depth_mm_device;
    m.organized = v.organized, m.organized_device = v.organized_device;
    m.cloud = v.cloud, m.cloud_device = v.cloud_device;
    m.cloud_pixel = v.cloud_pixel, m.cloud_pixel_device = v.cloud_pixel_device;
    m.mesh_vertices = v.mesh_vertices, m.mesh_vertices_device = v.mesh_vertices_device;
    m.mesh_normals = v.mesh_normals, m.mesh_normals_device = v.mesh_normals_device;
    m.mesh_triangles = v.mesh_triangles, m.mesh_triangles_device = v.mesh_triangles_device;
    return m;
  }

  // The error of the dense map the last interpolateMesh[Begin] / meshOutputsBegin left on the device (or params.map_device), on the
  // side stream beside the running solver (flame_nltgv2_map_error_begin / _end; the semantics are stated there).
  void mapErrorBegin(const MapErrorParams& params, int rows, int cols) {
    check(flame_nltgv2_map_error_begin(ctx_, &params, rows, cols), "map_error_begin");
  }
  MapError mapErrorEnd() {
    flame_nltgv2_map_error_view v;
    check(flame_nltgv2_map_error_end(ctx_, &v), "map_error_end");
    MapError m;
    m.rows = v.rows, m.cols = v.cols, m.source = v.source, m.win_size = v.win_size, m.hist_scale = v.hist_scale;
    m.stats = v.stats, m.stats_device = v.stats_device;
    m.error = v.error_map, m.error_device = v.error_map_device;
    m.debug_img_photo_error = v.image, m.image_device = v.image_device;
    return m;
  }

  // The triangles the last interpolateMesh[Begin] / meshOutputsBegin left on the device over the state's positions and x * graph_scale,
  // seen from the camera of `params`, on the side stream (flame_nltgv2_render_view_begin / _end; the rules are stated there).
  // rows x cols: the target's size.  tri_validity: a host array of one byte per triangle with params.validity == 1, else nullptr.
  void renderViewBegin(const ViewParams& params, const uint8_t* tri_validity, int rows, int cols, float graph_scale) {
    check(flame_nltgv2_render_view_begin(ctx_, &params, tri_validity, rows, cols, graph_scale), "render_view_begin");
  }
  RenderedView renderViewEnd() {
    flame_nltgv2_view_outputs_view v;
    check(flame_nltgv2_render_view_end(ctx_, &v), "render_view_end");
    RenderedView r;
    r.rows = v.rows, r.cols = v.cols, r.num_triangles = v.T, r.counts = v.counts;
    r.idepthmap = v.map, r.idepthmap_device = v.map_device;
    r.tri_index = v.tri_index, r.tri_index_device = v.tri_index_device;
    return r;
  }
  RenderedView renderView(const ViewParams& params, const uint8_t* tri_validity, int rows, int cols, float graph_scale) {
    renderViewBegin(params, tri_validity, rows, cols, graph_scale);
    return renderViewEnd();
  }

  // The mesh a pose-frame keeps (flame.cc:417-426, curr_pf_->tris / vtx / vtx_idepths): the resident triangles, positions and
  // x * graph_scale into `slot` (0 .. FLAME_NLTGV2_KEPT_MESHES - 1), device to device on the side stream; with_validity: with what the
  // last meshOutputsBegin left of the triangle filters.  dropMesh: prunePoseFrames.  (flame_nltgv2_keep_mesh / _drop_mesh)
  void keepMesh(int slot, float graph_scale, bool with_validity = false) {
    check(flame_nltgv2_keep_mesh(ctx_, slot, graph_scale, with_validity ? 2 : 0), "keep_mesh");
  }
  void dropMesh(int slot) { check(flame_nltgv2_drop_mesh(ctx_, slot), "drop_mesh"); }

  // Up to FLAME_NLTGV2_FUSE_SOURCES kept meshes (and the live one) rendered into one target camera and voted per pixel, on the side
  // stream (flame_nltgv2_fuse_views_begin / _end; the rules are stated there).  rows x cols: the target's size.
  void fuseViewsBegin(const FuseParams& params, int rows, int cols) {
    check(flame_nltgv2_fuse_views_begin(ctx_, &params, rows, cols), "fuse_views_begin");
  }
  FusedView fuseViewsEnd() {
    flame_nltgv2_fuse_outputs_view v;
    check(flame_nltgv2_fuse_views_end(ctx_, &v), "fuse_views_end");
    FusedView r;
    r.rows = v.rows, r.cols = v.cols, r.num_sources = v.n_sources, r.counts = v.counts;
    r.idepthmap = v.fused, r.idepthmap_device = v.fused_device;
    r.present_mask = v.present_mask, r.present_mask_device = v.present_mask_device;
    r.inlier_mask = v.inlier_mask, r.inlier_mask_device = v.inlier_mask_device;
    r.spread = v.spread, r.spread_device = v.spread_device;
    r.layers = v.layers, r.layers_device = v.layers_device;
    return r;
  }

  // The volumetric map of the context (flame_nltgv2_volume_*; the rules are stated there): one truncated-signed-distance volume that
  // outlives every upload() and sync(), a depth map folded into it from a pose, and the volume seen from any camera -- all on the side
  // stream.  volumeIntegrateBegin reads the resident map of the last interpolateMesh[Begin], the filtered one or params.map_device
  // (e.g. FusedView::idepthmap_device); RaycastView::idepthmap_device serves FeatureTracker::alignFrame, MapErrorParams::truth_device and
  // MetricParams::map_device.  K, Kinv: 9 floats row-major; T_cam_world, T_world_cam: 12 floats, row-major [R | t].
  void volumeCreate(const VolumeParams& params) { check(flame_nltgv2_volume_create(ctx_, &params), "volume_create"); }
  void volumeReset() { check(flame_nltgv2_volume_reset(ctx_), "volume_reset"); }
  void volumeDestroy() { check(flame_nltgv2_volume_destroy(ctx_), "volume_destroy"); }
  VolumeParams volumeInfo(int64_t* device_bytes = nullptr) {
    VolumeParams p;
    check(flame_nltgv2_volume_info(ctx_, &p, device_bytes), "volume_info");
    return p;
  }
  void volumeDownload(float* tsdf, float* weight) { check(flame_nltgv2_volume_download(ctx_, tsdf, weight), "volume_download"); }
  void volumeUpload(const float* tsdf, const float* weight) { check(flame_nltgv2_volume_upload(ctx_, tsdf, weight), "volume_upload"); }
  void volumeIntegrateBegin(const float K[9], const float T_cam_world[12], const IntegrateParams& params, int rows, int cols) {
    check(flame_nltgv2_volume_integrate_begin(ctx_, K, T_cam_world, &params, rows, cols), "volume_integrate_begin");
  }
  IntegratedMap volumeIntegrateEnd() {
    flame_nltgv2_integrate_view v;
    check(flame_nltgv2_volume_integrate_end(ctx_, &v), "volume_integrate_end");
    IntegratedMap r;
    r.rows = v.rows, r.cols = v.cols, r.counts = v.counts;
    return r;
  }
  void volumeRaycastBegin(const float Kinv[9], const float T_world_cam[12], const RaycastParams& params, int rows, int cols) {
    check(flame_nltgv2_volume_raycast_begin(ctx_, Kinv, T_world_cam, &params, rows, cols), "volume_raycast_begin");
  }
  RaycastView volumeRaycastEnd() {
    flame_nltgv2_raycast_view v;
    check(flame_nltgv2_volume_raycast_end(ctx_, &v), "volume_raycast_end");
    RaycastView r;
    r.rows = v.rows, r.cols = v.cols, r.counts = v.counts;
    r.idepthmap = v.map, r.idepthmap_device = v.map_device;
    return r;
  }
  // The surface of a box of the volume as a triangle mesh, on the side stream (flame_nltgv2_volume_mesh_begin / _end): for example every
  // N frames, or when a pose-frame is pruned and what it saw lives on in the volume alone.
  void volumeMeshBegin(const VolumeMeshParams& params) { check(flame_nltgv2_volume_mesh_begin(ctx_, &params), "volume_mesh_begin"); }
  VolumeMesh volumeMeshEnd() {
    flame_nltgv2_volume_mesh_view v;
    check(flame_nltgv2_volume_mesh_end(ctx_, &v), "volume_mesh_end");
    VolumeMesh m;
    m.counts = v.counts, m.device_ms = v.device_ms;
    m.vertices = v.vertices, m.vertices_device = v.vertices_device;
    m.normals = v.normals, m.normals_device = v.normals_device;
    m.triangles = v.triangles, m.triangles_device = v.triangles_device;
    return m;
  }

  // The window that follows the camera: the volume is a window on one infinite grid, volumeShiftBegin moves it by whole voxels on the
  // side stream (the records that stay keep their bytes and their world positions), volumeFollow says by how much for a camera pose.
  // Per frame: volumeFollow; volumeMeshBegin / End of each leaving box; volumeShiftBegin / End; volumeIntegrateBegin; volumeRaycastBegin.
  void volumeWindow(int32_t base[3]) { check(flame_nltgv2_volume_window(ctx_, base), "volume_window"); }
  void volumeShiftBegin(const int32_t shift[3]) { check(flame_nltgv2_volume_shift_begin(ctx_, shift), "volume_shift_begin"); }
  ShiftedWindow volumeShiftEnd() {
    flame_nltgv2_shift_view v;
    check(flame_nltgv2_volume_shift_end(ctx_, &v), "volume_shift_end");
    ShiftedWindow w;
    std::memcpy(w.shift, v.shift, sizeof(w.shift));
    std::memcpy(w.base, v.base, sizeof(w.base));
    w.record_bytes = v.record_bytes, w.device_ms = v.device_ms, w.counts = v.counts;
    return w;
  }
  FollowPlan volumeFollow(const float T_world_cam[12], const FollowParams& params) {
    FollowPlan plan;
    check(flame_nltgv2_volume_follow(ctx_, T_world_cam, &params, &plan), "volume_follow");
    return plan;
  }

  // drawInverseDepthMap (flame.cc:2699-2719) and interpolateMesh(w1), interpolateMesh(w2), drawNormals (flame.cc:497-506, 2667-2697) over
  // the dense map, the triangles and the state the last interpolateMesh[Begin] left on the device, on the side stream
  // (flame_nltgv2_debug_images_begin / _end).  The grey image fnew_->img[0] (rows of cols bytes, step_bytes apart): in host memory
  // (img_host) or in device memory (img_device, e.g. FeatureTracker::frameImageDevice: nothing is uploaded) -- exactly one of the two.
  void debugImagesBegin(const uint8_t* img_host, const void* img_device, int step_bytes, const float K[9], const DebugImageParams& params,
                        int rows, int cols) {
    flame_nltgv2_debug_image_params c;
    std::memcpy(&c, &params, sizeof(c));
    check(flame_nltgv2_debug_images_begin(ctx_, img_host, img_device, step_bytes, K, &c, rows, cols), "debug_images_begin");
  }
  DebugImages debugImagesEnd() {
    flame_nltgv2_debug_images_view v;
    check(flame_nltgv2_debug_images_end(ctx_, &v), "debug_images_end");
    DebugImages d;
    d.rows = v.rows, d.cols = v.cols;
    d.debug_img_idepthmap = v.idepthmap_img, d.debug_img_normals = v.normals_img, d.w1_map = v.w1_map, d.w2_map = v.w2_map;
    return d;
  }
  DebugImages debugImages(const uint8_t* img_host, const void* img_device, int step_bytes, const float K[9], const DebugImageParams& params,
                          int rows, int cols) {
    debugImagesBegin(img_host, img_device, step_bytes, K, params, rows, cols);
    return debugImagesEnd();
  }

  // drawWireframe (flame.cc:2414-2457) over the triangles the last interpolateMesh[Begin] / meshOutputsBegin left on the device and the
  // state's positions and x * graph_scale, on the side stream (flame_nltgv2_debug_wireframe_begin / _end).  The grey image as in
  // debugImagesBegin.  tri_validity: a host array of one byte per triangle with params.validity == 1, else nullptr.
  void debugWireframeBegin(const uint8_t* img_host, const void* img_device, int step_bytes, const uint8_t* tri_validity,
                           const WireframeParams& params, int rows, int cols, float graph_scale) {
    flame_nltgv2_wireframe_params c;
    std::memcpy(&c, &params, sizeof(c));
    check(flame_nltgv2_debug_wireframe_begin(ctx_, img_host, img_device, step_bytes, tri_validity, &c, rows, cols, graph_scale),
          "debug_wireframe_begin");
  }
  Wireframe debugWireframeEnd() {
    flame_nltgv2_wireframe_view v;
    check(flame_nltgv2_debug_wireframe_end(ctx_, &v), "debug_wireframe_end");
    Wireframe w;
    w.rows = v.rows, w.cols = v.cols, w.debug_img_wireframe = v.wireframe_img;
    w.lines_drawn = v.lines_drawn, w.lines_skipped = v.lines_skipped, w.refilled = v.refilled != 0;
    return w;
  }

  // utils::interpolateMesh (utils/image_utils.cc:373-396) at its call site flame.cc:409-415: rasterises
  // x*graph_scale of the device state over `triangles` (triangulator->triangles(), 3 ints each) into a
  // rows*cols float image (NaN = uncovered); returns the coverage count of flame.cc:428-437.
  int interpolateMesh(const std::vector<int32_t>& triangles, int rows, int cols, float graph_scale, float* idepthmap,
                      const uint8_t* tri_validity = nullptr) {
    int32_t coverage = 0;
    check(flame_nltgv2_interpolate_mesh(ctx_, triangles.data(), static_cast<int32_t>(triangles.size() / 3), tri_validity,
                                        rows, cols, graph_scale, idepthmap, &coverage),
          "interpolate_mesh");
    return coverage;
  }

  void step(const Params& p) { run(p, 1); }
  void run(const Params& p, int n_iters) {
    const flame_nltgv2_params c = to_c(p);
    check(flame_nltgv2_run(ctx_, &c, n_iters), "run");
  }
  void dualStep(const Params& p) { const flame_nltgv2_params c = to_c(p); check(flame_nltgv2_dual_step(ctx_, &c), "dualStep"); }
  void primalStep(const Params& p) { const flame_nltgv2_params c = to_c(p); check(flame_nltgv2_primal_step(ctx_, &c), "primalStep"); }
  void extraGradientStep(const Params& p) {
    const flame_nltgv2_params c = to_c(p);
    check(flame_nltgv2_extragradient_step(ctx_, &c), "extraGradientStep");
  }
  void savePrev() { check(flame_nltgv2_save_prev(ctx_), "savePrev"); }
  float smoothnessCost(const Params& p) { float s = 0, d = 0; costs(p, &s, &d); return s; }
  float dataCost(const Params& p) { float s = 0, d = 0; costs(p, &s, &d); return d; }
  float cost(const Params& p) { float s = 0, d = 0; costs(p, &s, &d); return s + d; }
  void costs(const Params& p, float* smooth, float* data) {
    const flame_nltgv2_params c = to_c(p);
    check(flame_nltgv2_costs(ctx_, &c, smooth, data), "costs");
  }
  // Asynchronous use (multi-GPU hosts, frame_gather.hpp): the solver's stream, a standing device target that every run
  // leaves x * scale in (the read-back of flame.cc:372-380, on the device), enqueue-only runs and the matching wait.
  void setStream(void* hip_stream) { check(flame_nltgv2_set_stream(ctx_, hip_stream), "set_stream"); }
  void setExportTarget(void* dst_device, float scale) { check(flame_nltgv2_set_export_target(ctx_, dst_device, scale), "set_export_target"); }
  void runAsync(const Params& p, int n_iters) {
    const flame_nltgv2_params c = to_c(p);
    check(flame_nltgv2_run_async(ctx_, &c, n_iters), "run_async");
  }
  void sync() { check(flame_nltgv2_sync(ctx_), "sync"); }
  // A run that goes on until the next call that needs the solver settled asks it to stop (flame_nltgv2_run_open: the reference's solver
  // thread is `while (true) step()`, flame.cc:99-112); at most max_iters (even) iterations.  false: not applicable to this graph or
  // configuration -- nothing was enqueued, use runAsync.
  bool runOpen(const Params& p, int max_iters) {
    const flame_nltgv2_params c = to_c(p);
    int32_t opened = 0;
    check(flame_nltgv2_run_open(ctx_, &c, max_iters, &opened), "run_open");
    return opened != 0;
  }
  // Iterations applied to the state by all runs so far; an open run is counted when it has been settled (*open_in_flight: one is not yet).
  // Never waits: right after a call that settled the solver this is the exact number the state has seen.
  uint64_t iterations(bool* open_in_flight = nullptr) {
    int64_t total = 0;
    int32_t open_ = 0;
    check(flame_nltgv2_iterations(ctx_, &total, &open_), "iterations");
    if (open_in_flight) *open_in_flight = open_ != 0;
    return static_cast<uint64_t>(total);
  }
  // Another stream of the caller waits for the runs enqueued so far (a consumer of the export row: a collective, a copy); right behind
  // runAsync() it costs the solver's stream nothing -- the launch carries the event.
  void streamWaitRun(void* other_hip_stream) { check(flame_nltgv2_stream_wait_run(ctx_, other_hip_stream), "stream_wait_run"); }
  // How many of the last two runAsync() runs the device has not finished yet (0..2; no wait, no check of their results).
  int runsInFlight() {
    int32_t n = 0;
    check(flame_nltgv2_runs_in_flight(ctx_, &n), "runs_in_flight");
    return static_cast<int>(n);
  }
  // Asynchronous runs that sync() had to take back and redo (an expired neighbour wait or a torn record: the state is
  // right again when sync() returns, but anything that consumed the export row BEFORE sync() -- a gather enqueued right
  // behind runAsync() -- read the previous frame's values).  A caller compares this before and after its sync().
  int replays() {
    flame_nltgv2_info info;
    check(flame_nltgv2_get_info(ctx_, &info), "get_info");
    return info.timeouts_recovered + info.torn_records_detected;
  }
  flame_nltgv2_ctx* handle() { return ctx_; }

 private:
  void check(int rc, const char* what) {
    if (rc != 0) throw flame_hip::Error(rc, what);
  }
  flame_nltgv2_ctx* ctx_;
  flame_hip::FlatArrays flat_;
  size_t uploaded_v_ = 0, uploaded_e_ = 0;
  uint64_t generation_ = 0, identity_ = 0;
  bool uploaded_ = false;
};

// ---- the reference's free functions, same signatures (h:134-168) -----------------------------------
// Stateless convenience forms: upload + compute + download on every call.  Exact, but they pay the
// transfer each time; a pipeline should own a DeviceGraph instead.
template <class Graph>
inline void step(const Params& params, Graph* graph) {
  DeviceGraph d;
  d.upload(*graph);
  d.step(params);
  d.download(graph);
}
template <class Graph>
inline float smoothnessCost(const Params& params, const Graph& graph) {
  DeviceGraph d;
  d.upload(graph);
  return d.smoothnessCost(params);
}
template <class Graph>
inline float dataCost(const Params& params, const Graph& graph) {
  DeviceGraph d;
  d.upload(graph);
  return d.dataCost(params);
}
template <class Graph>
inline float cost(const Params& params, const Graph& graph) {
  return smoothnessCost(params, graph) + dataCost(params, graph);
}

namespace internal {
template <class Graph>
inline void dualStep(const Params& params, Graph* graph) {
  DeviceGraph d;
  d.upload(*graph);
  d.dualStep(params);
  d.download(graph);
}
template <class Graph>
inline void primalStep(const Params& params, Graph* graph) {
  DeviceGraph d;
  d.upload(*graph);
  d.primalStep(params);
  d.download(graph);
}
template <class Graph>
inline void extraGradientStep(const Params& params, Graph* graph) {
  DeviceGraph d;
  d.upload(*graph);
  d.extraGradientStep(params);
  d.download(graph);
}
}  // namespace internal

}  // namespace hip
}  // namespace nltgv2_l1_graph_regularizer
}  // namespace optimizers
}  // namespace flame

#endif  // FLAME_HIP_NLTGV2_L1_GRAPH_REGULARIZER_HPP_
