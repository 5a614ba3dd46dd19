// side_stage.hpp -- the pure part of the stages on the side stream (nltgv2_frame_capi.hip: the dense map, the mesh outputs, the debug
// images, the wireframe, the metric outputs, the map error, the view renderer, the fusion of views), no HIP and no context: what the context knows about the triangles resident in r_tris, where each stage's
// outputs lie in its pinned buffer, and the triangle index check.  tests/cpp/side_stage_test.cc walks all of it (MetricLayout:
// tests/cpp/metric_layout_test.cc; MapErrorLayout: tests/cpp/map_error_layout_test.cc; ViewLayout: tests/cpp/view_layout_test.cc; FuseLayout: tests/cpp/fuse_layout_test.cc; VolumeLayout: tests/cpp/volume_layout_test.cc; VolumeMeshLayout and the box check: tests/cpp/volume_mesh_layout_test.cc).
#ifndef FLAME_AMD_SIDE_STAGE_HPP_
#define FLAME_AMD_SIDE_STAGE_HPP_

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace flame_hip {
namespace host {

// Which triangles r_tris holds, whether the key image r_keys names their winners, and whether the filter validity m_tvalid speaks of
// them.  Every upload into r_tris counts `uploads` up; the key image and the validity remember the upload they were made from, so
// another upload makes both stale without anybody having to say so.
//   An upload counts up in every transition that makes T >= 0, so a count remembered while the triangles were current cannot meet
// `uploads` again under other triangles, another T or another topology: the validity needs no T and no topology of its own.
class ResidentTris {
 public:
  // -- transitions ---------------------------------------------------------------------------------------------------------
  // T triangles of the graph of topology `topo` were uploaded and the graph's map rasterised from them (interpolate_mesh,
  // interpolate_mesh_begin); masked: with a validity mask, so the key image does not name the winners of the all-valid rasterisation.
  // interpolate_mesh_begin says so when the upload is enqueued, before mesh_state_on can fail: the triangles are resident then, whatever
  // becomes of the map.
  void uploaded(int32_t T, uint64_t topo, bool masked) {
    T_ = T, topo_ = topo, ++uploads_;
    keys_of_ = masked ? 0 : uploads_;
  }
  // Triangles that index the caller's arrays were uploaded and rasterised (interpolate_mesh_arrays): r_tris and r_keys are another
  // image's.  The counts may agree afterwards; nothing is current, because no triangles of the graph are resident.
  void uploaded_foreign(bool masked) {
    T_ = -1, ++uploads_;
    keys_of_ = masked ? 0 : uploads_;
  }
  // T triangles of the graph were uploaded and nothing rasterised (mesh_outputs_begin with a list of its own): the key image still
  // describes the list before.
  void uploaded_unrasterised(int32_t T, uint64_t topo) { T_ = T, topo_ = topo, ++uploads_; }
  // The filters wrote m_tvalid for the resident triangles (mesh_outputs_begin).
  void validity_written() { validity_of_ = uploads_; }
  // No triangles of the graph are resident: interpolate_mesh_arrays is about to replace them, or a synchronous interpolate_mesh
  // failed -- wherever it failed, also in its argument checks with the old list still in r_tris.
  void none_resident() { T_ = -1; }

  // -- predicates ----------------------------------------------------------------------------------------------------------
  int32_t T() const { return T_; }
  bool current(uint64_t topo) const { return T_ >= 0 && topo_ == topo; }
  bool matches(int32_t T, uint64_t topo) const { return T_ == T && topo_ == topo; }  // (the caller's T >= 0: mesh_outputs_begin(NULL))
  bool keys_name_winners() const { return T_ >= 0 && keys_of_ != 0 && keys_of_ == uploads_; }
  bool validity_current(uint64_t topo) const { return current(topo) && validity_of_ != 0 && validity_of_ == uploads_; }

 private:
  int32_t T_ = -1;         // triangles in r_tris (-1: none, or they index other arrays than the graph's)
  uint64_t topo_ = ~0ull;  // the topology their indices were checked against
  uint64_t uploads_ = 0;   // uploads into r_tris so far
  uint64_t keys_of_ = 0, validity_of_ = 0;  // the upload r_keys / m_tvalid describe (0: none)
};

inline size_t up16(size_t bytes) { return (bytes + 15) & ~size_t(15); }

// Byte offsets of a stage's outputs in its pinned buffer, and the bytes the buffer needs.
struct MeshLayout {
  size_t normals, idepth, counts, map, valid, total;  // 3V floats | V floats | {n_valid, coverage} | the filtered map | T bytes
};
inline MeshLayout mesh_layout(int32_t V, int32_t T, int rows, int cols, bool want_map) {
  MeshLayout m;
  m.normals = 0;
  m.idepth = sizeof(float) * 3 * (size_t)V;
  m.counts = m.idepth + sizeof(float) * (size_t)V;
  m.map = m.counts + 4 * sizeof(int32_t);
  m.valid = m.map + (want_map ? sizeof(float) * (size_t)rows * (size_t)cols : 0);
  m.total = m.valid + (size_t)T + 16;
  return m;
}

struct DebugLayout {
  size_t idimg, nimg, w1, w2, gray, total;  // idepth image | normals image | w1 map | w2 map | a host grey image on its way up
};
inline DebugLayout debug_layout(int rows, int cols, bool want_idepth, bool want_normals, bool host_gray) {
  const size_t n = (size_t)rows * (size_t)cols;
  DebugLayout d;
  d.idimg = 0;
  d.nimg = up16(want_idepth ? 3 * n : 0);
  d.w1 = d.nimg + up16(want_normals ? 3 * n : 0);
  d.w2 = d.w1 + up16(want_normals ? sizeof(float) * n : 0);
  d.gray = d.w2 + up16(want_normals ? sizeof(float) * n : 0);
  d.total = d.gray + up16(host_gray ? n : 0) + 16;
  return d;
}

constexpr size_t kWireCountBytes = 16;  // the wireframe's counters (wireframe_kernels.h: kWireCounts ints)
struct WireLayout {
  size_t img, counts, gray, total;  // the picture | the counters | a host grey image on its way up
};
inline WireLayout wire_layout(int rows, int cols, bool host_gray) {
  const size_t n = (size_t)rows * (size_t)cols;
  WireLayout w;
  w.img = 0;
  w.counts = up16(3 * n);
  w.gray = w.counts + kWireCountBytes;
  w.total = w.gray + up16(host_gray ? n : 0) + 16;
  return w;
}

// Which of the metric outputs a call asks for (flame_nltgv2_metric_params), and whether they travel to the host at all.
struct MetricWants {
  bool depth, depth_mm, organized, cloud, mesh, copy_out;
};
struct MetricLayout {
  // {n_points, n_valid} | rows*cols floats | rows*cols uint16 | 3*rows*cols floats | up to 3*rows*cols floats | up to rows*cols
  // uint32 | 3V floats | 3V floats | up to 3T int32.  The counters are always there; an output that is not wanted, and every output
  // without copy_out, takes no room.
  size_t counts, depth, depth_mm, organized, cloud, cloud_pixel, vertices, normals, triangles, total;
};
inline MetricLayout metric_layout(int rows, int cols, int32_t V, int32_t T, const MetricWants& w) {
  const size_t n = (size_t)rows * (size_t)cols, f = sizeof(float);
  const bool out = w.copy_out;
  MetricLayout m;
  m.counts = 0;
  m.depth = 16;
  m.depth_mm = m.depth + up16(out && w.depth ? f * n : 0);
  m.organized = m.depth_mm + up16(out && w.depth_mm ? sizeof(uint16_t) * n : 0);
  m.cloud = m.organized + up16(out && w.organized ? 3 * f * n : 0);
  m.cloud_pixel = m.cloud + up16(out && w.cloud ? 3 * f * n : 0);
  m.vertices = m.cloud_pixel + up16(out && w.cloud ? sizeof(uint32_t) * n : 0);
  m.normals = m.vertices + up16(out && w.mesh ? 3 * f * (size_t)V : 0);
  m.triangles = m.normals + up16(out && w.mesh ? 3 * f * (size_t)V : 0);
  m.total = m.triangles + up16(out && w.mesh ? 3 * sizeof(int32_t) * (size_t)T : 0) + 16;
  return m;
}

// What a map-error call asks for (flame_nltgv2_map_error_params) and what it stages on its way up.
struct MapErrorWants {
  bool stats, error_map, image, copy_out;
  bool host_truth, host_gray;  // a true map / a grey image of the caller's in host memory goes up through this buffer
};
constexpr size_t kMapErrorStatsBytes = 256 * sizeof(int32_t) + 3 * sizeof(int32_t) + sizeof(float) + sizeof(double);  // flame_nltgv2_map_error_stats
struct MapErrorLayout {
  // the statistics | rows*cols floats | 3*rows*cols bytes | a host true map on its way up | a host grey image on its way up.  The
  // statistics are always there; the error map and the picture take room only if wanted and copy_out.
  size_t stats, error_map, image, truth, gray, total;
};
inline MapErrorLayout map_error_layout(int rows, int cols, const MapErrorWants& w) {
  const size_t n = (size_t)rows * (size_t)cols;
  MapErrorLayout m;
  m.stats = 0;
  m.error_map = up16(kMapErrorStatsBytes);
  m.image = m.error_map + up16(w.copy_out && w.error_map ? sizeof(float) * n : 0);
  m.truth = m.image + up16(w.copy_out && w.image ? 3 * n : 0);
  m.gray = m.truth + up16(w.host_truth ? sizeof(float) * n : 0);
  m.total = m.gray + up16(w.host_gray ? n : 0) + 16;
  return m;
}

// The reference's choice of the box (flame.cc:919-922) where the caller names none; 0 for a size that is no odd number of
// 1 .. max_win.
inline int map_error_window(int win_size, int cols, int max_win) {
  if (win_size == 0) return cols < 640 ? 5 : 11;
  return (win_size >= 1 && win_size <= max_win && win_size % 2 == 1) ? win_size : 0;
}

// Which outputs a view-renderer call asks for (flame_nltgv2_view_params), and whether they travel to the host at all.
struct ViewWants {
  bool map, tri_index, copy_out;
};
constexpr size_t kViewCountBytes = 4 * sizeof(int32_t);  // flame_nltgv2_view_counts
struct ViewLayout {
  // the counters | rows*cols floats | rows*cols int32.  The counters are always there; the map and the owner indices take room only
  // if wanted and copy_out.
  size_t counts, map, tri_index, total;
};
inline ViewLayout view_layout(int rows, int cols, const ViewWants& w) {
  const size_t n = (size_t)rows * (size_t)cols;
  ViewLayout v;
  v.counts = 0;
  v.map = up16(kViewCountBytes);
  v.tri_index = v.map + up16(w.copy_out && w.map ? sizeof(float) * n : 0);
  v.total = v.tri_index + up16(w.copy_out && w.tri_index ? sizeof(int32_t) * n : 0) + 16;
  return v;
}

// Which outputs a fusion call asks for (flame_nltgv2_fuse_params), and whether they travel to the host at all.
struct FuseWants {
  bool fused, masks, spread, layers, copy_out;
};
constexpr size_t kFuseCountBytes = 32 * sizeof(int32_t);  // flame_nltgv2_fuse_counts
struct FuseLayout {
  // the counters | rows*cols floats | rows*cols bytes | rows*cols bytes | rows*cols floats | n_sources*rows*cols floats.  The counters
  // are always there; every other output takes room only if wanted and copy_out.
  size_t counts, fused, present, inlier, spread, layers, total;
};
inline FuseLayout fuse_layout(int rows, int cols, int n_sources, const FuseWants& w) {
  const size_t n = (size_t)rows * (size_t)cols, f = sizeof(float);
  const bool out = w.copy_out;
  FuseLayout l;
  l.counts = 0;
  l.fused = up16(kFuseCountBytes);
  l.present = l.fused + up16(out && w.fused ? f * n : 0);
  l.inlier = l.present + up16(out && w.masks ? n : 0);
  l.spread = l.inlier + up16(out && w.masks ? n : 0);
  l.layers = l.spread + up16(out && w.spread ? f * n : 0);
  l.total = l.layers + up16(out && w.layers ? f * n * (size_t)n_sources : 0) + 16;
  return l;
}

// The volume's two stages (flame_nltgv2_volume_integrate_begin, flame_nltgv2_volume_raycast_begin), each with a pinned buffer of its own.
constexpr size_t kIntegrateCountBytes = 8 * sizeof(int32_t);  // flame_nltgv2_integrate_counts
constexpr size_t kRaycastCountBytes = 4 * sizeof(int32_t);    // flame_nltgv2_raycast_counts
// The counters come down as the kernels keep them: kCountSets partial sets, one 128-byte line apart (volume_kernels.h), which _end sums.
constexpr int kCountSets = 16, kCountSetWords = 32;
constexpr size_t kCountSetsBytes = sizeof(int32_t) * kCountSets * kCountSetWords;
constexpr int kVolumeMaxAxis = 1024;
constexpr uint64_t kVolumeMaxVoxels = 1ull << 28;
struct VolumeLayout {
  // the counters' partial sets | rows*cols floats.  The counters are always there; an integration has no map, a raycast's takes room only
  // with copy_out.
  size_t counts, map, total;
};
inline VolumeLayout integrate_layout() {
  VolumeLayout v;
  v.counts = 0;
  v.map = up16(kCountSetsBytes);
  v.total = v.map + 16;
  return v;
}
inline VolumeLayout raycast_layout(int rows, int cols, bool copy_out) {
  VolumeLayout v;
  v.counts = 0;
  v.map = up16(kCountSetsBytes);
  v.total = v.map + up16(copy_out ? sizeof(float) * (size_t)rows * (size_t)cols : 0) + 16;
  return v;
}
// out[c] = the sum over the partial sets of their word c, for the n_words counters of a stage.
inline void sum_count_slots(const int32_t* slots, int n_words, int32_t* out) {
  for (int c = 0; c < n_words; ++c) {
    int32_t sum = 0;
    for (int s = 0; s < kCountSets; ++s) sum += slots[s * kCountSetWords + c];
    out[c] = sum;
  }
}
// Voxels of an nx x ny x nz volume; 0 for dimensions flame_nltgv2_volume_create refuses.
inline uint64_t volume_voxels(int nx, int ny, int nz) {
  if (nx < 1 || ny < 1 || nz < 1 || nx > kVolumeMaxAxis || ny > kVolumeMaxAxis || nz > kVolumeMaxAxis) return 0;
  const uint64_t n = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
  return n <= kVolumeMaxVoxels ? n : 0;
}

// The window that follows the camera (flame_nltgv2_volume_shift_begin, flame_nltgv2_volume_follow): tests/cpp/volume_window_layout_test.cc.
constexpr size_t kShiftCountBytes = 8 * sizeof(int32_t);  // flame_nltgv2_shift_counts
constexpr int32_t kVolumeMaxBase = 1 << 22;
// base + shift, per axis; false where it passes the limit (out is then untouched).
inline bool shifted_base(const int32_t base[3], const int32_t shift[3], int32_t out[3]) {
  int64_t b[3];
  for (int a = 0; a < 3; ++a) {
    b[a] = (int64_t)base[a] + (int64_t)shift[a];
    if (b[a] < -(int64_t)kVolumeMaxBase || b[a] > (int64_t)kVolumeMaxBase) return false;
  }
  for (int a = 0; a < 3; ++a) out[a] = (int32_t)b[a];
  return true;
}
// The shift as the kernel takes it: each component clamped to +-n_axis (nothing is kept from there on); true if anything moves.
inline bool clamped_shift(const int32_t dims[3], const int32_t shift[3], int clamped[3]) {
  bool moves = false;
  for (int a = 0; a < 3; ++a) {
    clamped[a] = shift[a] > dims[a] ? dims[a] : shift[a] < -dims[a] ? -dims[a] : shift[a];
    moves = moves || shift[a] != 0;
  }
  return moves;
}
// FOLLOW's arithmetic (float32, no FMA: this header is built with -ffp-contract=off); false for an invalid argument.
inline bool follow_shift(const float* T_world_cam, float focus_depth, int32_t step, const float origin[3], float voxel_size,
                         const int32_t base[3], const int32_t dims[3], int32_t shift[3]) {
  if (step < 1 || !std::isfinite(focus_depth)) return false;
  int32_t s[3];
  for (int a = 0; a < 3; ++a) {
    const float c = T_world_cam[4 * a + 3] + focus_depth * T_world_cam[4 * a + 2];
    if (!std::isfinite(c)) return false;
    const float g = (c - origin[a]) / voxel_size;
    const int32_t m = base[a] + dims[a] / 2;
    const float q = truncf((g - (float)m) / (float)step);
    if (!(q >= -(float)kVolumeMaxBase && q <= (float)kVolumeMaxBase)) return false;
    const int64_t prod = (int64_t)(int32_t)q * (int64_t)step;
    if (prod < INT32_MIN || prod > INT32_MAX) return false;
    s[a] = (int32_t)prod;
  }
  for (int a = 0; a < 3; ++a) shift[a] = s[a];
  return true;
}
// THE PLAN of a shift (flame_nltgv2_follow_plan, word for word).
struct WindowPlan {
  int32_t shift[3], n_leaving, has_kept, kept_lo[3], kept_hi[3], leaving_lo[3][3], leaving_hi[3][3], reserved[3];
};
inline void window_plan(const int32_t dims[3], const int32_t shift[3], WindowPlan* p) {
  *p = WindowPlan{};
  bool all_leave = false;
  for (int a = 0; a < 3; ++a) {
    p->shift[a] = shift[a];
    all_leave = all_leave || (int64_t)shift[a] >= dims[a] || (int64_t)shift[a] <= -(int64_t)dims[a];
  }
  if (all_leave) {
    p->n_leaving = 1;
    for (int a = 0; a < 3; ++a) p->leaving_hi[0][a] = dims[a];
    return;
  }
  p->has_kept = 1;
  for (int a = 0; a < 3; ++a) {
    p->kept_lo[a] = shift[a] > 0 ? shift[a] : 0;
    p->kept_hi[a] = shift[a] < 0 ? dims[a] + shift[a] : dims[a];
  }
  for (int a = 0; a < 3; ++a) {
    if (shift[a] == 0) continue;
    int32_t* lo = p->leaving_lo[p->n_leaving];
    int32_t* hi = p->leaving_hi[p->n_leaving];
    for (int b = 0; b < 3; ++b) {
      if (b < a) lo[b] = p->kept_lo[b], hi[b] = p->kept_hi[b];  // the axes whose slabs came before: their kept range
      else if (b > a) lo[b] = 0, hi[b] = dims[b];
      else if (shift[a] > 0) lo[b] = 0, hi[b] = shift[a] + 1;   // one layer towards the kept side
      else lo[b] = dims[a] + shift[a] - 1, hi[b] = dims[a];
    }
    ++p->n_leaving;
  }
}

// The volume's surface extraction (flame_nltgv2_volume_mesh_begin).
constexpr size_t kMeshCountBytes = 8 * sizeof(int32_t);   // flame_nltgv2_volume_mesh_counts
constexpr size_t kMeshTotalsBytes = 4 * sizeof(int32_t);  // what the scan leaves: n_vertices, n_triangles, 0, 0
constexpr uint64_t kMeshMaxBoxVoxels = 1ull << 26;        // 7 vertices and 12 triangles per voxel stay below 2^31
// The box lo <= index < hi of a volume of dims voxels (all-zero hi: the whole volume): its voxels, its lower corner and its extent; 0 for
// a box that is out of range, empty or over kMeshMaxBoxVoxels.
inline uint64_t mesh_box_voxels(const int32_t dims[3], const int32_t lo[3], const int32_t hi[3], int32_t lo_out[3], int32_t n_out[3]) {
  const bool whole = hi[0] == 0 && hi[1] == 0 && hi[2] == 0;
  uint64_t n = 1;
  for (int a = 0; a < 3; ++a) {
    const int32_t h = whole ? dims[a] : hi[a];
    if (lo[a] < 0 || lo[a] >= h || h > dims[a]) return 0;
    lo_out[a] = lo[a], n_out[a] = h - lo[a];
    n *= (uint64_t)(h - lo[a]);
  }
  return n <= kMeshMaxBoxVoxels ? n : 0;
}
// The elements the device arrays (and with copy_out the pinned ones) hold: the caller's capacity, but no more than the box can give.
inline int64_t mesh_vertex_room(uint64_t box_voxels, int32_t max_vertices) {
  const int64_t most = 7 * (int64_t)box_voxels;
  return max_vertices < most ? max_vertices : most;
}
inline int64_t mesh_triangle_room(uint64_t box_voxels, int32_t max_triangles) {
  const int64_t most = 12 * (int64_t)box_voxels;
  return max_triangles < most ? max_triangles : most;
}
struct VolumeMeshLayout {
  // the cube counters' partial sets | the scan's totals | 3 * room floats | 3 * room floats | 3 * room int32.  The counters are always
  // there; the arrays take room only with copy_out, the normals only if wanted.
  size_t counts, totals, vertices, normals, triangles, total;
};
inline VolumeMeshLayout volume_mesh_layout(int64_t vertex_room, int64_t triangle_room, bool want_normals, bool copy_out) {
  const size_t vb = copy_out ? 3 * sizeof(float) * (size_t)vertex_room : 0;
  VolumeMeshLayout m;
  m.counts = 0;
  m.totals = up16(kCountSetsBytes);
  m.vertices = m.totals + up16(kMeshTotalsBytes);
  m.normals = m.vertices + up16(vb);
  m.triangles = m.normals + up16(want_normals ? vb : 0);
  m.total = m.triangles + up16(copy_out ? 3 * sizeof(int32_t) * (size_t)triangle_room : 0) + 16;
  return m;
}

// Every index of T triangles names one of V vertices.
inline bool triangles_in_range(const int32_t* triangles, int32_t T, int32_t V) {
  for (int64_t t = 0; t < 3 * (int64_t)T; ++t)
    if (triangles[t] < 0 || triangles[t] >= V) return false;
  return true;
}

}  // namespace host
}  // namespace flame_hip

#endif  // FLAME_AMD_SIDE_STAGE_HPP_
