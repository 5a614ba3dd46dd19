// tests/cpp/select_graph_features_test.cc -- selectGraphFeatures and getRawIDepths of include/flame_hip/feature_tracker.hpp
// used with look-alikes of the reference's own types (Params, a Frame with id + SE3 pose, a std::map of shared frames,
// FeatureWithIDepth), the way a front-end would call them where the reference runs the preprocessing of Flame::syncGraph,
// and the pointer + count overloads of DeviceGraph::syncPrepare / sync of include/flame_hip/nltgv2_l1_graph_regularizer.hpp
// fed with the selection's arrays as they are.  The case (camera, pose-frames, parameters, features, their projected records)
// comes from a file written by tests/test_select_graph_features_cpp.py; the program dumps what it obtained -- the resident form
// after projectFeatures, the form on two vectors, getRawIDepths, the synced graphs -- and the Python side compares the dump
// with the checker.  In the file the current frame has the identity pose, so that fcur.pose.inverse() * pf.pose of the
// look-alike SE3 is exactly pf.pose: one pose per pose-frame serves the projection and the height.
// Exit code 0 = pass, 77 = no usable HIP device.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "flame_hip/feature_tracker.hpp"
#include "flame_hip/nltgv2_l1_graph_regularizer.hpp"

// ---- look-alikes of the reference types the template binding touches (test-only) -----------------------------
struct Quat {
  float w_, x_, y_, z_;
  float w() const { return w_; }
  float x() const { return x_; }
  float y() const { return y_; }
  float z() const { return z_; }
};
struct Vec3 {
  float v[3];
  float operator()(int i) const { return v[i]; }
};
static Vec3 rotate(const Quat& q, const Vec3& p) {
  const double w = q.w_, x = q.x_, y = q.y_, z = q.z_;
  const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z),
                       1 - 2 * (x * x + z * z), 2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x),
                       1 - 2 * (x * x + y * y)};
  Vec3 o;
  for (int i = 0; i < 3; ++i) o.v[i] = (float)(R[3 * i] * p.v[0] + R[3 * i + 1] * p.v[1] + R[3 * i + 2] * p.v[2]);
  return o;
}
struct SE3 {  // Sophus::SE3f look-alike
  Quat q;
  Vec3 t;
  const Quat& unit_quaternion() const { return q; }
  const Vec3& translation() const { return t; }
  SE3 inverse() const {
    SE3 o;
    o.q = Quat{q.w_, -q.x_, -q.y_, -q.z_};
    const Vec3 r = rotate(o.q, t);
    o.t = Vec3{{-r.v[0], -r.v[1], -r.v[2]}};
    return o;
  }
  SE3 operator*(const SE3& b) const {
    SE3 o;
    o.q = Quat{q.w_ * b.q.w_ - q.x_ * b.q.x_ - q.y_ * b.q.y_ - q.z_ * b.q.z_,
               q.w_ * b.q.x_ + q.x_ * b.q.w_ + q.y_ * b.q.z_ - q.z_ * b.q.y_,
               q.w_ * b.q.y_ - q.x_ * b.q.z_ + q.y_ * b.q.w_ + q.z_ * b.q.x_,
               q.w_ * b.q.z_ + q.x_ * b.q.y_ - q.y_ * b.q.x_ + q.z_ * b.q.w_};
    const Vec3 r = rotate(q, b.t);
    o.t = Vec3{{r.v[0] + t.v[0], r.v[1] + t.v[1], r.v[2] + t.v[2]}};
    return o;
  }
};
struct Frame {
  uint32_t id;
  SE3 pose;
  std::vector<uint8_t> img;
};
struct Point2f {
  float x, y;
};
struct FeatureWithIDepth {  // flame.h:88-99
  uint32_t id = 0;
  uint32_t frame_id = 0;
  Point2f xy;
  float idepth_mu = 0.0f;
  float idepth_var = 0.0f;
  bool valid = false;
  uint32_t num_updates = 0;
  uint32_t num_dropouts = 0;
  int search_status = 0;
};
struct LineStereoParams {
  float max_cost = 1300.0f;
  bool do_subpixel = true;
  float sample_dist = 1.0f;
  float second_best_factor = 1.5f;
};
struct FilterParams {
  int win_size = 5;
  float search_sigma = 2.0f, min_grad_mag = 5.0f, idepth_min = 1e-3f, idepth_max = 2.0f, epilength_min = 3.0f,
        epilength_max = 32.0f, process_var_factor = 1.01f, process_fail_var_factor = 1.1f;
  LineStereoParams sparams;
};
struct MeasParams {
  int win_size = 5;
  float pixel_var = 16.0f, epipolar_line_var = 1.0f;
};
struct FlameParams {
  float min_grad_mag = 5.0f;          // params.h:39 (detection)
  int detection_win_size = 16;        // params.h:48
  float idepth_init = 0.01f, idepth_var_init = 0.25f;  // params.h:60-61
  float min_baseline = 0.01f;
  bool do_letterbox = false;
  float rescale_factor_min = 0.7f, rescale_factor_max = 1.4f, idepth_var_max = 0.25f;
  int max_dropouts = 5;
  float outlier_sigma_thresh = 3.0f;
  bool do_meas_fusion = true;
  FilterParams fparams;
  MeasParams zparams;
  float idepth_var_max_graph = 1e-2f;  // params.h:88-91 (syncGraph's preprocessing)
  float min_height = 0.1f, max_height = 4.0f;
  bool adaptive_data_weights = false;
};
struct Mat3 {
  float m[9];
  float operator()(int r, int c) const { return m[3 * r + c]; }
};


typedef std::map<uint32_t, std::shared_ptr<Frame> > FrameMap;

struct Case {
  int32_t width, height, n, n_pfs, cur_id, adaptive;
  float var_max, min_height, max_height, graph_scale;
  float K[9], Kinv[9];
  std::vector<uint32_t> pf_id;
  std::vector<float> pf_qt;  // 7 per pose-frame: pf.pose
  std::vector<FeatureWithIDepth> feats, feats_in_curr;
};

template <class T>
static bool read_n(FILE* f, T* p, size_t n) {
  return n == 0 || std::fread(p, sizeof(T), n, f) == n;
}
template <class T>
static void write_n(FILE* f, const T* p, size_t n) {
  if (n) std::fwrite(p, sizeof(T), n, f);
}

static bool load(const char* path, Case* c) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  char magic[4];
  bool ok = read_n(f, magic, 4) && std::memcmp(magic, "SEL1", 4) == 0 && read_n(f, &c->width, 6) && read_n(f, &c->var_max, 4);
  ok = ok && c->n >= 0 && c->n < (1 << 24) && c->n_pfs > 0 && c->n_pfs < 1024;
  if (ok) {
    c->pf_id.resize(c->n_pfs), c->pf_qt.resize(7 * (size_t)c->n_pfs);
    c->feats.resize(c->n), c->feats_in_curr.resize(c->n);
    ok = read_n(f, c->K, 9) && read_n(f, c->Kinv, 9) && read_n(f, c->pf_id.data(), c->pf_id.size()) &&
         read_n(f, c->pf_qt.data(), c->pf_qt.size()) && read_n(f, c->feats.data(), c->feats.size()) &&
         read_n(f, c->feats_in_curr.data(), c->feats_in_curr.size());
  }
  std::fclose(f);
  return ok;
}

static void dump_inputs(FILE* f, const flame_stereo_graph_inputs& g) {
  const int32_t head[6] = {g.V, g.num_examined, g.num_invalid, g.num_fail_var, g.num_fail_height, g.error_feature};
  write_n(f, head, 6);
  write_n(f, g.feat_id, (size_t)g.V);
  write_n(f, g.pos, 2 * (size_t)g.V);
  write_n(f, g.data_term, (size_t)g.V);
  write_n(f, g.data_weight, (size_t)g.V);
  write_n(f, g.feat_index, (size_t)g.V);
}

// What a synced graph holds: sizes, topology with feature ids, and the vertex state the sync left (download_state brings
// the solver state down: x of a survivor is what it was, x of a new vertex its data term).
struct Synced {
  int32_t V, E;
  std::vector<int32_t> src, dst, feat_id;
  std::vector<float> x, x_bar;
};
static Synced read_back(flame::optimizers::nltgv2_l1_graph_regularizer::hip::DeviceGraph* graph) {
  Synced s;
  flame_nltgv2_ctx* ctx = graph->handle();
  if (flame_nltgv2_graph_size(ctx, &s.V, &s.E) != 0) throw flame_hip::Error(FLAME_NLTGV2_ERR_INVALID_ARG, "graph_size");
  s.src.resize(s.E), s.dst.resize(s.E), s.feat_id.resize(s.V);
  if (flame_nltgv2_get_topology(ctx, s.src.data(), s.dst.data(), s.feat_id.data()) != 0)
    throw flame_hip::Error(FLAME_NLTGV2_ERR_INVALID_ARG, "get_topology");
  std::vector<std::vector<float> > vtx(11, std::vector<float>((size_t)s.V)), edge(5, std::vector<float>((size_t)s.E));
  std::vector<float> pos(2 * (size_t)s.V);
  flame_nltgv2_graph g;
  std::memset(&g, 0, sizeof g);
  g.V = s.V, g.E = s.E, g.pos = pos.data();
  g.x = vtx[0].data(), g.w1 = vtx[1].data(), g.w2 = vtx[2].data(), g.x_bar = vtx[3].data(), g.w1_bar = vtx[4].data();
  g.w2_bar = vtx[5].data(), g.x_prev = vtx[6].data(), g.w1_prev = vtx[7].data(), g.w2_prev = vtx[8].data();
  g.data_term = vtx[9].data(), g.data_weight = vtx[10].data();
  g.src = s.src.data(), g.dst = s.dst.data();
  g.alpha = edge[0].data(), g.beta = edge[1].data(), g.q1 = edge[2].data(), g.q2 = edge[3].data(), g.q3 = edge[4].data();
  if (flame_nltgv2_download_state(ctx, &g) != 0) throw flame_hip::Error(FLAME_NLTGV2_ERR_INVALID_ARG, "download_state");
  s.x = vtx[0], s.x_bar = vtx[3];
  return s;
}
static bool same(const Synced& a, const Synced& b) {
  return a.V == b.V && a.E == b.E && a.src == b.src && a.dst == b.dst && a.feat_id == b.feat_id &&
         std::memcmp(a.x.data(), b.x.data(), a.x.size() * sizeof(float)) == 0 &&
         std::memcmp(a.x_bar.data(), b.x_bar.data(), a.x_bar.size() * sizeof(float)) == 0;
}

// Uploads the first V0 selected vertices, triangulated, as a fresh graph with their feature ids.
static void seed(flame::optimizers::nltgv2_l1_graph_regularizer::hip::DeviceGraph* graph, const flame_stereo_graph_inputs& sel,
                 int32_t V0) {
  int32_t n_tri = 0, E = 0;
  if (flame_delaunay_triangulate(sel.pos, V0, nullptr, 0, &n_tri, nullptr, 0, &E) != 0)
    throw flame_hip::Error(FLAME_NLTGV2_ERR_INVALID_ARG, "triangulate");
  std::vector<int32_t> edges(2 * (size_t)E), src((size_t)E), dst((size_t)E);
  if (flame_delaunay_triangulate(sel.pos, V0, nullptr, 0, &n_tri, edges.data(), E, &E) != 0)
    throw flame_hip::Error(FLAME_NLTGV2_ERR_INVALID_ARG, "triangulate");
  for (int32_t e = 0; e < E; ++e) src[e] = edges[2 * e], dst[e] = edges[2 * e + 1];
  std::vector<float> pos(sel.pos, sel.pos + 2 * (size_t)V0), x(sel.data_term, sel.data_term + V0), zero((size_t)V0, 0.0f),
      weight(sel.data_weight, sel.data_weight + V0), one((size_t)E, 1.0f), qzero((size_t)E, 0.0f);
  std::vector<float> x_bar = x, x_prev = x, term = x, w1 = zero, w2 = zero, w1_bar = zero, w2_bar = zero, w1_prev = zero,
                     w2_prev = zero, beta = one, q1 = qzero, q2 = qzero, q3 = qzero;
  flame_nltgv2_graph g;
  std::memset(&g, 0, sizeof g);
  g.V = V0, g.E = E, g.pos = pos.data();
  g.x = x.data(), g.w1 = w1.data(), g.w2 = w2.data(), g.x_bar = x_bar.data(), g.w1_bar = w1_bar.data(), g.w2_bar = w2_bar.data();
  g.x_prev = x_prev.data(), g.w1_prev = w1_prev.data(), g.w2_prev = w2_prev.data();
  g.data_term = term.data(), g.data_weight = weight.data();
  g.src = src.data(), g.dst = dst.data(), g.alpha = one.data(), g.beta = beta.data();
  g.q1 = q1.data(), g.q2 = q2.data(), g.q3 = q3.data();
  if (flame_nltgv2_upload_graph(graph->handle(), &g) != 0) throw flame_hip::Error(FLAME_NLTGV2_ERR_INVALID_ARG, "upload_graph");
  if (flame_nltgv2_set_feature_ids(graph->handle(), sel.feat_id) != 0)
    throw flame_hip::Error(FLAME_NLTGV2_ERR_INVALID_ARG, "set_feature_ids");
}

int main(int argc, char** argv) {
  static_assert(sizeof(FeatureWithIDepth) == 40, "FeatureWithIDepth is 40 bytes");
  Case c;
  const bool have_case = argc > 2 && load(argv[1], &c);
  bool ok = true;
  try {
    if (!have_case) {  // still reach the device, so that a box without one says so
      const Mat3 K1 = {{256, 0, 160, 0, 256, 120, 0, 0, 1}};
      const Mat3 Ki = {{1 / 256.0f, 0, -0.625f, 0, 1 / 256.0f, -0.46875f, 0, 0, 1}};
      flame_hip::FeatureTracker probe(K1, Ki, 320, 240);
      std::printf("no case file\n");
      return 2;
    }
    Mat3 K, Kinv;
    std::memcpy(K.m, c.K, sizeof K.m);
    std::memcpy(Kinv.m, c.Kinv, sizeof Kinv.m);
    FlameParams params;
    params.idepth_var_max_graph = c.var_max, params.min_height = c.min_height, params.max_height = c.max_height;
    params.adaptive_data_weights = c.adaptive != 0;
    const flame_stereo_graph_params gp = flame_hip::toGraphParams(params);
    ok = ok && gp.idepth_var_max_graph == c.var_max && gp.min_height == c.min_height && gp.max_height == c.max_height &&
         gp.adaptive_data_weights == c.adaptive;
    FrameMap pfs;
    for (int k = 0; k < c.n_pfs; ++k) {
      std::shared_ptr<Frame> fr(new Frame());
      const float* p = &c.pf_qt[7 * (size_t)k];
      fr->id = c.pf_id[k];
      fr->pose = SE3{Quat{p[0], p[1], p[2], p[3]}, Vec3{{p[4], p[5], p[6]}}};
      pfs[fr->id] = fr;
    }
    Frame fcur;
    fcur.id = (uint32_t)c.cur_id;
    fcur.pose = SE3{Quat{1, 0, 0, 0}, Vec3{{0, 0, 0}}};
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 3;

    flame_hip::FeatureTracker tracker(K, Kinv, c.width, c.height);
    // 1. the form on the reference's two vectors
    const flame_stereo_graph_inputs g1 = tracker.selectGraphFeatures(params, pfs, c.graph_scale, c.feats, c.feats_in_curr);
    dump_inputs(out, g1);
    std::printf("selectGraphFeatures (feats, feats_in_curr): %d of %d selected: ok\n", g1.V, g1.num_examined);

    // 2. the resident form: refused before the projection, then on the two resident sets
    flame_stereo_set_features(tracker.handle(), c.n, c.n ? flame_hip::adoptFeatures(c.feats.data()) : nullptr);
    bool refused = false;
    try {
      tracker.selectGraphFeatures(params, pfs, c.graph_scale);
    } catch (const flame_hip::StereoError& e) {
      refused = e.status == FLAME_NLTGV2_ERR_INVALID_ARG;
    }
    const int kept = tracker.projectFeatures(params, pfs, fcur);
    const flame_stereo_graph_inputs g2 = tracker.selectGraphFeatures(params, pfs, c.graph_scale);
    dump_inputs(out, g2);
    std::printf("selectGraphFeatures (resident set): refused before projectFeatures %d; %d kept, %d selected: %s\n", (int)refused,
                kept, g2.V, refused && g2.num_examined == kept ? "ok" : "FAIL");
    ok = ok && refused && g2.num_examined == kept;

    // 3. getRawIDepths
    std::vector<Point2f> vertices;
    std::vector<float> mu, var;
    tracker.getRawIDepths(&vertices, &mu, &var);
    const int32_t n_raw = (int32_t)vertices.size();
    write_n(out, &n_raw, 1);
    write_n(out, vertices.data(), vertices.size());
    write_n(out, mu.data(), mu.size());
    write_n(out, var.data(), var.size());
    ok = ok && mu.size() == vertices.size() && var.size() == vertices.size();

    // 4. the selection's arrays into the regulariser as they are: pointer + count against the vector form
    int32_t n_tri = 0, n_edge = 0;
    std::vector<int32_t> edges;
    if (g2.V >= 6) {
      if (flame_delaunay_triangulate(g2.pos, g2.V, nullptr, 0, &n_tri, nullptr, 0, &n_edge) != 0) return 4;
      edges.resize(2 * (size_t)n_edge);
      if (flame_delaunay_triangulate(g2.pos, g2.V, nullptr, 0, &n_tri, edges.data(), n_edge, &n_edge) != 0) return 4;
    }
    flame::optimizers::nltgv2_l1_graph_regularizer::hip::DeviceGraph by_pointer, by_pointer_halves, by_vector;
    // every graph starts as the first half of the selection (a sync needs a graph), so that the sync below has survivors,
    // new vertices and new edges
    seed(&by_pointer, g2, g2.V / 2), seed(&by_pointer_halves, g2, g2.V / 2), seed(&by_vector, g2, g2.V / 2);
    by_pointer.sync(g2.V, g2.feat_id, g2.pos, g2.data_term, g2.data_weight, edges, false, nullptr, 0.0f, true);
    by_pointer_halves.syncPrepare(g2.V, g2.feat_id, g2.pos, g2.data_term, g2.data_weight, edges, false, nullptr, 0.0f, true);
    by_pointer_halves.syncCommit();
    const std::vector<int32_t> fid(g2.feat_id, g2.feat_id + g2.V);
    const std::vector<float> pos(g2.pos, g2.pos + 2 * (size_t)g2.V), term(g2.data_term, g2.data_term + g2.V),
        weight(g2.data_weight, g2.data_weight + g2.V);
    by_vector.sync(fid, pos, term, weight, edges, false, nullptr, 0.0f, true);
    const Synced a = read_back(&by_pointer), b = read_back(&by_pointer_halves), v = read_back(&by_vector);
    const bool good = same(a, v) && same(b, v) && v.V == g2.V && v.E == n_edge && v.feat_id == fid &&
                      std::memcmp(v.x.data(), g2.data_term, (size_t)g2.V * sizeof(float)) == 0;
    std::printf("sync / syncPrepare by pointer + count: V %d, E %d: %s\n", v.V, v.E, good ? "ok" : "FAIL");
    if (!good)
      std::printf("  sync == vector %d, prepare + commit == vector %d, V %d / %d, E %d / %d, ids %d, x == data terms %d\n", (int)same(a, v),
                  (int)same(b, v), v.V, g2.V, v.E, n_edge, (int)(v.feat_id == fid),
                  (int)(std::memcmp(v.x.data(), g2.data_term, (size_t)g2.V * sizeof(float)) == 0));
    ok = ok && good;
    const int32_t ve[2] = {v.V, v.E};
    write_n(out, ve, 2);
    write_n(out, v.feat_id.data(), v.feat_id.size());
    write_n(out, v.x.data(), v.x.size());
    write_n(out, v.x_bar.data(), v.x_bar.size());
    std::fclose(out);
  } catch (const flame_hip::StereoError& e) {
    std::printf("StereoError: %s (status %d, feature %d)\n", e.what(), e.status, e.feature);
    return e.status == FLAME_NLTGV2_ERR_NO_DEVICE ? 77 : 1;
  } catch (const flame_hip::Error& e) {
    std::printf("Error: %s\n", e.what());
    return 1;
  }
  return ok ? 0 : 1;
}
