// DeviceGraph::debugImagesBegin / End, FeatureTracker::drawFeatures and ::frameImageDevice (include/flame_hip/) round trip: reads a
// case the Python test dumped (graph with its w1 / w2, triangles, K, the grey image in a buffer wider than the image, features, and
// the pictures the Python mirror obtained for them), goes through the facades and compares byte for byte.
//   debug_images_test <case file>      exit 0: all equal; 77: no usable HIP device; 1: a difference or a bad file
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "flame_hip/feature_tracker.hpp"
#include "flame_hip/nltgv2_l1_graph_regularizer.hpp"

namespace reg = flame::optimizers::nltgv2_l1_graph_regularizer::hip;

// ---- look-alikes of the reference types the template binding touches (test-only; every pose is the identity) ----
struct Quat {
  float w() const { return 1.0f; }
  float x() const { return 0.0f; }
  float y() const { return 0.0f; }
  float z() const { return 0.0f; }
};
struct Vec3 {
  float operator()(int) const { return 0.0f; }
};
struct Pose {
  Quat q;
  Vec3 t;
  const Quat& unit_quaternion() const { return q; }
  const Vec3& translation() const { return t; }
  Pose inverse() const { return *this; }
  Pose operator*(const Pose&) const { return *this; }
};
struct Frame {
  uint32_t id;
  Pose pose;
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
  float min_baseline = 0.01f;
  bool do_letterbox = false;
  float rescale_factor_min = 0.7f, rescale_factor_max = 1.4f, idepth_var_max = 0.25f;
  int max_dropouts = 5;
  float outlier_sigma_thresh = 3.0f;
  bool do_meas_fusion = true;
  FilterParams fparams;
  MeasParams zparams;
  float idepth_var_max_graph = 1e-2f;  // params.h:88
  float scene_color_scale = 1.0f;      // params.h:109
  bool debug_flip_images = false;
};
struct Mat3 {
  float m[9];
  float operator()(int r, int c) const { return m[3 * r + c]; }
};

template <class T>
static bool take(std::FILE* f, std::vector<T>* v, size_t n) {
  v->resize(n);
  return n == 0 || std::fread(v->data(), sizeof(T), n, f) == n;
}

static bool same(const void* a, const void* b, size_t bytes, const char* what) {
  if (a && (bytes == 0 || std::memcmp(a, b, bytes) == 0)) return true;
  std::printf("FAIL: %s differs\n", what);
  return false;
}

int main(int argc, char** argv) {
  reg::DebugImageParams defaults;
  if (defaults.scene_color_scale != 1.0f || defaults.debug_flip_images != 0 || defaults.debug_draw_idepthmap != 1 ||
      defaults.debug_draw_normals != 1) {
    std::printf("FAIL: defaults\n");
    return 1;
  }
  if (argc < 2) {
    std::printf("usage: debug_images_test <case file>\n");
    return 1;
  }
  try {
    reg::DeviceGraph d(0);
    std::FILE* f = std::fopen(argv[1], "rb");
    char magic[4];
    int32_t hdr[10];  // V, E, T, rows, cols, step, n_feats, flip, num_converged, num_unconverged
    float sc[3];      // graph_scale, scene_color_scale, idepth_var_max_graph
    bool ok = f && std::fread(magic, 1, 4, f) == 4 && std::memcmp(magic, "DBG1", 4) == 0 && std::fread(hdr, sizeof(int32_t), 10, f) == 10 &&
              std::fread(sc, sizeof(float), 3, f) == 3;
    if (!ok) {
      std::printf("FAIL: cannot read %s\n", argv[1]);
      return 1;
    }
    const size_t V = hdr[0], E = hdr[1], T = hdr[2], n = static_cast<size_t>(hdr[3]) * hdr[4], NF = hdr[6];
    const int rows = hdr[3], cols = hdr[4], step = hdr[5];
    std::vector<float> K, Kinv, pos, x, w1, w2, alpha, beta, w1_map, w2_map;
    std::vector<int32_t> src, dst, tris;
    std::vector<uint8_t> gray, idepth_img, normals_img, features_img;
    std::vector<FeatureWithIDepth> feats, in_curr;
    ok = take(f, &K, 9) && take(f, &Kinv, 9) && take(f, &pos, 2 * V) && take(f, &x, V) && take(f, &w1, V) && take(f, &w2, V) &&
         take(f, &src, E) && take(f, &dst, E) && take(f, &alpha, E) && take(f, &beta, E) && take(f, &tris, 3 * T) &&
         take(f, &gray, static_cast<size_t>(rows) * step) && take(f, &feats, NF) && take(f, &idepth_img, 3 * n) &&
         take(f, &normals_img, 3 * n) && take(f, &w1_map, n) && take(f, &w2_map, n) && take(f, &features_img, 3 * n);
    std::fclose(f);
    if (!ok) {
      std::printf("FAIL: short file\n");
      return 1;
    }
    flame_hip::FlatGraph g;
    g.vertices.resize(V), g.edges.resize(E);
    for (size_t v = 0; v < V; ++v) {
      g.vertices[v].pos_x = pos[2 * v], g.vertices[v].pos_y = pos[2 * v + 1];
      g.vertices[v].x = g.vertices[v].x_bar = g.vertices[v].data_term = x[v];
      g.vertices[v].w1 = g.vertices[v].w1_bar = w1[v], g.vertices[v].w2 = g.vertices[v].w2_bar = w2[v];
    }
    for (size_t e = 0; e < E; ++e) g.edges[e].source = src[e], g.edges[e].target = dst[e], g.edges[e].alpha = alpha[e], g.edges[e].beta = beta[e];
    d.upload(g);
    reg::DebugImageParams dp;
    dp.scene_color_scale = sc[1], dp.debug_flip_images = hdr[7];
    const uint8_t* img = gray.data() + 7;  // (the image starts 7 bytes into each row of the buffer)

    // the pictures beside the map: interpolateMeshBegin, debugImagesBegin, the two Ends
    d.interpolateMeshBegin(tris, rows, cols, sc[0]);
    d.debugImagesBegin(img, nullptr, step, K.data(), dp, rows, cols);
    const float* dense = nullptr;
    d.interpolateMeshEnd(&dense);
    reg::DebugImages out = d.debugImagesEnd();
    ok = out.rows == rows && out.cols == cols;
    ok = same(out.debug_img_idepthmap, idepth_img.data(), 3 * n, "debug_img_idepthmap") && ok;
    ok = same(out.debug_img_normals, normals_img.data(), 3 * n, "debug_img_normals") && ok;
    ok = same(out.w1_map, w1_map.data(), sizeof(float) * n, "w1_map") && ok;
    ok = same(out.w2_map, w2_map.data(), sizeof(float) * n, "w2_map") && ok;
    if (!ok) return 1;
    std::printf("debug images, host image: ok\n");

    // drawFeatures over the resident frame, and the same frame's device image under the map's pictures
    const Mat3 Km = {{K[0], K[1], K[2], K[3], K[4], K[5], K[6], K[7], K[8]}};
    const Mat3 Kim = {{Kinv[0], Kinv[1], Kinv[2], Kinv[3], Kinv[4], Kinv[5], Kinv[6], Kinv[7], Kinv[8]}};
    flame_hip::FeatureTracker tracker(Km, Kim, cols, rows);
    tracker.addFrame(11, img, step);
    std::map<uint32_t, std::shared_ptr<Frame> > pfs;
    pfs[10] = std::make_shared<Frame>();
    pfs[10]->id = 10;
    Frame fcur;
    fcur.id = 11;
    FlameParams params;
    params.idepth_var_max_graph = sc[2], params.scene_color_scale = sc[1], params.debug_flip_images = hdr[7] != 0;
    tracker.projectFeatures(params, pfs, fcur, &feats, &in_curr);
    std::vector<uint8_t> drawn(3 * n);
    int nc = -1, nu = -1;
    tracker.drawFeatures(params, fcur.id, drawn.data(), &nc, &nu);
    ok = nc == hdr[8] && nu == hdr[9] && nc + nu == static_cast<int>(in_curr.size());
    if (!ok) std::printf("FAIL: counters (%d converged, %d not, %d projected)\n", nc, nu, static_cast<int>(in_curr.size()));
    ok = same(drawn.data(), features_img.data(), 3 * n, "debug_img_features") && ok;
    if (!ok) return 1;
    std::printf("features image: ok\n");

    int dev_step = 0;
    const void* dev_img = tracker.frameImageDevice(fcur.id, &dev_step);
    out = d.debugImages(nullptr, dev_img, dev_step, K.data(), dp, rows, cols);
    ok = dev_img != nullptr && dev_step >= cols;
    ok = same(out.debug_img_idepthmap, idepth_img.data(), 3 * n, "debug_img_idepthmap (device image)") && ok;
    ok = same(out.debug_img_normals, normals_img.data(), 3 * n, "debug_img_normals (device image)") && ok;
    if (!ok) return 1;
    std::printf("debug images, device image: ok\n");

    bool threw = false;
    try {
      d.debugImagesBegin(img, dev_img, step, K.data(), dp, rows, cols);
    } catch (const flame_hip::Error& e) {
      threw = e.status == FLAME_NLTGV2_ERR_INVALID_ARG;
    }
    if (!threw) {
      std::printf("FAIL: both image pointers were accepted\n");
      return 1;
    }
    std::printf("both image pointers refused: ok\n");
    return 0;
  } catch (const flame_hip::Error& e) {
    if (e.status == FLAME_NLTGV2_ERR_NO_DEVICE) {
      std::printf("%s\n", e.what());
      return 77;
    }
    std::printf("FAIL: %s\n", e.what());
    return 1;
  }
}
