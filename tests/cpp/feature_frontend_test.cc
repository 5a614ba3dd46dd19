// tests/cpp/feature_frontend_test.cc -- the projectFeatures / detectFeatures part of include/flame_hip/feature_tracker.hpp
// used with look-alikes of the reference's own types (Params with detection members, a Frame with id + SE3 pose, a map of
// shared frames, FeatureWithIDepth, cv::Point2f), the way Flame::update() and Flame::detectionLoop would call it.  The
// host-vector forms must equal the resident forms bit for bit; the results are checked against the closed form of a
// fronto-parallel wall.  Build+run: tests/test_feature_frontend.py.  Exit code 0 = pass, 77 = no usable HIP device.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "flame_hip/feature_tracker.hpp"

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
};
struct Mat3 {
  float m[9];
  float operator()(int r, int c) const { return m[3 * r + c]; }
};

// A fronto-parallel textured wall at depth Z seen by cameras translated by (tx, 0, 0): view(u) = tex(u.x + f tx / Z).
static const int W = 320, H = 240;
static const float F = 262.5f, Z = 2.0f;
static float tex(double x, double y) {
  return (float)(128.0 + 50.0 * std::sin(0.31 * x + 0.05 * y) * std::cos(0.23 * y - 0.02 * x) + 40.0 * std::sin(0.11 * x * 1.7 + 0.4) +
                 25.0 * std::cos(0.57 * y + 0.13 * x));
}
static std::vector<uint8_t> render(float tx) {
  std::vector<uint8_t> img((size_t)W * H);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      float v = tex(x - F * tx / Z, y);
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
      img[(size_t)y * W + x] = (uint8_t)std::lrintf(v);
    }
  return img;
}

template <class F>
static bool same_records(const std::vector<F>& a, const std::vector<F>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(F)) == 0);
}

int main() {
  const Mat3 K = {{F, 0, W / 2.0f, 0, F, H / 2.0f, 0, 0, 1}};
  const Mat3 Kinv = {{1 / F, 0, -(W / 2.0f) / F, 0, 1 / F, -(H / 2.0f) / F, 0, 0, 1}};
  const Quat I = {1, 0, 0, 0};
  // camera poses in the world: 9 (the frame before pose-frame 10), pose-frame 10, current frame 12
  const float cam_x[3] = {-0.03f, 0.0f, 0.12f};
  std::shared_ptr<Frame> fr[3];
  for (int k = 0; k < 3; ++k) {
    fr[k].reset(new Frame());
    fr[k]->id = k == 0 ? 9 : (k == 1 ? 10 : 12);
    fr[k]->pose = SE3{I, Vec3{{cam_x[k], 0, 0}}};
    fr[k]->img = render(-cam_x[k]);
  }
  std::map<uint32_t, std::shared_ptr<Frame>> pfs;
  pfs[10] = fr[1];
  const Frame &fprev = *fr[0], &fref = *fr[1], &fcur = *fr[2];
  FlameParams params;
  bool ok = true;
  try {
    flame_hip::FeatureTracker tracker(K, Kinv, W, H);
    for (int k = 0; k < 3; ++k) tracker.addFrame(fr[k]->id, fr[k]->img.data(), W);

    // detectFeatures, host form: no map, a mask of two points
    std::vector<Point2f> curr_feats = {{40.5f, 40.5f}, {200.0f, 100.0f}};
    uint32_t feat_count = 100;
    std::vector<FeatureWithIDepth> new_feats;
    tracker.detectFeatures(params, fref, fprev, nullptr, curr_feats, &feat_count, &new_feats);
    bool good = !new_feats.empty() && feat_count == 100 + new_feats.size();
    for (size_t i = 0; i < new_feats.size(); ++i) {
      const FeatureWithIDepth& f = new_feats[i];
      good = good && f.id == 100 + i && f.frame_id == 10 && f.valid && f.idepth_mu == params.idepth_init &&
             f.idepth_var == params.idepth_var_init && f.xy.x >= 4 && f.xy.x < W - 4 && f.xy.y >= 4 && f.xy.y < H - 4 &&
             f.xy.x == std::floor(f.xy.x) && !((int)f.xy.x / 16 == 2 && (int)f.xy.y / 16 == 2) &&
             !((int)f.xy.x / 16 == 12 && (int)f.xy.y / 16 == 6);
      if (i > 0) {  // row-major cell order
        const FeatureWithIDepth& p = new_feats[i - 1];
        good = good && ((int)p.xy.y / 16 < (int)f.xy.y / 16 ||
                        ((int)p.xy.y / 16 == (int)f.xy.y / 16 && (int)p.xy.x / 16 < (int)f.xy.x / 16));
      }
    }
    std::printf("detectFeatures (host form): %d new features, ids 100.., masked cells empty: %s\n", (int)new_feats.size(),
                good ? "ok" : "BAD");
    ok = ok && good;

    // the same through the resident form, with a map of the wall's inverse depth on the device side of the call
    // (host map here: the resident form takes device pointers only, so the host form is run with the map first)
    std::vector<float> map((size_t)W * H, 1.0f / Z);
    for (size_t i = 0; i < map.size(); i += 3) map[i] = NAN;
    uint32_t c1 = 0, c2 = 0;
    std::vector<FeatureWithIDepth> with_map;
    tracker.detectFeatures(params, fref, fprev, map.data(), std::vector<Point2f>(), &c1, &with_map);
    flame_stereo_set_features(tracker.handle(), 0, nullptr);
    const int n_res = tracker.detectFeaturesResident(params, fref, fprev, nullptr, false, &c2);
    std::vector<FeatureWithIDepth> resident(n_res);
    int got = 0;
    flame_stereo_get_features(tracker.handle(), n_res, flame_hip::adoptFeatures(resident.data()), &got);
    int from_map = 0;
    good = n_res == (int)with_map.size() && c1 == c2 && c2 == (uint32_t)n_res;
    for (int i = 0; good && i < n_res; ++i) {
      const FeatureWithIDepth &a = with_map[i], &b = resident[i];
      good = a.id == b.id && a.xy.x == b.xy.x && a.xy.y == b.xy.y && b.idepth_mu == params.idepth_init;
      const bool hole = std::isnan(map[(size_t)a.xy.y * W + (size_t)a.xy.x]);
      good = good && a.idepth_mu == (hole ? params.idepth_init : 1.0f / Z);
      from_map += !hole;
    }
    std::printf("detectFeatures host map vs resident form: %d features, %d from the map: %s\n", n_res, from_map,
                good && from_map > 0 ? "ok" : "BAD");
    ok = ok && good && from_map > 0;

    // projectFeatures: the detected features at the wall's inverse depth, projected into frame 12 (camera 0.12 to the
    // right: the wall moves by -F * 0.12 / Z pixels); host form and resident form
    std::vector<FeatureWithIDepth> feats = with_map;
    for (size_t i = 0; i < feats.size(); ++i) feats[i].idepth_mu = 1.0f / Z, feats[i].num_updates = 3;
    feats[1].valid = false;
    std::vector<FeatureWithIDepth> kept = feats, in_curr;
    tracker.projectFeatures(params, pfs, fcur, &kept, &in_curr);
    good = !kept.empty() && kept.size() < feats.size() - 1 && in_curr.size() == kept.size();
    for (size_t i = 0; good && i < kept.size(); ++i) {
      const float dx = in_curr[i].xy.x - (kept[i].xy.x - F * 0.12f / Z);
      good = kept[i].valid && in_curr[i].id == kept[i].id && in_curr[i].frame_id == 12 && std::fabs(dx) < 1e-3f &&
             in_curr[i].xy.x >= 4 && in_curr[i].num_updates == 3 && std::fabs(in_curr[i].idepth_mu - 1.0f / Z) < 1e-6f &&
             kept[i].id != feats[1].id;
    }
    flame_stereo_set_features(tracker.handle(), (int)feats.size(), flame_hip::adoptFeatures(feats.data()));
    const int n_kept = tracker.projectFeatures(params, pfs, fcur);
    std::vector<FeatureWithIDepth> kept2(n_kept), in_curr2(n_kept);
    flame_stereo_get_features(tracker.handle(), n_kept, flame_hip::adoptFeatures(kept2.data()), &got);
    flame_stereo_get_projected(tracker.handle(), n_kept, flame_hip::adoptFeatures(in_curr2.data()), &got);
    good = good && same_records(kept, kept2) && same_records(in_curr, in_curr2);
    std::printf("projectFeatures: %d of %d kept, shifted by -F t / Z, host form == resident form: %s\n", (int)kept.size(),
                (int)feats.size(), good ? "ok" : "BAD");
    ok = ok && good;

    // the resident form of detection masked by the projected set: no new feature in a cell a projected feature covers
    uint32_t c3 = 1000;
    const int n_new = tracker.detectFeaturesResident(params, fcur, fref, nullptr, true, &c3);
    std::vector<FeatureWithIDepth> all(n_kept + n_new);
    flame_stereo_get_features(tracker.handle(), (int)all.size(), flame_hip::adoptFeatures(all.data()), &got);
    good = n_new > 0 && got == n_kept + n_new && std::memcmp(all.data(), kept2.data(), n_kept * sizeof(FeatureWithIDepth)) == 0;
    for (int i = n_kept; good && i < got; ++i)
      for (int j = 0; good && j < n_kept; ++j)
        good = !((int)(in_curr2[j].xy.x / 16) == (int)all[i].xy.x / 16 && (int)(in_curr2[j].xy.y / 16) == (int)all[i].xy.y / 16);
    std::printf("detectFeatures masked by the projected set: %d new after %d kept: %s\n", n_new, n_kept, good ? "ok" : "BAD");
    ok = ok && good;

    // errors: an unknown pose-frame on projection
    std::vector<FeatureWithIDepth> bad = feats, bad_curr;
    bad[5].frame_id = 77;
    try {
      tracker.projectFeatures(params, pfs, fcur, &bad, &bad_curr);
      std::printf("unknown frame: no exception BAD\n");
      ok = false;
    } catch (const flame_hip::StereoError& e) {
      std::printf("unknown frame: StereoError status %d feature %d %s\n", e.status, e.feature,
                  (e.status == FLAME_NLTGV2_ERR_INVALID_ARG && e.feature == 5) ? "ok" : "BAD");
      ok = ok && e.status == FLAME_NLTGV2_ERR_INVALID_ARG && e.feature == 5;
    }
  } catch (const flame_hip::StereoError& e) {
    std::printf("StereoError: %s (status %d)\n", e.what(), e.status);
    return e.status == FLAME_NLTGV2_ERR_NO_DEVICE ? 77 : 1;
  }
  return ok ? 0 : 1;
}
