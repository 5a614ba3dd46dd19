// FeatureTracker::drawDetections / getDebugImageDetections (include/flame_hip/feature_tracker.hpp) with look-alikes of the
// reference's own types, the way Flame::detectFeatures' caller would use it: with params.debug_draw_detections off nothing is
// drawn and false returned; with it on the bytes and the counters equal flame_stereo_draw_detections called by hand for the same
// 160x96 case (that entry point is checked against tests/detections_ref.py by tests/test_gpu_detections.py).
//   detections_test      exit 0: all equal; 77: no usable HIP device; 1: a difference
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "flame_hip/feature_tracker.hpp"

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
struct SE3 {  // Sophus::SE3f look-alike, translations only (all this test needs)
  Quat q;
  Vec3 t;
  const Quat& unit_quaternion() const { return q; }
  const Vec3& translation() const { return t; }
  SE3 inverse() const { return SE3{q, Vec3{{-t.v[0], -t.v[1], -t.v[2]}}}; }
  SE3 operator*(const SE3& b) const { return SE3{q, Vec3{{t.v[0] + b.t.v[0], t.v[1] + b.t.v[1], t.v[2] + b.t.v[2]}}}; }
};
struct Frame {
  uint32_t id;
  SE3 pose;
  std::vector<uint8_t> img;
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
struct FlameParams {  // the members of flame::Params the facade reads for this picture (params.h)
  float min_grad_mag = 5.0f;
  int detection_win_size = 16;
  float idepth_init = 0.01f, idepth_var_init = 0.25f;
  float min_baseline = 0.01f;
  bool do_letterbox = false;
  float rescale_factor_min = 0.7f, rescale_factor_max = 1.4f, idepth_var_max = 0.25f;
  int max_dropouts = 5;
  float outlier_sigma_thresh = 3.0f;
  bool do_meas_fusion = true;
  FilterParams fparams;
  MeasParams zparams;
  bool debug_draw_detections = false;
  bool debug_flip_images = false;
};
struct Mat3 {
  float m[9];
  float operator()(int r, int c) const { return m[3 * r + c]; }
};

static const int W = 160, H = 96;
static const float F = 131.25f;

static std::vector<uint8_t> render(float shift) {
  std::vector<uint8_t> img((size_t)W * H);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const double u = x - shift;
      float v = (float)(128.0 + 50.0 * std::sin(0.31 * u + 0.05 * y) * std::cos(0.23 * y - 0.02 * u) + 40.0 * std::sin(0.187 * u + 0.4) +
                        25.0 * std::cos(0.57 * y + 0.13 * u));
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
      img[(size_t)y * W + x] = (uint8_t)std::lrintf(v);
    }
  return img;
}

static bool same(const void* a, const void* b, size_t bytes, const char* what) {
  if (std::memcmp(a, b, bytes) == 0) return true;
  std::printf("FAIL: %s differs\n", what);
  return false;
}

int main() {
  const Mat3 K = {{F, 0, W / 2.0f, 0, F, H / 2.0f, 0, 0, 1}};
  const Mat3 Kinv = {{1 / F, 0, -(W / 2.0f) / F, 0, 1 / F, -(H / 2.0f) / F, 0, 0, 1}};
  const Quat I = {1, 0, 0, 0};
  Frame fprev{9, SE3{I, Vec3{{-0.03f, 0.002f, 0.01f}}}, render(2.0f)};
  Frame fref{10, SE3{I, Vec3{{0, 0, 0}}}, render(0.0f)};
  const size_t bytes = 3 * (size_t)W * H;
  try {
    flame_hip::FeatureTracker tracker(K, Kinv, W, H);
    tracker.addFrame(fprev.id, fprev.img.data(), W);
    tracker.addFrame(fref.id, fref.img.data(), W);
    FlameParams params;
    params.do_letterbox = true;

    // off: false, and not a byte written
    std::vector<uint8_t> img(bytes, 0xA5), untouched(bytes, 0xA5);
    flame_hip::DetectionsStats st;
    std::memset(&st, 0x5A, sizeof st);
    const flame_hip::DetectionsStats st_before = st;
    bool ok = !tracker.getDebugImageDetections(params, fref, fprev, img.data(), 0.005f, &st);
    ok = same(img.data(), untouched.data(), bytes, "the image with debug_draw_detections off") && ok;
    ok = same(&st, &st_before, sizeof st, "the stats with debug_draw_detections off") && ok;
    if (!ok) return 1;
    std::printf("switched off: ok\n");

    // on: the bytes of the C call, for the reference's literal max_score and for one that spreads the colours, flipped or not
    params.debug_draw_detections = true;
    const flame_stereo_params sp = flame_hip::toStereoParams(params);
    const flame_stereo_detect_params dp = flame_hip::toDetectParams(params);
    float q[4], t[3];
    flame_hip::toQuatTrans(fprev.pose.inverse() * fref.pose, q, t);
    for (int variant = 0; variant < 2; ++variant) {
      const float max_score = variant ? 64.0f : 0.005f;
      params.debug_flip_images = variant != 0;
      std::vector<uint8_t> want(bytes, 0);
      flame_stereo_detections_stats want_st;
      const int rc = flame_stereo_draw_detections(tracker.handle(), &sp, &dp, fref.id, q, t, max_score, variant, want.data(), &want_st);
      if (rc != 0 || want_st.num_scored <= 0 || want_st.num_scored > want_st.num_examined ||
          want_st.num_examined != (W - 8) * (H - 8 - 2 * (H / 3)) || want_st.error_pixel != -1) {
        std::printf("FAIL: flame_stereo_draw_detections: %d (%d of %d scored)\n", rc, want_st.num_scored, want_st.num_examined);
        return 1;
      }
      std::fill(img.begin(), img.end(), 0xA5);
      ok = tracker.getDebugImageDetections(params, fref, fprev, img.data(), max_score, &st);
      ok = same(img.data(), want.data(), bytes, "debug_img_detections") && ok;
      ok = same(&st, &want_st, sizeof st, "the stats") && ok;
      if (!ok) return 1;
      std::printf("detections image (max_score %g, flip %d, %d of %d scored): ok\n", max_score, variant, st.num_scored,
                  st.num_examined);
    }

    // an error of the C call comes up as StereoError
    bool threw = false;
    try {
      tracker.drawDetections(params, fref, fprev, false, img.data(), -1.0f);
    } catch (const flame_hip::StereoError& e) {
      threw = e.status == FLAME_NLTGV2_ERR_INVALID_ARG;
    }
    if (!threw) {
      std::printf("FAIL: a negative max_score went through\n");
      return 1;
    }
    std::printf("errors: ok\n");
    return 0;
  } catch (const flame_hip::StereoError& e) {
    if (e.status == FLAME_NLTGV2_ERR_NO_DEVICE) {
      std::printf("%s\n", e.what());
      return 77;
    }
    std::printf("FAIL: %s\n", e.what());
    return 1;
  }
}
