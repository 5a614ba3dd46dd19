// tests/cpp/prune_pose_frames_test.cc -- prunePoseFrames of include/flame_hip/feature_tracker.hpp used with look-alikes of the
// reference's own types (Params, a Frame with id + SE3 pose, a std::map of shared frames, FeatureWithIDepth), the way a
// front-end would call it where the reference calls Flame::prunePoseFrames(pfs_to_keep).  The case (camera, pose-frames,
// pfs_to_keep, features, first_new) and the result the Python mirror obtained for it come from a file written by
// tests/test_prune_pose_frames_cpp.py; both reference-shaped calls (resident set, two host vectors) must reproduce it bit
// for bit, the call must be refused when the current pose-frame is not kept, and the dropped entries must leave the map.
// In the file the target pose-frame has the identity pose and every other pose-frame the relative pose towards it, so that
// target.pose.inverse() * pf.pose of the look-alike SE3 is exactly the pair the mirror passed.
// Exit code 0 = pass, 77 = no usable HIP device.
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


typedef std::map<uint32_t, std::shared_ptr<Frame> > FrameMap;

struct Case {
  int32_t width, height, n, first_new, n_pfs, n_keep_list, curr_pf, letterbox, n_out;
  float K[9], Kinv[9];
  std::vector<uint32_t> pf_id;
  std::vector<float> pf_qt;  // 7 per pose-frame
  std::vector<uint32_t> keep_list;
  std::vector<FeatureWithIDepth> in, out;
  int32_t stats[7];
};

template <class T>
static bool read_n(FILE* f, T* p, size_t n) {
  return n == 0 || std::fread(p, sizeof(T), n, f) == n;
}

static bool load(const char* path, Case* c) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  char magic[4];
  bool ok = read_n(f, magic, 4) && std::memcmp(magic, "PRN1", 4) == 0 && read_n(f, &c->width, 9);
  ok = ok && c->n >= 0 && c->n < (1 << 24) && c->n_out >= 0 && c->n_out <= c->n && c->n_pfs > 0 && c->n_pfs < 1024 &&
       c->n_keep_list >= 0 && c->n_keep_list < 1024 && c->first_new >= 0 && c->first_new <= c->n;
  if (ok) {
    c->pf_id.resize(c->n_pfs), c->pf_qt.resize(7 * (size_t)c->n_pfs), c->keep_list.resize(c->n_keep_list);
    c->in.resize(c->n), c->out.resize(c->n_out);
    ok = read_n(f, c->K, 9) && read_n(f, c->Kinv, 9) && read_n(f, c->pf_id.data(), c->pf_id.size()) &&
         read_n(f, c->pf_qt.data(), c->pf_qt.size()) && read_n(f, c->keep_list.data(), c->keep_list.size()) &&
         read_n(f, c->in.data(), c->in.size()) && read_n(f, c->out.data(), c->out.size()) && read_n(f, c->stats, 7);
  }
  std::fclose(f);
  return ok;
}

static FrameMap make_map(const Case& c) {
  FrameMap pfs;
  for (int k = 0; k < c.n_pfs; ++k) {
    std::shared_ptr<Frame> fr(new Frame());
    const float* p = &c.pf_qt[7 * (size_t)k];
    fr->id = c.pf_id[k];
    fr->pose = SE3{Quat{p[0], p[1], p[2], p[3]}, Vec3{{p[4], p[5], p[6]}}};
    pfs[fr->id] = fr;
  }
  return pfs;
}

template <class F>
static bool same_records(const std::vector<F>& a, const std::vector<F>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(F)) == 0);
}

static bool same_stats(const flame_stereo_prune_stats& s, const int32_t* e, int frames_dropped) {
  return s.num_examined == e[0] && s.num_moved == e[1] && s.num_invalidated == e[2] && s.num_removed == e[3] &&
         s.num_features == e[4] && s.num_frames_dropped == frames_dropped && s.error_feature == e[6];
}

int main(int argc, char** argv) {
  static_assert(sizeof(FeatureWithIDepth) == 40, "FeatureWithIDepth is 40 bytes");
  Case c;
  const bool have_case = argc > 1 && load(argv[1], &c);
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
    params.do_letterbox = c.letterbox != 0;
    const std::vector<uint8_t> blank((size_t)c.width * c.height, 0);
    int n_kept = 0;
    {
      const FrameMap all = make_map(c);
      for (size_t i = 0; i < c.keep_list.size(); ++i) {
        bool dup = false;
        for (size_t j = 0; j < i; ++j) dup = dup || c.keep_list[j] == c.keep_list[i];
        n_kept += !dup && all.count(c.keep_list[i]) > 0;
      }
    }
    const int n_dropped = c.n_pfs - n_kept;

    // 1. refused: the current pose-frame is not in pfs_to_keep -> false, nothing changes
    {
      flame_hip::FeatureTracker tracker(K, Kinv, c.width, c.height);
      FrameMap pfs = make_map(c);
      for (FrameMap::const_iterator it = pfs.begin(); it != pfs.end(); ++it) tracker.addFrame(it->first, blank.data(), c.width);
      flame_stereo_set_features(tracker.handle(), c.n, flame_hip::adoptFeatures(c.in.data()));
      std::vector<uint32_t> without;
      for (size_t i = 0; i < c.keep_list.size(); ++i)
        if (c.keep_list[i] != (uint32_t)c.curr_pf) without.push_back(c.keep_list[i]);
      const bool r = tracker.prunePoseFrames(params, &pfs, *pfs[c.curr_pf], without, c.first_new);
      std::vector<FeatureWithIDepth> now(c.n);
      int got = 0;
      flame_stereo_get_features(tracker.handle(), c.n, flame_hip::adoptFeatures(now.data()), &got);
      std::vector<FeatureWithIDepth> a = c.in, b;
      const bool r2 = tracker.prunePoseFrames(params, &pfs, *pfs[c.curr_pf], without, &a, &b);
      const bool good = !r && !r2 && got == c.n && same_records(now, c.in) && same_records(a, c.in) && b.empty() &&
                        (int)pfs.size() == c.n_pfs && tracker.frameCount() == c.n_pfs;
      std::printf("current pose-frame not kept: refused, %d features and %d frames untouched: %s\n", got, tracker.frameCount(),
                  good ? "ok" : "FAIL");
      ok = ok && good;

      // 2. the resident form
      flame_stereo_prune_stats st;
      const bool r3 = tracker.prunePoseFrames(params, &pfs, *pfs[c.curr_pf], c.keep_list, c.first_new, &st);
      std::vector<FeatureWithIDepth> res(st.num_features > 0 ? st.num_features : 0);
      flame_stereo_get_features(tracker.handle(), (int)res.size(), res.empty() ? nullptr : flame_hip::adoptFeatures(res.data()), &got);
      bool erased = (int)pfs.size() == n_kept;
      for (FrameMap::const_iterator it = pfs.begin(); it != pfs.end(); ++it) {
        bool listed = false;
        for (size_t i = 0; i < c.keep_list.size(); ++i) listed = listed || c.keep_list[i] == it->first;
        erased = erased && listed;
      }
      const bool good2 = r3 && same_records(res, c.out) && same_stats(st, c.stats, n_dropped) && erased &&
                         tracker.frameCount() == n_kept;
      std::printf("prunePoseFrames (resident set): %d -> %d features, %d moved, %d invalidated, %d removed, map %d -> %d, frames %d: %s\n",
                  c.n, st.num_features, st.num_moved, st.num_invalidated, st.num_removed, c.n_pfs, (int)pfs.size(),
                  tracker.frameCount(), good2 ? "ok" : "FAIL");
      ok = ok && good2;
      tracker.clearFeatures();
      flame_stereo_get_features(tracker.handle(), 0, nullptr, &got);
      ok = ok && got == 0;
    }

    // 3. the two-vector form on a fresh map
    {
      flame_hip::FeatureTracker tracker(K, Kinv, c.width, c.height);
      FrameMap pfs = make_map(c);
      std::vector<FeatureWithIDepth> feats(c.in.begin(), c.in.begin() + c.first_new), new_feats(c.in.begin() + c.first_new, c.in.end());
      flame_stereo_prune_stats st;
      const bool r = tracker.prunePoseFrames(params, &pfs, *pfs[c.curr_pf], c.keep_list, &feats, &new_feats, &st);
      std::vector<FeatureWithIDepth> joined = feats;
      joined.insert(joined.end(), new_feats.begin(), new_feats.end());
      const bool good = r && (int)feats.size() == c.first_new && same_records(joined, c.out) && same_stats(st, c.stats, 0) &&
                        (int)pfs.size() == n_kept;
      std::printf("prunePoseFrames (feats, new_feats): %d + %d -> %d + %d: %s\n", c.first_new, c.n - c.first_new, (int)feats.size(),
                  (int)new_feats.size(), good ? "ok" : "FAIL");
      ok = ok && good;
    }
  } catch (const flame_hip::StereoError& e) {
    std::printf("StereoError: %s (status %d, feature %d)\n", e.what(), e.status, e.feature);
    return e.status == FLAME_NLTGV2_ERR_NO_DEVICE ? 77 : 1;
  }
  return ok ? 0 : 1;
}
