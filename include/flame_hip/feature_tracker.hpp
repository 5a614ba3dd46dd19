// flame_hip/feature_tracker.hpp -- header-only C++11 binding of include/flame_stereo.h, shaped after the call the
// reference makes per image:
//
//   reference  bool Flame::updateFeatureIDepths(params, K, Kinv, pfs, fnew, curr_pf, &feats, &stats, &debug_img)
//              (/root/reference/src/flame/flame.cc:1280-1288, call site flame.cc:265-267)
//   here       flame_hip::FeatureTracker tracker(K, Kinv, width, height);      // next to K_, Kinv_ (flame.h:520-523)
//              tracker.addFrame(frame->id, frame->img[0].data, frame->img[0].step);   // where Frame::create ran
//              bool ok = tracker.updateFeatureIDepths(params, pfs, *fnew_, *curr_pf_, &feats_, &stats);
//
//   reference  Flame::projectFeatures(params, K, Kinv, pfs, fcur, &feats, &feats_in_curr, &stats)  (flame.cc:1754, call
//              sites flame.cc:222 and 277)
//   here       tracker.projectFeatures(params, pfs, *fcur, &feats_, &feats_in_curr_);
//   reference  Flame::detectFeatures(params, K, Kinv, fref, fprev, fcmp, idepthmap, curr_feats, ...) + the feature
//              initialisation of Flame::detectionLoop (flame.cc:708-773)
//   here       tracker.detectFeatures(params, fref, fprev, idepthmap, curr_feats, &feat_count_, &new_feats);
//   (and the resident-set forms projectFeatures(params, pfs, fcur) / detectFeaturesResident(...), which keep the
//   features on the device)
//   reference  void Flame::prunePoseFrames(pfs_to_keep)  (flame.cc:554-706; on pfs_, curr_pf_, feats_, new_feats_)
//   here       tracker.prunePoseFrames(params, &pfs_, *curr_pf_, pfs_to_keep, first_new);            // resident set
//              tracker.prunePoseFrames(params, &pfs_, *curr_pf_, pfs_to_keep, &feats_, &new_feats_);  // host vectors
//   reference  the preprocessing of Flame::syncGraph (flame.cc:1954-1980: which features become vertices) and the data-term
//              lines of its vertex loops (flame.cc:2001-2004, 2041-2044)
//   here       flame_stereo_graph_inputs g = tracker.selectGraphFeatures(params, pfs_, graph_scale_);            // resident
//              ... = tracker.selectGraphFeatures(params, pfs_, graph_scale_, feats_, feats_in_curr_);           // vectors
//              g.feat_id / g.pos / g.data_term / g.data_weight go into DeviceGraph::syncPrepare as they are
//   reference  getDebugImageMatches() (flame.h:294-306): the picture updateFeatureIDepths draws into its debug_img argument when
//              params.debug_draw_matches is set (flame.cc:265-267, 1293-1295)
//   here       tracker.recordMatches(params.debug_draw_matches);                 // once, e.g. beside the constructor
//              tracker.updateFeatureIDepths(...);                                // any form
//              tracker.getDebugImageMatches(params, debug_img_matches_.data);    // height * width * 3 bytes
//   reference  getDebugImageDetections() (flame.h:294-306): the picture detectFeatures draws into its debug_img argument when
//              params.debug_draw_detections is set (flame.cc:1272-1275, drawDetections flame.cc:2363-2412)
//   here       tracker.getDebugImageDetections(params, fref, fprev, debug_img_detections_.data);   // beside detectFeatures
//   reference  Flame::getRawIDepths(&vertices, &idepths_mu, &idepths_var)  (flame.h:255-273)
//   here       tracker.getRawIDepths(&vertices, &idepths_mu, &idepths_var);
//
// Works with the reference's own types through templates (no Eigen/Sophus/OpenCV headers are needed here):
//   Matrix3    anything with operator()(row, col)                      (Eigen::Matrix3f)
//   SE3        .inverse(), operator*, .unit_quaternion().{w,x,y,z}(), .translation()(i)   (Sophus::SE3f)
//   Frame      .id, .pose                                               (utils::Frame, frame.h)
//   FrameMap   iterable of (id, pointer-to-Frame) pairs                 (FrameIDToFrame, flame.h:72);
//              prunePoseFrames also uses its find / count / erase (std::map)
//   Feature    layout of FeatureWithIDepth (flame.h:88-99); checked with static_asserts by adoptFeatures()
#ifndef FLAME_HIP_FEATURE_TRACKER_HPP_
#define FLAME_HIP_FEATURE_TRACKER_HPP_

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "flame_stereo.h"

namespace flame_hip {

typedef flame_stereo_matches_stats MatchesStats;  // what getDebugImageMatches drew, by kind (flame_stereo.h)
typedef flame_stereo_detections_stats DetectionsStats;  // what getDebugImageDetections scored (flame_stereo.h)

struct StereoError : std::runtime_error {
  int status;
  int feature;  // lowest failing feature index, or -1
  StereoError(int s, int f, const std::string& what)
      : std::runtime_error(what + ": " + flame_nltgv2_status_string(s)), status(s), feature(f) {}
};

// flame::Params -> flame_stereo_params (the members updateFeatureIDepths / trackFeature read, params.h:36-126).
template <class FlameParams>
inline flame_stereo_params toStereoParams(const FlameParams& p) {
  flame_stereo_params o;
  flame_stereo_default_params(&o);
  o.min_baseline = p.min_baseline;
  o.do_letterbox = p.do_letterbox ? 1 : 0;
  o.rescale_factor_min = p.rescale_factor_min;
  o.rescale_factor_max = p.rescale_factor_max;
  o.idepth_var_max = p.idepth_var_max;
  o.max_dropouts = p.max_dropouts;
  o.outlier_sigma_thresh = p.outlier_sigma_thresh;
  o.do_meas_fusion = p.do_meas_fusion ? 1 : 0;
  o.win_size = p.fparams.win_size;
  o.search_sigma = p.fparams.search_sigma;
  o.min_grad_mag = p.fparams.min_grad_mag;
  o.idepth_min = p.fparams.idepth_min;
  o.idepth_max = p.fparams.idepth_max;
  o.epilength_min = p.fparams.epilength_min;
  o.epilength_max = p.fparams.epilength_max;
  o.process_var_factor = p.fparams.process_var_factor;
  o.process_fail_var_factor = p.fparams.process_fail_var_factor;
  o.max_cost = p.fparams.sparams.max_cost;
  o.do_subpixel = p.fparams.sparams.do_subpixel ? 1 : 0;
  o.sample_dist = p.fparams.sparams.sample_dist;
  o.second_best_factor = p.fparams.sparams.second_best_factor;
  o.z_win_size = p.zparams.win_size;
  o.pixel_var = p.zparams.pixel_var;
  o.epipolar_line_var = p.zparams.epipolar_line_var;
  return o;
}

// flame::Params -> flame_stereo_detect_params (the members detectFeatures and detectionLoop read beyond
// toStereoParams: params.h:39, 48, 60, 61).  Note: Params::min_grad_mag, not fparams.min_grad_mag.
template <class FlameParams>
inline flame_stereo_detect_params toDetectParams(const FlameParams& p) {
  flame_stereo_detect_params o;
  flame_stereo_default_detect_params(&o);
  o.detection_win_size = p.detection_win_size;
  o.min_grad_mag = p.min_grad_mag;
  o.idepth_init = p.idepth_init;
  o.idepth_var_init = p.idepth_var_init;
  return o;
}

// flame::Params -> flame_stereo_graph_params (the members syncGraph's preprocessing reads, params.h:88-91).
template <class FlameParams>
inline flame_stereo_graph_params toGraphParams(const FlameParams& p) {
  flame_stereo_graph_params o;
  flame_stereo_default_graph_params(&o);
  o.idepth_var_max_graph = p.idepth_var_max_graph;
  o.min_height = p.min_height;
  o.max_height = p.max_height;
  o.adaptive_data_weights = p.adaptive_data_weights ? 1 : 0;
  return o;
}

// (quaternion, translation) of an SE3 into the C arrays of a flame_stereo_pose.
template <class SE3>
inline void toQuatTrans(const SE3& T, float q[4], float t[3]) {
  q[0] = T.unit_quaternion().w(), q[1] = T.unit_quaternion().x(), q[2] = T.unit_quaternion().y(),
  q[3] = T.unit_quaternion().z();
  t[0] = T.translation()(0), t[1] = T.translation()(1), t[2] = T.translation()(2);
}

// One pose table entry for pose-frame `pf`: the two relative poses the reference forms per feature
// (flame.cc:1315 and flame.cc:1614), formed once per pose-frame here.
template <class Frame>
inline flame_stereo_pose makePose(const Frame& pf, const Frame& fnew, const Frame& curr_pf) {
  flame_stereo_pose p;
  std::memset(&p, 0, sizeof p);
  p.frame_id = pf.id;
  toQuatTrans(fnew.pose.inverse() * pf.pose, p.q_ref_to_new, p.t_ref_to_new);
  toQuatTrans(curr_pf.pose.inverse() * pf.pose, p.q_ref_to_pf, p.t_ref_to_pf);
  return p;
}

// Reinterprets an array of the reference's FeatureWithIDepth as flame_stereo_feature after checking the layout.
template <class Feature>
inline flame_stereo_feature* adoptFeatures(Feature* feats) {
  static_assert(sizeof(Feature) == sizeof(flame_stereo_feature), "FeatureWithIDepth layout changed");
  static_assert(offsetof(Feature, frame_id) == offsetof(flame_stereo_feature, frame_id), "frame_id");
  static_assert(offsetof(Feature, xy) == offsetof(flame_stereo_feature, x), "xy");
  static_assert(offsetof(Feature, idepth_mu) == offsetof(flame_stereo_feature, idepth_mu), "idepth_mu");
  static_assert(offsetof(Feature, idepth_var) == offsetof(flame_stereo_feature, idepth_var), "idepth_var");
  static_assert(offsetof(Feature, valid) == offsetof(flame_stereo_feature, valid), "valid");
  static_assert(offsetof(Feature, num_updates) == offsetof(flame_stereo_feature, num_updates), "num_updates");
  static_assert(offsetof(Feature, num_dropouts) == offsetof(flame_stereo_feature, num_dropouts), "num_dropouts");
  static_assert(offsetof(Feature, search_status) == offsetof(flame_stereo_feature, search_status), "search_status");
  return reinterpret_cast<flame_stereo_feature*>(feats);
}

template <class Feature>
inline const flame_stereo_feature* adoptFeatures(const Feature* feats) {
  return adoptFeatures(const_cast<Feature*>(feats));
}

class FeatureTracker {
 public:
  template <class Matrix3>
  FeatureTracker(const Matrix3& K, const Matrix3& Kinv, int width, int height, int border = 5, int device = 0)
      : ctx_(nullptr) {
    float k[9], ki[9];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) k[3 * r + c] = K(r, c), ki[3 * r + c] = Kinv(r, c);
    check(flame_stereo_create(&ctx_, device), -1, "flame_stereo_create");
    const int rc = flame_stereo_set_camera(ctx_, k, ki, width, height, border);
    if (rc != 0) {
      flame_stereo_destroy(ctx_);
      ctx_ = nullptr;
      throw StereoError(rc, -1, "flame_stereo_set_camera");
    }
  }
  ~FeatureTracker() { flame_stereo_destroy(ctx_); }
  FeatureTracker(const FeatureTracker&) = delete;
  FeatureTracker& operator=(const FeatureTracker&) = delete;

  // utils::Frame::create, level 0 (frame.cc:33-71), on the device.  Call it where the reference creates fnew_
  // (flame.cc:150); a frame that becomes a pose-frame simply stays resident.
  void addFrame(uint32_t frame_id, const uint8_t* img, int row_stride_bytes) {
    check(flame_stereo_add_frame(ctx_, frame_id, img, row_stride_bytes), -1, "flame_stereo_add_frame");
  }
  // Where the front-end ran cv::cvtColor and cv::undistort before Flame::update: setInput once per camera (after the
  // constructor; flame_stereo_default_input_params fills the struct), then addRawFrame per frame with the frame as the camera
  // delivered it, in host memory (on_device false: waits, as addFrame) or in device memory (on_device true: with stats NULL
  // only enqueued -- the caller keeps `raw` alive and unchanged until the tracker's stream has passed it).
  void setInput(const flame_stereo_input_params& input) { check(flame_stereo_set_input(ctx_, &input), -1, "flame_stereo_set_input"); }
  void addRawFrame(uint32_t frame_id, const void* raw, int row_stride_bytes, bool on_device = false,
                   flame_stereo_input_stats* stats = nullptr) {
    check(flame_stereo_add_raw_frame(ctx_, frame_id, raw, row_stride_bytes, on_device ? 1 : 0, stats), -1,
          "flame_stereo_add_raw_frame");
  }
  // Refining a frame's pose against a pose-frame's map (flame_stereo.h, "direct image alignment"): after addFrame / addRawFrame of
  // the new frame and before updateFeatureIDepths, against curr_pf_ and the dense map that pose-frame kept.  buildPyramid once per
  // frame (enqueue-only), then alignFrame from the pose the caller has: T_ref_to_new = fnew.pose.inverse() * curr_pf.pose as
  // (q (w x y z), t) in double.  The refined pose comes back in `out` (double, and as the float32 values flame_stereo_pose takes).
  // The map is host memory (map_on_device false) or device memory read in place.  `trace` may be NULL.
  void buildPyramid(uint32_t frame_id, int n_levels) {
    check(flame_stereo_build_pyramid(ctx_, frame_id, n_levels), -1, "flame_stereo_build_pyramid");
  }
  flame_stereo_align_system alignLinearize(const flame_stereo_align_params& params, uint32_t ref_frame_id, uint32_t new_frame_id,
                                           int level, const float* idepthmap, bool map_on_device, const double q_ref_to_new[4],
                                           const double t_ref_to_new[3]) {
    flame_stereo_align_system out;
    std::memset(&out, 0, sizeof out);
    check(flame_stereo_align_linearize(ctx_, &params, ref_frame_id, new_frame_id, level, map_on_device ? nullptr : idepthmap,
                                       map_on_device ? idepthmap : nullptr, q_ref_to_new, t_ref_to_new, &out),
          -1, "flame_stereo_align_linearize");
    return out;
  }
  flame_stereo_align_result alignFrame(const flame_stereo_align_params& params, uint32_t ref_frame_id, uint32_t new_frame_id,
                                       const float* idepthmap, bool map_on_device, const double q_init[4], const double t_init[3],
                                       std::vector<flame_stereo_align_trace>* trace = nullptr, int max_trace = 256) {
    flame_stereo_align_result out;
    std::memset(&out, 0, sizeof out);
    int n = 0;
    if (trace) trace->resize((size_t)(max_trace > 0 ? max_trace : 0));
    const int rc = flame_stereo_align_frame(ctx_, &params, ref_frame_id, new_frame_id, map_on_device ? nullptr : idepthmap,
                                            map_on_device ? idepthmap : nullptr, q_init, t_init, &out,
                                            trace && max_trace > 0 ? trace->data() : nullptr, trace ? (max_trace > 0 ? max_trace : 0) : 0,
                                            &n);
    if (trace) trace->resize((size_t)(rc == 0 ? (n < max_trace ? n : (max_trace > 0 ? max_trace : 0)) : 0));
    check(rc, -1, "flame_stereo_align_frame");
    return out;
  }
  void dropFrame(uint32_t frame_id) { check(flame_stereo_drop_frame(ctx_, frame_id), -1, "flame_stereo_drop_frame"); }
  int frameCount() const { return flame_stereo_frame_count(ctx_); }

  // == Flame::updateFeatureIDepths (flame.cc:1280-1536).  Returns what the reference returns; `stats` (optional)
  // receives the counters the reference hands to StatsTracker (flame.cc:1497-1502).
  bool updateFeatureIDepths(const flame_stereo_params& params, uint32_t new_frame_id, uint32_t curr_pf_id,
                            const std::vector<flame_stereo_pose>& poses, flame_stereo_feature* feats, int n_feats,
                            flame_stereo_stats* stats = nullptr) {
    flame_stereo_stats local;
    flame_stereo_stats* st = stats ? stats : &local;
    const int rc = flame_stereo_update_feature_idepths(ctx_, &params, new_frame_id, curr_pf_id, (int)poses.size(),
                                                       poses.empty() ? nullptr : poses.data(), n_feats, feats, st);
    check(rc, st->error_feature, "flame_stereo_update_feature_idepths");
    return st->success != 0;
  }

  // The reference's argument list: pfs (id -> shared_ptr<Frame>), fnew, curr_pf, std::vector<FeatureWithIDepth>.
  template <class FlameParams, class FrameMap, class Frame, class Feature>
  bool updateFeatureIDepths(const FlameParams& params, const FrameMap& pfs, const Frame& fnew, const Frame& curr_pf,
                            std::vector<Feature>* feats, flame_stereo_stats* stats = nullptr) {
    std::vector<flame_stereo_pose> poses;
    for (typename FrameMap::const_iterator it = pfs.begin(); it != pfs.end(); ++it)
      poses.push_back(makePose(*it->second, fnew, curr_pf));
    return updateFeatureIDepths(toStereoParams(params), fnew.id, curr_pf.id, poses,
                                feats->empty() ? nullptr : adoptFeatures(feats->data()), (int)feats->size(), stats);
  }

  // ---- projectFeatures / detectFeatures ----
  // Resident forms: on the resident set (flame_stereo_set_features / update_resident), which stays on the device.
  // == Flame::projectFeatures on feats_; the projected set (feats_in_curr_) stays resident too (projected()).  Returns
  // the number of features kept.
  template <class FlameParams, class FrameMap, class Frame>
  int projectFeatures(const FlameParams& params, const FrameMap& pfs, const Frame& fcur) {
    std::vector<flame_stereo_pose> poses;
    for (typename FrameMap::const_iterator it = pfs.begin(); it != pfs.end(); ++it)
      poses.push_back(makePose(*it->second, fcur, fcur));  // (only the *_to_new half is read)
    const flame_stereo_params sp = toStereoParams(params);
    flame_stereo_feature_stats st;
    const int rc = flame_stereo_project_features(ctx_, &sp, fcur.id, (int)poses.size(), poses.empty() ? nullptr : poses.data(),
                                                 &st);
    check(rc, st.error_feature, "flame_stereo_project_features");
    return st.num_features;
  }
  // == Flame::detectFeatures + detectionLoop's initialisation; the new features are appended to the resident set with
  // ids *feat_count, *feat_count + 1, ... (feat_count_++).  idepthmap_device: width x height floats on the device, or
  // NULL; mask_with_projected: the projected set of the last projectFeatures as curr_feats (else no mask).  Returns the
  // number of new features.
  template <class FlameParams, class Frame>
  int detectFeaturesResident(const FlameParams& params, const Frame& fref, const Frame& fprev, const void* idepthmap_device,
                             bool mask_with_projected, uint32_t* feat_count) {
    return detect(params, fref, fprev, nullptr, idepthmap_device, mask_with_projected ? -1 : 0, nullptr, feat_count);
  }

  // Host forms, in the reference's argument shape (they use the resident set as their working storage: it holds `feats`
  // after projectFeatures and the new features after detectFeatures).
  template <class FlameParams, class FrameMap, class Frame, class Feature>
  void projectFeatures(const FlameParams& params, const FrameMap& pfs, const Frame& fcur, std::vector<Feature>* feats,
                       std::vector<Feature>* feats_in_curr) {
    check(flame_stereo_set_features(ctx_, (int)feats->size(), feats->empty() ? nullptr : adoptFeatures(feats->data())), -1,
          "flame_stereo_set_features");
    const int n = projectFeatures(params, pfs, fcur);
    feats->resize(n);
    feats_in_curr->resize(n);
    int got = 0;
    check(flame_stereo_get_features(ctx_, n, n ? adoptFeatures(feats->data()) : nullptr, &got), -1, "flame_stereo_get_features");
    check(flame_stereo_get_projected(ctx_, n, n ? adoptFeatures(feats_in_curr->data()) : nullptr, &got), -1,
          "flame_stereo_get_projected");
  }
  // idepthmap: width x height floats in host memory (the reference's fref.idepthmap[0]), or NULL (all NaN).
  // curr_feats: anything with .x / .y per element (std::vector<cv::Point2f>).  new_feats receives the
  // FeatureWithIDepth's the detection loop would push into new_feats_.
  template <class FlameParams, class Frame, class Point, class Feature>
  void detectFeatures(const FlameParams& params, const Frame& fref, const Frame& fprev, const float* idepthmap,
                      const std::vector<Point>& curr_feats, uint32_t* feat_count, std::vector<Feature>* new_feats) {
    std::vector<float> mask(2 * curr_feats.size());
    for (size_t i = 0; i < curr_feats.size(); ++i) mask[2 * i] = curr_feats[i].x, mask[2 * i + 1] = curr_feats[i].y;
    check(flame_stereo_set_features(ctx_, 0, nullptr), -1, "flame_stereo_set_features");
    const int n = detect(params, fref, fprev, idepthmap, nullptr, (int)curr_feats.size(), mask.empty() ? nullptr : mask.data(),
                         feat_count);
    new_feats->resize(n);
    int got = 0;
    check(flame_stereo_get_features(ctx_, n, n ? adoptFeatures(new_feats->data()) : nullptr, &got), -1,
          "flame_stereo_get_features");
  }

  // ---- getDebugImageFeatures ----
  // == Flame::drawFeatures(params, fnew_->img[0], feats_in_curr_, &stats_, &debug_img_features_) (flame.cc:2459-2510, call site
  // flame.cc:292-295) on the projected set of the last projectFeatures over the resident frame `fcur_id`; the image never
  // comes down and goes up again.  debug_img: height * width * 3 bytes (cv::Vec3b, c[0], c[1], c[2]).  The text overlay
  // (debug_draw_text_overlay) is not drawn; its two counters are returned instead.
  void drawFeatures(uint32_t fcur_id, float idepth_var_max_graph, float scene_color_scale, bool debug_flip_images,
                    uint8_t* debug_img, int* num_converged = nullptr, int* num_unconverged = nullptr) {
    int32_t nc = 0, nu = 0;
    check(flame_stereo_draw_features(ctx_, fcur_id, idepth_var_max_graph, scene_color_scale, debug_flip_images ? 1 : 0, debug_img,
                                     &nc, &nu), -1, "flame_stereo_draw_features");
    if (num_converged) *num_converged = nc;
    if (num_unconverged) *num_unconverged = nu;
  }
  template <class FlameParams>
  void drawFeatures(const FlameParams& params, uint32_t fcur_id, uint8_t* debug_img, int* num_converged = nullptr,
                    int* num_unconverged = nullptr) {
    drawFeatures(fcur_id, params.idepth_var_max_graph, params.scene_color_scale, params.debug_flip_images, debug_img,
                 num_converged, num_unconverged);
  }
  // ---- getDebugImageMatches ----
  // While on, every updateFeatureIDepths (and the resident forms of the C-ABI) also records what the reference draws into its
  // debug_img argument with params.debug_draw_matches (flame.cc:1293-1295 and the draws of trackFeature); what the update
  // computes and returns is the same.
  void recordMatches(bool on) {
    check(flame_stereo_set_option(ctx_, FLAME_STEREO_OPT_RECORD_MATCHES, on ? 1 : 0), -1, "flame_stereo_set_option");
  }
  // The picture of the last update, over the resident frame it named as new; debug_img: height * width * 3 bytes (cv::Vec3b,
  // c[0], c[1], c[2]).  The text overlay (debug_draw_text_overlay) is not drawn.  Throws (FLAME_NLTGV2_ERR_INVALID_ARG) when no
  // update ran since recordMatches(true), when it failed, or when that frame was dropped.
  void getDebugImageMatches(uint8_t* debug_img, bool debug_flip_images, MatchesStats* stats = nullptr) {
    check(flame_stereo_draw_matches(ctx_, debug_flip_images ? 1 : 0, debug_img, stats), -1, "flame_stereo_draw_matches");
  }
  // With the reference's parameters: nothing is drawn, and false returned, unless params.debug_draw_matches is set.
  template <class FlameParams>
  bool getDebugImageMatches(const FlameParams& params, uint8_t* debug_img, MatchesStats* stats = nullptr) {
    if (!params.debug_draw_matches) return false;
    getDebugImageMatches(debug_img, params.debug_flip_images ? true : false, stats);
    return true;
  }
  // ---- getDebugImageDetections ----
  // == the picture Flame::detectFeatures draws into its debug_img argument with params.debug_draw_detections (flame.cc:1272-1275,
  // drawDetections flame.cc:2363-2412): the epipolar-gradient score of the detectFeatures call with the same params, fref and
  // fprev, over the resident frame fref.id.  A pure function of the frame's resident gradients: nothing is recorded at
  // detection time, and nothing but scratch changes.  debug_img: height * width * 3 bytes (cv::Vec3b, c[0], c[1], c[2]).
  // max_score: the reference passes the literal 0.005f (then every scored pixel has the colour of the maximum); a larger value
  // shows the gradient strengths.  The text overlay and the (commented out) keypoints are not drawn.
  template <class FlameParams, class Frame>
  void drawDetections(const FlameParams& params, const Frame& fref, const Frame& fprev, bool debug_flip_images, uint8_t* debug_img,
                      float max_score = 0.005f, DetectionsStats* stats = nullptr) {
    float q[4], t[3];
    toQuatTrans(fprev.pose.inverse() * fref.pose, q, t);  // T_ref_to_prev (flame.cc:1207)
    const flame_stereo_params sp = toStereoParams(params);
    const flame_stereo_detect_params dp = toDetectParams(params);
    DetectionsStats local;
    DetectionsStats* st = stats ? stats : &local;
    const int rc = flame_stereo_draw_detections(ctx_, &sp, &dp, fref.id, q, t, max_score, debug_flip_images ? 1 : 0, debug_img, st);
    check(rc, st->error_pixel, "flame_stereo_draw_detections");
  }
  // With the reference's parameters: nothing is drawn, and false returned, unless params.debug_draw_detections is set.
  template <class FlameParams, class Frame>
  bool getDebugImageDetections(const FlameParams& params, const Frame& fref, const Frame& fprev, uint8_t* debug_img,
                               float max_score = 0.005f, DetectionsStats* stats = nullptr) {
    if (!params.debug_draw_detections) return false;
    drawDetections(params, fref, fprev, params.debug_flip_images ? true : false, debug_img, max_score, stats);
    return true;
  }
  // fnew_->img[0] of a resident frame in device memory (address, pitch): what DeviceGraph::debugImagesBegin takes as
  // img_device.  Valid until the frame is dropped or replaced.
  const void* frameImageDevice(uint32_t frame_id, int* step_bytes) {
    const void* img = nullptr;
    check(flame_stereo_frame_image_device(ctx_, frame_id, &img, step_bytes), -1, "flame_stereo_frame_image_device");
    return img;
  }

  // ---- which features become vertices of the graph ----
  // == the preprocessing of Flame::syncGraph (flame.cc:1954-1980) on the resident and the projected set, which must be
  // index-aligned: call it after projectFeatures(params, pfs, fcur).  pfs: the pose-frames, whose pose (camera -> world,
  // pfs.at(id)->pose) gives the height.  The arrays of the result belong to the tracker and stay valid until the next
  // selectGraphFeatures; they are what DeviceGraph::sync / syncPrepare take (pointer + count forms).
  template <class FlameParams, class FrameMap>
  flame_stereo_graph_inputs selectGraphFeatures(const FlameParams& params, const FrameMap& pfs, float graph_scale) {
    const std::vector<flame_stereo_world_pose> poses = worldPoses(pfs);
    const flame_stereo_graph_params gp = toGraphParams(params);
    flame_stereo_graph_inputs out;
    const int rc = flame_stereo_select_graph_features(ctx_, &gp, graph_scale, (int)poses.size(),
                                                      poses.empty() ? nullptr : poses.data(), &out);
    check(rc, out.error_feature, "flame_stereo_select_graph_features");
    return out;
  }
  // The same on the reference's two vectors (feats_, feats_in_curr_: index-aligned); neither resident set is touched.
  template <class FlameParams, class FrameMap, class Feature>
  flame_stereo_graph_inputs selectGraphFeatures(const FlameParams& params, const FrameMap& pfs, float graph_scale,
                                                const std::vector<Feature>& feats, const std::vector<Feature>& feats_in_curr) {
    if (feats.size() != feats_in_curr.size()) throw StereoError(FLAME_NLTGV2_ERR_INVALID_ARG, -1, "selectGraphFeatures");
    const std::vector<flame_stereo_world_pose> poses = worldPoses(pfs);
    const flame_stereo_graph_params gp = toGraphParams(params);
    flame_stereo_graph_inputs out;
    const int rc = flame_stereo_select_graph_features_arrays(
        ctx_, &gp, graph_scale, (int)poses.size(), poses.empty() ? nullptr : poses.data(), (int)feats.size(),
        feats.empty() ? nullptr : adoptFeatures(feats.data()), feats.empty() ? nullptr : adoptFeatures(feats_in_curr.data()), &out);
    check(rc, out.error_feature, "flame_stereo_select_graph_features_arrays");
    return out;
  }
  // == Flame::getRawIDepths (flame.h:255-273): the valid records of the projected set (feats_in_curr_), copied back.
  // Point: anything with .x / .y (cv::Point2f).
  template <class Point>
  void getRawIDepths(std::vector<Point>* vertices, std::vector<float>* idepths_mu, std::vector<float>* idepths_var) {
    vertices->clear(), idepths_mu->clear(), idepths_var->clear();
    int n = 0;
    check(flame_stereo_get_projected(ctx_, 0, nullptr, &n), -1, "flame_stereo_get_projected");
    std::vector<flame_stereo_feature> cur((size_t)n);
    check(flame_stereo_get_projected(ctx_, n, n ? cur.data() : nullptr, &n), -1, "flame_stereo_get_projected");
    for (int i = 0; i < n; ++i) {
      if (!cur[i].valid) continue;
      Point p;
      p.x = cur[i].x, p.y = cur[i].y;
      vertices->push_back(p);
      idepths_mu->push_back(cur[i].idepth_mu);
      idepths_var->push_back(cur[i].idepth_var);
    }
  }

  // ---- prunePoseFrames ----
  // == Flame::prunePoseFrames(pfs_to_keep) on the resident set.  Does the host half of flame.cc:562-607 here: the kept
  // pose-frames are pfs_to_keep intersected with *pfs; when curr_pf is not among them nothing changes and false is
  // returned (the reference prints "Current poseframe is not in to_keep list" and returns); the target is the kept
  // pose-frame with the largest id (pruned_pfs.crbegin() of a std::map); every other entry of *pfs goes away, with
  // T = target.pose.inverse() * pf.pose (flame.cc:612).  After the call the dropped entries are erased from *pfs
  // (pfs_.swap(pruned_pfs)) and their resident frames released.  Records [first_new, n) of the resident set are
  // new_feats_ (the detections appended since the last update); first_new < 0 = all are feats_.
  // Not imitated: the `pruned_pfs.size() == 0 -> clear()` branch (flame.cc:591-595), which cannot be reached once
  // curr_pf was found in the list (clearFeatures() is there for a caller who wants it), and the detection queue
  // (flame.cc:580-589), which is the caller's: drop its entries whose ref or cmp pose-frame is no longer in *pfs.
  template <class FlameParams, class FrameMap, class Frame>
  bool prunePoseFrames(const FlameParams& params, FrameMap* pfs, const Frame& curr_pf, const std::vector<uint32_t>& pfs_to_keep,
                       int first_new = -1, flame_stereo_prune_stats* stats = nullptr) {
    PrunePlan plan;
    if (!planPrune(*pfs, curr_pf, pfs_to_keep, &plan)) return false;
    if (first_new < 0) check(flame_stereo_features_device(ctx_, nullptr, &first_new), -1, "flame_stereo_features_device");
    const flame_stereo_params sp = toStereoParams(params);
    flame_stereo_prune_stats local;
    flame_stereo_prune_stats* st = stats ? stats : &local;
    const int rc = flame_stereo_prune_pose_frames(ctx_, &sp, plan.target, (int)plan.keep.size(), plan.keep.data(),
                                                  (int)plan.dropped.size(), plan.dropped.empty() ? nullptr : plan.dropped.data(),
                                                  first_new, st);
    check(rc, st->error_feature, "flame_stereo_prune_pose_frames");
    for (size_t k = 0; k < plan.dropped.size(); ++k) pfs->erase(plan.dropped[k].frame_id);
    return true;
  }
  // The same on the reference's two vectors: one call on feats + new_feats with first_new = feats->size(), split again
  // afterwards (a failed feats record is marked invalid and stays, a failed new_feats record is gone).
  template <class FlameParams, class FrameMap, class Frame, class Feature>
  bool prunePoseFrames(const FlameParams& params, FrameMap* pfs, const Frame& curr_pf, const std::vector<uint32_t>& pfs_to_keep,
                       std::vector<Feature>* feats, std::vector<Feature>* new_feats, flame_stereo_prune_stats* stats = nullptr) {
    PrunePlan plan;
    if (!planPrune(*pfs, curr_pf, pfs_to_keep, &plan)) return false;
    const size_t n_old = feats->size();
    std::vector<Feature> all(*feats);
    all.insert(all.end(), new_feats->begin(), new_feats->end());
    int n = (int)all.size();
    const flame_stereo_params sp = toStereoParams(params);
    flame_stereo_prune_stats local;
    flame_stereo_prune_stats* st = stats ? stats : &local;
    const int rc = flame_stereo_prune_features(ctx_, &sp, plan.target, (int)plan.keep.size(), plan.keep.data(),
                                               (int)plan.dropped.size(), plan.dropped.empty() ? nullptr : plan.dropped.data(),
                                               (int)n_old, &n, all.empty() ? nullptr : adoptFeatures(all.data()), st);
    check(rc, st->error_feature, "flame_stereo_prune_features");
    feats->assign(all.begin(), all.begin() + n_old);
    new_feats->assign(all.begin() + n_old, all.begin() + n);
    for (size_t k = 0; k < plan.dropped.size(); ++k) pfs->erase(plan.dropped[k].frame_id);
    return true;
  }
  // The feature half of Flame::clear(): no resident features, no projected set; the frames stay.
  void clearFeatures() { check(flame_stereo_clear_features(ctx_), -1, "flame_stereo_clear_features"); }

  flame_stereo_ctx* handle() const { return ctx_; }

 private:
  // pfs.at(id)->pose of every pose-frame, as makePose forms the relative poses.
  template <class FrameMap>
  static std::vector<flame_stereo_world_pose> worldPoses(const FrameMap& pfs) {
    std::vector<flame_stereo_world_pose> poses;
    for (typename FrameMap::const_iterator it = pfs.begin(); it != pfs.end(); ++it) {
      flame_stereo_world_pose p;
      std::memset(&p, 0, sizeof p);
      p.frame_id = it->first;
      toQuatTrans(it->second->pose, p.q, p.t);
      poses.push_back(p);
    }
    return poses;
  }
  struct PrunePlan {
    uint32_t target;
    std::vector<uint32_t> keep;
    std::vector<flame_stereo_pose> dropped;
  };
  // flame.cc:562-578 and 607-615: false when curr_pf is not kept.
  template <class FrameMap, class Frame>
  static bool planPrune(const FrameMap& pfs, const Frame& curr_pf, const std::vector<uint32_t>& pfs_to_keep, PrunePlan* plan) {
    bool found_curr_pf = false;
    for (size_t i = 0; i < pfs_to_keep.size(); ++i) {
      if (pfs.count(pfs_to_keep[i]) == 0) continue;
      bool seen = false;
      for (size_t k = 0; k < plan->keep.size(); ++k) seen = seen || plan->keep[k] == pfs_to_keep[i];
      if (!seen) plan->keep.push_back(pfs_to_keep[i]);
      found_curr_pf = found_curr_pf || pfs_to_keep[i] == curr_pf.id;
    }
    if (!found_curr_pf) return false;
    plan->target = plan->keep[0];
    for (size_t k = 1; k < plan->keep.size(); ++k) plan->target = plan->keep[k] > plan->target ? plan->keep[k] : plan->target;
    const typename FrameMap::const_iterator target = pfs.find(plan->target);
    for (typename FrameMap::const_iterator it = pfs.begin(); it != pfs.end(); ++it) {
      bool kept = false;
      for (size_t k = 0; k < plan->keep.size(); ++k) kept = kept || plan->keep[k] == it->first;
      if (kept) continue;
      flame_stereo_pose p;
      std::memset(&p, 0, sizeof p);
      p.frame_id = it->first;
      toQuatTrans(target->second->pose.inverse() * it->second->pose, p.q_ref_to_new, p.t_ref_to_new);
      plan->dropped.push_back(p);
    }
    return true;
  }
  template <class FlameParams, class Frame>
  int detect(const FlameParams& params, const Frame& fref, const Frame& fprev, const float* map_host, const void* map_device,
             int n_mask, const float* mask, uint32_t* feat_count) {
    float q[4], t[3];
    toQuatTrans(fprev.pose.inverse() * fref.pose, q, t);  // T_ref_to_prev (flame.cc:1012)
    const flame_stereo_params sp = toStereoParams(params);
    const flame_stereo_detect_params dp = toDetectParams(params);
    flame_stereo_feature_stats st;
    const int rc = flame_stereo_detect_features(ctx_, &sp, &dp, fref.id, q, t, map_host, map_device, n_mask, mask, *feat_count,
                                                &st);
    check(rc, st.error_feature, "flame_stereo_detect_features");
    *feat_count += (uint32_t)st.num_features;
    return st.num_features;
  }
  static void check(int rc, int feature, const char* what) {
    if (rc != 0) throw StereoError(rc, feature, what);
  }
  flame_stereo_ctx* ctx_;
};

}  // namespace flame_hip
#endif  // FLAME_HIP_FEATURE_TRACKER_HPP_
