/*
 * flame_stereo.h -- C-ABI of the per-feature epipolar inverse-depth update of robustrobotics/flame on MI355X
 * (gfx950); part of libflame_nltgv2_hip.so.  SURVEY.md section 8(f) rank 4: the per-frame loop that produces the
 * regularizer's data terms.
 *
 * Replaces, for the level-0 images the path reads:
 *   Flame::updateFeatureIDepths      /root/reference/src/flame/flame.cc:1280-1536  (the `omp parallel for` over features)
 *   Flame::trackFeature              flame.cc:1538-1752
 *   stereo::EpipolarGeometry<float>  src/flame/stereo/epipolar_geometry.h
 *   stereo::inverse_depth_filter::{predict,getSearchRegion,search,update}   src/flame/stereo/inverse_depth_filter.cc
 *   stereo::line_stereo::match       src/flame/stereo/line_stereo.h:73-385
 *   stereo::InverseDepthMeasModel::idepth   src/flame/stereo/inverse_depth_meas_model.cc:48-154
 *   utils::Frame::create (level 0: padded image + padded central gradients)   src/flame/utils/frame.cc:33-71
 *
 * The boundary sits where the reference hands Eigen/Sophus values to its stereo code: the caller keeps the
 * pose algebra (Sophus::SE3f products, flame.cc:1315-1316, 1614) and passes one (quaternion, translation) pair
 * per pose-frame; everything from EpipolarGeometry::loadGeometry down runs on the GPU, a 16-lane row per feature.
 * Results are bit-identical to the reference's scalar float code (same expression order, no FMA contraction).
 * Debug drawing (params.debug_draw_matches) is optional: flame_stereo_draw_matches, below.  The stderr diagnostics are not part
 * of the path.
 *
 * Status codes are flame_nltgv2_status (flame_nltgv2.h).  Where the reference would FLAME_ASSERT -> exit(1)
 * (negative inverse depth into project(), a sample outside the padded image, ...), the call returns
 * FLAME_NLTGV2_ERR_ASSERT and stats.error_feature names the lowest such feature index; the feature array is
 * then unspecified.  There is no CPU fallback.
 */
#ifndef FLAME_STEREO_H_
#define FLAME_STEREO_H_

#include <stdint.h>

#include "flame_nltgv2.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct flame_stereo_ctx flame_stereo_ctx;

/* The members of flame::Params this path reads (params.h), with the reference's defaults
 * (flame_stereo_default_params). */
typedef struct flame_stereo_params {
  float min_baseline;            /* Params::min_baseline            0.01  (params.h:72) */
  int32_t do_letterbox;          /* Params::do_letterbox            0     (params.h:47) */
  float rescale_factor_min;      /* Params::rescale_factor_min      0.7   (params.h:64) */
  float rescale_factor_max;      /* Params::rescale_factor_max      1.4   (params.h:65) */
  float idepth_var_max;          /* Params::idepth_var_max          0.25  (params.h:68) */
  int32_t max_dropouts;          /* Params::max_dropouts            5     (params.h:69) */
  float outlier_sigma_thresh;    /* Params::outlier_sigma_thresh    3     (params.h:70) */
  int32_t do_meas_fusion;        /* Params::do_meas_fusion          1     (params.h:73) */
  /* Params::fparams -- inverse_depth_filter::Params (inverse_depth_filter.h:50-71) */
  int32_t win_size;              /* 5 (the only supported value, as in the reference: inverse_depth_filter.cc:195) */
  float search_sigma;            /* 2 */
  float min_grad_mag;            /* 5 */
  float idepth_min;              /* 1e-3 */
  float idepth_max;              /* 2 */
  float epilength_min;           /* 3 */
  float epilength_max;           /* 32 */
  float process_var_factor;      /* 1.01 */
  float process_fail_var_factor; /* 1.1 */
  /* Params::fparams.sparams -- line_stereo::Params (line_stereo.h:47-60) */
  float max_cost;                /* 1300 */
  int32_t do_subpixel;           /* 1 */
  float sample_dist;             /* 1 */
  float second_best_factor;      /* 1.5 */
  /* Params::zparams -- InverseDepthMeasModel::Params (inverse_depth_meas_model.h:43-51) */
  int32_t z_win_size;            /* 5 */
  float pixel_var;               /* 16 */
  float epipolar_line_var;       /* 1 */
} flame_stereo_params;
void flame_stereo_default_params(flame_stereo_params* p);

/* == struct FeatureWithIDepth (flame.h:88-99); 40 bytes. */
typedef struct flame_stereo_feature {
  uint32_t id;
  uint32_t frame_id;     /* the pose-frame the feature is anchored in; rewritten when the feature is moved (flame.cc:1634) */
  float x, y;            /* xy in that frame (unpadded pixel coordinates) */
  float idepth_mu;
  float idepth_var;
  uint8_t valid;
  uint8_t reserved_[3];
  uint32_t num_updates;
  uint32_t num_dropouts;
  int32_t search_status; /* inverse_depth_filter::Status: 0 SUCCESS, 1 FAIL_REF_PATCH_GRADIENT, 2 FAIL_AMBIGUOUS_MATCH,
                            3 FAIL_MAX_COST (inverse_depth_filter.h:39-44) */
} flame_stereo_feature;

/* One entry per pose-frame that features may refer to (the reference's `pfs` map, flame.h:526).
 * q = (w, x, y, z). */
typedef struct flame_stereo_pose {
  uint32_t frame_id;
  float q_ref_to_new[4], t_ref_to_new[3]; /* fnew.pose.inverse() * pf.pose        (flame.cc:1315) */
  float q_ref_to_pf[4], t_ref_to_pf[3];   /* curr_pf.pose.inverse() * pf.pose     (flame.cc:1614), used when a feature
                                             is moved to the newest pose-frame */
} flame_stereo_pose;

/* The counters updateFeatureIDepths reports through StatsTracker (flame.cc:1497-1502) + its return value. */
typedef struct flame_stereo_stats {
  int32_t num_idepth_updates;
  int32_t num_fail_max_var;
  int32_t num_fail_max_dropouts;
  int32_t num_fail_ref_patch_grad;
  int32_t num_fail_ambiguous_match;
  int32_t num_fail_max_cost;
  int32_t success;       /* the bool updateFeatureIDepths returns (any feature updated) */
  int32_t error_feature; /* -1, or the lowest feature index that hit a reference assert / an unknown frame id */
} flame_stereo_stats;

int flame_stereo_create(flame_stereo_ctx** out, int device);
void flame_stereo_destroy(flame_stereo_ctx* ctx);
int flame_stereo_set_stream(flame_stereo_ctx* ctx, void* hip_stream);

/* Camera and image geometry (Flame::Flame, flame.cc:48-60: K_, Kinv_, width_, height_).  K, Kinv row-major.
 * `border` is the padding Frame::create gets (flame.cc:149-150: params.fparams.win_size = 5).  Drops all frames.
 *
 * Which entries are read.  Both matrices are stored whole and nothing about their form is checked here.  The stages read them as the
 * reference's EpipolarGeometry does (epipolar_geometry.h), which is written for a pinhole camera -- K = [fx 0 cx; 0 fy cy; 0 0 1]
 * and its inverse -- and mixes two kinds of expression:
 *   - the shortcuts read K[0], K[2], K[4], K[5] and Kinv[0], Kinv[2], Kinv[4], Kinv[5] only: project(), the epipole, the epipolar line
 *     of a pixel and minDepthProjection (epipolar_geometry.h:97-99, 165-172, 242-259, 317-320), hence the epipolar search, the
 *     prediction of a feature in the new frame, projectFeatures and prunePoseFrames; flame_stereo_align_frame reads the same four of
 *     K divided by the level's scale, and REFUSES a K whose [1], [3], [6] or [7] is not 0 or whose [8] is not 1;
 *   - the full 3x3 products: KRKinv = (K * R) * Kinv and Kt = K * t (epipolar_geometry.h:91-93), read by the disparity-to-depth
 *     conversion and by the projection at infinity; the height rule of flame_stereo_select_graph_features (xyz = Kinv * pix, all nine
 *     entries); and flame_stereo_add_raw_frame, which reads Kinv[0..5], the first two rows, in full.
 * For a pinhole K the two kinds agree.  For a K with a skew, or a last row other than 0 0 1, they describe different cameras and the
 * stereo update is not meaningful (the reference has the same property and checks it no more than this call does); the selection's
 * height and the raw-frame map are well defined for any Kinv and are tested with a general one. */
int flame_stereo_set_camera(flame_stereo_ctx* ctx, const float K[9], const float Kinv[9], int width, int height,
                            int border);

/* (drop_frame hands the frame's buffers to the next add_frame; at most 4 sets wait there, the rest is freed.)  */
/* utils::Frame::create, level 0 (frame.cc:33-71): uploads the width x height 8-bit image and builds, on the
 * device, img_pad (cv::BORDER_REFLECT_101) and gradx_pad / grady_pad (getCentralGradient, image_utils.h:425-470,
 * then cv::BORDER_CONSTANT 0).  BORDER_REFLECT_101 is cv::borderInterpolate's rule, per axis of length len: a source
 * coordinate p outside [0, len) becomes -p where p < 0 and 2 (len - 1) - p where p >= len, REPEATED until it lies inside.
 * set_camera relates border to neither width nor height, so a border of len or more (up to 64 on a frame of 2) takes
 * several rounds; the result has the period 2 (len - 1) in p.  The frame stays resident until dropped (a pose-frame is
 * read by every later frame); adding an existing id replaces it. */
int flame_stereo_add_frame(flame_stereo_ctx* ctx, uint32_t frame_id, const uint8_t* img, int row_stride_bytes);
int flame_stereo_drop_frame(flame_stereo_ctx* ctx, uint32_t frame_id);
int flame_stereo_frame_count(const flame_stereo_ctx* ctx);

/* ---- Raw camera frames: colour to grey, undistort / resize, then Frame::create ------------------------------------------
 * flame_stereo_add_frame takes what Flame::update takes: an 8-bit grey image, rectified, of the camera's size, in host memory.
 * The reference's front-end (flame_ros, not part of the reference tree) makes that image on the host with cv::cvtColor and
 * cv::undistort.  flame_stereo_add_raw_frame takes the frame as the camera delivers it -- grey or colour, any row stride,
 * with lens distortion, of another size, in host or device memory -- and leaves the same resident frame under the same id
 * (img_pad, gradx_pad, grady_pad): a kernel writes the rectified grey image, and the kernel behind flame_stereo_add_frame
 * builds the padded planes from it, unchanged.  THE DEFINITION (tests/input_ref.py restates it; all of it is this library's
 * own statement, see UNPINNED below):
 *   Grey of a tap.  Integer arithmetic on the tap's bytes: (4899 * R + 9617 * G + 1868 * B + 8192) >> 14; alpha is ignored;
 *      GREY8 is taken as is.  These are the coefficients of OpenCV's 8-bit cvtColor (they sum to 16384).  No OpenCV is part of
 *      this tree or of the reference tree, so the formula is stated, not checked against OpenCV: it is the definition.
 *   remap == 0.  The rectified pixel (u, v) is the grey of the raw pixel (u, v).
 *   remap == 1.  For the rectified pixel (u, v), in float32, one rounding per operation, in exactly this association (the
 *      library is built with -ffp-contract=off); Kinv is the context's (set_camera; its third row is not read), dist =
 *      k1 k2 p1 p2 k3 k4 k5 k6:
 *        x  = (Kinv[0]*u + Kinv[1]*v) + Kinv[2]          y  = (Kinv[3]*u + Kinv[4]*v) + Kinv[5]
 *        r2 = x*x + y*y     r4 = r2*r2     r6 = r4*r2
 *        rad = (((1 + k1*r2) + k2*r4) + k3*r6) / (((1 + k4*r2) + k5*r4) + k6*r6)
 *        tx = 2*x   ty = 2*y   a1 = tx*y   a2 = r2 + tx*x   a3 = r2 + ty*y
 *        xd = (x*rad + p1*a1) + p2*a2                    yd = (y*rad + p1*a3) + p2*a1
 *        xs = (K_raw[0]*xd + K_raw[1]*yd) + K_raw[2]     ys = K_raw[4]*yd + K_raw[5]
 *        inside = xs >= 0 && ys >= 0 && xs < (float)(raw_width - 1) && ys < (float)(raw_height - 1)
 *      `inside` has the bounds bilinearInterp asserts in the reference (utils/image_utils.h:233-236); a NaN or an infinity
 *      fails it by itself.  It is decided before any conversion to an integer and before any address is formed.  An outside
 *      pixel is 0 and is counted in n_outside.  An inside pixel has x0 = (int)xs, y0 = (int)ys, dx = xs - x0, dy = ys - y0
 *      and the reference's weights (bilinearWeights, image_utils.h:199-214):
 *        w11 = dx*dy    w01 = dx - w11    w10 = dy - w11    w00 = ((1 - dx) - dy) + w11
 *      over the grey g of its four taps, g00 at (x0, y0), g01 at (x0 + 1, y0), g10 at (x0, y0 + 1), g11 at (x0 + 1, y0 + 1):
 *        value = ((w00*g00 + w01*g01) + w10*g10) + w11*g11       stored as (uint8_t)(int)(value + 0.5f)
 *   UNPINNED: cv::undistort interpolates in fixed point (INTER_BITS = 5) from a map it builds in double, so neither the map
 *      nor the rounding above equals OpenCV's to the bit, and the grey coefficients are restated, not checked against OpenCV.
 *   OUT OF SCOPE: the fisheye (equidistant) model needs atan, which a host checker and the device do not reproduce bit for
 *      bit; a rectifying rotation (cv::initUndistortRectifyMap's R); tilted-sensor and thin-prism terms. */
enum { FLAME_STEREO_FMT_GREY8 = 0, FLAME_STEREO_FMT_BGR8 = 1, FLAME_STEREO_FMT_RGB8 = 2, FLAME_STEREO_FMT_BGRA8 = 3,
       FLAME_STEREO_FMT_RGBA8 = 4 };

typedef struct flame_stereo_input_params {
  int32_t format;                /* one of the above */
  int32_t remap;                 /* 0: raw is rectified already and has the camera's size; 1: undistort / resize */
  int32_t raw_width, raw_height; /* >= 2 each */
  float K_raw[9];                /* the raw camera, row-major; [0] [1] [2] [4] [5] are read */
  float dist[8];                 /* k1 k2 p1 p2 k3 k4 k5 k6, OpenCV's order (radial-tangential + rational) */
} flame_stereo_input_params;

typedef struct flame_stereo_input_stats {
  int32_t n_outside;             /* rectified pixels that have no source in the raw frame (written as 0) */
} flame_stereo_input_stats;

/* GREY8, remap 0, sizes 0, K_raw = I, dist = 0. */
void flame_stereo_default_input_params(flame_stereo_input_params* p);
/* What the raw frames look like.  After set_camera; set_camera forgets it.  FLAME_NLTGV2_ERR_NO_GRAPH without a camera;
 * FLAME_NLTGV2_ERR_INVALID_ARG for an unknown format, a raw dimension below 2 or above 16384, a remap other than 0 or 1, or
 * remap == 0 with a raw size other than the camera's; the input set before stays as it was then. */
int flame_stereo_set_input(flame_stereo_ctx* ctx, const flame_stereo_input_params* p);
/* Adds (or replaces) resident frame `frame_id` from a raw frame of raw_height rows of row_stride_bytes bytes, the first
 * raw_width * bytes_per_pixel of each being pixels; neither `raw` nor the stride needs any alignment.
 *   raw_on_device == 0: `raw` is host memory.  It is staged through a device buffer the context owns, and the call waits for
 *      the stream, as flame_stereo_add_frame does (the source is pageable memory).
 *   raw_on_device != 0: `raw` is device memory, read in place.  With stats == NULL the call only enqueues on the context's
 *      stream and returns: no copy, no allocation once the frame's buffers exist (flame_stereo_drop_frame hands them on), no
 *      wait.  THE CALLER keeps `raw` alive and unchanged until the context's stream has passed the call, and orders the work
 *      that produces `raw` before it: either by producing it on the stream given to flame_stereo_set_stream, or by waiting
 *      for its own stream before the call.  With stats != NULL the call waits once and fills `stats`.
 * FLAME_NLTGV2_ERR_NO_GRAPH when no camera is set; FLAME_NLTGV2_ERR_INVALID_ARG without flame_stereo_set_input since the last
 * set_camera, for raw == NULL, or for row_stride_bytes < raw_width * bytes_per_pixel.  A call that fails these checks leaves
 * flame_stereo_frame_count and every resident frame as they were.  flame_stereo_last_kernel_ms covers its two kernels. */
int flame_stereo_add_raw_frame(flame_stereo_ctx* ctx, uint32_t frame_id, const void* raw, int row_stride_bytes,
                               int raw_on_device, flame_stereo_input_stats* stats);
/* Copies a resident frame's derived images back ((height + 2 border) x (width + 2 border) each; any may be NULL). */
int flame_stereo_download_frame(flame_stereo_ctx* ctx, uint32_t frame_id, uint8_t* img_pad, float* gradx_pad,
                                float* grady_pad);

/* Flame::updateFeatureIDepths (flame.cc:1280-1536).  `new_frame_id` is fnew, `curr_pf_id` is curr_pf.id; both and
 * every pose's frame must be resident.  `feats` (host) is updated in place. */
int flame_stereo_update_feature_idepths(flame_stereo_ctx* ctx, const flame_stereo_params* params, uint32_t new_frame_id,
                                        uint32_t curr_pf_id, int n_poses, const flame_stereo_pose* poses, int n_feats,
                                        flame_stereo_feature* feats, flame_stereo_stats* stats);
/* Same on a feature array that lives in device memory (n_feats * 40 bytes); enqueues on the context's stream and,
 * unless `stats` is NULL, waits and reports. */
int flame_stereo_update_feature_idepths_device(flame_stereo_ctx* ctx, const flame_stereo_params* params,
                                               uint32_t new_frame_id, uint32_t curr_pf_id, int n_poses,
                                               const flame_stereo_pose* poses, int n_feats, void* feats_device,
                                               flame_stereo_stats* stats);
/* The resident feature set -- the default way to run the path: the features live in device memory from detection to
 * removal (as Flame::feats_ lives in the Flame object, flame.h:529), every frame runs the update on them in place, and the
 * host need not read them back at all: detections are appended on the device (detect_features) and the graph's vertices
 * and data terms come down as the arrays the regulariser's sync takes (select_graph_features).
 *   set_features     replaces the resident set (host array of n_feats records);
 *   update_resident  Flame::updateFeatureIDepths on it; `stats` NULL = enqueue only (results are ordered on the stream);
 *   get_features     copies it back (feats may be NULL to query the count);
 *   features_device  its device address and count (valid until the next set_features, project_features or
 *                    detect_features, or a prune_pose_frames that removes a record). */
int flame_stereo_set_features(flame_stereo_ctx* ctx, int n_feats, const flame_stereo_feature* feats);
int flame_stereo_update_resident(flame_stereo_ctx* ctx, const flame_stereo_params* params, uint32_t new_frame_id,
                                 uint32_t curr_pf_id, int n_poses, const flame_stereo_pose* poses, flame_stereo_stats* stats);
int flame_stereo_get_features(flame_stereo_ctx* ctx, int max_feats, flame_stereo_feature* feats, int* n_feats);
int flame_stereo_features_device(flame_stereo_ctx* ctx, void** feats_device, int* n_feats);

/* ---- Where the resident features come from and where they go ----------------------------------------------------
 * Flame::projectFeatures (flame.cc:1754-1860) and Flame::detectFeatures + the feature initialisation of
 * Flame::detectionLoop (flame.cc:822-1278, the live single-pass part; flame.cc:736-757), on the resident set.  Both
 * calls enqueue on the context's stream and wait once, to return the new counts (the host needs them for the next
 * update_resident); there is no enqueue-only form.  Both leave the resident set and the projected set unchanged when
 * they fail.  Both may move the resident set: the address from flame_stereo_features_device is valid until the next
 * set_features, project_features or detect_features (and flame_stereo_projected_device's until the next
 * project_features). */

/* The members of flame::Params detection reads beyond flame_stereo_params (whose do_letterbox, rescale_factor_max and
 * win_size it also reads), with the reference's defaults (flame_stereo_default_detect_params). */
typedef struct flame_stereo_detect_params {
  int32_t detection_win_size; /* Params::detection_win_size  16    (params.h:48): cells are win x win pixels */
  float min_grad_mag;         /* Params::min_grad_mag        5     (params.h:39) -- not fparams.min_grad_mag */
  float idepth_init;          /* Params::idepth_init         0.01  (params.h:60) */
  float idepth_var_init;      /* Params::idepth_var_init     0.25  (params.h:61) */
} flame_stereo_detect_params;
void flame_stereo_default_detect_params(flame_stereo_detect_params* p);

typedef struct flame_stereo_feature_stats {
  int32_t num_features;  /* project: features kept; detect: new features appended */
  int32_t num_examined;  /* project: resident features examined; detect: cells of the grid (hc x wc) */
  int32_t error_feature; /* -1; project: the lowest feature index that hit a reference assert or names an unknown
                            frame; detect: the lowest row-major pixel index (row * width + col) whose
                            referenceEpiline asserted */
} flame_stereo_feature_stats;

/* Flame::projectFeatures(params, K, Kinv, pfs, fcur, &feats_, &feats_in_curr_) on the resident set.  `poses` holds one
 * entry per pose-frame the features may refer to, with q/t_ref_to_new = fcur.pose.inverse() * pf.pose (the *_to_pf
 * members are not read).  Every feature, valid or not, must name a pose (pfs.at(), flame.cc:1784), else
 * FLAME_NLTGV2_ERR_INVALID_ARG; a valid feature whose projection asserts in the reference (negative or NaN idepth_mu)
 * gives FLAME_NLTGV2_ERR_ASSERT.  The features that stay inside the valid region in front of the camera are kept, in
 * order, in the resident set (unchanged records) and in the projected set (feats_in_curr: valid = 1, the same id and
 * num_updates, frame_id = cur_frame_id, the projected xy and idepth_mu, idepth_var scaled by (cur/ref)^4;
 * num_dropouts = search_status = 0, where the reference leaves the vector's previous contents).  The frames need not
 * be resident.  `stats` may be NULL. */
int flame_stereo_project_features(flame_stereo_ctx* ctx, const flame_stereo_params* params, uint32_t cur_frame_id,
                                  int n_poses, const flame_stereo_pose* poses, flame_stereo_feature_stats* stats);
/* The projected set of the last project_features (empty before the first): copy back (feats NULL = count only), or its
 * device address and count. */
int flame_stereo_get_projected(flame_stereo_ctx* ctx, int max_feats, flame_stereo_feature* feats, int* n_feats);
int flame_stereo_projected_device(flame_stereo_ctx* ctx, void** feats_device, int* n_feats);

/* Flame::detectFeatures on resident frame `ref_frame_id` (its gradients, built by add_frame) with the geometry of
 * T_ref_to_prev = fprev.pose.inverse() * fref.pose, then the detection loop's initialisation of every new feature:
 * id = first_id + k (k-th new feature, in row-major cell order), frame_id = ref_frame_id, xy = the cell's best pixel,
 * idepth_mu = idepthmap(y, x) unless NaN, else idepth_init, idepth_var = idepth_var_init, valid = 1, counters 0.
 * The new features are appended to the resident set (feats_.insert(feats_.end(), new_feats_) at the next update()).
 *   idepthmap   width x height floats, row-major: in host memory (idepthmap_host), in device memory
 *               (idepthmap_device, e.g. the rasteriser's map), or neither (all NaN: every feature gets idepth_init).
 *   mask        the points whose cells get no new feature (curr_feats): n_mask (x, y) pairs in host memory, or
 *               n_mask = -1 for the projected set of the last project_features (data.ref_xy, flame.cc:474-477).  A
 *               host point outside the image is FLAME_NLTGV2_ERR_INVALID_ARG.
 * A pixel that passes the gradient test where the reference's referenceEpiline asserts (zero translation) gives
 * FLAME_NLTGV2_ERR_ASSERT and appends nothing.  `stats` may be NULL. */
int flame_stereo_detect_features(flame_stereo_ctx* ctx, const flame_stereo_params* params,
                                 const flame_stereo_detect_params* dparams, uint32_t ref_frame_id,
                                 const float q_ref_to_prev[4], const float t_ref_to_prev[3], const float* idepthmap_host,
                                 const void* idepthmap_device, int n_mask, const float* mask_xy, uint32_t first_id,
                                 flame_stereo_feature_stats* stats);

/* ---- Letting a pose-frame go -------------------------------------------------------------------------------------
 * Flame::prunePoseFrames(pfs_to_keep) (flame.cc:554-706, flame.h:174): every feature anchored in a pose-frame that
 * goes away is re-anchored in the target pose-frame, then the frames are released.  The caller does the host half
 * (flame.cc:562-607: intersect pfs_to_keep with its map, give up when the current pose-frame is not kept, pick the
 * target, form the relative poses); include/flame_hip/feature_tracker.hpp does exactly that.  What the reference's
 * loops (flame.cc:608-700) do is reproduced literally; our numpy restatement tests/prune_ref.py is the checker, and
 * like the rest of the front-end the parity with the reference binary is unpinned:
 *   1. The target is `pruned_pfs.crbegin()` of a std::map<uint32_t, ...>: the kept pose-frame with the LARGEST id
 *      (the comment beside it says "oldest").  The caller passes it as target_frame_id.
 *   2. `valid` is not tested: invalid features of a dropped pose-frame are moved too.  `valid` is only ever cleared.
 *   3. Records [0, first_new) (feats_): frame_id, xy, idepth_mu and idepth_var are overwritten BEFORE the success
 *      test, so also when the move fails (idepth_mu is then the 0 that predict returns, xy the projected point).
 *   4. idepth_var is scaled by (idepth_pf / old_idepth)^4, formed as two squarings, and by 1 when idepth_pf < 1e-6
 *      (the NEW value, a float compared with a double literal).  predict's own var_pred is discarded, so
 *      process_var_factor has no effect.
 *   5. The valid region is an integer cv::Rect (border, border + row_offset, width - 2 border, height - 2 border -
 *      2 row_offset; border = int(rescale_factor_max * win_size / 2 + 1), row_offset = height / 3 with do_letterbox)
 *      tested against a cv::Point2f, which OpenCV first rounds to an integer point (cvRound: to nearest, ties to
 *      even): x <= round(p.x) < x + w.  projectFeatures' rectangle is float; this one is not.  It is the rule the
 *      update already uses when it moves a feature to the newest pose-frame.  UNPINNED: OpenCV is not available to
 *      check this reading against.  A NaN coordinate is outside (cvRound gives INT_MIN on x86).
 *   6. A feature of a dropped pose-frame whose input makes EpipolarGeometry::project assert (negative or NaN
 *      idepth_mu, a zero third coordinate; epipolar_geometry.h:128, 139) gives FLAME_NLTGV2_ERR_ASSERT with the lowest
 *      such index; nothing changes.
 *   7. A failed move (behind the target camera, or outside the region) of a record in [0, first_new) marks it invalid
 *      and keeps it; a failed record in [first_new, n) (new_feats_) is removed, unrewritten, and the survivors keep
 *      their order.  The resident set holds both lists because detect_features appends at once where the reference
 *      parks detections in new_feats_ until the next update() (flame.cc:257); the two outcomes differ downstream (the
 *      update does not test `valid` on entry and can set it again), hence first_new.
 *   8. The `pruned_pfs.size() == 0 -> clear()` branch (flame.cc:591-595) cannot be reached once the current pose-frame
 *      was found in the list; flame_stereo_clear_features is there for a caller that wants Flame::clear().
 * The detection queue (flame.cc:580-589) is the caller's. */
typedef struct flame_stereo_prune_stats {
  int32_t num_examined;       /* features looked at */
  int32_t num_moved;          /* re-anchored in the target pose-frame, move succeeded */
  int32_t num_invalidated;    /* index <  first_new: move failed or left the valid region, marked invalid */
  int32_t num_removed;        /* index >= first_new: the same, removed */
  int32_t num_features;       /* features in the set afterwards */
  int32_t num_frames_dropped; /* resident frames released */
  int32_t error_feature;      /* -1, or the lowest offending feature index */
} flame_stereo_prune_stats;

/* Flame::prunePoseFrames on the resident set.  Records [0, first_new) are feats_, records [first_new, n) are
 * new_feats_ (the detections appended since the last update_resident); first_new = the resident count means "all
 * feats_"; 0 <= first_new <= n.
 *   keep_ids   the ids of the pose-frames that stay (n_keep >= 1); target_frame_id must be one of them.
 *   dropped    one entry per pose-frame that goes away, with q/t_ref_to_new = target.pose.inverse() * pf.pose
 *              (flame.cc:612-615; the *_to_pf members are not read).  An id in both lists is an error.
 * A feature whose frame is neither kept nor listed in `dropped` gives FLAME_NLTGV2_ERR_INVALID_ARG with its index.  On
 * any error the resident set, the projected set and the resident frames are unchanged.  After success every resident
 * frame named in `dropped` is released as by flame_stereo_drop_frame: its buffers wait for the next add_frame, at most
 * 4 sets of them (what a front-end that prunes every few frames reuses); further ones are freed with hipFree, which
 * waits for the whole device -- acceptable in a call made every few seconds.  Frames named in neither list (the current
 * and previous non-pose frames) stay.  The projected set is not touched.
 * The move is in place: the address from flame_stereo_features_device stays valid when nothing was removed
 * (stats.num_removed == 0); otherwise the call may move the resident set, like project_features, and the address is
 * valid until then.  Enqueues on the context's stream and waits once.  `stats` may be NULL. */
int flame_stereo_prune_pose_frames(flame_stereo_ctx* ctx, const flame_stereo_params* params, uint32_t target_frame_id,
                                   int n_keep, const uint32_t* keep_ids, int n_dropped, const flame_stereo_pose* dropped,
                                   int first_new, flame_stereo_prune_stats* stats);
/* The same on a host array (the four-edit integration): `feats` (*n_feats records) is updated in place and *n_feats
 * rewritten; the resident set is not read or changed, the resident frames named in `dropped` are released. */
int flame_stereo_prune_features(flame_stereo_ctx* ctx, const flame_stereo_params* params, uint32_t target_frame_id, int n_keep,
                                const uint32_t* keep_ids, int n_dropped, const flame_stereo_pose* dropped, int first_new,
                                int* n_feats, flame_stereo_feature* feats, flame_stereo_prune_stats* stats);
/* The feature half of Flame::clear() (flame.h:179-202): no resident features, no projected set.  Frames stay, as pfs_
 * does in the reference. */
int flame_stereo_clear_features(flame_stereo_ctx* ctx);

/* ---- Which features become vertices of the graph ------------------------------------------------------------------
 * The preprocessing of Flame::syncGraph (flame.cc:1954-1980) and the data-term lines of its two vertex loops
 * (flame.cc:2001-2004, 2041-2044): which features become graph vertices, and with which position, data term and data
 * weight.  The result is exactly what flame_nltgv2_sync_input takes (flame_nltgv2.h): feat_id, pos, data_term,
 * data_weight, member for member.  The reference's loop is reproduced literally; our numpy restatement
 * tests/select_ref.py is the checker, and like the rest of the front-end the parity with the reference binary is unpinned:
 *   1. The predicate reads the RESIDENT record feats[i] (anchored frame): valid, idepth_var, xy, idepth_mu, frame_id.
 *      The variance tested is the resident record's, not the projected one.
 *   2. The outputs read the PROJECTED record feats_in_curr[i] at the same index (feat_id_to_idx, flame.cc:1998, 2032):
 *      pos = its xy, data_term = its idepth_mu / graph_scale, data_weight = adaptive_data_weights ? 1.0f / its idepth_var
 *      : 1.0f.  Its `valid` flag and its `id` are not read; feat_id is feats[i].id.
 *   3. Height: pix = (x, y, 1) / idepth_mu; xyz = Kinv * pix; world = pose * xyz.  A feature is selected iff
 *      valid && idepth_var < idepth_var_max_graph && -world.y >= min_height && -world.y <= max_height.  Only world.y is
 *      formed.  Every comparison with a NaN is false: idepth_mu == 0 gives infinite or NaN points and plain IEEE results,
 *      so the feature is not selected and counts under num_fail_height.
 *   4. FLAME_ASSERT(idepth >= 0.0f) (flame.cc:1968) runs for EVERY record, valid or not: a negative or NaN idepth_mu gives
 *      FLAME_NLTGV2_ERR_ASSERT.  pfs.at(feat.frame_id) (flame.cc:1974) also runs for every record: a frame that `poses`
 *      does not name gives FLAME_NLTGV2_ERR_INVALID_ARG.  error_feature is the lowest index that fails either, the status
 *      that of this record (the assert comes first within a record), as the reference's loop would stop there.  On any
 *      error nothing is selected: V = 0 and the pointers are NULL.
 *   5. Vertex order: the reference's is BGL hash order, unspecified; here ascending record index (a stable compaction),
 *      like every other vertex order in this library.
 *   6. feat.id is uint32_t, the sync's feat_id int32_t >= 0: an id >= 2^31 among the selected gives
 *      FLAME_NLTGV2_ERR_INVALID_ARG with its index.  Duplicate ids are the caller's error and stay the sync's to reject
 *      (in the reference feat_id_to_idx would keep the last; ids are unique by construction, feat_count_).
 *   7. The resident form needs the resident and the projected set index-aligned, as they are right after
 *      flame_stereo_project_features.  The context keeps a flag: project_features sets it; whatever changes membership or
 *      order of the resident set clears it (set_features, a detect_features that appends a record, a prune that removes
 *      a record, clear_features).  A call with the flag clear gives FLAME_NLTGV2_ERR_INVALID_ARG.  update_resident and a
 *      prune in place between the two calls do not clear it.
 *   8. No features: V = 0 with num_examined = 0 is a valid answer, and the pointers are NULL.
 *   9. `do_nltgv2 == false` (flame.cc:2006-2009) and the existing-vertex loop's sticky-obstacle test are not part of
 *      this call; the sticky-obstacle test lives in the sync (flame_nltgv2_sync_input.check_sticky_obstacles).
 * UNPINNED arithmetic (Eigen and Sophus are not part of this tree; the same kind of statement as for the mesh outputs in
 * flame_nltgv2.h), all in float, no FMA contraction:
 *   pix       three true divisions by idepth_mu: x / mu, y / mu, 1 / mu.  That is Eigen >= 3.3; Eigen 3.2 multiplies by
 *             1 / idepth_mu instead, which rounds differently.
 *   Kinv*pix  the full 3 x 3 product, each row (a + b) + c, left to right.
 *   rotation  row 1 of Eigen's Quaternion::toRotationMatrix() from q: tx = 2x, ty = 2y, tz = 2z; R10 = tx*y + tz*w,
 *             R11 = 1 - (tx*x + tz*z), R12 = ty*z - tx*w.
 *   world.y   ((R10*X + R11*Y) + R12*Z) + t[1]. */

/* The members of flame::Params that syncGraph's preprocessing reads (params.h:88-91), with the reference's defaults
 * (flame_stereo_default_graph_params). */
typedef struct flame_stereo_graph_params {
  float idepth_var_max_graph;    /* Params::idepth_var_max_graph   1e-2 */
  float min_height;              /* Params::min_height             0.1  */
  float max_height;              /* Params::max_height             4    */
  int32_t adaptive_data_weights; /* Params::adaptive_data_weights  0    */
} flame_stereo_graph_params;
void flame_stereo_default_graph_params(flame_stereo_graph_params* p);

/* pf.pose of one pose-frame (camera -> world, what pfs.at(id)->pose holds).  q = (w, x, y, z). */
typedef struct flame_stereo_world_pose {
  uint32_t frame_id;
  float q[4], t[3];
} flame_stereo_world_pose;

/* The arrays are pinned host memory of the context: valid until the next call of either select function or until
 * destroy.  The first four map one to one onto flame_nltgv2_sync_input. */
typedef struct flame_stereo_graph_inputs {
  int32_t V;                 /* selected features = vertices of the frame's graph */
  const int32_t* feat_id;    /* [V]   -> flame_nltgv2_sync_input.feat_id      feats[i].id */
  const float* pos;          /* [2V]  -> .pos          feats_in_curr[i].xy */
  const float* data_term;    /* [V]   -> .data_term    feats_in_curr[i].idepth_mu / graph_scale */
  const float* data_weight;  /* [V]   -> .data_weight  adaptive ? 1.0f / feats_in_curr[i].idepth_var : 1.0f */
  const int32_t* feat_index; /* [V]   index i of the record in the resident / projected set, ascending */
  int32_t num_examined;      /* records looked at */
  int32_t num_invalid;       /* the first failing test, in this order: !valid, */
  int32_t num_fail_var;      /*   idepth_var >= idepth_var_max_graph, */
  int32_t num_fail_height;   /*   outside the height band or not finite; the three sum to num_examined - V */
  int32_t error_feature;     /* -1, or the lowest index that hit the reference's assert / names an unknown frame / has
                                an id >= 2^31 */
} flame_stereo_graph_inputs;

/* On the resident and the projected set (point 7).  Reads both, changes neither.  Enqueues on the context's stream and
 * waits once. */
int flame_stereo_select_graph_features(flame_stereo_ctx* ctx, const flame_stereo_graph_params* gp, float graph_scale,
                                       int n_poses, const flame_stereo_world_pose* poses, flame_stereo_graph_inputs* out);
/* The same on two index-aligned host arrays (feats_, feats_in_curr_; n_feats records each), as flame_stereo_prune_features
 * is to flame_stereo_prune_pose_frames: uploads them, runs the same kernels, touches neither resident set nor the flag. */
int flame_stereo_select_graph_features_arrays(flame_stereo_ctx* ctx, const flame_stereo_graph_params* gp, float graph_scale,
                                              int n_poses, const flame_stereo_world_pose* poses, int n_feats,
                                              const flame_stereo_feature* feats, const flame_stereo_feature* feats_in_curr,
                                              flame_stereo_graph_inputs* out);

/* ---- getDebugImageFeatures (flame.h:294-306) ------------------------------------------------------------------------
 * Flame::drawFeatures (flame.cc:2459-2510) on the projected set of the last project_features, over the image of resident
 * frame `cur_frame_id`: the grey image as three equal bytes, then, in index order, every feature with
 * idepth_var < idepth_var_max_graph (strict; a NaN is not drawn) fills the rectangle [xi - 2, xi + 2] x [yi - 2, yi + 2],
 * both corners inclusive, clipped to the image, xi = (int)(x + 0.5f), yi = (int)(y + 0.5f) (C truncation), with
 * jet(idepth_mu * scene_color_scale, 0, 2) (utils/visualization.h:142-167; bytes c[0], c[1], c[2]).  Where rectangles
 * overlap the feature with the higher index wins, as in the sequential loop.  flip != 0: cv::flip(img, img, -1), the
 * image in reversed linear pixel order.  debug_draw_text_overlay (cv::putText) is treated as false.
 *   *num_converged    the features drawn (the reference's num_converged)
 *   *num_unconverged  the others (the counter the reference calls num_valid); either pointer may be NULL
 * UNPINNED: cv::rectangle's fill rule (thickness -1) is restated here, not checked against OpenCV.  UNPINNED too: a NaN
 * idepth_mu is undefined in the reference (it casts a NaN to uint8_t); this library's colour for it is (0, 0, 255), which
 * is what x86 produces.  A coordinate that does not fit an int saturates (the reference's cast is undefined there).
 * img_out: height * width * 3 bytes of host memory.  Enqueues on the context's stream and waits once. */
int flame_stereo_draw_features(flame_stereo_ctx* ctx, uint32_t cur_frame_id, float idepth_var_max_graph,
                               float scene_color_scale, int flip, uint8_t* img_out, int32_t* num_converged,
                               int32_t* num_unconverged);
/* Address and pitch of the unpadded image (fnew_->img[0]) of a resident frame, inside its padded device image: what
 * flame_nltgv2_debug_images_begin takes as img_device, so a frame loop uploads no image twice.  Valid until the frame is
 * dropped or replaced (add_frame with the same id, set_camera). */
int flame_stereo_frame_image_device(flame_stereo_ctx* ctx, uint32_t frame_id, const void** img, int* step_bytes);

/* ---- getDebugImageMatches (flame.h:294-306) -------------------------------------------------------------------------
 * The picture updateFeatureIDepths / trackFeature draw with params.debug_draw_matches (flame.cc:265-267, 1293-1295): why each
 * feature failed this frame.  With FLAME_STEREO_OPT_RECORD_MATCHES on, all three update entry points (update_resident,
 * update_feature_idepths, update_feature_idepths_device) run the recording instance of the update kernel, which also writes one
 * 32-byte draw record per feature at the branches where the reference draws, and the context keeps the records of the LAST
 * update with its new_frame_id and feature count.  Feature records, flame_stereo_stats and return codes are bit-identical to
 * the option off (the default), which launches the kernels it always launched.  flame_stereo_draw_matches paints the records
 * over the image of the frame that update named as new.  The rule, restated by tests/matches_ref.py (the checker; like the rest
 * of the front-end not pinned to the reference binary):
 *   1. Order.  The reference's `omp parallel for` (flame.cc:1307) is inert (-fopenmp is never set): the loop is sequential in
 *      feature index.  Feature i issues at most four draws, draw id = 4 i + k.  Rectangles and rings overwrite, the segment
 *      blends; a pixel's final value is the fold, in increasing draw id, over the draws that touch it.
 *   2. Base image: cvtColor(fnew.img[0], GRAY2RGB), three equal bytes.  Colours are the bytes c[0], c[1], c[2] in memory.
 *   3. k = 0, a filled rectangle (cv::rectangle, thickness -1, both corners inclusive, clipped to the image) of half-width
 *      r1 = width / 320 (integer division; 0 below 320 columns: a single pixel) around ((int)(u_cmp.x + 0.5f),
 *      (int)(u_cmp.y + 0.5f)), C truncation, u_cmp = the point the FIRST predict returned (search writes it on success only,
 *      line_stereo.h:381-382).  kind_count index, outcome, where, colour:
 *        0  move to the newest pose-frame failed   flame.cc:1624-1632   (0, 51, 102)
 *        1  moved                                  :1651-1656           (255, 0, 255)
 *        2  getSearchRegion false                  :1667-1674           (0, 0, 0)
 *        3  search: FAIL_REF_PATCH_GRADIENT        :1703-1707           (255, 255, 0)
 *        4  the same with num_updates == 0         :1705-1707           (255, 255, 255)
 *        5  search: FAIL_AMBIGUOUS_MATCH           :1708                (0, 0, 255)
 *        6  search: FAIL_MAX_COST                  :1710                (0, 255, 255)
 *      Nothing is drawn for the baseline skip (:1321), a failed first predict (:1561), !valid_region.contains(feat->xy)
 *      (:1680) and a success.
 *   4. k = 1, only after a failed search (:1723-1724): applyColorMapLine(u_start, u_end, 1, 1, the rectangle's colour, 0.5)
 *      (utils/visualization.h:236-260).  Endpoints are rounded as cv::LineIterator takes them (cvRound: to nearest, ties to
 *      even) and walked as flame_nltgv2_debug_wireframe walks (flame_nltgv2.h); per visited pixel and channel
 *      colour * 0.5f + pixel * 0.5f truncated to a byte, which is exact in float and equals (colour + pixel) >> 1.
 *      getSearchRegion clips to [1, width - 1] x [1, height - 1], so a rounded endpoint is never outside the image; if one
 *      is (or is not finite) the segment is left out and counted in lines_skipped, as the wireframe does.
 *   5. k = 2, a green ring (0, 255, 0) when this frame's failure pushed idepth_var over idepth_var_max (:1350, 1405, 1454;
 *      kind_count[7]); k = 3, a blue ring (255, 0, 0) when num_dropouts > max_dropouts (:1365, 1420, 1469; kind_count[8]).
 *      cv::circle(centre, r2 = 4 * width / 320, colour): thickness 1, LINE_8.  centre = ((int)(p.x + 0.5f), (int)(p.y + 0.5f)),
 *      p = epigeo.project(fii.xy, fii.idepth_mu) with the geometry loaded at :1316 and the record AS IT STANDS at that moment:
 *      after a successful move xy and idepth_mu are those in the newest pose-frame while the geometry is the old anchor's.
 *      Kept as written.
 *   6. After all draws flip != 0 reverses the linear pixel order (cv::flip(img, img, -1)); debug_draw_text_overlay
 *      (cv::putText) is treated as false.
 * UNPINNED (OpenCV is not part of this tree; restated here and in the checker): cv::rectangle's fill rule, the line walk, and
 * the ring's pixel set: err = 0, dx = r, dy = 0, plus = 1, minus = 2 r - 1; while dx >= dy: plot the eight points
 * (cx +- dx, cy +- dy), (cx +- dy, cy +- dx), each clipped to the image on its own (coinciding points once); dy += 1,
 * err += plus, plus += 2; if err > 0: err -= minus, dx -= 1, minus -= 2.  (r = 4: 20 pixels, r = 8: 44, r = 24: 132.)
 * UNPINNED too: a coordinate that does not fit an int, or is NaN, is undefined in the reference; here the cast saturates and a
 * NaN gives 0, as in flame_stereo_draw_features.
 * ONE DELIBERATE DEVIATION: the ring's centre goes through project(), which can FLAME_ASSERT (a negative or NaN idepth_mu, a
 * zero third coordinate).  Recording never changes what the update computes or returns: a ring whose projection would assert
 * is not drawn and is counted in rings_skipped. */
typedef struct flame_stereo_matches_stats {
  int32_t num_features;   /* records of the update the picture shows */
  int32_t kind_count[9];  /* draws by kind: the seven rectangles in the order of rule 3, then the green and the blue rings */
  int32_t lines_drawn;    /* searched segments blended in */
  int32_t lines_skipped;  /* ... left out (rule 4) */
  int32_t rings_skipped;  /* rings left out because their projection would assert */
  int32_t refilled;       /* 1: the entry buffer was too small, fill and fold ran twice */
  int64_t entries;        /* pixels touched, summed over the draws (clipped to the image) */
} flame_stereo_matches_stats;
/* Paints the records of the last update over the image of the frame that update named as new.  FLAME_NLTGV2_ERR_INVALID_ARG
 * when no records stand (the option is off, no update ran with it on, the last update returned an error, or set_camera came
 * since) or when that frame is no longer resident.  img_out: height * width * 3 bytes of host memory; `stats` may be NULL.
 * The fold's entry buffer holds max(2 * height * width, 1.25 x the previous call's entries); a call that needs more grows
 * it, repeats fill and fold and reports refilled = 1 (the wireframe's contract).  Enqueues on the context's stream and waits
 * once (twice when it refills), so it is ordered behind an enqueue-only update; flame_stereo_last_kernel_ms covers its
 * kernels. */
int flame_stereo_draw_matches(flame_stereo_ctx* ctx, int flip, uint8_t* img_out, flame_stereo_matches_stats* stats);

/* ---- getDebugImageDetections (flame.h:294-306) ----------------------------------------------------------------------
 * The picture detectFeatures draws with params.debug_draw_detections (flame.cc:1272-1275): the epipolar-gradient score of
 * every scanned pixel over the image of resident frame `ref_frame_id`.  It is a pure function of its pixel, recomputed from the
 * frame's resident gradients: nothing is recorded at detection time, flame_stereo_detect_features launches what it always
 * launched, and this call takes the arguments of the detect_features call it illustrates.  The rule, restated by
 * tests/detections_ref.py (the checker; like the rest of the front-end not pinned to the reference binary):
 *   1. Score (flame.cc:1212-1251).  `score` starts all NaN.  The scan covers rows ii in [border + row_offset,
 *      height - border - row_offset) and columns jj in [border, width - border), border and row_offset as in
 *      flame_stereo_detect_features: (int)(rescale_factor_max * win_size / 2 + 1) in float, and height / 3 with do_letterbox,
 *      else 0.  Per pixel, with g2 = min_grad_mag * min_grad_mag in float: skipped if gx * gx + gy * gy < g2;
 *      epi = referenceEpiline(cv::Point2f(ii, jj)) -- (row, col) passed as (x, y), kept as written --;
 *      epigrad = gx * epi.x + gy * epi.y; skipped if epigrad * epigrad < g2; else score(ii, jj) = |epigrad|.
 *      The score does not depend on detection_win_size, the cell mask or the inverse-depth map: of `dparams` only
 *      min_grad_mag is read, of `params` rescale_factor_max, win_size and do_letterbox.
 *   2. Colour (drawDetections, flame.cc:2363-2412).  The picture starts (0, 0, 0); a pixel with a non-NaN score v becomes
 *      utils::jet(v, 0, max_score) (utils/visualization.h:142-167: the first branch in float, the other three through double,
 *      truncated to a byte; bytes c[0], c[1], c[2] in memory); a NaN score (never scanned, skipped, or a NaN epigrad, which
 *      fails `epigrad * epigrad < g2` and stays NaN through fast_abs) keeps (0, 0, 0).  The reference passes the literal
 *      max_score = 0.005f: with the default min_grad_mag = 5 every scored pixel then clamps to vmax and the picture is
 *      two-valued, so max_score is a parameter here (0.005f reproduces the reference).
 *   3. Blend (flame.cc:2388) with cvtColor(img, GRAY2RGB), three equal bytes g: per channel
 *      t = (float)c * (float)0.7 + (float)g * (float)0.3 in float -- two rounded products, one rounded sum, no FMA --, then
 *      saturate_cast<uchar>(t): round to nearest, ties to even, clamped to [0, 255].  An unscored pixel is rne(g * 0.3f).
 *      UNPINNED: this reads the MatExpr `0.7 * A + 0.3 * B` on 8-bit data as cv::addWeighted(A, 0.7, B, 0.3, 0); OpenCV is
 *      not part of this tree, so the rounding is restated here and in the checker, not checked against it.
 *   4. flip != 0 reverses the linear pixel order of the finished picture (cv::flip(img, img, -1)).  debug_draw_text_overlay
 *      (cv::putText) is treated as false; cv::drawKeypoints is commented out in the reference.
 * A pixel that passes the first gradient test where the reference's referenceEpiline asserts (zero translation) is treated as
 * unscored on the device and reported: FLAME_NLTGV2_ERR_ASSERT, stats->error_pixel set, img_out unspecified. */
typedef struct flame_stereo_detections_stats {
  int32_t num_scored;    /* pixels with a non-NaN score */
  int32_t num_examined;  /* pixels of the scan rectangle */
  int32_t error_pixel;   /* -1, or the lowest row * width + col whose referenceEpiline asserted */
} flame_stereo_detections_stats;
/* FLAME_NLTGV2_ERR_INVALID_ARG, before anything is enqueued or written, for a NULL params, dparams, q, t or img_out, a
 * max_score that is not finite or <= 0, a frame that is not resident, or a negative border; FLAME_NLTGV2_ERR_NO_GRAPH when no
 * camera is set.  Changes nothing in the context but its scratch buffers: the resident set, the projected set, the frames and
 * the match records stay as they are.  img_out: height * width * 3 bytes of host memory; `stats` may be NULL.  Enqueues on the
 * context's stream and waits once; flame_stereo_last_kernel_ms covers its kernel. */
int flame_stereo_draw_detections(flame_stereo_ctx* ctx, const flame_stereo_params* params,
                                 const flame_stereo_detect_params* dparams, uint32_t ref_frame_id,
                                 const float q_ref_to_prev[4], const float t_ref_to_prev[3], float max_score, int flip,
                                 uint8_t* img_out, flame_stereo_detections_stats* stats);

/* ---- Refining a frame's pose against a pose-frame's map: direct image alignment ---------------------------------------------
 * Every other stage takes the pose of every frame on trust (flame_stereo_pose, KRKinv / Kt, T_world_cam).  These calls correct
 * the relative pose T = T_ref_to_new of a new frame against a resident reference frame that has a dense inverse-depth map, by
 * Gauss-Newton on the photometric error over a few pyramid levels.  UNPINNED: the reference has no direct alignment (it takes
 * its poses from outside, flame.h:134-140), so everything about the alignment below is this library's own statement;
 * tests/align_ref.py restates it in numpy and is the checker, bit for bit.  The pyramid follows utils::Frame::create with
 * num_levels > 1 (frame.cc:33-71): getGaussianPyramid (pyramids.h:42-51: cv::pyrDown per level), getGradientPyramid
 * (pyramids.h:72-90) and getCentralGradient (image_utils.h:425-474).
 *
 * PYRAMID LEVELS.  Level 0 is the resident frame (flame_stereo_add_frame / add_raw_frame) and needs no call.  Level l >= 1 has the
 * size ((w + 1) / 2, (h + 1) / 2) of level l - 1 (integer division) and is cv::pyrDown's rule stated in integers:
 *     out(y, x) = (sum_{i, j = -2 .. 2} k_i k_j * src(r(2 y + i), r(2 x + j)) + 128) >> 8,     k = 1 4 6 4 1,
 * r = the BORDER_REFLECT_101 rule stated at flame_stereo_add_frame, repeated until the coordinate lies inside (a coarse level can
 * be narrower than 3).  UNPINNED against OpenCV, which is on neither tree: the formula is the definition.  The gradients of
 * level l >= 1 are getCentralGradient's of that level's image: 0.5f * ((float)right - (float)left) inside, (float)next -
 * (float)this in the first column / row, (float)this - (float)previous in the last.  Levels >= 1 are stored unpadded, image and
 * both gradient planes.
 *   flame_stereo_build_pyramid   builds levels 1 .. n_levels - 1 of resident frame `frame_id`; 1 <= n_levels <= 5 and every level
 *      must keep w_l, h_l >= 4, else FLAME_NLTGV2_ERR_INVALID_ARG (also for an unknown frame) and nothing changes.  The levels
 *      belong to the frame: flame_stereo_drop_frame, replacing the frame (add_frame / add_raw_frame with its id), a prune that
 *      releases it and flame_stereo_set_camera release them; their buffer travels with the frame's other buffers (it waits with them
 *      for the next add_frame and is reused by the next build_pyramid of that frame).  Building again with the same n_levels is a
 *      no-op; with another n_levels all levels are rebuilt.  One kernel per level; enqueue-only on the context's stream once the
 *      frame's buffer exists (the first build of a buffer set allocates).
 *   flame_stereo_download_pyramid_level  copies level `level` back: w_l x h_l each, unpadded, any pointer may be NULL; for level 0
 *      the inner width x height of the padded planes.  FLAME_NLTGV2_ERR_INVALID_ARG for an unknown frame or a level not built.
 *
 * THE LINEARISATION (flame_stereo_align_linearize): one Gauss-Newton system at the pose (q, t) = T_ref_to_new on level `level`.
 *   The map      width x height floats at level-0 resolution, in host memory (idepthmap_host) or in device memory
 *                (idepthmap_device, read in place: the caller orders the work that produces it before the call), exactly one of
 *                the two.  Level l reads it by decimation: d = map(y * 2^l, x * 2^l).  No map pyramid, nothing is averaged.
 *   The camera   the context's; K[1] = K[3] = K[6] = K[7] = 0 and K[8] = 1 are required.  fx_l = K[0] / 2^l, cx_l = K[2] / 2^l,
 *                fy_l = K[4] / 2^l, cy_l = K[5] / 2^l (exact divisions).
 *   The pose     q = (w, x, y, z) and t in double.  R is formed in double, + - * only, in this association:
 *                  tx = 2 x, ty = 2 y, tz = 2 z;  twx = tx w, twy = ty w, twz = tz w;  txx = tx x, txy = ty x, txz = tz x;
 *                  tyy = ty y, tyz = tz y, tzz = tz z;
 *                  R = [1 - (tyy + tzz), txy - twz, txz + twy;  txy + twz, 1 - (txx + tzz), tyz - twx;
 *                       txz - twy, tyz + twx, 1 - (txx + tyy)]       (q is not normalised here)
 *                then R and t are rounded to float32.  The kernel sees only those 12 floats.
 *   Per level pixel (x, y), linear index y * w_l + x, all in float32, one rounding per operation, in exactly this association:
 *     1. eligible iff border <= x < w_l - border, the same in y, and d == d && d > 0 && d < inf; a pixel inside the border ring
 *        whose d fails is counted in n_no_depth.  Pixels of the border ring are counted nowhere.
 *     2. a = ((float)x - cx_l) / fx_l,  b = ((float)y - cy_l) / fy_l
 *     3. Xx = ((R0 a + R1 b) + R2) + t0 d,  Xy = ((R3 a + R4 b) + R5) + t1 d,  Xz = ((R6 a + R7 b) + R8) + t2 d;
 *        !(Xz > 0): counted in n_behind.
 *     4. xn = Xx / Xz,  yn = Xy / Xz,  rho = d / Xz,  u = fx_l xn + cx_l,  v = fy_l yn + cy_l
 *     5. inside iff u >= border && v >= border && u < (float)(w_l - 1 - border) && v < (float)(h_l - 1 - border), decided before
 *        any conversion to an integer (a NaN fails it); else counted in n_outside.  border >= 1.
 *     6. x0 = (int)u, y0 = (int)v, dx = u - x0, dy = v - y0 and the weights and sum order of flame_stereo_add_raw_frame:
 *        w11 = dx dy, w01 = dx - w11, w10 = dy - w11, w00 = ((1 - dx) - dy) + w11,
 *        value = ((w00 g00 + w01 g01) + w10 g10) + w11 g11, on the new frame's level image (I), gradx (gx) and grady (gy).
 *     7. r = I - (float)I_ref(x, y);  Gx = fx_l gx,  Gy = fy_l gy,  xy = xn yn
 *        J0 = Gx rho    J1 = Gy rho    J2 = -((Gx xn + Gy yn) rho)
 *        J3 = -(Gx xy + Gy (1 + yn yn))    J4 = Gx (1 + xn xn) + Gy xy    J5 = Gy xn - Gx yn
 *        the derivative of r for the left increment T <- exp(xi) T, xi = (v, omega), in the new camera's frame.
 *     8. ar = |r|,  wgt = ar <= huber_k ? 1 : huber_k / ar; a pixel with wgt < 1 is also counted in n_huber.
 *   Sums     28 doubles, each term formed in double from the float32 factors: H_ij = ((double)wgt (double)J_i) (double)J_j for
 *            i <= j, row-major over the upper triangle (21); b_i = ((double)wgt (double)J_i) (double)r (6);
 *            cost = ((double)wgt (double)r) (double)r.  The order of each sum is the rule of flame_nltgv2_map_error's `sum`
 *            (flame_nltgv2.h) over the linear level-pixel index, +0.0 from every pixel that contributes nothing: chunks of 1024
 *            consecutive indices, the last one padded; within a chunk p[t] += p[t + s] for s = 512 .. 1; the chunk partials
 *            strided (q[t] = b[t] + b[t + 1024] + ... from +0.0), then pairwise.  No floating-point atomics: two calls give
 *            the same bytes.
 *   Counts   n_used + n_no_depth + n_behind + n_outside = the pixels inside the border ring; n_huber <= n_used.
 *   Enqueues on the context's stream and waits once; the result comes through the context's pinned block;
 *   flame_stereo_last_kernel_ms covers its kernels.  FLAME_NLTGV2_ERR_INVALID_ARG, with nothing changed, for: a NULL params, q, t
 *   or out; an unknown frame id; a level not built for both frames; border < 1 or 2 border + 2 > min(w_l, h_l); both or neither
 *   map pointer; huber_k <= 0 or not finite; a non-finite pose; a camera that is not of the form above.
 *   FLAME_NLTGV2_ERR_NO_GRAPH without a camera.
 *
 * THE DRIVER (flame_stereo_align_frame).  State: q (unit, double) and t (double), from q_init (normalised on entry: q / sqrt(((w w +
 * x x) + y y) + z z)) and t_init.  For level = coarsest_level down to finest_level:
 *     1. linearise at T (the level's first evaluation; trace: delta = 0, accepted = 1).
 *     2. n_used < min_pixels: end with status FLAME_STEREO_ALIGN_TOO_FEW and T as it is.
 *     3. solve (H + lm_lambda diag H) delta = -b by a 6 x 6 Cholesky in double (L L^T, pivots in order, no pivoting); a pivot that
 *        is not > 0 or a non-finite delta: raise FLAME_STEREO_ALIGN_FLAG_NOT_PD and end the level.
 *     4. T' = exp(delta) T, delta = (v, o):  th2 = (o0 o0 + o1 o1) + o2 o2.  th2 < 1e-10:  A = 1 - th2 / 6, B = 0.5 - th2 / 24,
 *        C = 1 / 6 - th2 / 120, Hs = 0.5 - th2 / 48, Hc = 1 - th2 / 8.  Else th = sqrt(th2):  A = sin th / th,
 *        B = (1 - cos th) / th2, C = (th - sin th) / (th2 th), Hs = sin(0.5 th) / th, Hc = cos(0.5 th).
 *        t' = ((t + A (o x t)) + B (o x (o x t))) + ((v + B (o x v)) + C (o x (o x v)))   per component,
 *        (a x b)_0 = a1 b2 - a2 b1 and cyclic;  dq = (Hc, Hs o);  q' = dq (x) q (Hamilton product, each component left to right),
 *        then q' / sqrt(((w w + x x) + y y) + z z).
 *     5. linearise at T' (trace: the delta that led to it).  This is also the next iteration's system: one launch per iteration.
 *     6. accept iff cost' / n_used' < cost / n_used, compared in double (n_used' = 0 is never accepted).  Rejected: keep T, raise
 *        FLAME_STEREO_ALIGN_FLAG_REJECTED, end the level.
 *     7. accepted: T = T'; end the level when max |delta_i| < min_step, or after max_iters_per_level iterations (then
 *        FLAME_STEREO_ALIGN_FLAG_MAX_ITERS is raised).
 *   Every evaluation appends one trace entry while there is room (max_trace); *n_trace is the number of evaluations made.
 *   The defaults of flame_stereo_default_align_params are design choices of this library, not the reference's and not test
 *   thresholds: border 2, huber_k 10 grey levels, coarsest_level 2, finest_level 0, max_iters_per_level 10, min_pixels 100,
 *   min_step 1e-5, lm_lambda 0.
 *   FLAME_NLTGV2_ERR_INVALID_ARG as for the linearisation at every level of the range, and for coarsest_level < finest_level,
 *   finest_level < 0, max_iters_per_level < 1, min_pixels < 1, a negative or non-finite min_step or lm_lambda, a zero q_init,
 *   max_trace < 0 or a NULL trace with max_trace > 0; nothing is enqueued then. */
typedef struct flame_stereo_align_params {
  int32_t border;              /* 2 */
  float huber_k;               /* 10 */
  int32_t coarsest_level;      /* 2 */
  int32_t finest_level;        /* 0 */
  int32_t max_iters_per_level; /* 10 */
  int32_t min_pixels;          /* 100 */
  double min_step;             /* 1e-5 */
  double lm_lambda;            /* 0 */
} flame_stereo_align_params;
void flame_stereo_default_align_params(flame_stereo_align_params* p);

typedef struct flame_stereo_align_system {
  double H[21];   /* upper triangle, row-major: H00 H01 .. H05 H11 .. H55 */
  double b[6];
  double cost;
  int32_t n_used, n_no_depth, n_behind, n_outside, n_huber;
  int32_t reserved_;
} flame_stereo_align_system;

typedef struct flame_stereo_align_trace {
  int32_t level;
  int32_t accepted;   /* 1: a level's first evaluation, or an accepted step; 0: rejected */
  double q[4], t[3];  /* the pose the evaluation was made at */
  double delta[6];    /* the step that led to it (0 for a level's first evaluation) */
  flame_stereo_align_system sys;
} flame_stereo_align_trace;

enum { FLAME_STEREO_ALIGN_OK = 0, FLAME_STEREO_ALIGN_TOO_FEW = 1 };
enum { FLAME_STEREO_ALIGN_FLAG_NOT_PD = 1, FLAME_STEREO_ALIGN_FLAG_REJECTED = 2, FLAME_STEREO_ALIGN_FLAG_MAX_ITERS = 4 };

typedef struct flame_stereo_align_result {
  int32_t status;          /* FLAME_STEREO_ALIGN_OK or FLAME_STEREO_ALIGN_TOO_FEW */
  int32_t flags;           /* FLAME_STEREO_ALIGN_FLAG_* */
  double q[4], t[3];       /* the final pose */
  float q_f32[4], t_f32[3], R_f32[9]; /* its roundings: what flame_stereo_pose takes, and the R the kernel saw */
  double first_mean_cost;  /* cost / n_used of the first evaluation (NaN when n_used = 0) */
  double last_mean_cost;   /* ... of the evaluation at the final pose */
  int32_t iters[5];        /* accepted steps per level, by level */
  int32_t n_evals;         /* linearisations made */
} flame_stereo_align_result;

int flame_stereo_build_pyramid(flame_stereo_ctx* ctx, uint32_t frame_id, int n_levels);
int flame_stereo_download_pyramid_level(flame_stereo_ctx* ctx, uint32_t frame_id, int level, uint8_t* img, float* gradx,
                                        float* grady);
int flame_stereo_align_linearize(flame_stereo_ctx* ctx, const flame_stereo_align_params* params, uint32_t ref_frame_id,
                                 uint32_t new_frame_id, int level, const float* idepthmap_host, const void* idepthmap_device,
                                 const double q_ref_to_new[4], const double t_ref_to_new[3], flame_stereo_align_system* out);
int flame_stereo_align_frame(flame_stereo_ctx* ctx, const flame_stereo_align_params* params, uint32_t ref_frame_id,
                             uint32_t new_frame_id, const float* idepthmap_host, const void* idepthmap_device,
                             const double q_init[4], const double t_init[3], flame_stereo_align_result* out,
                             flame_stereo_align_trace* trace, int max_trace, int* n_trace);

/* Options.  LANES_PER_FEATURE: 16 (a 16-lane row shares a feature and splits the epipolar walk), 1 (one lane walks the
 * whole per-feature body) or 0 (default: 16 up to 10240 features, 1 above -- whichever is faster on MI355X); same results
 * bit for bit.  GRAPH_COPY: how select_graph_features brings its arrays down: 0 (default) the whole output block in one
 * copy and one wait, its sections spaced by the record count; 1 the counters first, then 24 bytes per selected vertex
 * (two waits); same results (profiles/graph_inputs.txt has both timings).  RECORD_MATCHES: 0 (default) or 1: the updates also
 * record what flame_stereo_draw_matches paints; same feature records, statistics and return codes. */
enum { FLAME_STEREO_OPT_LANES_PER_FEATURE = 1, FLAME_STEREO_OPT_GRAPH_COPY = 2, FLAME_STEREO_OPT_RECORD_MATCHES = 3 };
int flame_stereo_set_option(flame_stereo_ctx* ctx, int option, int value);

/* Device time of the last update kernel (or of the kernels of the last project_features / detect_features /
 * prune_pose_frames / prune_features / select_graph_features[_arrays] / draw_matches / draw_detections /
 * build_pyramid / align_linearize, or of the last linearisation of align_frame) in milliseconds (HIP events on the context's stream); < 0 if none. */
float flame_stereo_last_kernel_ms(flame_stereo_ctx* ctx);
int flame_stereo_last_hip_error(const flame_stereo_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* FLAME_STEREO_H_ */
