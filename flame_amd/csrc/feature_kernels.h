// feature_kernels.h -- launch wrappers of feature_kernels.hip: projectFeatures and detectFeatures on the resident
// feature set (include/flame_stereo.h's device side).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stereo_kernels.h"

namespace flame_hip {

// One per pose-frame the resident features may refer to: the geometry of T_ref_to_cur = fcur.pose.inverse() *
// fref.pose (flame.cc:1786), loaded by the host (load_geometry) from flame_stereo_pose.q/t_ref_to_new.
struct ProjectPoseEntry {
  uint32_t frame_id;
  Geo geo;
};

// cv::Rect_<float> valid_region(border, border + row_offset, cols - 2 border, rows - 2 border - 2 row_offset)
// (flame.cc:1772-1774), as the float values the reference's Rect holds.
struct ProjectRegion {
  float x, y, w, h;
};

// The candidate pixels and the cell grid of detectFeatures (flame.cc:1001-1004, 1020-1021).
struct DetectGrid {
  int win, hc, wc;
  int r_lo, r_hi, c_lo, c_hi;  // rows [r_lo, r_hi), cols [c_lo, c_hi)
  float g2;                    // Params::min_grad_mag^2
};

// What the detection loop writes into a new FeatureWithIDepth (flame.cc:739-753).
struct DetectInit {
  uint32_t first_id, ref_frame_id;
  float idepth_init, idepth_var_init;
};

// cv::Rect valid_region(border, border + row_offset, width - 2 border, height - 2 border - 2 row_offset) of
// prunePoseFrames (flame.cc:604-606): integers, tested with rect_contains (stereo_geometry.hpp).
struct PruneRegion {
  int x, y, w, h;
};

// k_prune_move's flag byte per feature.
constexpr uint8_t kPruneKeep = 1, kPruneRewritten = 2, kPruneMoved = 4, kPruneInvalidated = 8;

// stats words of the stages: [kFrontAssert] lowest index that hit a reference assert, [kFrontBadFrame] lowest
// feature index with an unknown frame id (both start at INT_MAX), [kFrontCount] kept / new features;
// the prune adds [kPruneStatMoved] and [kPruneStatInvalidated].
constexpr int kFrontAssert = 0, kFrontBadFrame = 1, kFrontCount = 2, kPruneStatMoved = 3, kPruneStatInvalidated = 4,
              kFrontWords = 8;

// k_project_flag + k_project_scatter: `feats` (n) -> stably compacted `feats_out` / `proj_out`; proj_tmp and keep are
// n-sized scratch, counts (n + 255) / 256 ints.
hipError_t launch_project_features(const StereoCamera& cam, const ProjectRegion& region, int n_poses,
                                   const ProjectPoseEntry* poses, uint32_t cur_frame_id, int n, const StereoFeature* feats,
                                   StereoFeature* proj_tmp, uint8_t* keep, int* counts, StereoFeature* feats_out,
                                   StereoFeature* proj_out, int* stats, hipStream_t stream);
// clear + k_detect_mask + k_detect_cells + k_detect_count + k_detect_emit: the new features go to out[0 .. count);
// `blocked` and `cell_key` hold hc * wc entries, counts (hc * wc + 255) / 256, `out` room for hc * wc records.  mask_xy: n_mask points, `mask_stride` floats apart.
// idepthmap: width x height floats in device memory, or NULL.
hipError_t launch_detect_features(const DetectGrid& grid, const Geo& geo, const StereoCamera& cam, const float* gx_pad,
                                  const float* gy_pad, int n_mask, const float* mask_xy, int mask_stride, uint8_t* blocked,
                                  unsigned long long* cell_key, int* counts, const DetectInit& init, const float* idepthmap,
                                  StereoFeature* out, int* stats, hipStream_t stream);
// k_prune_move + k_prune_commit (Flame::prunePoseFrames, flame.cc:608-700) on `feats` (n records; [first_new, n) are
// new_feats_).  keep_ids: n_keep ids; dropped: n_dropped entries with the geometry of target.pose.inverse() * pf.pose.
// `moved` is n records of scratch, `flags` n bytes, `counts` 3 * ((n + 255) / 256) ints, `feats_out` room for n records.
// Afterwards, unless stats[kFrontAssert] or stats[kFrontBadFrame] left INT_MAX (then nothing was written to feats or
// feats_out): stats[kFrontCount] records remain -- in `feats`, in place, when that is n, else compacted in `feats_out`.
hipError_t launch_prune_features(const StereoCamera& cam, const PruneRegion& region, int n_keep, const uint32_t* keep_ids,
                                 int n_dropped, const ProjectPoseEntry* dropped, uint32_t target_frame_id, int first_new, int n,
                                 StereoFeature* feats, StereoFeature* moved, uint8_t* flags, int* counts,
                                 StereoFeature* feats_out, int* stats, hipStream_t stream);

// syncGraph's preprocessing (flame.cc:1954-1980): what the rule reads of flame::Params, and graph_scale.
struct SelectRule {
  float idepth_var_max_graph, min_height, max_height, graph_scale;
  int adaptive_data_weights;
};
// One per pose-frame: row 1 of the rotation of pf.pose (camera -> world) and the y of its translation -- all that
// -world.y needs (select_pose_entry forms them on the host from the quaternion).
struct SelectPoseEntry {
  uint32_t frame_id;
  float r10, r11, r12, ty;
};
SelectPoseEntry select_pose_entry(uint32_t frame_id, const float q[4], const float t[3]);
// k_select_flag's class byte per record.
constexpr uint8_t kSelectTaken = 0, kSelectInvalid = 1, kSelectFailVar = 2, kSelectFailHeight = 3, kSelectNone = 255;
// The selection's stats words beyond kFrontAssert / kFrontBadFrame / kFrontCount (= V): the three reject counts and
// [kSelectBadId], the lowest selected index whose id does not fit int32_t (starts at INT_MAX).
constexpr int kSelectStatInvalid = 3, kSelectStatFailVar = 4, kSelectStatFailHeight = 5, kSelectBadId = 6;
// k_select_flag + k_select_scatter on `feats` / `proj` (n index-aligned records each, only read).  `cls` n bytes,
// `counts` 4 * ((n + 255) / 256) ints.  `out`: kFrontWords stats words (preset by the caller: the three error words at
// INT_MAX, the rest 0), then feat_id[V] | pos[2V] | data_term[V] | data_weight[V] | feat_index[V] with the sections
// `section` words apart (section >= n), or V words apart when section <= 0; room for kFrontWords + 6 n words.  Nothing but
// the error words is written when one of them was raised.
hipError_t launch_select_graph_features(const StereoCamera& cam, const SelectRule& rule, int n_poses,
                                        const SelectPoseEntry* poses, int n, const StereoFeature* feats,
                                        const StereoFeature* proj, uint8_t* cls, int* counts, int section, int* out,
                                        hipStream_t stream);

}  // namespace flame_hip
