// stereo_capi.hip -- C-ABI of include/flame_stereo.h: resident frames (padded image + gradients built on the
// device), the per-launch pose table, the host/device feature-array entry points of the per-feature epipolar
// inverse-depth update, projectFeatures / detectFeatures / prunePoseFrames on the resident set, and the selection of the
// graph's vertices (syncGraph's preprocessing).  All arithmetic of the path runs in
// stereo_kernels.hip and feature_kernels.hip; this file only moves bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <unordered_map>
#include <vector>

#include "flame_stereo.h"
#include "stereo_kernels.h"
#include "feature_kernels.h"
#include "debug_kernels.h"
#include "detections_kernels.h"
#include "matches_kernels.h"
#include "input_kernels.h"
#include "input_params.hpp"
#include "align_kernels.h"
#include "align_host.hpp"
#include "roctx_ranges.hpp"

using namespace flame_hip;

namespace {

struct Frame {
  uint8_t* img_pad = nullptr;
  float* gx_pad = nullptr;
  float* gy_pad = nullptr;
  uint8_t* pyr = nullptr;  // levels >= 1 (align_host.hpp, place_levels), allocated by the first build_pyramid; travels with the set
  int pyr_levels = 0;      // n_levels of the last build_pyramid; 0: none since the frame was added
};

}  // namespace

struct flame_stereo_ctx {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool timed = false;
  int last_hip = 0;
  bool have_camera = false;
  StereoCamera cam{};
  std::unordered_map<uint32_t, Frame> frames;
  std::vector<Frame> spare;  // buffers of dropped frames, reused by the next add_frame: hipFree waits for every stream of the device, also
                             // for a solver that runs beside the tracker (tools/frame_loop.py --pipelined: 0.5 ms per frame).
                             // At most kSpareFrames of them (release_frame).
  uint8_t* d_raw = nullptr;  // staging of the unpadded upload; the rectified grey image of add_raw_frame
  size_t raw_cap = 0;
  // add_raw_frame (input_kernels.hip)
  bool have_input = false;  // set_input since the last set_camera
  flame_stereo_input_params input{};
  uint8_t* d_rawsrc = nullptr;  // staging of a raw frame that comes from the host
  size_t rawsrc_cap = 0;
  int* d_istats = nullptr;  // kInputWords ints
  int* h_istats = nullptr;  // pinned, the same
  StereoPoseEntry* d_poses = nullptr;
  size_t poses_cap = 0;
  StereoPoseEntry* h_poses = nullptr;  // pinned
  size_t h_poses_cap = 0;
  StereoFeature* d_feats = nullptr;
  size_t feats_cap = 0;
  int* d_stats = nullptr;
  int* h_stats = nullptr;  // pinned, kStatWords ints
  StereoFeature* d_res = nullptr;  // the resident feature set (flame_stereo_set_features)
  size_t res_cap = 0;
  int n_res = 0;
  int lanes_per_feature = 0;  // 0 = by feature count (pick_lanes)
  // projectFeatures / detectFeatures (feature_kernels.hip)
  StereoFeature* d_res_alt = nullptr;  // the other buffer of the resident set's ping-pong pair
  size_t res_alt_cap = 0;
  StereoFeature* d_proj = nullptr;  // the projected set (Flame::feats_in_curr_) and its other buffer
  size_t proj_cap = 0;
  StereoFeature* d_proj_alt = nullptr;
  size_t proj_alt_cap = 0;
  int n_proj = 0;
  StereoFeature* d_proj_tmp = nullptr;  // one projected record per resident feature
  size_t proj_tmp_cap = 0;
  uint8_t* d_keep = nullptr;
  size_t keep_cap = 0;
  int* d_groups = nullptr;  // per-workgroup counts of the compactions
  size_t groups_cap = 0;
  ProjectPoseEntry* d_ppose = nullptr;
  size_t ppose_cap = 0;
  uint32_t* d_keep_ids = nullptr;  // prune_pose_frames: the ids of the kept pose-frames
  size_t keep_ids_cap = 0;
  unsigned long long* d_cell_key = nullptr;
  size_t cell_key_cap = 0;
  uint8_t* d_blocked = nullptr;
  size_t blocked_cap = 0;
  float* d_map = nullptr;  // a host idepth map, uploaded
  size_t map_cap = 0;
  float* d_mask = nullptr;  // a host mask, uploaded
  size_t mask_cap = 0;
  int* d_fstats = nullptr;
  int* h_fstats = nullptr;  // pinned, kFrontWords ints
  // select_graph_features (feature_kernels.hip)
  bool aligned = false;  // the resident and the projected set are index-aligned (set by project_features)
  SelectPoseEntry* d_spose = nullptr;
  size_t spose_cap = 0;
  int* d_sel = nullptr;  // the output block: kFrontWords stats words + 6 words per record
  size_t sel_cap = 0;
  int* h_sel = nullptr;  // pinned, the same
  size_t h_sel_cap = 0;
  int graph_copy = 0;  // FLAME_STEREO_OPT_GRAPH_COPY
  // draw_features (debug_kernels.hip): per-pixel owner words + the two counters behind them, and the image;
  // draw_detections (detections_kernels.hip) keeps its kDetWords stats words in d_owner and paints into d_draw too
  uint32_t* d_owner = nullptr;
  size_t owner_cap = 0;
  uint8_t* d_draw = nullptr;
  size_t draw_cap = 0;
  // draw_matches (matches_kernels.hip): the draw records of the last update, and the lists of the fold
  int record_matches = 0;  // FLAME_STEREO_OPT_RECORD_MATCHES
  MatchRecord* d_match = nullptr;
  size_t match_cap = 0;
  bool match_stand = false;  // records of an enqueued update stand (whether it hit an assert shows in h_stats once the stream is idle)
  int match_n = 0;
  uint32_t match_frame = 0;
  uint32_t* d_mlist = nullptr;  // cnt, offset, fill (one word per pixel each) and the kMatchCounts counters behind them
  size_t mlist_cap = 0;
  uint64_t* d_mentries = nullptr;
  size_t mentries_cap = 0;
  size_t match_last_total = 0;
  // align_linearize / align_frame (align_kernels.hip)
  double* d_apart = nullptr;  // [kAlignSums][chunks] partials
  size_t apart_cap = 0;
  AlignSystem* d_asys = nullptr;
  AlignSystem* h_asys = nullptr;  // pinned
};

namespace {

#define SCHK(ctx, expr)                  \
  do {                                   \
    hipError_t _e = (expr);              \
    if (_e != hipSuccess) {              \
      (ctx)->last_hip = (int)_e;         \
      return _e == hipErrorOutOfMemory ? FLAME_NLTGV2_ERR_OOM : FLAME_NLTGV2_ERR_HIP; \
    }                                    \
  } while (0)

int enter(flame_stereo_ctx* ctx) {
  if (!ctx) return FLAME_NLTGV2_ERR_INVALID_ARG;
  SCHK(ctx, hipSetDevice(ctx->device));
  return 0;
}

void free_frame(Frame& f) {
  if (f.img_pad) (void)hipFree(f.img_pad);
  if (f.gx_pad) (void)hipFree(f.gx_pad);
  if (f.gy_pad) (void)hipFree(f.gy_pad);
  if (f.pyr) (void)hipFree(f.pyr);
  f = Frame{};
}

void drop_all_frames(flame_stereo_ctx* ctx) {
  for (auto& kv : ctx->frames) free_frame(kv.second);
  ctx->frames.clear();
  for (Frame& f : ctx->spare) free_frame(f);  // (the camera changes: another padded size)
  ctx->spare.clear();
}

// The buffers of a frame that leaves go to `spare` for the next add_frame, up to kSpareFrames sets; the rest is freed
// (hipFree waits for the device).  4 covers the steady state of a front-end that drops one non-pose frame per frame and
// prunes one or two pose-frames every few frames, and bounds the idle memory at 4 x 3 padded planes (72 MB at 1080p).
constexpr size_t kSpareFrames = 4;
void release_frame(flame_stereo_ctx* ctx, std::unordered_map<uint32_t, Frame>::iterator it) {
  it->second.pyr_levels = 0;  // (the levels go with the frame; their buffer stays with the set)
  if (ctx->spare.size() < kSpareFrames) ctx->spare.push_back(it->second); else free_frame(it->second);
  ctx->frames.erase(it);
}

size_t padded_pixels(const StereoCamera& c) { return (size_t)(c.width + 2 * c.border) * (size_t)(c.height + 2 * c.border); }

// The buffer set of frame `frame_id` for add_frame / add_raw_frame to fill: the one the id has (adding an existing id replaces
// it), else one from `spare`, else a new one.  On failure the id is not resident.
int acquire_frame(flame_stereo_ctx* ctx, uint32_t frame_id, Frame** out) {
  Frame& f = ctx->frames[frame_id];
  const size_t px = padded_pixels(ctx->cam);
  if (!f.img_pad && !ctx->spare.empty()) {
    f = ctx->spare.back();
    ctx->spare.pop_back();
  }
  if (!f.img_pad) {
    hipError_t e = hipMalloc((void**)&f.img_pad, px);
    if (e == hipSuccess) e = hipMalloc((void**)&f.gx_pad, px * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&f.gy_pad, px * sizeof(float));
    if (e != hipSuccess) {
      free_frame(f);
      ctx->frames.erase(frame_id);
      ctx->last_hip = (int)e;
      return e == hipErrorOutOfMemory ? FLAME_NLTGV2_ERR_OOM : FLAME_NLTGV2_ERR_HIP;
    }
  }
  f.pyr_levels = 0;  // (a replaced frame's levels describe the old image)
  *out = &f;
  return 0;
}

template <typename T>
int grow(flame_stereo_ctx* ctx, T** p, size_t* cap, size_t count) {
  if (*cap >= count) return 0;
  if (*p) SCHK(ctx, hipFree(*p));
  *p = nullptr, *cap = 0;
  const size_t want = count + count / 2 + 16;
  SCHK(ctx, hipMalloc((void**)p, want * sizeof(T)));
  *cap = want;
  return 0;
}

// Fills the device pose table and launches; the feature array is already on the device.
// 16 lanes per feature shorten a feature's dependent chain (3.1 k instead of 6.0 k instructions per wave: the epipolar walk
// is split over the row) but replicate its scalar part 16 times: 4 features per wave.  That pays while the chip has room for
// the 16x as many waves -- measured on MI355X (1024 SIMDs): 20.2 vs 24.0 us at 8.4 k features, 32 vs 26 us at 18 k,
// 75 vs 30 us at 57 k.  Above ~2.5 waves per SIMD one lane per feature is faster.
int pick_lanes(const flame_stereo_ctx* ctx, int n_feats) {
  if (ctx->lanes_per_feature) return ctx->lanes_per_feature;
  return n_feats <= 10240 ? 16 : 1;
}

int enqueue_update(flame_stereo_ctx* ctx, const flame_stereo_params* params, uint32_t new_frame_id, uint32_t curr_pf_id,
                   int n_poses, const flame_stereo_pose* poses, int n_feats, StereoFeature* d_feats) {
  ctx->match_stand = false;  // (whatever this update comes to, the records of an earlier one no longer describe the last update)
  if (!params || n_poses < 0 || n_feats < 0 || (n_poses > 0 && !poses)) return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (!ctx->have_camera) return FLAME_NLTGV2_ERR_NO_GRAPH;
  auto nf = ctx->frames.find(new_frame_id);
  if (nf == ctx->frames.end()) return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (ctx->h_poses_cap < (size_t)n_poses) {
    if (ctx->h_poses) SCHK(ctx, hipHostFree(ctx->h_poses));
    ctx->h_poses = nullptr, ctx->h_poses_cap = 0;
    const size_t want = (size_t)n_poses * 2 + 16;
    SCHK(ctx, hipHostMalloc((void**)&ctx->h_poses, want * sizeof(StereoPoseEntry), hipHostMallocDefault));
    ctx->h_poses_cap = want;
  }
  if (int rc = grow(ctx, &ctx->d_poses, &ctx->poses_cap, (size_t)n_poses + 1)) return rc;
  MatchRecord* records = nullptr;
  if (ctx->record_matches) {
    if (int rc = grow(ctx, &ctx->d_match, &ctx->match_cap, (size_t)n_feats + 1)) return rc;
    records = ctx->d_match;
  }
  // the pinned table may still be in flight from the previous launch on this stream
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < n_poses; ++k) {
    auto it = ctx->frames.find(poses[k].frame_id);
    if (it == ctx->frames.end()) return FLAME_NLTGV2_ERR_INVALID_ARG;
    StereoPoseEntry& e = ctx->h_poses[k];
    std::memset(&e, 0, sizeof e);
    e.frame_id = poses[k].frame_id;
    e.img_pad = it->second.img_pad;
    fill_pose_entry(&e, ctx->cam, poses[k]);
  }
  if (n_poses > 0)
    SCHK(ctx, hipMemcpyAsync(ctx->d_poses, ctx->h_poses, (size_t)n_poses * sizeof(StereoPoseEntry), hipMemcpyHostToDevice,
                             ctx->stream));
  std::memset(ctx->h_stats, 0, kStatWords * sizeof(int));
  ctx->h_stats[kStatAssert] = ctx->h_stats[kStatBadFrame] = INT_MAX;
  SCHK(ctx, hipMemcpyAsync(ctx->d_stats, ctx->h_stats, kStatWords * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  if (records && n_feats > 0)  // (all zero = nothing drawn: the early returns of the kernel need no code)
    SCHK(ctx, hipMemsetAsync(records, 0, (size_t)n_feats * sizeof(MatchRecord), ctx->stream));
  SCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  SCHK(ctx, launch_update_feature_idepths(*params, ctx->cam, n_poses, ctx->d_poses, nf->second.img_pad, nf->second.gx_pad,
                                          nf->second.gy_pad, curr_pf_id, n_feats, d_feats, ctx->d_stats, pick_lanes(ctx, n_feats),
                                          records, ctx->stream));
  SCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed = true;
  SCHK(ctx, hipMemcpyAsync(ctx->h_stats, ctx->d_stats, kStatWords * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if (records) ctx->match_stand = true, ctx->match_n = n_feats, ctx->match_frame = new_frame_id;
  return 0;
}

int report(flame_stereo_ctx* ctx, flame_stereo_stats* stats) {
  int* s = ctx->h_stats;
  for (int c = 0; c < 6; ++c) {  // the counters were accumulated in kStatSlots copies (stereo_kernels.h)
    int sum = 0;
    for (int k = 0; k < kStatSlots; ++k) sum += s[kStatCount + k * kStatSlotStride + c];
    s[c] = sum;
  }
  stats->num_idepth_updates = s[0];
  stats->num_fail_max_var = s[1];
  stats->num_fail_max_dropouts = s[2];
  stats->num_fail_ref_patch_grad = s[3];
  stats->num_fail_ambiguous_match = s[4];
  stats->num_fail_max_cost = s[5];
  stats->success = s[0] > 0;
  stats->error_feature = -1;
  if (s[kStatBadFrame] != INT_MAX) {  // pfs.at() would throw
    stats->error_feature = s[kStatBadFrame];
    return FLAME_NLTGV2_ERR_INVALID_ARG;
  }
  if (s[kStatAssert] != INT_MAX) {
    stats->error_feature = s[kStatAssert];
    return FLAME_NLTGV2_ERR_ASSERT;
  }
  return 0;
}

// grow() for the resident set when it is appended to: the first `keep` records move to the new buffer.
int grow_keep(flame_stereo_ctx* ctx, StereoFeature** p, size_t* cap, size_t count, size_t keep) {
  if (*cap >= count) return 0;
  const size_t want = count + count / 2 + 16;
  StereoFeature* np = nullptr;
  SCHK(ctx, hipMalloc((void**)&np, want * sizeof(StereoFeature)));
  if (keep > 0) {
    hipError_t e = hipMemcpyAsync(np, *p, keep * sizeof(StereoFeature), hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
      (void)hipFree(np);
      ctx->last_hip = (int)e;
      return FLAME_NLTGV2_ERR_HIP;
    }
  }
  if (*p) SCHK(ctx, hipFree(*p));
  *p = np, *cap = want;
  return 0;
}

// `int border = params.rescale_factor_max * params.fparams.win_size / 2 + 1;` (flame.cc:847, 1771): float arithmetic
int front_border(const flame_stereo_params& P) { return (int)(P.rescale_factor_max * P.win_size / 2 + 1); }

// Enqueues the front-end stats block reset (the two error indices at INT_MAX, the count at 0).
int reset_front_stats(flame_stereo_ctx* ctx) {
  ctx->h_fstats[kFrontAssert] = ctx->h_fstats[kFrontBadFrame] = INT_MAX;
  for (int w = kFrontCount; w < kFrontWords; ++w) ctx->h_fstats[w] = 0;
  SCHK(ctx, hipMemcpyAsync(ctx->d_fstats, ctx->h_fstats, kFrontWords * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  return 0;
}

// Flame::prunePoseFrames' feature loops on `d_in` (n records in device memory): validates, uploads the tables, launches
// and waits.  On success *moved_out tells where the records are: false = in place in d_in (nothing was removed), true =
// compacted in ctx->d_res_alt.  Nothing of the context changes here; the callers commit.
int run_prune(flame_stereo_ctx* ctx, const flame_stereo_params* params, uint32_t target_frame_id, int n_keep,
              const uint32_t* keep_ids, int n_dropped, const flame_stereo_pose* dropped, int first_new, int n,
              StereoFeature* d_in, bool* moved_out, flame_stereo_prune_stats* stats) {
  *moved_out = false;
  if (stats) {
    std::memset(stats, 0, sizeof *stats);
    stats->error_feature = -1;
  }
  if (!params || n_keep < 1 || !keep_ids || n_dropped < 0 || (n_dropped > 0 && !dropped) || first_new < 0 || first_new > n)
    return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (!ctx->have_camera) return FLAME_NLTGV2_ERR_NO_GRAPH;
  if (std::find(keep_ids, keep_ids + n_keep, target_frame_id) == keep_ids + n_keep) return FLAME_NLTGV2_ERR_INVALID_ARG;
  for (int k = 0; k < n_dropped; ++k)  // a pose-frame cannot both stay and go (this also keeps the target out of `dropped`)
    if (std::find(keep_ids, keep_ids + n_keep, dropped[k].frame_id) != keep_ids + n_keep) return FLAME_NLTGV2_ERR_INVALID_ARG;
  const int border = front_border(*params);
  if (border < 1) return FLAME_NLTGV2_ERR_INVALID_ARG;  // (rect_contains relies on a rectangle that excludes 0)
  const int row_offset = params->do_letterbox ? ctx->cam.height / 3 : 0;
  const PruneRegion region = {border, border + row_offset, ctx->cam.width - 2 * border,
                              ctx->cam.height - 2 * border - 2 * row_offset};
  if (stats) stats->num_examined = n, stats->num_features = n;
  if (n == 0) return 0;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (buffers may be reallocated; the pinned stats block is reused)
  const size_t groups = ((size_t)n + 255) / 256;
  if (int rc = grow(ctx, &ctx->d_res_alt, &ctx->res_alt_cap, (size_t)n)) return rc;
  if (int rc = grow(ctx, &ctx->d_proj_tmp, &ctx->proj_tmp_cap, (size_t)n)) return rc;
  if (int rc = grow(ctx, &ctx->d_keep, &ctx->keep_cap, (size_t)n)) return rc;
  if (int rc = grow(ctx, &ctx->d_groups, &ctx->groups_cap, 3 * groups)) return rc;
  if (int rc = grow(ctx, &ctx->d_ppose, &ctx->ppose_cap, (size_t)n_dropped + 1)) return rc;
  if (int rc = grow(ctx, &ctx->d_keep_ids, &ctx->keep_ids_cap, (size_t)n_keep)) return rc;
  std::vector<ProjectPoseEntry> table((size_t)n_dropped);
  for (int k = 0; k < n_dropped; ++k) {
    std::memset(&table[k], 0, sizeof table[k]);
    table[k].frame_id = dropped[k].frame_id;
    load_geometry(table[k].geo, ctx->cam, dropped[k].q_ref_to_new, dropped[k].t_ref_to_new);
  }
  if (n_dropped > 0)
    SCHK(ctx, hipMemcpyAsync(ctx->d_ppose, table.data(), (size_t)n_dropped * sizeof(ProjectPoseEntry), hipMemcpyHostToDevice,
                             ctx->stream));
  SCHK(ctx, hipMemcpyAsync(ctx->d_keep_ids, keep_ids, (size_t)n_keep * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  if (int rc = reset_front_stats(ctx)) return rc;
  SCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  SCHK(ctx, launch_prune_features(ctx->cam, region, n_keep, ctx->d_keep_ids, n_dropped, ctx->d_ppose, target_frame_id, first_new,
                                  n, d_in, ctx->d_proj_tmp, ctx->d_keep, ctx->d_groups, ctx->d_res_alt, ctx->d_fstats,
                                  ctx->stream));
  SCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed = true;
  SCHK(ctx, hipMemcpyAsync(ctx->h_fstats, ctx->d_fstats, kFrontWords * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (also: `table` and keep_ids were pageable memory)
  const int* s = ctx->h_fstats;
  if (s[kFrontBadFrame] != INT_MAX) {  // pfs_[feat.frame_id] of a frame that is neither kept nor listed
    if (stats) stats->error_feature = s[kFrontBadFrame];
    return FLAME_NLTGV2_ERR_INVALID_ARG;
  }
  if (s[kFrontAssert] != INT_MAX) {
    if (stats) stats->error_feature = s[kFrontAssert];
    return FLAME_NLTGV2_ERR_ASSERT;
  }
  *moved_out = s[kFrontCount] != n;
  if (stats) {
    stats->num_moved = s[kPruneStatMoved];
    stats->num_invalidated = s[kPruneStatInvalidated];
    stats->num_removed = n - s[kFrontCount];
    stats->num_features = s[kFrontCount];
  }
  return 0;
}

// Releases the resident frames named in `dropped` (the stream is idle: run_prune waited, or nothing was enqueued).
int release_dropped(flame_stereo_ctx* ctx, int n_dropped, const flame_stereo_pose* dropped) {
  int released = 0;
  for (int k = 0; k < n_dropped; ++k) {
    auto it = ctx->frames.find(dropped[k].frame_id);
    if (it == ctx->frames.end()) continue;
    release_frame(ctx, it);
    ++released;
  }
  return released;
}

void clear_graph_inputs(flame_stereo_graph_inputs* out) {
  std::memset(out, 0, sizeof *out);
  out->error_feature = -1;
}

// syncGraph's preprocessing on the index-aligned device arrays d_feats / d_proj (n records each, only read): validates,
// uploads the pose table, launches, copies the result into the pinned block and waits for it.
int run_select(flame_stereo_ctx* ctx, const flame_stereo_graph_params* gp, float graph_scale, int n_poses,
               const flame_stereo_world_pose* poses, int n, const StereoFeature* d_feats, const StereoFeature* d_proj,
               flame_stereo_graph_inputs* out) {
  out->num_examined = n;
  if (n == 0) return 0;
  const size_t groups = ((size_t)n + 255) / 256;
  const size_t words = (size_t)kFrontWords + 6 * (size_t)n;
  if (int rc = grow(ctx, &ctx->d_keep, &ctx->keep_cap, (size_t)n)) return rc;
  if (int rc = grow(ctx, &ctx->d_groups, &ctx->groups_cap, 4 * groups)) return rc;
  if (int rc = grow(ctx, &ctx->d_spose, &ctx->spose_cap, (size_t)n_poses + 1)) return rc;
  if (int rc = grow(ctx, &ctx->d_sel, &ctx->sel_cap, words)) return rc;
  if (ctx->h_sel_cap < words) {
    if (ctx->h_sel) SCHK(ctx, hipHostFree(ctx->h_sel));
    ctx->h_sel = nullptr, ctx->h_sel_cap = 0;
    const size_t want = words + words / 2 + 16;
    SCHK(ctx, hipHostMalloc((void**)&ctx->h_sel, want * sizeof(int), hipHostMallocDefault));
    ctx->h_sel_cap = want;
  }
  std::vector<SelectPoseEntry> table((size_t)n_poses);
  for (int k = 0; k < n_poses; ++k) table[k] = select_pose_entry(poses[k].frame_id, poses[k].q, poses[k].t);
  if (n_poses > 0)
    SCHK(ctx, hipMemcpyAsync(ctx->d_spose, table.data(), (size_t)n_poses * sizeof(SelectPoseEntry), hipMemcpyHostToDevice,
                             ctx->stream));
  for (int w = 0; w < kFrontWords; ++w) ctx->h_fstats[w] = 0;
  ctx->h_fstats[kFrontAssert] = ctx->h_fstats[kFrontBadFrame] = ctx->h_fstats[kSelectBadId] = INT_MAX;
  SCHK(ctx, hipMemcpyAsync(ctx->d_sel, ctx->h_fstats, kFrontWords * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  const SelectRule rule = {gp->idepth_var_max_graph, gp->min_height, gp->max_height, graph_scale, gp->adaptive_data_weights};
  // The copy-out.  0: the whole block in one copy, sections n words apart, one wait.  1: the stats words, a wait, then the
  // 6 V words the kernel packed V words apart, a second wait.  Which is faster: profiles/graph_inputs.txt.
  const bool count_first = ctx->graph_copy == 1;
  SCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  SCHK(ctx, launch_select_graph_features(ctx->cam, rule, n_poses, ctx->d_spose, n, d_feats, d_proj, ctx->d_keep, ctx->d_groups,
                                         count_first ? 0 : n, ctx->d_sel, ctx->stream));
  SCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed = true;
  SCHK(ctx, hipMemcpyAsync(ctx->h_sel, ctx->d_sel, (count_first ? (size_t)kFrontWords : words) * sizeof(int),
                           hipMemcpyDeviceToHost, ctx->stream));
  SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (also: `table` was pageable memory)
  const int* s = ctx->h_sel;
  if (s[kFrontAssert] != INT_MAX || s[kFrontBadFrame] != INT_MAX) {
    // the reference's loop stops at the first record that fails either; within a record the assert comes first
    const bool is_assert = s[kFrontAssert] <= s[kFrontBadFrame];
    out->error_feature = is_assert ? s[kFrontAssert] : s[kFrontBadFrame];
    return is_assert ? FLAME_NLTGV2_ERR_ASSERT : FLAME_NLTGV2_ERR_INVALID_ARG;
  }
  if (s[kSelectBadId] != INT_MAX) {  // an id >= 2^31 among the selected
    out->error_feature = s[kSelectBadId];
    return FLAME_NLTGV2_ERR_INVALID_ARG;
  }
  const int V = s[kFrontCount];
  if (V < 0 || V > n) return FLAME_NLTGV2_ERR_HIP;  // (cannot happen: the kernel counted n records)
  if (count_first && V > 0) {
    SCHK(ctx, hipMemcpyAsync(ctx->h_sel + kFrontWords, ctx->d_sel + kFrontWords, 6 * (size_t)V * sizeof(int), hipMemcpyDeviceToHost,
                             ctx->stream));
    SCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  const size_t S = count_first ? (size_t)V : (size_t)n;
  const int* body = ctx->h_sel + kFrontWords;
  out->V = V;
  out->num_invalid = s[kSelectStatInvalid];
  out->num_fail_var = s[kSelectStatFailVar];
  out->num_fail_height = s[kSelectStatFailHeight];
  if (V > 0) {
    out->feat_id = body;
    out->pos = (const float*)(body + S);
    out->data_term = (const float*)(body + 3 * S);
    out->data_weight = (const float*)(body + 4 * S);
    out->feat_index = body + 5 * S;
  }
  return 0;
}

}  // namespace

extern "C" {

void flame_stereo_default_params(flame_stereo_params* p) {
  if (!p) return;
  p->min_baseline = 0.01f;
  p->do_letterbox = 0;
  p->rescale_factor_min = 0.7f;
  p->rescale_factor_max = 1.4f;
  p->idepth_var_max = 0.5f * 0.5f;
  p->max_dropouts = 5;
  p->outlier_sigma_thresh = 3.0f;
  p->do_meas_fusion = 1;
  p->win_size = 5;
  p->search_sigma = 2.0f;
  p->min_grad_mag = 5.0f;
  p->idepth_min = 1e-3f;
  p->idepth_max = 2.0f;
  p->epilength_min = 3.0f;
  p->epilength_max = 32.0f;
  p->process_var_factor = 1.01f;
  p->process_fail_var_factor = 1.1f;
  p->max_cost = 1300.0f;
  p->do_subpixel = 1;
  p->sample_dist = 1.0f;
  p->second_best_factor = 1.5f;
  p->z_win_size = 5;
  p->pixel_var = 16.0f;
  p->epipolar_line_var = 1.0f;
}

int flame_stereo_create(flame_stereo_ctx** out, int device) {
  if (!out) return FLAME_NLTGV2_ERR_INVALID_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return FLAME_NLTGV2_ERR_NO_DEVICE;
  if (device < 0 || device >= count) return FLAME_NLTGV2_ERR_NO_DEVICE;
  if (hipSetDevice(device) != hipSuccess) return FLAME_NLTGV2_ERR_NO_DEVICE;
  flame_stereo_ctx* ctx = new (std::nothrow) flame_stereo_ctx();
  if (!ctx) return FLAME_NLTGV2_ERR_OOM;
  ctx->device = device;
  if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess ||
      hipMalloc((void**)&ctx->d_stats, kStatWords * sizeof(int)) != hipSuccess ||
      hipHostMalloc((void**)&ctx->h_stats, kStatWords * sizeof(int), hipHostMallocDefault) != hipSuccess ||
      hipMalloc((void**)&ctx->d_fstats, kFrontWords * sizeof(int)) != hipSuccess ||
      hipHostMalloc((void**)&ctx->h_fstats, kFrontWords * sizeof(int), hipHostMallocDefault) != hipSuccess ||
      hipMalloc((void**)&ctx->d_istats, kInputWords * sizeof(int)) != hipSuccess ||
      hipHostMalloc((void**)&ctx->h_istats, kInputWords * sizeof(int), hipHostMallocDefault) != hipSuccess) {
    flame_stereo_destroy(ctx);
    return FLAME_NLTGV2_ERR_HIP;
  }
  ctx->stream = ctx->own_stream;
  *out = ctx;
  return 0;
}

void flame_stereo_destroy(flame_stereo_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  drop_all_frames(ctx);
  if (ctx->d_raw) (void)hipFree(ctx->d_raw);
  if (ctx->d_poses) (void)hipFree(ctx->d_poses);
  if (ctx->h_poses) (void)hipHostFree(ctx->h_poses);
  if (ctx->d_feats) (void)hipFree(ctx->d_feats);
  if (ctx->d_res) (void)hipFree(ctx->d_res);
  for (void* p : {(void*)ctx->d_res_alt, (void*)ctx->d_proj, (void*)ctx->d_proj_alt, (void*)ctx->d_proj_tmp, (void*)ctx->d_keep,
                  (void*)ctx->d_groups, (void*)ctx->d_ppose, (void*)ctx->d_keep_ids, (void*)ctx->d_cell_key, (void*)ctx->d_blocked, (void*)ctx->d_map, (void*)ctx->d_mask,
                  (void*)ctx->d_fstats, (void*)ctx->d_spose, (void*)ctx->d_sel, (void*)ctx->d_owner, (void*)ctx->d_draw,
                  (void*)ctx->d_match, (void*)ctx->d_mlist, (void*)ctx->d_mentries, (void*)ctx->d_rawsrc, (void*)ctx->d_istats,
                  (void*)ctx->d_apart, (void*)ctx->d_asys})
    if (p) (void)hipFree(p);
  if (ctx->h_fstats) (void)hipHostFree(ctx->h_fstats);
  if (ctx->h_sel) (void)hipHostFree(ctx->h_sel);
  if (ctx->h_istats) (void)hipHostFree(ctx->h_istats);
  if (ctx->h_asys) (void)hipHostFree(ctx->h_asys);
  if (ctx->d_stats) (void)hipFree(ctx->d_stats);
  if (ctx->h_stats) (void)hipHostFree(ctx->h_stats);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
}

int flame_stereo_set_stream(flame_stereo_ctx* ctx, void* hip_stream) {
  if (int rc = enter(ctx)) return rc;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
  return 0;
}

int flame_stereo_set_camera(flame_stereo_ctx* ctx, const float K[9], const float Kinv[9], int width, int height,
                            int border) {
  if (int rc = enter(ctx)) return rc;
  if (!K || !Kinv || width < 2 || height < 2 || border < 0 || width > 16384 || height > 16384 || border > 64)
    return FLAME_NLTGV2_ERR_INVALID_ARG;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  drop_all_frames(ctx);
  ctx->match_stand = false;
  ctx->have_input = false;  // (the input describes raw frames for one working camera)
  std::memcpy(ctx->cam.K, K, sizeof ctx->cam.K);
  std::memcpy(ctx->cam.Kinv, Kinv, sizeof ctx->cam.Kinv);
  ctx->cam.width = width, ctx->cam.height = height, ctx->cam.border = border;
  ctx->have_camera = true;
  return 0;
}

int flame_stereo_add_frame(flame_stereo_ctx* ctx, uint32_t frame_id, const uint8_t* img, int row_stride_bytes) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_add_frame");
  if (int rc = enter(ctx)) return rc;
  if (!ctx->have_camera) return FLAME_NLTGV2_ERR_NO_GRAPH;
  const int w = ctx->cam.width, h = ctx->cam.height;
  if (!img || row_stride_bytes < w) return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (int rc = grow(ctx, &ctx->d_raw, &ctx->raw_cap, (size_t)w * h)) return rc;
  Frame* f = nullptr;
  if (int rc = acquire_frame(ctx, frame_id, &f)) return rc;
  SCHK(ctx, hipMemcpy2DAsync(ctx->d_raw, (size_t)w, img, (size_t)row_stride_bytes, (size_t)w, (size_t)h,
                             hipMemcpyHostToDevice, ctx->stream));
  SCHK(ctx, launch_frame_pad_gradient(ctx->d_raw, w, h, ctx->cam.border, f->img_pad, f->gx_pad, f->gy_pad, ctx->stream));
  // the staging buffer is reused by the next add_frame and `img` is pageable host memory
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  return 0;
}

void flame_stereo_default_input_params(flame_stereo_input_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->format = FLAME_STEREO_FMT_GREY8;
  p->K_raw[0] = p->K_raw[4] = p->K_raw[8] = 1.0f;
}

int flame_stereo_set_input(flame_stereo_ctx* ctx, const flame_stereo_input_params* p) {
  if (int rc = enter(ctx)) return rc;
  if (!ctx->have_camera) return FLAME_NLTGV2_ERR_NO_GRAPH;
  if (!input_params_valid(p, ctx->cam.width, ctx->cam.height)) return FLAME_NLTGV2_ERR_INVALID_ARG;
  ctx->input = *p;
  ctx->have_input = true;
  return 0;
}

int flame_stereo_add_raw_frame(flame_stereo_ctx* ctx, uint32_t frame_id, const void* raw, int row_stride_bytes,
                               int raw_on_device, flame_stereo_input_stats* stats) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_add_raw_frame");
  if (int rc = enter(ctx)) return rc;
  if (!ctx->have_camera) return FLAME_NLTGV2_ERR_NO_GRAPH;
  const flame_stereo_input_params& in = ctx->input;
  const int w = ctx->cam.width, h = ctx->cam.height;
  if (!ctx->have_input || !input_params_valid(&in, w, h) || !input_frame_valid(in, raw, row_stride_bytes))
    return FLAME_NLTGV2_ERR_INVALID_ARG;
  // (both buffers hold their size after the first frame: grow() reallocates, and so waits for the device, only then)
  if (ctx->raw_cap < (size_t)w * h) SCHK(ctx, hipStreamSynchronize(ctx->stream));  // an enqueued frame may still read d_raw
  if (int rc = grow(ctx, &ctx->d_raw, &ctx->raw_cap, (size_t)w * h)) return rc;
  const uint8_t* src = (const uint8_t*)raw;
  if (!raw_on_device) {
    const size_t bytes = input_frame_bytes(in, row_stride_bytes);
    if (int rc = grow(ctx, &ctx->d_rawsrc, &ctx->rawsrc_cap, bytes)) return rc;
    src = ctx->d_rawsrc;
  }
  Frame* f = nullptr;
  if (int rc = acquire_frame(ctx, frame_id, &f)) return rc;
  if (!raw_on_device)  // rows and their padding in one run: the kernel reads the caller's stride
    SCHK(ctx, hipMemcpyAsync(ctx->d_rawsrc, raw, input_frame_bytes(in, row_stride_bytes), hipMemcpyHostToDevice, ctx->stream));
  InputMap m;
  std::memcpy(m.kinv, ctx->cam.Kinv, sizeof m.kinv);
  m.fx = in.K_raw[0], m.skew = in.K_raw[1], m.cx = in.K_raw[2], m.fy = in.K_raw[4], m.cy = in.K_raw[5];
  m.k1 = in.dist[0], m.k2 = in.dist[1], m.p1 = in.dist[2], m.p2 = in.dist[3];
  m.k3 = in.dist[4], m.k4 = in.dist[5], m.k5 = in.dist[6], m.k6 = in.dist[7];
  m.raw_width = in.raw_width, m.raw_height = in.raw_height;
  SCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  SCHK(ctx, (hipError_t)launch_input_rectify(m, in.format, in.remap != 0, src, row_stride_bytes, w, h, ctx->d_istats, ctx->d_raw,
                                             ctx->stream));
  SCHK(ctx, launch_frame_pad_gradient(ctx->d_raw, w, h, ctx->cam.border, f->img_pad, f->gx_pad, f->gy_pad, ctx->stream));
  SCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed = true;
  if (stats) SCHK(ctx, hipMemcpyAsync(ctx->h_istats, ctx->d_istats, kInputWords * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  // a host source is pageable memory; a device source is the caller's to keep until the stream has passed (flame_stereo.h)
  if (!raw_on_device || stats) SCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (stats) {
    int sum = 0;
    for (int k = 0; k < kInputSlots; ++k) sum += ctx->h_istats[k * kInputSlotStride];
    stats->n_outside = sum;
  }
  return 0;
}

int flame_stereo_drop_frame(flame_stereo_ctx* ctx, uint32_t frame_id) {
  if (int rc = enter(ctx)) return rc;
  auto it = ctx->frames.find(frame_id);
  if (it == ctx->frames.end()) return FLAME_NLTGV2_ERR_INVALID_ARG;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  release_frame(ctx, it);
  return 0;
}

int flame_stereo_frame_count(const flame_stereo_ctx* ctx) { return ctx ? (int)ctx->frames.size() : 0; }

int flame_stereo_download_frame(flame_stereo_ctx* ctx, uint32_t frame_id, uint8_t* img_pad, float* gradx_pad,
                                float* grady_pad) {
  if (int rc = enter(ctx)) return rc;
  auto it = ctx->frames.find(frame_id);
  if (it == ctx->frames.end()) return FLAME_NLTGV2_ERR_INVALID_ARG;
  const size_t px = padded_pixels(ctx->cam);
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (img_pad) SCHK(ctx, hipMemcpy(img_pad, it->second.img_pad, px, hipMemcpyDeviceToHost));
  if (gradx_pad) SCHK(ctx, hipMemcpy(gradx_pad, it->second.gx_pad, px * sizeof(float), hipMemcpyDeviceToHost));
  if (grady_pad) SCHK(ctx, hipMemcpy(grady_pad, it->second.gy_pad, px * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int flame_stereo_update_feature_idepths(flame_stereo_ctx* ctx, const flame_stereo_params* params, uint32_t new_frame_id,
                                        uint32_t curr_pf_id, int n_poses, const flame_stereo_pose* poses, int n_feats,
                                        flame_stereo_feature* feats, flame_stereo_stats* stats) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_update_feature_idepths");
  if (int rc = enter(ctx)) return rc;
  if (!stats || n_feats < 0 || (n_feats > 0 && !feats)) return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (int rc = grow(ctx, &ctx->d_feats, &ctx->feats_cap, (size_t)n_feats + 1)) return rc;
  if (n_feats > 0)
    SCHK(ctx, hipMemcpyAsync(ctx->d_feats, feats, (size_t)n_feats * sizeof(StereoFeature), hipMemcpyHostToDevice, ctx->stream));
  if (int rc = enqueue_update(ctx, params, new_frame_id, curr_pf_id, n_poses, poses, n_feats, ctx->d_feats)) return rc;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  const int rc = report(ctx, stats);
  if (rc == 0 && n_feats > 0)
    SCHK(ctx, hipMemcpy(feats, ctx->d_feats, (size_t)n_feats * sizeof(StereoFeature), hipMemcpyDeviceToHost));
  return rc;
}

int flame_stereo_update_feature_idepths_device(flame_stereo_ctx* ctx, const flame_stereo_params* params,
                                               uint32_t new_frame_id, uint32_t curr_pf_id, int n_poses,
                                               const flame_stereo_pose* poses, int n_feats, void* feats_device,
                                               flame_stereo_stats* stats) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_update_feature_idepths_device");
  if (int rc = enter(ctx)) return rc;
  if (n_feats < 0 || (n_feats > 0 && !feats_device)) return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (int rc = enqueue_update(ctx, params, new_frame_id, curr_pf_id, n_poses, poses, n_feats, (StereoFeature*)feats_device))
    return rc;
  if (!stats) return 0;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  return report(ctx, stats);
}

int flame_stereo_set_option(flame_stereo_ctx* ctx, int option, int value) {
  if (!ctx) return FLAME_NLTGV2_ERR_INVALID_ARG;
  switch (option) {
    case FLAME_STEREO_OPT_LANES_PER_FEATURE:
      if (value != 0 && value != 1 && value != 16) return FLAME_NLTGV2_ERR_INVALID_ARG;
      ctx->lanes_per_feature = value;
      return 0;
    case FLAME_STEREO_OPT_GRAPH_COPY:
      if (value != 0 && value != 1) return FLAME_NLTGV2_ERR_INVALID_ARG;
      ctx->graph_copy = value;
      return 0;
    case FLAME_STEREO_OPT_RECORD_MATCHES:
      if (value != 0 && value != 1) return FLAME_NLTGV2_ERR_INVALID_ARG;
      if (value != ctx->record_matches) ctx->match_stand = false;  // (records come from an update that ran with the option on)
      ctx->record_matches = value;
      return 0;
    default:
      return FLAME_NLTGV2_ERR_INVALID_ARG;
  }
}

int flame_stereo_set_features(flame_stereo_ctx* ctx, int n_feats, const flame_stereo_feature* feats) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_set_features");
  if (int rc = enter(ctx)) return rc;
  if (n_feats < 0 || (n_feats > 0 && !feats)) return FLAME_NLTGV2_ERR_INVALID_ARG;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (the array may be reallocated)
  if (int rc = grow(ctx, &ctx->d_res, &ctx->res_cap, (size_t)n_feats + 1)) return rc;
  if (n_feats > 0) {
    SCHK(ctx, hipMemcpyAsync(ctx->d_res, feats, (size_t)n_feats * sizeof(StereoFeature), hipMemcpyHostToDevice, ctx->stream));
    SCHK(ctx, hipStreamSynchronize(ctx->stream));  // `feats` is the caller's (pageable) memory
  }
  ctx->n_res = n_feats;
  ctx->aligned = false;
  return 0;
}

int flame_stereo_get_features(flame_stereo_ctx* ctx, int max_feats, flame_stereo_feature* feats, int* n_feats) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_get_features");
  if (int rc = enter(ctx)) return rc;
  if (n_feats) *n_feats = ctx->n_res;
  if (!feats) return 0;
  if (max_feats < ctx->n_res) return FLAME_NLTGV2_ERR_INVALID_ARG;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->n_res > 0)
    SCHK(ctx, hipMemcpy(feats, ctx->d_res, (size_t)ctx->n_res * sizeof(StereoFeature), hipMemcpyDeviceToHost));
  return 0;
}

int flame_stereo_features_device(flame_stereo_ctx* ctx, void** feats_device, int* n_feats) {
  if (!ctx) return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (feats_device) *feats_device = ctx->d_res;
  if (n_feats) *n_feats = ctx->n_res;
  return 0;
}

int flame_stereo_update_resident(flame_stereo_ctx* ctx, const flame_stereo_params* params, uint32_t new_frame_id,
                                 uint32_t curr_pf_id, int n_poses, const flame_stereo_pose* poses, flame_stereo_stats* stats) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_update_resident");
  if (int rc = enter(ctx)) return rc;
  if (int rc = enqueue_update(ctx, params, new_frame_id, curr_pf_id, n_poses, poses, ctx->n_res, ctx->d_res)) return rc;
  if (!stats) return 0;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  return report(ctx, stats);
}

void flame_stereo_default_detect_params(flame_stereo_detect_params* p) {
  if (!p) return;
  p->detection_win_size = 16;
  p->min_grad_mag = 5.0f;
  p->idepth_init = 0.01f;
  p->idepth_var_init = 0.5f * 0.5f;
}

int flame_stereo_project_features(flame_stereo_ctx* ctx, const flame_stereo_params* params, uint32_t cur_frame_id,
                                  int n_poses, const flame_stereo_pose* poses, flame_stereo_feature_stats* stats) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_project_features");
  if (int rc = enter(ctx)) return rc;
  if (stats) stats->num_features = 0, stats->num_examined = 0, stats->error_feature = -1;
  if (!params || n_poses < 0 || (n_poses > 0 && !poses)) return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (!ctx->have_camera) return FLAME_NLTGV2_ERR_NO_GRAPH;
  const int n = ctx->n_res;
  if (stats) stats->num_examined = n;
  if (n == 0) {
    ctx->n_proj = 0;
    ctx->aligned = true;
    return 0;
  }
  SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (buffers may be reallocated; the pinned stats block is reused)
  if (int rc = grow(ctx, &ctx->d_res_alt, &ctx->res_alt_cap, (size_t)n)) return rc;
  if (int rc = grow(ctx, &ctx->d_proj_alt, &ctx->proj_alt_cap, (size_t)n)) return rc;
  if (int rc = grow(ctx, &ctx->d_proj_tmp, &ctx->proj_tmp_cap, (size_t)n)) return rc;
  if (int rc = grow(ctx, &ctx->d_keep, &ctx->keep_cap, (size_t)n)) return rc;
  if (int rc = grow(ctx, &ctx->d_groups, &ctx->groups_cap, (size_t)n / 256 + 1)) return rc;
  if (int rc = grow(ctx, &ctx->d_ppose, &ctx->ppose_cap, (size_t)n_poses + 1)) return rc;
  std::vector<ProjectPoseEntry> table((size_t)n_poses);
  for (int k = 0; k < n_poses; ++k) {
    std::memset(&table[k], 0, sizeof table[k]);
    table[k].frame_id = poses[k].frame_id;
    load_geometry(table[k].geo, ctx->cam, poses[k].q_ref_to_new, poses[k].t_ref_to_new);
  }
  const int border = front_border(*params);
  const int row_offset = params->do_letterbox ? ctx->cam.height / 3 : 0;
  const ProjectRegion region = {(float)border, (float)(border + row_offset), (float)(ctx->cam.width - 2 * border),
                                (float)(ctx->cam.height - 2 * border - 2 * row_offset)};
  if (n_poses > 0)
    SCHK(ctx, hipMemcpyAsync(ctx->d_ppose, table.data(), (size_t)n_poses * sizeof(ProjectPoseEntry), hipMemcpyHostToDevice,
                             ctx->stream));
  if (int rc = reset_front_stats(ctx)) return rc;
  SCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  SCHK(ctx, launch_project_features(ctx->cam, region, n_poses, ctx->d_ppose, cur_frame_id, n, ctx->d_res, ctx->d_proj_tmp,
                                    ctx->d_keep, ctx->d_groups, ctx->d_res_alt, ctx->d_proj_alt, ctx->d_fstats, ctx->stream));
  SCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed = true;
  SCHK(ctx, hipMemcpyAsync(ctx->h_fstats, ctx->d_fstats, kFrontWords * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  const int* s = ctx->h_fstats;
  if (s[kFrontBadFrame] != INT_MAX) {  // pfs.at() would throw
    if (stats) stats->error_feature = s[kFrontBadFrame];
    return FLAME_NLTGV2_ERR_INVALID_ARG;
  }
  if (s[kFrontAssert] != INT_MAX) {
    if (stats) stats->error_feature = s[kFrontAssert];
    return FLAME_NLTGV2_ERR_ASSERT;
  }
  std::swap(ctx->d_res, ctx->d_res_alt);
  std::swap(ctx->res_cap, ctx->res_alt_cap);
  std::swap(ctx->d_proj, ctx->d_proj_alt);
  std::swap(ctx->proj_cap, ctx->proj_alt_cap);
  ctx->n_res = ctx->n_proj = s[kFrontCount];
  ctx->aligned = true;
  if (stats) stats->num_features = s[kFrontCount];
  return 0;
}

int flame_stereo_get_projected(flame_stereo_ctx* ctx, int max_feats, flame_stereo_feature* feats, int* n_feats) {
  if (int rc = enter(ctx)) return rc;
  if (n_feats) *n_feats = ctx->n_proj;
  if (!feats) return 0;
  if (max_feats < ctx->n_proj) return FLAME_NLTGV2_ERR_INVALID_ARG;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->n_proj > 0)
    SCHK(ctx, hipMemcpy(feats, ctx->d_proj, (size_t)ctx->n_proj * sizeof(StereoFeature), hipMemcpyDeviceToHost));
  return 0;
}

int flame_stereo_projected_device(flame_stereo_ctx* ctx, void** feats_device, int* n_feats) {
  if (!ctx) return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (feats_device) *feats_device = ctx->d_proj;
  if (n_feats) *n_feats = ctx->n_proj;
  return 0;
}

int flame_stereo_frame_image_device(flame_stereo_ctx* ctx, uint32_t frame_id, const void** img, int* step_bytes) {
  if (!ctx || !img || !step_bytes || !ctx->have_camera) return FLAME_NLTGV2_ERR_INVALID_ARG;
  auto it = ctx->frames.find(frame_id);
  if (it == ctx->frames.end()) return FLAME_NLTGV2_ERR_INVALID_ARG;
  const int pitch = ctx->cam.width + 2 * ctx->cam.border;
  *img = it->second.img_pad + (size_t)ctx->cam.border * pitch + ctx->cam.border;
  *step_bytes = pitch;
  return 0;
}

int flame_stereo_draw_features(flame_stereo_ctx* ctx, uint32_t cur_frame_id, float idepth_var_max_graph,
                               float scene_color_scale, int flip, uint8_t* img_out, int32_t* num_converged,
                               int32_t* num_unconverged) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_draw_features");
  if (int rc = enter(ctx)) return rc;
  if (!img_out) return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (!ctx->have_camera) return FLAME_NLTGV2_ERR_NO_GRAPH;
  auto fr = ctx->frames.find(cur_frame_id);
  if (fr == ctx->frames.end()) return FLAME_NLTGV2_ERR_INVALID_ARG;
  const int width = ctx->cam.width, height = ctx->cam.height, pitch = width + 2 * ctx->cam.border;
  const size_t px = (size_t)width * height;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (buffers may be reallocated)
  if (int rc = grow(ctx, &ctx->d_owner, &ctx->owner_cap, px + 2)) return rc;
  if (int rc = grow(ctx, &ctx->d_draw, &ctx->draw_cap, 3 * px + 16)) return rc;
  DebugImageArgs a;
  a.rows = height, a.cols = width;
  a.gray = fr->second.img_pad + (size_t)ctx->cam.border * pitch + ctx->cam.border, a.gray_step = pitch;
  a.scene_color_scale = scene_color_scale, a.flip = flip != 0;
  a.k00 = a.k11 = 0.0f;
  int* d_counts = (int*)(ctx->d_owner + px);
  SCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  SCHK(ctx, (hipError_t)launch_draw_features(a, ctx->n_proj, ctx->n_proj > 0 ? (const void*)&ctx->d_proj->x : nullptr,
                                             (int)sizeof(StereoFeature), idepth_var_max_graph, ctx->d_owner, d_counts, ctx->d_draw,
                                             ctx->stream));
  SCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed = true;
  int counts[2] = {0, 0};
  SCHK(ctx, hipMemcpyAsync(img_out, ctx->d_draw, 3 * px, hipMemcpyDeviceToHost, ctx->stream));
  SCHK(ctx, hipMemcpyAsync(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost, ctx->stream));
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (num_converged) *num_converged = counts[0];
  if (num_unconverged) *num_unconverged = counts[1];
  return 0;
}

int flame_stereo_draw_matches(flame_stereo_ctx* ctx, int flip, uint8_t* img_out, flame_stereo_matches_stats* stats) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_draw_matches");
  if (int rc = enter(ctx)) return rc;
  if (stats) std::memset(stats, 0, sizeof *stats);
  if (!img_out || !ctx->record_matches || !ctx->match_stand || !ctx->have_camera) return FLAME_NLTGV2_ERR_INVALID_ARG;
  auto fr = ctx->frames.find(ctx->match_frame);
  if (fr == ctx->frames.end()) return FLAME_NLTGV2_ERR_INVALID_ARG;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (an enqueue-only update has finished and reported; buffers may be reallocated)
  if (ctx->h_stats[kStatAssert] != INT_MAX || ctx->h_stats[kStatBadFrame] != INT_MAX) {  // that update returned an error
    ctx->match_stand = false;
    return FLAME_NLTGV2_ERR_INVALID_ARG;
  }
  const int width = ctx->cam.width, height = ctx->cam.height, pitch = width + 2 * ctx->cam.border, n = ctx->match_n;
  const size_t px = (size_t)width * height;
  auto entry_capacity = [&] { return std::max(2 * px, ctx->match_last_total + ctx->match_last_total / 4); };
  if (int rc = grow(ctx, &ctx->d_mlist, &ctx->mlist_cap, 3 * px + kMatchCounts)) return rc;
  if (int rc = grow(ctx, &ctx->d_mentries, &ctx->mentries_cap, entry_capacity())) return rc;
  if (int rc = grow(ctx, &ctx->d_draw, &ctx->draw_cap, 3 * px + 16)) return rc;
  MatchBuffers b;
  b.cnt = ctx->d_mlist, b.offset = ctx->d_mlist + px, b.fill = ctx->d_mlist + 2 * px, b.counts = (int*)(ctx->d_mlist + 3 * px);
  b.entries = ctx->d_mentries, b.capacity = (uint32_t)std::min<size_t>(entry_capacity(), UINT32_MAX);
  MatchImageArgs a;
  a.rows = height, a.cols = width;
  a.gray = fr->second.img_pad + (size_t)ctx->cam.border * pitch + ctx->cam.border, a.gray_step = pitch;
  a.flip = flip != 0;
  int counts[kMatchCounts] = {0};
  SCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  SCHK(ctx, (hipError_t)launch_matches_lists(n, ctx->d_match, b, height, width, ctx->stream));
  SCHK(ctx, hipMemcpyAsync(counts, b.counts, sizeof counts, hipMemcpyDeviceToHost, ctx->stream));
  SCHK(ctx, (hipError_t)launch_matches_paint(n, ctx->d_match, b, a, ctx->d_draw, ctx->stream));
  SCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed = true;
  SCHK(ctx, hipMemcpyAsync(img_out, ctx->d_draw, 3 * px, hipMemcpyDeviceToHost, ctx->stream));
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  const size_t total = (size_t)(uint32_t)counts[kMatchTotal];
  ctx->match_last_total = total;
  int refilled = 0;
  if (total > (size_t)b.capacity) {  // the entry buffer was too small: grow it, repeat fill and fold (cnt and offset stand)
    if (int rc = grow(ctx, &ctx->d_mentries, &ctx->mentries_cap, entry_capacity())) return rc;
    b.entries = ctx->d_mentries, b.capacity = (uint32_t)std::min<size_t>(entry_capacity(), UINT32_MAX);
    SCHK(ctx, (hipError_t)launch_matches_paint(n, ctx->d_match, b, a, ctx->d_draw, ctx->stream));
    SCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));  // (ev0 .. ev1 now spans both passes and the first picture's copy)
    SCHK(ctx, hipMemcpyAsync(img_out, ctx->d_draw, 3 * px, hipMemcpyDeviceToHost, ctx->stream));
    SCHK(ctx, hipStreamSynchronize(ctx->stream));
    refilled = 1;
  }
  if (stats) {
    stats->num_features = n;
    for (int k = 0; k < kMatchKinds; ++k) stats->kind_count[k] = counts[k];
    stats->lines_drawn = counts[kMatchLinesDrawn], stats->lines_skipped = counts[kMatchLinesSkipped];
    stats->rings_skipped = counts[kMatchRingsSkippedCount];
    stats->entries = (int64_t)total;
    stats->refilled = refilled;
  }
  return 0;
}

int flame_stereo_draw_detections(flame_stereo_ctx* ctx, const flame_stereo_params* params,
                                 const flame_stereo_detect_params* dparams, uint32_t ref_frame_id,
                                 const float q_ref_to_prev[4], const float t_ref_to_prev[3], float max_score, int flip,
                                 uint8_t* img_out, flame_stereo_detections_stats* stats) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_draw_detections");
  if (int rc = enter(ctx)) return rc;
  if (stats) stats->num_scored = 0, stats->num_examined = 0, stats->error_pixel = -1;
  if (!params || !dparams || !q_ref_to_prev || !t_ref_to_prev || !img_out || !std::isfinite(max_score) || !(max_score > 0.0f))
    return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (!ctx->have_camera) return FLAME_NLTGV2_ERR_NO_GRAPH;
  auto fr = ctx->frames.find(ref_frame_id);
  if (fr == ctx->frames.end()) return FLAME_NLTGV2_ERR_INVALID_ARG;
  const int width = ctx->cam.width, height = ctx->cam.height, pitch = width + 2 * ctx->cam.border;
  const int border = front_border(*params);
  if (border < 0) return FLAME_NLTGV2_ERR_INVALID_ARG;
  const int row_offset = params->do_letterbox ? height / 3 : 0;
  DetectGrid G;  // the scan rectangle and the threshold of flame_stereo_detect_features; the cell grid is not read
  G.win = 1, G.hc = G.wc = 0;
  G.r_lo = border + row_offset, G.r_hi = height - border - row_offset;
  G.c_lo = border, G.c_hi = width - border;
  G.g2 = dparams->min_grad_mag * dparams->min_grad_mag;
  const size_t px = (size_t)width * height;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (buffers may be reallocated)
  if (int rc = grow(ctx, &ctx->d_owner, &ctx->owner_cap, (size_t)kDetWords)) return rc;  // (scratch of the pictures: the stats words)
  if (int rc = grow(ctx, &ctx->d_draw, &ctx->draw_cap, 3 * px + 16)) return rc;
  DebugImageArgs a;
  a.rows = height, a.cols = width;
  a.gray = fr->second.img_pad + (size_t)ctx->cam.border * pitch + ctx->cam.border, a.gray_step = pitch;
  a.scene_color_scale = 1.0f, a.flip = flip != 0;
  a.k00 = a.k11 = 0.0f;
  Geo geo;
  load_geometry(geo, ctx->cam, q_ref_to_prev, t_ref_to_prev);
  int* d_stats = (int*)ctx->d_owner;
  int s[kDetWords] = {0};
  SCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  SCHK(ctx, (hipError_t)launch_draw_detections(a, G, geo, ctx->cam, fr->second.gx_pad, fr->second.gy_pad, max_score, d_stats,
                                               ctx->d_draw, ctx->stream));
  SCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed = true;
  SCHK(ctx, hipMemcpyAsync(img_out, ctx->d_draw, 3 * px, hipMemcpyDeviceToHost, ctx->stream));
  SCHK(ctx, hipMemcpyAsync(s, d_stats, sizeof s, hipMemcpyDeviceToHost, ctx->stream));
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (stats) {
    for (int k = 0; k < kDetSlots; ++k) stats->num_scored += s[kDetCount + k * kDetSlotStride];
    stats->num_examined = std::max(G.r_hi - G.r_lo, 0) * std::max(G.c_hi - G.c_lo, 0);
  }
  if (s[kDetAssert] != 0) {
    if (stats) stats->error_pixel = INT_MAX - s[kDetAssert];
    return FLAME_NLTGV2_ERR_ASSERT;
  }
  return 0;
}

int flame_stereo_detect_features(flame_stereo_ctx* ctx, const flame_stereo_params* params,
                                 const flame_stereo_detect_params* dparams, uint32_t ref_frame_id,
                                 const float q_ref_to_prev[4], const float t_ref_to_prev[3], const float* idepthmap_host,
                                 const void* idepthmap_device, int n_mask, const float* mask_xy, uint32_t first_id,
                                 flame_stereo_feature_stats* stats) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_detect_features");
  if (int rc = enter(ctx)) return rc;
  if (stats) stats->num_features = 0, stats->num_examined = 0, stats->error_feature = -1;
  if (!params || !dparams || !q_ref_to_prev || !t_ref_to_prev || (idepthmap_host && idepthmap_device) || n_mask < -1 ||
      (n_mask > 0 && !mask_xy) || dparams->detection_win_size < 1)
    return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (!ctx->have_camera) return FLAME_NLTGV2_ERR_NO_GRAPH;
  auto fr = ctx->frames.find(ref_frame_id);
  if (fr == ctx->frames.end()) return FLAME_NLTGV2_ERR_INVALID_ARG;
  const int width = ctx->cam.width, height = ctx->cam.height;
  const int border = front_border(*params);
  if (border < 0) return FLAME_NLTGV2_ERR_INVALID_ARG;
  const int row_offset = params->do_letterbox ? height / 3 : 0;
  DetectGrid G;
  G.win = dparams->detection_win_size;
  const float fh = (float)height / G.win, fw = (float)width / G.win;  // utils::fast_ceil (image_utils.h:82-85)
  G.hc = (int)fh < fh ? (int)fh + 1 : (int)fh;
  G.wc = (int)fw < fw ? (int)fw + 1 : (int)fw;
  G.r_lo = border + row_offset, G.r_hi = height - border - row_offset;
  G.c_lo = border, G.c_hi = width - border;
  G.g2 = dparams->min_grad_mag * dparams->min_grad_mag;
  const int n_cells = G.hc * G.wc;
  if (stats) stats->num_examined = n_cells;
  // the mask: host points are checked here (the reference indexes its cell mask with them unchecked)
  const int n_pts = n_mask < 0 ? ctx->n_proj : n_mask;
  for (int i = 0; i < n_mask; ++i) {
    const float x = mask_xy[2 * i], y = mask_xy[2 * i + 1];
    if (!(x >= 0.0f && y >= 0.0f && x < (float)width && y < (float)height)) return FLAME_NLTGV2_ERR_INVALID_ARG;
    if ((uint32_t)(x / (float)G.win) >= (uint32_t)G.wc || (uint32_t)(y / (float)G.win) >= (uint32_t)G.hc)
      return FLAME_NLTGV2_ERR_INVALID_ARG;
  }
  SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (buffers may be reallocated; the pinned stats block is reused)
  const int n_res = ctx->n_res;
  if (int rc = grow_keep(ctx, &ctx->d_res, &ctx->res_cap, (size_t)n_res + (size_t)n_cells + 1, (size_t)n_res)) return rc;
  if (int rc = grow(ctx, &ctx->d_cell_key, &ctx->cell_key_cap, (size_t)n_cells + 1)) return rc;
  if (int rc = grow(ctx, &ctx->d_blocked, &ctx->blocked_cap, (size_t)n_cells + 1)) return rc;
  if (int rc = grow(ctx, &ctx->d_groups, &ctx->groups_cap, (size_t)n_cells / 256 + 1)) return rc;
  const float* d_map = (const float*)idepthmap_device;
  if (idepthmap_host) {
    if (int rc = grow(ctx, &ctx->d_map, &ctx->map_cap, (size_t)width * height)) return rc;
    SCHK(ctx, hipMemcpyAsync(ctx->d_map, idepthmap_host, (size_t)width * height * sizeof(float), hipMemcpyHostToDevice,
                             ctx->stream));
    d_map = ctx->d_map;
  }
  const float* d_mask = nullptr;
  int mask_stride = 2;
  if (n_mask > 0) {
    if (int rc = grow(ctx, &ctx->d_mask, &ctx->mask_cap, (size_t)n_mask * 2)) return rc;
    SCHK(ctx, hipMemcpyAsync(ctx->d_mask, mask_xy, (size_t)n_mask * 2 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    d_mask = ctx->d_mask;
  } else if (n_mask < 0 && n_pts > 0) {
    d_mask = &ctx->d_proj->x;
    mask_stride = (int)(sizeof(StereoFeature) / sizeof(float));
  }
  Geo geo;
  load_geometry(geo, ctx->cam, q_ref_to_prev, t_ref_to_prev);
  DetectInit init = {first_id, ref_frame_id, dparams->idepth_init, dparams->idepth_var_init};
  if (int rc = reset_front_stats(ctx)) return rc;
  SCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  SCHK(ctx, launch_detect_features(G, geo, ctx->cam, fr->second.gx_pad, fr->second.gy_pad, n_pts, d_mask, mask_stride,
                                   ctx->d_blocked, ctx->d_cell_key, ctx->d_groups, init, d_map, ctx->d_res + n_res, ctx->d_fstats,
                                   ctx->stream));
  SCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed = true;
  SCHK(ctx, hipMemcpyAsync(ctx->h_fstats, ctx->d_fstats, kFrontWords * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (also: the host map and mask were pageable memory)
  const int* s = ctx->h_fstats;
  if (s[kFrontAssert] != INT_MAX) {  // the records written past n_res are not part of the set
    if (stats) stats->error_feature = s[kFrontAssert];
    return FLAME_NLTGV2_ERR_ASSERT;
  }
  ctx->n_res = n_res + s[kFrontCount];
  if (s[kFrontCount] > 0) ctx->aligned = false;  // (records without a projected counterpart)
  if (stats) stats->num_features = s[kFrontCount];
  return 0;
}

int flame_stereo_prune_pose_frames(flame_stereo_ctx* ctx, const flame_stereo_params* params, uint32_t target_frame_id,
                                   int n_keep, const uint32_t* keep_ids, int n_dropped, const flame_stereo_pose* dropped,
                                   int first_new, flame_stereo_prune_stats* stats) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_prune_pose_frames");
  if (int rc = enter(ctx)) return rc;
  bool moved = false;
  flame_stereo_prune_stats local;
  if (!stats) stats = &local;
  if (int rc = run_prune(ctx, params, target_frame_id, n_keep, keep_ids, n_dropped, dropped, first_new, ctx->n_res, ctx->d_res,
                         &moved, stats))
    return rc;
  if (moved) {
    std::swap(ctx->d_res, ctx->d_res_alt);
    std::swap(ctx->res_cap, ctx->res_alt_cap);
    ctx->n_res = stats->num_features;
    ctx->aligned = false;  // a record was removed
  }
  if (ctx->n_res == 0) SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (run_prune returned before it waited)
  stats->num_frames_dropped = release_dropped(ctx, n_dropped, dropped);
  return 0;
}

int flame_stereo_prune_features(flame_stereo_ctx* ctx, const flame_stereo_params* params, uint32_t target_frame_id, int n_keep,
                                const uint32_t* keep_ids, int n_dropped, const flame_stereo_pose* dropped, int first_new,
                                int* n_feats, flame_stereo_feature* feats, flame_stereo_prune_stats* stats) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_prune_features");
  if (int rc = enter(ctx)) return rc;
  if (stats) {
    std::memset(stats, 0, sizeof *stats);
    stats->error_feature = -1;
  }
  if (!n_feats || *n_feats < 0 || (*n_feats > 0 && !feats)) return FLAME_NLTGV2_ERR_INVALID_ARG;
  const int n = *n_feats;
  if (int rc = grow(ctx, &ctx->d_feats, &ctx->feats_cap, (size_t)n + 1)) return rc;
  if (n > 0)
    SCHK(ctx, hipMemcpyAsync(ctx->d_feats, feats, (size_t)n * sizeof(StereoFeature), hipMemcpyHostToDevice, ctx->stream));
  bool moved = false;
  flame_stereo_prune_stats local;
  if (!stats) stats = &local;
  if (int rc = run_prune(ctx, params, target_frame_id, n_keep, keep_ids, n_dropped, dropped, first_new, n, ctx->d_feats, &moved,
                         stats))
    return rc;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (stats->num_features > 0)
    SCHK(ctx, hipMemcpy(feats, moved ? ctx->d_res_alt : ctx->d_feats, (size_t)stats->num_features * sizeof(StereoFeature),
                        hipMemcpyDeviceToHost));
  *n_feats = stats->num_features;
  stats->num_frames_dropped = release_dropped(ctx, n_dropped, dropped);
  return 0;
}

int flame_stereo_clear_features(flame_stereo_ctx* ctx) {
  if (int rc = enter(ctx)) return rc;
  ctx->n_res = 0;
  ctx->n_proj = 0;
  ctx->aligned = false;
  return 0;
}

void flame_stereo_default_graph_params(flame_stereo_graph_params* p) {
  if (!p) return;
  p->idepth_var_max_graph = 1e-2f;
  p->min_height = 0.1f;
  p->max_height = 4.0f;
  p->adaptive_data_weights = 0;
}

int flame_stereo_select_graph_features(flame_stereo_ctx* ctx, const flame_stereo_graph_params* gp, float graph_scale, int n_poses,
                                       const flame_stereo_world_pose* poses, flame_stereo_graph_inputs* out) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_select_graph_features");
  if (out) clear_graph_inputs(out);
  if (int rc = enter(ctx)) return rc;
  if (!gp || !out || n_poses < 0 || (n_poses > 0 && !poses)) return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (!ctx->have_camera) return FLAME_NLTGV2_ERR_NO_GRAPH;
  if (!ctx->aligned || ctx->n_proj != ctx->n_res) return FLAME_NLTGV2_ERR_INVALID_ARG;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (buffers may be reallocated; the pinned blocks are reused)
  const int rc = run_select(ctx, gp, graph_scale, n_poses, poses, ctx->n_res, ctx->d_res, ctx->d_proj, out);
  if (rc != 0) {
    const int e = out->error_feature, n = out->num_examined;
    clear_graph_inputs(out);
    out->error_feature = e, out->num_examined = n;
  }
  return rc;
}

int flame_stereo_select_graph_features_arrays(flame_stereo_ctx* ctx, const flame_stereo_graph_params* gp, float graph_scale,
                                              int n_poses, const flame_stereo_world_pose* poses, int n_feats,
                                              const flame_stereo_feature* feats, const flame_stereo_feature* feats_in_curr,
                                              flame_stereo_graph_inputs* out) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_select_graph_features_arrays");
  if (out) clear_graph_inputs(out);
  if (int rc = enter(ctx)) return rc;
  if (!gp || !out || n_poses < 0 || (n_poses > 0 && !poses) || n_feats < 0 || (n_feats > 0 && (!feats || !feats_in_curr)))
    return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (!ctx->have_camera) return FLAME_NLTGV2_ERR_NO_GRAPH;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (buffers may be reallocated; the pinned blocks are reused)
  if (int rc = grow(ctx, &ctx->d_feats, &ctx->feats_cap, (size_t)n_feats + 1)) return rc;
  if (int rc = grow(ctx, &ctx->d_proj_tmp, &ctx->proj_tmp_cap, (size_t)n_feats + 1)) return rc;
  if (n_feats > 0) {
    const size_t bytes = (size_t)n_feats * sizeof(StereoFeature);
    SCHK(ctx, hipMemcpyAsync(ctx->d_feats, feats, bytes, hipMemcpyHostToDevice, ctx->stream));
    SCHK(ctx, hipMemcpyAsync(ctx->d_proj_tmp, feats_in_curr, bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  const int rc = run_select(ctx, gp, graph_scale, n_poses, poses, n_feats, ctx->d_feats, ctx->d_proj_tmp, out);
  if (rc != 0) {
    const int e = out->error_feature, n = out->num_examined;
    clear_graph_inputs(out);
    out->error_feature = e, out->num_examined = n;
  }
  return rc;
}

// ---- pyramid levels and direct alignment (include/flame_stereo.h; align_kernels.hip, align_host.hpp) ----

void flame_stereo_default_align_params(flame_stereo_align_params* p) {
  if (!p) return;
  p->border = 2;
  p->huber_k = 10.0f;
  p->coarsest_level = 2;
  p->finest_level = 0;
  p->max_iters_per_level = 10;
  p->min_pixels = 100;
  p->min_step = 1e-5;
  p->lm_lambda = 0.0;
}

}  // extern "C"

namespace {

// Level `level` of frame f, or false when it is not built.
bool frame_level(const flame_stereo_ctx* ctx, const Frame& f, int level, AlignLevel* L) {
  const int w = ctx->cam.width, h = ctx->cam.height, b = ctx->cam.border;
  if (level == 0) {
    const int pitch = w + 2 * b;
    const size_t o = (size_t)b * pitch + b;
    *L = AlignLevel{f.img_pad + o, f.gx_pad + o, f.gy_pad + o, w, h, pitch};
    return true;
  }
  if (level < 0 || level >= f.pyr_levels || !f.pyr) return false;
  align::LevelPlace place[align::kMaxLevels];
  align::place_levels(w, h, f.pyr_levels, place);
  const align::LevelPlace& pl = place[level];
  *L = AlignLevel{f.pyr + pl.img, (const float*)(f.pyr + pl.gx), (const float*)(f.pyr + pl.gy), pl.w, pl.h, pl.w};
  return true;
}

// What both alignment calls check before anything is enqueued, for the levels [level_lo, level_hi].
int align_check(flame_stereo_ctx* ctx, const flame_stereo_align_params* P, uint32_t ref_id, uint32_t new_id, int level_lo,
                int level_hi, const float* map_host, const void* map_device) {
  if (!P || (map_host != nullptr) == (map_device != nullptr)) return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (!ctx->have_camera) return FLAME_NLTGV2_ERR_NO_GRAPH;
  const float* K = ctx->cam.K;
  if (K[1] != 0.0f || K[3] != 0.0f || K[6] != 0.0f || K[7] != 0.0f || K[8] != 1.0f) return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (!(P->huber_k > 0.0f) || !std::isfinite(P->huber_k) || P->border < 1) return FLAME_NLTGV2_ERR_INVALID_ARG;
  auto fr = ctx->frames.find(ref_id), fn = ctx->frames.find(new_id);
  if (fr == ctx->frames.end() || fn == ctx->frames.end()) return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (level_lo < 0 || level_hi < level_lo || level_hi >= align::kMaxLevels) return FLAME_NLTGV2_ERR_INVALID_ARG;
  for (int l = level_lo; l <= level_hi; ++l) {
    AlignLevel a, b;
    if (!frame_level(ctx, fr->second, l, &a) || !frame_level(ctx, fn->second, l, &b)) return FLAME_NLTGV2_ERR_INVALID_ARG;
    if (2L * P->border + 2 > std::min(a.w, a.h)) return FLAME_NLTGV2_ERR_INVALID_ARG;
  }
  return 0;
}

// Scratch of the linearisation and the map on the device; after this nothing allocates.  *d_map_out: the map to read.
int align_prepare(flame_stereo_ctx* ctx, const float* map_host, const void* map_device, const float** d_map_out) {
  const int w = ctx->cam.width, h = ctx->cam.height;
  const size_t want = (size_t)kAlignSums * (size_t)align_chunks((long)w * h);
  if (ctx->apart_cap < want || (map_host && ctx->map_cap < (size_t)w * h) || !ctx->d_asys)
    SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (buffers are about to be reallocated)
  if (int rc = grow(ctx, &ctx->d_apart, &ctx->apart_cap, want)) return rc;
  if (!ctx->d_asys) SCHK(ctx, hipMalloc((void**)&ctx->d_asys, sizeof(AlignSystem)));
  if (!ctx->h_asys) SCHK(ctx, hipHostMalloc((void**)&ctx->h_asys, sizeof(AlignSystem), hipHostMallocDefault));
  *d_map_out = (const float*)map_device;
  if (map_host) {
    if (int rc = grow(ctx, &ctx->d_map, &ctx->map_cap, (size_t)w * h)) return rc;
    SCHK(ctx, hipMemcpyAsync(ctx->d_map, map_host, (size_t)w * h * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (`map_host` is pageable memory)
    *d_map_out = ctx->d_map;
  }
  return 0;
}

// One linearisation at (q, t) on `level`: enqueues, waits once, fills *out from the pinned block.
int align_eval(flame_stereo_ctx* ctx, const flame_stereo_align_params& P, const Frame& ref, const Frame& cur, int level,
               const float* d_map, const double q[4], const double t[3], flame_stereo_align_system* out) {
  AlignArgs a;
  frame_level(ctx, ref, level, &a.ref);
  frame_level(ctx, cur, level, &a.cur);
  a.map = d_map, a.map_w = ctx->cam.width, a.shift = level;
  a.border = P.border, a.huber_k = P.huber_k;
  const float scale = (float)(1 << level);
  a.fx = ctx->cam.K[0] / scale, a.cx = ctx->cam.K[2] / scale, a.fy = ctx->cam.K[4] / scale, a.cy = ctx->cam.K[5] / scale;
  align::pose_to_float(q, t, a.R, a.t);
  SCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  SCHK(ctx, (hipError_t)launch_align_linearize(a, ctx->d_apart, ctx->d_asys, ctx->stream));
  SCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed = true;
  SCHK(ctx, hipMemcpyAsync(ctx->h_asys, ctx->d_asys, sizeof(AlignSystem), hipMemcpyDeviceToHost, ctx->stream));
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  static_assert(sizeof(AlignSystem) == sizeof(flame_stereo_align_system), "the device block is the C struct");
  std::memcpy(out, ctx->h_asys, sizeof *out);
  return 0;
}

}  // namespace

extern "C" {

int flame_stereo_build_pyramid(flame_stereo_ctx* ctx, uint32_t frame_id, int n_levels) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_build_pyramid");
  if (int rc = enter(ctx)) return rc;
  if (!ctx->have_camera) return FLAME_NLTGV2_ERR_NO_GRAPH;
  auto it = ctx->frames.find(frame_id);
  const int w = ctx->cam.width, h = ctx->cam.height;
  if (it == ctx->frames.end() || !align::levels_valid(w, h, n_levels)) return FLAME_NLTGV2_ERR_INVALID_ARG;
  Frame& f = it->second;
  if (f.pyr_levels == n_levels) return 0;
  align::LevelPlace place[align::kMaxLevels];
  if (!f.pyr && n_levels > 1) {  // (sized for every level the camera could have: one size per camera, so the buffer can be handed on)
    const size_t bytes = align::place_levels(w, h, align::kMaxLevels, place);
    SCHK(ctx, hipMalloc((void**)&f.pyr, bytes));
  }
  align::place_levels(w, h, n_levels, place);
  AlignLevel src;
  frame_level(ctx, f, 0, &src);
  const uint8_t* s_img = src.img;
  int sw = src.w, sh = src.h, sp = src.pitch;
  SCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  for (int l = 1; l < n_levels; ++l) {
    const align::LevelPlace& pl = place[l];
    SCHK(ctx, (hipError_t)launch_pyr_down(s_img, sw, sh, sp, f.pyr + pl.img, (float*)(f.pyr + pl.gx), (float*)(f.pyr + pl.gy),
                                          ctx->stream));
    s_img = f.pyr + pl.img, sw = pl.w, sh = pl.h, sp = pl.w;
  }
  SCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed = true;
  f.pyr_levels = n_levels;
  return 0;
}

int flame_stereo_download_pyramid_level(flame_stereo_ctx* ctx, uint32_t frame_id, int level, uint8_t* img, float* gradx,
                                        float* grady) {
  if (int rc = enter(ctx)) return rc;
  if (!ctx->have_camera) return FLAME_NLTGV2_ERR_NO_GRAPH;
  auto it = ctx->frames.find(frame_id);
  AlignLevel L;
  if (it == ctx->frames.end() || !frame_level(ctx, it->second, level, &L)) return FLAME_NLTGV2_ERR_INVALID_ARG;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (img) SCHK(ctx, hipMemcpy2D(img, (size_t)L.w, L.img, (size_t)L.pitch, (size_t)L.w, (size_t)L.h, hipMemcpyDeviceToHost));
  if (gradx)
    SCHK(ctx, hipMemcpy2D(gradx, (size_t)L.w * 4, L.gx, (size_t)L.pitch * 4, (size_t)L.w * 4, (size_t)L.h, hipMemcpyDeviceToHost));
  if (grady)
    SCHK(ctx, hipMemcpy2D(grady, (size_t)L.w * 4, L.gy, (size_t)L.pitch * 4, (size_t)L.w * 4, (size_t)L.h, hipMemcpyDeviceToHost));
  return 0;
}

int flame_stereo_align_linearize(flame_stereo_ctx* ctx, const flame_stereo_align_params* params, uint32_t ref_frame_id,
                                 uint32_t new_frame_id, int level, const float* idepthmap_host, const void* idepthmap_device,
                                 const double q_ref_to_new[4], const double t_ref_to_new[3], flame_stereo_align_system* out) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_align_linearize");
  if (int rc = enter(ctx)) return rc;
  if (!q_ref_to_new || !t_ref_to_new || !out) return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (int rc = align_check(ctx, params, ref_frame_id, new_frame_id, level, level, idepthmap_host, idepthmap_device)) return rc;
  if (!align::pose_finite(q_ref_to_new, t_ref_to_new)) return FLAME_NLTGV2_ERR_INVALID_ARG;
  const float* d_map = nullptr;
  if (int rc = align_prepare(ctx, idepthmap_host, idepthmap_device, &d_map)) return rc;
  return align_eval(ctx, *params, ctx->frames.find(ref_frame_id)->second, ctx->frames.find(new_frame_id)->second, level, d_map,
                    q_ref_to_new, t_ref_to_new, out);
}

int flame_stereo_align_frame(flame_stereo_ctx* ctx, const flame_stereo_align_params* params, uint32_t ref_frame_id,
                             uint32_t new_frame_id, const float* idepthmap_host, const void* idepthmap_device,
                             const double q_init[4], const double t_init[3], flame_stereo_align_result* out,
                             flame_stereo_align_trace* trace, int max_trace, int* n_trace) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_align_frame");
  if (int rc = enter(ctx)) return rc;
  if (n_trace) *n_trace = 0;
  if (!params || !q_init || !t_init || !out || max_trace < 0 || (max_trace > 0 && !trace)) return FLAME_NLTGV2_ERR_INVALID_ARG;
  const flame_stereo_align_params& P = *params;
  if (P.max_iters_per_level < 1 || P.min_pixels < 1 || !(P.min_step >= 0.0) || !std::isfinite(P.min_step) ||
      !(P.lm_lambda >= 0.0) || !std::isfinite(P.lm_lambda))
    return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (int rc = align_check(ctx, params, ref_frame_id, new_frame_id, P.finest_level, P.coarsest_level, idepthmap_host,
                           idepthmap_device))
    return rc;
  if (!align::pose_finite(q_init, t_init)) return FLAME_NLTGV2_ERR_INVALID_ARG;
  double q[4], t[3] = {t_init[0], t_init[1], t_init[2]};
  const double qn = std::sqrt(((q_init[0] * q_init[0] + q_init[1] * q_init[1]) + q_init[2] * q_init[2]) + q_init[3] * q_init[3]);
  if (!(qn > 0.0) || !std::isfinite(qn)) return FLAME_NLTGV2_ERR_INVALID_ARG;
  for (int k = 0; k < 4; ++k) q[k] = q_init[k] / qn;
  const float* d_map = nullptr;
  if (int rc = align_prepare(ctx, idepthmap_host, idepthmap_device, &d_map)) return rc;
  const Frame& ref = ctx->frames.find(ref_frame_id)->second;
  const Frame& cur = ctx->frames.find(new_frame_id)->second;

  std::memset(out, 0, sizeof *out);
  int n_evals = 0;
  bool have_first = false;
  flame_stereo_align_system sys;
  const double zero6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  auto eval = [&](int level, const double* eq, const double* et, const double* delta, flame_stereo_align_system* s) -> int {
    if (int rc = align_eval(ctx, P, ref, cur, level, d_map, eq, et, s)) return rc;
    if (n_evals < max_trace) {
      flame_stereo_align_trace& e = trace[n_evals];
      std::memset(&e, 0, sizeof e);
      e.level = level, e.accepted = 1;
      std::memcpy(e.q, eq, sizeof e.q);
      std::memcpy(e.t, et, sizeof e.t);
      std::memcpy(e.delta, delta, sizeof e.delta);
      e.sys = *s;
    }
    ++n_evals;
    return 0;
  };
  int status = FLAME_STEREO_ALIGN_OK, flags = 0;
  for (int level = P.coarsest_level; level >= P.finest_level && status == FLAME_STEREO_ALIGN_OK; --level) {
    if (int rc = eval(level, q, t, zero6, &sys)) return rc;
    if (!have_first) out->first_mean_cost = sys.cost / (double)sys.n_used, have_first = true;
    for (int iter = 0;; ++iter) {
      if (sys.n_used < P.min_pixels) {
        status = FLAME_STEREO_ALIGN_TOO_FEW;
        break;
      }
      if (iter >= P.max_iters_per_level) {
        flags |= FLAME_STEREO_ALIGN_FLAG_MAX_ITERS;
        break;
      }
      double delta[6];
      if (!align::solve(sys.H, sys.b, P.lm_lambda, delta)) {
        flags |= FLAME_STEREO_ALIGN_FLAG_NOT_PD;
        break;
      }
      double q2[4], t2[3];
      align::exp_left(delta, q, t, q2, t2);
      flame_stereo_align_system sys2;
      const int slot = n_evals;
      if (int rc = eval(level, q2, t2, delta, &sys2)) return rc;
      if (!align::accept(sys2.cost, sys2.n_used, sys.cost, sys.n_used)) {
        if (slot < max_trace) trace[slot].accepted = 0;
        flags |= FLAME_STEREO_ALIGN_FLAG_REJECTED;
        break;
      }
      std::memcpy(q, q2, sizeof q);
      std::memcpy(t, t2, sizeof t);
      sys = sys2;
      out->iters[level] += 1;
      if (align::max_abs(delta) < P.min_step) break;
    }
  }
  out->status = status, out->flags = flags;
  std::memcpy(out->q, q, sizeof q);
  std::memcpy(out->t, t, sizeof t);
  for (int k = 0; k < 4; ++k) out->q_f32[k] = (float)q[k];
  align::pose_to_float(q, t, out->R_f32, out->t_f32);
  out->last_mean_cost = sys.cost / (double)sys.n_used;
  out->n_evals = n_evals;
  if (n_trace) *n_trace = n_evals;
  return 0;
}

float flame_stereo_last_kernel_ms(flame_stereo_ctx* ctx) {
  if (!ctx || !ctx->timed) return -1.0f;
  if (hipSetDevice(ctx->device) != hipSuccess || hipEventSynchronize(ctx->ev1) != hipSuccess) return -1.0f;
  float ms = -1.0f;
  if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) != hipSuccess) return -1.0f;
  return ms;
}

int flame_stereo_last_hip_error(const flame_stereo_ctx* ctx) { return ctx ? ctx->last_hip : 0; }

}  // extern "C"
