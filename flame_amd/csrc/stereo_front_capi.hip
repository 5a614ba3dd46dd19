// stereo_front_capi.hip -- C-ABI of include/flame_stereo.h, the front end on the resident feature set: projectFeatures,
// detectFeatures, prunePoseFrames and the selection of the graph's vertices (syncGraph's preprocessing).  The context:
// stereo_context.hpp; all arithmetic runs in feature_kernels.hip, this file only moves bytes.
#include <algorithm>
#include <cstring>
#include <vector>

#include "stereo_context.hpp"
#include "roctx_ranges.hpp"

using namespace flame_hip;

namespace {

// The table of the pose-frames a stage projects from, in pageable memory: the caller waits before it goes.
std::vector<ProjectPoseEntry> project_pose_table(const StereoCamera& cam, int n_poses, const flame_stereo_pose* poses) {
  std::vector<ProjectPoseEntry> table((size_t)n_poses);
  for (int k = 0; k < n_poses; ++k) {
    std::memset(&table[k], 0, sizeof table[k]);
    table[k].frame_id = poses[k].frame_id;
    load_geometry(table[k].geo, cam, poses[k].q_ref_to_new, poses[k].t_ref_to_new);
  }
  return table;
}

// A stage that reports through the front-end stats block: resets it (the two error indices at INT_MAX, the rest 0), enqueues
// `launch` between the events, copies the block back and waits.  Buffers are grown and tables uploaded before.  Returns the
// stage's status by `rule`, the failing record in *error_feature; at 0 ctx->h_fstats holds the stage's words.
template <typename F>
int front_stage(flame_stereo_ctx* ctx, host::ErrorRule rule, int* error_feature, F&& launch) {
  int* s = ctx->h_fstats;
  s[kFrontAssert] = s[kFrontBadFrame] = INT_MAX;
  for (int w = kFrontCount; w < kFrontWords; ++w) s[w] = 0;
  SCHK(ctx, hipMemcpyAsync(ctx->d_fstats, s, kFrontWords * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  if (int rc = timed(ctx, launch)) return rc;
  SCHK(ctx, hipMemcpyAsync(s, ctx->d_fstats, kFrontWords * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (also: tables, maps and masks of the caller's were pageable memory)
  return decode_error(s[kFrontAssert], s[kFrontBadFrame], rule, error_feature);
}

void clear_prune_stats(flame_stereo_prune_stats* stats) {
  std::memset(stats, 0, sizeof *stats);
  stats->error_feature = -1;
}

// Flame::prunePoseFrames' feature loops on `d_in` (n records in device memory): validates, uploads the tables, launches
// and waits.  On success *moved_out tells where the records are: false = in place in d_in (nothing was removed), true =
// compacted in ctx->d_res_alt.  Nothing of the context changes here; the callers commit.
int run_prune(flame_stereo_ctx* ctx, const flame_stereo_params* params, uint32_t target_frame_id, int n_keep,
              const uint32_t* keep_ids, int n_dropped, const flame_stereo_pose* dropped, int first_new, int n,
              StereoFeature* d_in, bool* moved_out, flame_stereo_prune_stats* stats) {
  *moved_out = false;
  clear_prune_stats(stats);
  if (!params || n_keep < 1 || !keep_ids || n_dropped < 0 || (n_dropped > 0 && !dropped) || first_new < 0 || first_new > n)
    return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (!ctx->have_camera) return FLAME_NLTGV2_ERR_NO_GRAPH;
  if (std::find(keep_ids, keep_ids + n_keep, target_frame_id) == keep_ids + n_keep) return FLAME_NLTGV2_ERR_INVALID_ARG;
  for (int k = 0; k < n_dropped; ++k)  // a pose-frame cannot both stay and go (this also keeps the target out of `dropped`)
    if (std::find(keep_ids, keep_ids + n_keep, dropped[k].frame_id) != keep_ids + n_keep) return FLAME_NLTGV2_ERR_INVALID_ARG;
  const int border = host::front_border(params->rescale_factor_max, params->win_size);
  if (border < 1) return FLAME_NLTGV2_ERR_INVALID_ARG;  // (rect_contains relies on a rectangle that excludes 0)
  const host::ScanRect r = host::scan_rect(ctx->cam.width, ctx->cam.height, border, params->do_letterbox != 0);
  const PruneRegion region = {r.c_lo, r.r_lo, r.w(), r.h()};
  stats->num_examined = n, stats->num_features = n;
  if (n == 0) return 0;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (buffers may be reallocated; the pinned stats block is reused)
  const size_t groups = ((size_t)n + 255) / 256;
  if (int rc = grow(ctx, ctx->d_res_alt, (size_t)n)) return rc;
  if (int rc = grow(ctx, ctx->d_proj_tmp, (size_t)n)) return rc;
  if (int rc = grow(ctx, ctx->d_keep, (size_t)n)) return rc;
  if (int rc = grow(ctx, ctx->d_groups, 3 * groups)) return rc;
  if (int rc = grow(ctx, ctx->d_ppose, (size_t)n_dropped + 1)) return rc;
  if (int rc = grow(ctx, ctx->d_keep_ids, (size_t)n_keep)) return rc;
  const std::vector<ProjectPoseEntry> table = project_pose_table(ctx->cam, n_dropped, dropped);
  if (n_dropped > 0)
    SCHK(ctx, hipMemcpyAsync(ctx->d_ppose, table.data(), (size_t)n_dropped * sizeof(ProjectPoseEntry), hipMemcpyHostToDevice,
                             ctx->stream));
  SCHK(ctx, hipMemcpyAsync(ctx->d_keep_ids, keep_ids, (size_t)n_keep * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  // pfs_[feat.frame_id] of a frame that is neither kept nor listed comes before any assert
  if (int rc = front_stage(ctx, host::ErrorRule::kBadFrameFirst, &stats->error_feature, [&] {
        return launch_prune_features(ctx->cam, region, n_keep, ctx->d_keep_ids, n_dropped, ctx->d_ppose, target_frame_id, first_new,
                                     n, d_in, ctx->d_proj_tmp, ctx->d_keep, ctx->d_groups, ctx->d_res_alt, ctx->d_fstats,
                                     ctx->stream);
      })) return rc;
  const int* s = ctx->h_fstats;
  *moved_out = s[kFrontCount] != n;
  stats->num_moved = s[kPruneStatMoved], stats->num_invalidated = s[kPruneStatInvalidated];
  stats->num_removed = n - s[kFrontCount], stats->num_features = s[kFrontCount];
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
// uploads the pose table, launches, copies the result into the pinned block and waits for it.  Every error return leaves
// *out as the caller cleared it, but for num_examined and error_feature.
int run_select(flame_stereo_ctx* ctx, const flame_stereo_graph_params* gp, float graph_scale, int n_poses,
               const flame_stereo_world_pose* poses, int n, const StereoFeature* d_feats, const StereoFeature* d_proj,
               flame_stereo_graph_inputs* out) {
  out->num_examined = n;
  if (n == 0) return 0;
  const size_t groups = ((size_t)n + 255) / 256;
  const size_t words = (size_t)kFrontWords + 6 * (size_t)n;
  if (int rc = grow(ctx, ctx->d_keep, (size_t)n)) return rc;
  if (int rc = grow(ctx, ctx->d_groups, 4 * groups)) return rc;
  if (int rc = grow(ctx, ctx->d_spose, (size_t)n_poses + 1)) return rc;
  if (int rc = grow(ctx, ctx->d_sel, words)) return rc;
  if (int rc = grow(ctx, ctx->h_sel, words)) return rc;
  std::vector<SelectPoseEntry> table((size_t)n_poses);
  for (int k = 0; k < n_poses; ++k) table[k] = select_pose_entry(poses[k].frame_id, poses[k].q, poses[k].t);
  if (n_poses > 0)
    SCHK(ctx, hipMemcpyAsync(ctx->d_spose, table.data(), (size_t)n_poses * sizeof(SelectPoseEntry), hipMemcpyHostToDevice, ctx->stream));
  for (int w = 0; w < kFrontWords; ++w) ctx->h_fstats[w] = 0;
  ctx->h_fstats[kFrontAssert] = ctx->h_fstats[kFrontBadFrame] = ctx->h_fstats[kSelectBadId] = INT_MAX;
  SCHK(ctx, hipMemcpyAsync(ctx->d_sel, ctx->h_fstats, kFrontWords * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  const SelectRule rule = {gp->idepth_var_max_graph, gp->min_height, gp->max_height, graph_scale, gp->adaptive_data_weights};
  // The copy-out.  0: the whole block in one copy, sections n words apart, one wait.  1: the stats words, a wait, then the
  // 6 V words the kernel packed V words apart, a second wait.  Which is faster: profiles/graph_inputs.txt.
  const bool count_first = ctx->graph_copy == 1;
  if (int rc = timed(ctx, [&] {
        return launch_select_graph_features(ctx->cam, rule, n_poses, ctx->d_spose, n, d_feats, d_proj, ctx->d_keep, ctx->d_groups,
                                            count_first ? 0 : n, ctx->d_sel, ctx->stream);
      })) return rc;
  SCHK(ctx, hipMemcpyAsync(ctx->h_sel, ctx->d_sel, (count_first ? (size_t)kFrontWords : words) * sizeof(int),
                           hipMemcpyDeviceToHost, ctx->stream));
  SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (also: `table` was pageable memory)
  const int* s = ctx->h_sel;
  // the reference's loop stops at the first record that fails either check
  if (int rc = decode_error(s[kFrontAssert], s[kFrontBadFrame], host::ErrorRule::kLowerIndex, &out->error_feature)) return rc;
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
  out->num_invalid = s[kSelectStatInvalid], out->num_fail_var = s[kSelectStatFailVar], out->num_fail_height = s[kSelectStatFailHeight];
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

void flame_stereo_default_detect_params(flame_stereo_detect_params* p) {
  if (!p) return;
  p->detection_win_size = 16, p->min_grad_mag = 5.0f;
  p->idepth_init = 0.01f, p->idepth_var_init = 0.5f * 0.5f;
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
  if (int rc = grow(ctx, ctx->d_res_alt, (size_t)n)) return rc;
  if (int rc = grow(ctx, ctx->d_proj_alt, (size_t)n)) return rc;
  if (int rc = grow(ctx, ctx->d_proj_tmp, (size_t)n)) return rc;
  if (int rc = grow(ctx, ctx->d_keep, (size_t)n)) return rc;
  if (int rc = grow(ctx, ctx->d_groups, (size_t)n / 256 + 1)) return rc;
  if (int rc = grow(ctx, ctx->d_ppose, (size_t)n_poses + 1)) return rc;
  const std::vector<ProjectPoseEntry> table = project_pose_table(ctx->cam, n_poses, poses);
  const int border = host::front_border(params->rescale_factor_max, params->win_size);  // (no guard here, as before)
  const host::ScanRect r = host::scan_rect(ctx->cam.width, ctx->cam.height, border, params->do_letterbox != 0);
  const ProjectRegion region = {(float)r.c_lo, (float)r.r_lo, (float)r.w(), (float)r.h()};
  if (n_poses > 0)
    SCHK(ctx, hipMemcpyAsync(ctx->d_ppose, table.data(), (size_t)n_poses * sizeof(ProjectPoseEntry), hipMemcpyHostToDevice, ctx->stream));
  // pfs.at() of an unknown frame would throw before any assert
  if (int rc = front_stage(ctx, host::ErrorRule::kBadFrameFirst, stats ? &stats->error_feature : nullptr, [&] {
        return launch_project_features(ctx->cam, region, n_poses, ctx->d_ppose, cur_frame_id, n, ctx->d_res, ctx->d_proj_tmp,
                                       ctx->d_keep, ctx->d_groups, ctx->d_res_alt, ctx->d_proj_alt, ctx->d_fstats, ctx->stream);
      })) return rc;
  ctx->d_res.swap(ctx->d_res_alt);
  ctx->d_proj.swap(ctx->d_proj_alt);
  ctx->n_res = ctx->n_proj = ctx->h_fstats[kFrontCount];
  ctx->aligned = true;
  if (stats) stats->num_features = ctx->n_res;
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
  const int border = host::front_border(params->rescale_factor_max, params->win_size);
  if (border < 0) return FLAME_NLTGV2_ERR_INVALID_ARG;  // (0 scans the whole image, as the reference's loops do)
  const host::ScanRect r = host::scan_rect(ctx->cam.width, ctx->cam.height, border, params->do_letterbox != 0);
  DetectGrid G;
  G.win = dparams->detection_win_size;
  G.hc = host::ceil_cells(height, G.win), G.wc = host::ceil_cells(width, G.win);
  G.r_lo = r.r_lo, G.r_hi = r.r_hi, G.c_lo = r.c_lo, G.c_hi = r.c_hi;
  G.g2 = dparams->min_grad_mag * dparams->min_grad_mag;
  const int n_cells = G.hc * G.wc;
  if (stats) stats->num_examined = n_cells;
  const int n_pts = n_mask < 0 ? ctx->n_proj : n_mask;
  for (int i = 0; i < n_mask; ++i)  // host points are checked here
    if (!host::mask_point_valid(mask_xy[2 * i], mask_xy[2 * i + 1], width, height, G.win, G.wc, G.hc))
      return FLAME_NLTGV2_ERR_INVALID_ARG;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (buffers may be reallocated; the pinned stats block is reused)
  const int n_res = ctx->n_res;
  if (int rc = grow_keep(ctx, ctx->d_res, (size_t)n_res + (size_t)n_cells + 1, (size_t)n_res)) return rc;
  if (int rc = grow(ctx, ctx->d_cell_key, (size_t)n_cells + 1)) return rc;
  if (int rc = grow(ctx, ctx->d_blocked, (size_t)n_cells + 1)) return rc;
  if (int rc = grow(ctx, ctx->d_groups, (size_t)n_cells / 256 + 1)) return rc;
  const float* d_map = (const float*)idepthmap_device;
  if (idepthmap_host) {
    if (int rc = grow(ctx, ctx->d_map, (size_t)width * height)) return rc;
    SCHK(ctx, hipMemcpyAsync(ctx->d_map, idepthmap_host, (size_t)width * height * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    d_map = ctx->d_map;
  }
  const float* d_mask = nullptr;
  int mask_stride = 2;
  if (n_mask > 0) {
    if (int rc = grow(ctx, ctx->d_mask, (size_t)n_mask * 2)) return rc;
    SCHK(ctx, hipMemcpyAsync(ctx->d_mask, mask_xy, (size_t)n_mask * 2 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    d_mask = ctx->d_mask;
  } else if (n_mask < 0 && n_pts > 0) {
    d_mask = &ctx->d_proj.p->x;
    mask_stride = (int)(sizeof(StereoFeature) / sizeof(float));
  }
  Geo geo;
  load_geometry(geo, ctx->cam, q_ref_to_prev, t_ref_to_prev);
  DetectInit init = {first_id, ref_frame_id, dparams->idepth_init, dparams->idepth_var_init};
  // on an assert the records written past n_res are not part of the set
  if (int rc = front_stage(ctx, host::ErrorRule::kAssertOnly, stats ? &stats->error_feature : nullptr, [&] {
        return launch_detect_features(G, geo, ctx->cam, fr->second.gx_pad, fr->second.gy_pad, n_pts, d_mask, mask_stride,
                                      ctx->d_blocked, ctx->d_cell_key, ctx->d_groups, init, d_map, ctx->d_res + n_res, ctx->d_fstats,
                                      ctx->stream);
      })) return rc;
  const int n_new = ctx->h_fstats[kFrontCount];
  ctx->n_res = n_res + n_new;
  if (n_new > 0) ctx->aligned = false;  // (records without a projected counterpart)
  if (stats) stats->num_features = n_new;
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
    ctx->d_res.swap(ctx->d_res_alt);
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
  flame_stereo_prune_stats local;
  if (!stats) stats = &local;
  clear_prune_stats(stats);
  if (!n_feats || *n_feats < 0 || (*n_feats > 0 && !feats)) return FLAME_NLTGV2_ERR_INVALID_ARG;
  const int n = *n_feats;
  if (int rc = grow(ctx, ctx->d_feats, (size_t)n + 1)) return rc;
  if (n > 0)
    SCHK(ctx, hipMemcpyAsync(ctx->d_feats, feats, (size_t)n * sizeof(StereoFeature), hipMemcpyHostToDevice, ctx->stream));
  bool moved = false;
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

void flame_stereo_default_graph_params(flame_stereo_graph_params* p) {
  if (!p) return;
  p->idepth_var_max_graph = 1e-2f, p->adaptive_data_weights = 0;
  p->min_height = 0.1f, p->max_height = 4.0f;
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
  return run_select(ctx, gp, graph_scale, n_poses, poses, ctx->n_res, ctx->d_res, ctx->d_proj, out);
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
  if (int rc = grow(ctx, ctx->d_feats, (size_t)n_feats + 1)) return rc;
  if (int rc = grow(ctx, ctx->d_proj_tmp, (size_t)n_feats + 1)) return rc;
  if (n_feats > 0) {
    const size_t bytes = (size_t)n_feats * sizeof(StereoFeature);
    SCHK(ctx, hipMemcpyAsync(ctx->d_feats, feats, bytes, hipMemcpyHostToDevice, ctx->stream));
    SCHK(ctx, hipMemcpyAsync(ctx->d_proj_tmp, feats_in_curr, bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  return run_select(ctx, gp, graph_scale, n_poses, poses, n_feats, ctx->d_feats, ctx->d_proj_tmp, out);
}

}  // extern "C"
