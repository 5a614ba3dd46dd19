// stereo_debug_align_capi.hip -- C-ABI of include/flame_stereo.h: the three pictures of the front end (features, matches,
// detections), the pyramid levels and the direct alignment.  The context: stereo_context.hpp; all arithmetic runs in
// debug_kernels.hip, matches_kernels.hip, detections_kernels.hip and align_kernels.hip (the alignment's host steps: align_host.hpp).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "stereo_context.hpp"
#include "debug_kernels.h"
#include "detections_kernels.h"
#include "matches_kernels.h"
#include "align_host.hpp"
#include "roctx_ranges.hpp"

using namespace flame_hip;

namespace {

// What the pictures read of the frame they are painted over.
template <typename Args>
void set_gray(const flame_stereo_ctx* ctx, const Frame& f, int flip, Args* a) {
  a->rows = ctx->cam.height, a->cols = ctx->cam.width;
  a->gray = interior(ctx->cam, f.img_pad), a->gray_step = padded_pitch(ctx->cam);
  a->flip = flip != 0;
}

// ---- pyramid levels and direct alignment ----

// Level `level` of frame f, or false when it is not built.
bool frame_level(const flame_stereo_ctx* ctx, const Frame& f, int level, AlignLevel* L) {
  const int w = ctx->cam.width, h = ctx->cam.height;
  if (level == 0) {
    *L = AlignLevel{interior(ctx->cam, f.img_pad), interior(ctx->cam, f.gx_pad), interior(ctx->cam, f.gy_pad), w, h,
                    padded_pitch(ctx->cam)};
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
  if (ctx->d_apart.cap < want || (map_host && ctx->d_map.cap < (size_t)w * h) || !ctx->d_asys)
    SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (buffers are about to be reallocated)
  if (int rc = grow(ctx, ctx->d_apart, want)) return rc;
  if (!ctx->d_asys) SCHK(ctx, ctx->d_asys.alloc(1));
  if (!ctx->h_asys) SCHK(ctx, ctx->h_asys.alloc(1));
  *d_map_out = (const float*)map_device;
  if (map_host) {
    if (int rc = grow(ctx, ctx->d_map, (size_t)w * h)) return rc;
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
  if (int rc = timed(ctx, [&] { return launch_align_linearize(a, ctx->d_apart, ctx->d_asys, ctx->stream); })) return rc;
  SCHK(ctx, hipMemcpyAsync(ctx->h_asys, ctx->d_asys, sizeof(AlignSystem), hipMemcpyDeviceToHost, ctx->stream));
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  static_assert(sizeof(AlignSystem) == sizeof(flame_stereo_align_system), "the device block is the C struct");
  std::memcpy(out, ctx->h_asys, sizeof *out);
  return 0;
}

}  // namespace

extern "C" {

int flame_stereo_draw_features(flame_stereo_ctx* ctx, uint32_t cur_frame_id, float idepth_var_max_graph,
                               float scene_color_scale, int flip, uint8_t* img_out, int32_t* num_converged,
                               int32_t* num_unconverged) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_draw_features");
  if (int rc = enter(ctx)) return rc;
  if (!img_out) return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (!ctx->have_camera) return FLAME_NLTGV2_ERR_NO_GRAPH;
  auto fr = ctx->frames.find(cur_frame_id);
  if (fr == ctx->frames.end()) return FLAME_NLTGV2_ERR_INVALID_ARG;
  const size_t px = (size_t)ctx->cam.width * ctx->cam.height;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (buffers may be reallocated)
  if (int rc = grow(ctx, ctx->d_owner, px + 2)) return rc;
  if (int rc = grow(ctx, ctx->d_draw, 3 * px + 16)) return rc;
  DebugImageArgs a;
  set_gray(ctx, fr->second, flip, &a);
  a.scene_color_scale = scene_color_scale;
  a.k00 = a.k11 = 0.0f;
  int* d_counts = (int*)(ctx->d_owner + px);
  if (int rc = timed(ctx, [&] {
        return launch_draw_features(a, ctx->n_proj, ctx->n_proj > 0 ? (const void*)&ctx->d_proj.p->x : nullptr,
                                    (int)sizeof(StereoFeature), idepth_var_max_graph, ctx->d_owner, d_counts, ctx->d_draw,
                                    ctx->stream);
      })) return rc;
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
  if (decode_error(ctx->h_stats[kStatAssert], ctx->h_stats[kStatBadFrame], host::ErrorRule::kBadFrameFirst, nullptr) != 0) {
    ctx->match_stand = false;  // that update returned an error
    return FLAME_NLTGV2_ERR_INVALID_ARG;
  }
  const int width = ctx->cam.width, height = ctx->cam.height, n = ctx->match_n;
  const size_t px = (size_t)width * height;
  if (int rc = grow(ctx, ctx->d_mlist, 3 * px + kMatchCounts)) return rc;
  if (int rc = grow(ctx, ctx->d_mentries, host::entry_capacity(px, ctx->match_last_total))) return rc;
  if (int rc = grow(ctx, ctx->d_draw, 3 * px + 16)) return rc;
  MatchBuffers b;
  b.cnt = ctx->d_mlist, b.offset = ctx->d_mlist + px, b.fill = ctx->d_mlist + 2 * px, b.counts = (int*)(ctx->d_mlist + 3 * px);
  b.entries = ctx->d_mentries, b.capacity = (uint32_t)std::min<size_t>(host::entry_capacity(px, ctx->match_last_total), UINT32_MAX);
  MatchImageArgs a;
  set_gray(ctx, fr->second, flip, &a);
  int counts[kMatchCounts] = {0};
  if (int rc = timed(ctx, [&] {
        hipError_t e = (hipError_t)launch_matches_lists(n, ctx->d_match, b, height, width, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(counts, b.counts, sizeof counts, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = (hipError_t)launch_matches_paint(n, ctx->d_match, b, a, ctx->d_draw, ctx->stream);
        return e;
      })) return rc;
  SCHK(ctx, hipMemcpyAsync(img_out, ctx->d_draw, 3 * px, hipMemcpyDeviceToHost, ctx->stream));
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  const size_t total = (size_t)(uint32_t)counts[kMatchTotal];
  ctx->match_last_total = total;
  int refilled = 0;
  if (total > (size_t)b.capacity) {  // the entry buffer was too small: grow it, repeat fill and fold (cnt and offset stand)
    if (int rc = grow(ctx, ctx->d_mentries, host::entry_capacity(px, ctx->match_last_total))) return rc;
    b.entries = ctx->d_mentries, b.capacity = (uint32_t)std::min<size_t>(host::entry_capacity(px, ctx->match_last_total), UINT32_MAX);
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
  const int border = host::front_border(params->rescale_factor_max, params->win_size);
  if (border < 0) return FLAME_NLTGV2_ERR_INVALID_ARG;  // (as flame_stereo_detect_features)
  const host::ScanRect r = host::scan_rect(ctx->cam.width, ctx->cam.height, border, params->do_letterbox != 0);
  DetectGrid G;  // the scan rectangle and the threshold of flame_stereo_detect_features; the cell grid is not read
  G.win = 1, G.hc = G.wc = 0;
  G.r_lo = r.r_lo, G.r_hi = r.r_hi, G.c_lo = r.c_lo, G.c_hi = r.c_hi;
  G.g2 = dparams->min_grad_mag * dparams->min_grad_mag;
  const size_t px = (size_t)ctx->cam.width * ctx->cam.height;
  SCHK(ctx, hipStreamSynchronize(ctx->stream));  // (buffers may be reallocated)
  if (int rc = grow(ctx, ctx->d_owner, (size_t)kDetWords)) return rc;  // (scratch of the pictures: the stats words)
  if (int rc = grow(ctx, ctx->d_draw, 3 * px + 16)) return rc;
  DebugImageArgs a;
  set_gray(ctx, fr->second, flip, &a);
  a.scene_color_scale = 1.0f;
  a.k00 = a.k11 = 0.0f;
  Geo geo;
  load_geometry(geo, ctx->cam, q_ref_to_prev, t_ref_to_prev);
  int* d_stats = (int*)ctx->d_owner.p;
  int s[kDetWords] = {0};
  if (int rc = timed(ctx, [&] {
        return launch_draw_detections(a, G, geo, ctx->cam, fr->second.gx_pad, fr->second.gy_pad, max_score, d_stats, ctx->d_draw,
                                      ctx->stream);
      })) return rc;
  SCHK(ctx, hipMemcpyAsync(img_out, ctx->d_draw, 3 * px, hipMemcpyDeviceToHost, ctx->stream));
  SCHK(ctx, hipMemcpyAsync(s, d_stats, sizeof s, hipMemcpyDeviceToHost, ctx->stream));
  SCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (stats) {
    host::sum_slots(s, kDetCount, kDetSlots, kDetSlotStride, 1, &stats->num_scored);
    stats->num_examined = std::max(r.h(), 0) * std::max(r.w(), 0);
  }
  if (s[kDetAssert] != 0) {
    if (stats) stats->error_pixel = INT_MAX - s[kDetAssert];
    return FLAME_NLTGV2_ERR_ASSERT;
  }
  return 0;
}

void flame_stereo_default_align_params(flame_stereo_align_params* p) {
  if (!p) return;
  p->border = 2, p->huber_k = 10.0f;
  p->coarsest_level = 2, p->finest_level = 0;
  p->max_iters_per_level = 10, p->min_pixels = 100, p->min_step = 1e-5, p->lm_lambda = 0.0;
}

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
  AlignLevel s;
  frame_level(ctx, f, 0, &s);
  if (int rc = timed(ctx, [&] {  // (every level inside one pair of events)
        hipError_t e = hipSuccess;
        for (int l = 1; l < n_levels && e == hipSuccess; ++l) {
          const align::LevelPlace& pl = place[l];
          e = (hipError_t)launch_pyr_down(s.img, s.w, s.h, s.pitch, f.pyr + pl.img, (float*)(f.pyr + pl.gx), (float*)(f.pyr + pl.gy),
                                          ctx->stream);
          s.img = f.pyr + pl.img, s.w = pl.w, s.h = pl.h, s.pitch = pl.w;
        }
        return e;
      })) return rc;
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

}  // extern "C"
