// stereo_capi.hip -- C-ABI of include/flame_stereo.h: the context, the camera, resident frames (padded image + gradients built on
// the device, from grey or raw images), the per-launch pose table, the host/device feature-array entry points of the per-feature
// epipolar inverse-depth update, and the resident feature set.  projectFeatures / detectFeatures / prunePoseFrames and the selection
// of the graph's vertices: stereo_front_capi.hip; the pictures, the pyramid and the alignment: stereo_debug_align_capi.hip.  All
// arithmetic of the path runs in stereo_kernels.hip, feature_kernels.hip and input_kernels.hip; this file only moves bytes.
#include <cstring>
#include <new>

#include "stereo_context.hpp"
#include "input_kernels.h"
#include "input_params.hpp"
#include "roctx_ranges.hpp"

using namespace flame_hip;

namespace {

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
  if (int rc = grow(ctx, ctx->h_poses, (size_t)n_poses)) return rc;
  if (int rc = grow(ctx, ctx->d_poses, (size_t)n_poses + 1)) return rc;
  MatchRecord* records = nullptr;
  if (ctx->record_matches) {
    if (int rc = grow(ctx, ctx->d_match, (size_t)n_feats + 1)) return rc;
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
    SCHK(ctx, hipMemcpyAsync(ctx->d_poses, ctx->h_poses, (size_t)n_poses * sizeof(StereoPoseEntry), hipMemcpyHostToDevice, ctx->stream));
  std::memset(ctx->h_stats, 0, kStatWords * sizeof(int));
  ctx->h_stats[kStatAssert] = ctx->h_stats[kStatBadFrame] = INT_MAX;
  SCHK(ctx, hipMemcpyAsync(ctx->d_stats, ctx->h_stats, kStatWords * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  if (records && n_feats > 0)  // (all zero = nothing drawn: the early returns of the kernel need no code)
    SCHK(ctx, hipMemsetAsync(records, 0, (size_t)n_feats * sizeof(MatchRecord), ctx->stream));
  const Frame& f = nf->second;
  if (int rc = timed(ctx, [&] {
        return launch_update_feature_idepths(*params, ctx->cam, n_poses, ctx->d_poses, f.img_pad, f.gx_pad, f.gy_pad, curr_pf_id,
                                             n_feats, d_feats, ctx->d_stats, pick_lanes(ctx, n_feats), records, ctx->stream);
      })) return rc;
  SCHK(ctx, hipMemcpyAsync(ctx->h_stats, ctx->d_stats, kStatWords * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if (records) ctx->match_stand = true, ctx->match_n = n_feats, ctx->match_frame = new_frame_id;
  return 0;
}

int report(flame_stereo_ctx* ctx, flame_stereo_stats* stats) {
  const int* s = ctx->h_stats;
  int sums[6];  // the counters were accumulated in kStatSlots copies (stereo_kernels.h)
  host::sum_slots(s, kStatCount, kStatSlots, kStatSlotStride, 6, sums);
  stats->num_idepth_updates = sums[0], stats->num_fail_max_var = sums[1], stats->num_fail_max_dropouts = sums[2];
  stats->num_fail_ref_patch_grad = sums[3], stats->num_fail_ambiguous_match = sums[4], stats->num_fail_max_cost = sums[5];
  stats->success = sums[0] > 0;
  stats->error_feature = -1;
  return decode_error(s[kStatAssert], s[kStatBadFrame], host::ErrorRule::kBadFrameFirst, &stats->error_feature);
}

}  // namespace

extern "C" {

void flame_stereo_default_params(flame_stereo_params* p) {
  if (!p) return;
  p->min_baseline = 0.01f, p->do_letterbox = 0;
  p->rescale_factor_min = 0.7f, p->rescale_factor_max = 1.4f;
  p->idepth_var_max = 0.5f * 0.5f, p->max_dropouts = 5, p->outlier_sigma_thresh = 3.0f, p->do_meas_fusion = 1;
  p->win_size = 5, p->search_sigma = 2.0f, p->min_grad_mag = 5.0f;
  p->idepth_min = 1e-3f, p->idepth_max = 2.0f, p->epilength_min = 3.0f, p->epilength_max = 32.0f;
  p->process_var_factor = 1.01f, p->process_fail_var_factor = 1.1f;
  p->max_cost = 1300.0f, p->do_subpixel = 1, p->sample_dist = 1.0f, p->second_best_factor = 1.5f;
  p->z_win_size = 5, p->pixel_var = 16.0f, p->epipolar_line_var = 1.0f;
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
      ctx->d_stats.alloc(kStatWords) != hipSuccess || ctx->h_stats.alloc(kStatWords) != hipSuccess ||
      ctx->d_fstats.alloc(kFrontWords) != hipSuccess || ctx->h_fstats.alloc(kFrontWords) != hipSuccess ||
      ctx->d_istats.alloc(kInputWords) != hipSuccess || ctx->h_istats.alloc(kInputWords) != hipSuccess) {
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
  delete ctx;  // every array releases itself, then the events and the stream go (StereoStreams)
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
  if (int rc = grow(ctx, ctx->d_raw, (size_t)w * h)) return rc;
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
  if (ctx->d_raw.cap < (size_t)w * h) SCHK(ctx, hipStreamSynchronize(ctx->stream));  // an enqueued frame may still read d_raw
  if (int rc = grow(ctx, ctx->d_raw, (size_t)w * h)) return rc;
  const uint8_t* src = (const uint8_t*)raw;
  if (!raw_on_device) {
    if (int rc = grow(ctx, ctx->d_rawsrc, input_frame_bytes(in, row_stride_bytes))) return rc;
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
  if (int rc = timed(ctx, [&] {
        const hipError_t e = (hipError_t)launch_input_rectify(m, in.format, in.remap != 0, src, row_stride_bytes, w, h,
                                                              ctx->d_istats, ctx->d_raw, ctx->stream);
        if (e != hipSuccess) return e;
        return launch_frame_pad_gradient(ctx->d_raw, w, h, ctx->cam.border, f->img_pad, f->gx_pad, f->gy_pad, ctx->stream);
      })) return rc;
  if (stats) SCHK(ctx, hipMemcpyAsync(ctx->h_istats, ctx->d_istats, kInputWords * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  // a host source is pageable memory; a device source is the caller's to keep until the stream has passed (flame_stereo.h)
  if (!raw_on_device || stats) SCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (stats) host::sum_slots(ctx->h_istats, 0, kInputSlots, kInputSlotStride, 1, &stats->n_outside);
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

int flame_stereo_frame_image_device(flame_stereo_ctx* ctx, uint32_t frame_id, const void** img, int* step_bytes) {
  if (!ctx || !img || !step_bytes || !ctx->have_camera) return FLAME_NLTGV2_ERR_INVALID_ARG;
  auto it = ctx->frames.find(frame_id);
  if (it == ctx->frames.end()) return FLAME_NLTGV2_ERR_INVALID_ARG;
  *img = interior(ctx->cam, it->second.img_pad);
  *step_bytes = padded_pitch(ctx->cam);
  return 0;
}

int flame_stereo_update_feature_idepths(flame_stereo_ctx* ctx, const flame_stereo_params* params, uint32_t new_frame_id,
                                        uint32_t curr_pf_id, int n_poses, const flame_stereo_pose* poses, int n_feats,
                                        flame_stereo_feature* feats, flame_stereo_stats* stats) {
  flame_hip::RoctxRange roctx_range_("flame_stereo_update_feature_idepths");
  if (int rc = enter(ctx)) return rc;
  if (!stats || n_feats < 0 || (n_feats > 0 && !feats)) return FLAME_NLTGV2_ERR_INVALID_ARG;
  if (int rc = grow(ctx, ctx->d_feats, (size_t)n_feats + 1)) return rc;
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
  if (int rc = grow(ctx, ctx->d_res, (size_t)n_feats + 1)) return rc;
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

int flame_stereo_clear_features(flame_stereo_ctx* ctx) {
  if (int rc = enter(ctx)) return rc;
  ctx->n_res = 0;
  ctx->n_proj = 0;
  ctx->aligned = false;
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

float flame_stereo_last_kernel_ms(flame_stereo_ctx* ctx) {
  if (!ctx || !ctx->timed) return -1.0f;
  if (hipSetDevice(ctx->device) != hipSuccess || hipEventSynchronize(ctx->ev1) != hipSuccess) return -1.0f;
  float ms = -1.0f;
  if (hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) != hipSuccess) return -1.0f;
  return ms;
}

int flame_stereo_last_hip_error(const flame_stereo_ctx* ctx) { return ctx ? ctx->last_hip : 0; }

}  // extern "C"
