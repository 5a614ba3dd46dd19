// nltgv2_frame_capi.hip -- the rows around the solver that work on its device state (see nltgv2_context.hpp):
//   the mesh rasteriser       interpolate_mesh, interpolate_mesh_arrays on the solver's stream; interpolate_mesh_begin / _end beside it
//   the mesh outputs          mesh_outputs_begin / _end: triangle filters, vertex normals and idepths, the filtered map
//   the debug images          debug_images_begin / _end: idepth colours, normals, the w1 / w2 maps
//   the wireframe             debug_wireframe_begin / _end
//   the metric outputs        metric_outputs_begin / _end: depth image, millimetre image, point clouds, 3-D mesh
//   the map error             map_error_begin / _end: photometric or against a true map; box mean, histogram, ranks, sum, picture
//   the view renderer         render_view_begin / _end, render_view_arrays: the mesh seen from another camera, the nearest surface kept
//   the kept meshes           keep_mesh, keep_mesh_arrays, drop_mesh, kept_mesh_info, get_kept_mesh: what a pose-frame keeps of its mesh
//   the fusion of views       fuse_views_begin / _end: up to eight kept or live meshes in one camera, a vote per pixel
//   the volumetric map        volume_create / _reset / _destroy / _info / _download / _upload; volume_integrate_begin / _end: a depth map folded
//                             into the truncated-signed-distance volume; volume_raycast_begin / _end: the volume seen from a camera;
//                             volume_mesh_begin / _end: its surface as a triangle mesh with normals; volume_shift_begin / _end,
//                             volume_window, volume_follow: the window that follows the camera
//   the photometric residual  photo_set_images, photo_residual, photo_fuse, photo_residual_last
// The eleven begin / end pairs are stages on the side stream (raster_stream) and share one skeleton: every argument is checked before the
// stream or a buffer is touched, so an error leaves what an earlier begin put into the stage's pinned outputs, and its pending _end, as
// they are; open_stage; the stage's device buffers; its work between ev0 and ev1 with side_kernels_read_last behind the last reader of
// the canonical arrays; the copies out; close_stage.  What is a function of sizes and of the calls so far (the pinned layouts, the
// record of the resident triangles) is in side_stage.hpp.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include "debug_kernels.h"
#include "fuse_kernels.h"
#include "map_error_kernels.h"
#include "mesh_kernels.h"
#include "metric_kernels.h"
#include "nltgv2_context.hpp"
#include "view_kernels.h"
#include "volume_kernels.h"
#include "volume_mesh_kernels.h"
#include "wireframe_kernels.h"

// Which state a mesh stage on the side stream describes (interpolate_mesh_begin, mesh_outputs_begin), and the wait that lets `rs` read
// it in the canonical arrays.  FLAME_NLTGV2_OPT_MESH_STATE = 1 and runs enqueued since the last settle: the state that settle left,
// which the canonical arrays still hold (enqueue_run recorded ev_snap behind their last writer); the runs in flight are not waited
// for.  Otherwise the runs are settled and the state unpacked; the caller may enqueue the next run as soon as this returns.
static int mesh_state_on(flame_nltgv2_ctx* ctx, hipStream_t rs) {
  if (ctx->opt_mesh_state == 1 && !ctx->canon_valid && ctx->snap_topo == ctx->topo) {
    HIPCHK(ctx, hipStreamWaitEvent(rs, ctx->ev_snap, 0));
    return FLAME_NLTGV2_OK;
  }
  const int rc = ensure_canon(ctx);
  if (rc) return rc;
  HIPCHK(ctx, hipEventRecord(ctx->ev_canon, ctx->stream));
  HIPCHK(ctx, hipStreamWaitEvent(rs, ctx->ev_canon, 0));
  return FLAME_NLTGV2_OK;
}

// A begin without its end may still be writing the pinned outputs and the device buffers that are about to be reused: the side stream
// is waited for, then the pinned buffer holds `bytes` (grow_pinned; *replaced: what a pending _end would have returned is gone).
static int open_stage(flame_nltgv2_ctx* ctx, PinnedBuf& h, size_t bytes, bool* replaced) {
  HIPCHK(ctx, hipStreamSynchronize(ctx->raster_stream));
  return grow_pinned(ctx, h, bytes, replaced);
}
static int open_stage(flame_nltgv2_ctx* ctx, SideStage& st, size_t bytes) {
  bool replaced = false;
  const int rc = open_stage(ctx, st.h, bytes, &replaced);
  if (replaced) st.active = false;
  return rc;
}

// The side stream's kernels enqueued so far are the last readers of the canonical arrays (and the writers of the stage's device
// outputs): whoever rewrites those waits for THEM, not for the outputs' way to the host (the map: 0.05 ms at 640x480, 0.3 ms at
// 1920x1080 -- time a commit would stand still for).
static int side_kernels_read_last(flame_nltgv2_ctx* ctx) {
  HIPCHK(ctx, hipEventRecord(ctx->ev_raster_done, ctx->raster_stream));
  ctx->raster_inflight = true;
  return FLAME_NLTGV2_OK;
}

// Everything of the stage is enqueued: its _end may hand the pinned outputs out.
static int close_stage(flame_nltgv2_ctx* ctx, SideStage& st) {
  HIPCHK(ctx, hipEventRecord(st.ev1, ctx->raster_stream));
  st.active = true;
  return FLAME_NLTGV2_OK;
}

// Device time between the stage's two events, which must have completed; 0 where the runtime cannot tell.
static float stage_ms(const SideStage& st) {
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, st.ev0, st.ev1) != hipSuccess) (void)hipGetLastError(), ms = 0.0f;
  return ms;
}

// The dense inverse-depth map a stage reads: the caller's device map, else the filtered map of mesh_outputs_begin, else the resident map
// of interpolate_mesh -- either of the graph's own must have been made at rows x cols.
static int resident_map(flame_nltgv2_ctx* ctx, const void* map_device, int use_filtered, int rows, int cols, const float** map) {
  *map = (const float*)map_device;
  if (map_device) return FLAME_NLTGV2_OK;
  const bool f = use_filtered != 0;
  if ((f ? ctx->fmap_rows : ctx->map_rows) != rows || (f ? ctx->fmap_cols : ctx->map_cols) != cols) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  *map = (const float*)(f ? ctx->m_img.p : ctx->r_img.p);
  return *map ? FLAME_NLTGV2_OK : fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
}

// What the view renderer and the fusion of views share: a camera, the three kinds of source, the projection's enqueue.
static flame_hip::ViewCamera view_camera(const float* Kinv_src, const float* K_dst, const float* R, const float* t, float near_depth) {
  flame_hip::ViewCamera cam;
  std::memcpy(cam.Kinv_src, Kinv_src, sizeof(cam.Kinv_src));
  std::memcpy(cam.K_dst, K_dst, sizeof(cam.K_dst));
  std::memcpy(cam.R, R, sizeof(cam.R));
  std::memcpy(cam.t, t, sizeof(cam.t));
  cam.near_depth = near_depth;
  return cam;
}
static flame_hip::FuseSource mesh_source(const void* pos, const void* values, float value_scale, const void* tris, const void* tri_valid) {
  flame_hip::FuseSource o{};  // (the camera, and weight / v0 / t0 where there is a batch: the caller's)
  o.pos = (const float2*)pos, o.values = (const float*)values, o.value_scale = value_scale;
  o.tris = (const int32_t*)tris, o.tri_valid = (const uint8_t*)tri_valid;
  return o;
}
// The graph's live mesh: the resident triangles over the canonical pos / x * graph_scale; validity 2: the filters' validity.
static flame_hip::FuseSource live_source(const flame_nltgv2_ctx* ctx, int validity, float graph_scale) {
  return mesh_source(ctx->c.pos, ctx->c.x, graph_scale, ctx->r_tris.p, validity == 2 ? ctx->m_tvalid.p : nullptr);
}
static flame_hip::FuseSource kept_source(const flame_nltgv2_ctx::KeptMesh& k) {
  return mesh_source(k.pos.p, k.id.p, 1.0f, k.tris.p, k.has_valid ? k.valid.p : nullptr);  // (id * 1.0f == id: what the snapshot stored)
}
static flame_hip::FuseSource arrays_source(const flame_nltgv2_ctx* ctx) {  // what render_view_arrays puts into the view stage's own buffers
  return mesh_source(ctx->v_apos.p, ctx->v_aid.p, 1.0f, ctx->v_atris.p, nullptr);
}

// Rules 1 - 5 of a stage on the side stream, from its ev0 on: vertices(), clear() and raster() launch the stage's kernels.  live: a
// source is the graph's mesh, whose canonical pos / x the vertex kernel reads, and nothing after it.
template <class Vertices, class Clear, class Raster>
static int enqueue_projection(flame_nltgv2_ctx* ctx, SideStage& st, bool live, Vertices vertices, Clear clear, Raster raster) {
  hipStream_t rs = ctx->raster_stream;
  int rc = live ? mesh_state_on(ctx, rs) : FLAME_NLTGV2_OK;
  if (rc) return rc;
  HIPCHK(ctx, hipEventRecord(st.ev0, rs));
  LAUNCHCHK(ctx, vertices());
  rc = live ? side_kernels_read_last(ctx) : FLAME_NLTGV2_OK;
  if (rc) return rc;
  LAUNCHCHK(ctx, clear());
  LAUNCHCHK(ctx, raster());
  return FLAME_NLTGV2_OK;
}

// The grey image a stage draws over.  A host image goes through pinned memory (`staging`, rows packed) into `d`, so the caller's buffer
// is free again when this returns; a device image is read where it lies.
static int stage_gray(flame_nltgv2_ctx* ctx, const uint8_t* img_host, const void* img_device, int step_bytes, int rows, int cols,
                      char* staging, DevBuf& d, const uint8_t** gray, int* gray_step) {
  *gray = (const uint8_t*)img_device, *gray_step = step_bytes;
  if (!img_host) return FLAME_NLTGV2_OK;
  for (int r = 0; r < rows; ++r) std::memcpy(staging + (size_t)r * cols, img_host + (size_t)r * step_bytes, (size_t)cols);
  HIPCHK(ctx, hipMemcpyAsync(d.p, staging, (size_t)rows * (size_t)cols, hipMemcpyHostToDevice, ctx->raster_stream));
  *gray = (const uint8_t*)d.p, *gray_step = cols;
  return FLAME_NLTGV2_OK;
}

static flame_hip::WireBuffers wire_buffers(const flame_nltgv2_ctx* ctx) {
  flame_hip::WireBuffers wb;
  wb.draws = (flame_hip::WireDraw*)ctx->w_draws.p, wb.cnt = (uint32_t*)ctx->w_cnt.p, wb.offset = (uint32_t*)ctx->w_off.p;
  wb.fill = (uint32_t*)ctx->w_fill.p, wb.entries = (uint64_t*)ctx->w_entries.p, wb.capacity = (uint32_t)ctx->w_cap;
  wb.counts = (int*)ctx->w_counts.p;
  return wb;
}
static_assert(flame_hip::kWireCounts * sizeof(int) <= kWireCountBytes, "wire_layout reserves too little for the counters");
static_assert(sizeof(flame_hip::MapErrorStats) == sizeof(flame_nltgv2_map_error_stats) && sizeof(flame_nltgv2_map_error_stats) == kMapErrorStatsBytes,
              "the statistics on the device, in the header and in map_error_layout are one struct");
static_assert(sizeof(flame_hip::ViewCounts) == sizeof(flame_nltgv2_view_counts) && sizeof(flame_nltgv2_view_counts) == kViewCountBytes,
              "the counters on the device, in the header and in view_layout are one struct");
static_assert(sizeof(flame_hip::FuseCounts) == sizeof(flame_nltgv2_fuse_counts) && sizeof(flame_nltgv2_fuse_counts) == kFuseCountBytes,
              "the counters on the device, in the header and in fuse_layout are one struct");
static_assert(sizeof(flame_hip::IntegrateCounts) == sizeof(flame_nltgv2_integrate_counts) && sizeof(flame_nltgv2_integrate_counts) == kIntegrateCountBytes,
              "the counters on the device, in the header and in integrate_layout are one struct");
static_assert(sizeof(flame_hip::RaycastCounts) == sizeof(flame_nltgv2_raycast_counts) && sizeof(flame_nltgv2_raycast_counts) == kRaycastCountBytes,
              "the counters on the device, in the header and in raycast_layout are one struct");
static_assert(sizeof(flame_hip::ShiftCounts) == sizeof(flame_nltgv2_shift_counts) && sizeof(flame_nltgv2_shift_counts) == kShiftCountBytes,
              "the counters on the device, in the header and in side_stage.hpp are one struct");
static_assert(sizeof(WindowPlan) == sizeof(flame_nltgv2_follow_plan) && offsetof(WindowPlan, leaving_hi) == offsetof(flame_nltgv2_follow_plan, leaving_hi),
              "the plan in side_stage.hpp and in the header are one struct");
static_assert(flame_hip::kVolumeCountsBytes == kCountSetsBytes && flame_hip::kVolumeCountSlots == kCountSets &&
              flame_hip::kVolumeCountSlotWords == kCountSetWords, "the kernels' and the layouts' partial sets of counters");
static_assert(sizeof(flame_nltgv2_volume_mesh_counts) == kMeshCountBytes && sizeof(flame_hip::MeshTotals) == kMeshTotalsBytes,
              "the counters in the header and the scan's totals on the device and in volume_mesh_layout");
static_assert(flame_hip::kMeshPasses == 4 && sizeof(((flame_nltgv2_volume_mesh_view*)nullptr)->pass_ms) == 4 * sizeof(float), "one time per pass");
static_assert(flame_hip::kFuseSources == FLAME_NLTGV2_FUSE_SOURCES, "the kernels' and the header's number of sources");

extern "C" {

// Shared tail of the two interpolate_mesh entry points: triangles/validity -> device, rasterise, copy back.
static int interpolate_common(flame_nltgv2_ctx* ctx, const int32_t* triangles, int32_t T, int32_t V, bool foreign,
                              const uint8_t* vtx_valid, const uint8_t* tri_valid, const float2* d_vtx,
                              const float* d_val, float value_scale, int rows, int cols, float* out, int32_t* coverage) {
  if (T < 0 || rows <= 0 || cols <= 0 || !out || (T > 0 && !triangles)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (!triangles_in_range(triangles, T, V)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const size_t n = (size_t)rows * (size_t)cols;
  int rc = ensure(ctx, ctx->r_tris, sizeof(int32_t) * 3 * (size_t)T);
  if (!rc) rc = ensure(ctx, ctx->r_valid, (size_t)T + (size_t)V + 16);
  if (!rc) rc = ensure(ctx, ctx->r_keys, sizeof(unsigned long long) * n);
  if (!rc) rc = ensure(ctx, ctx->r_img, sizeof(float) * n);
  if (!rc) rc = ensure(ctx, ctx->r_cov, sizeof(int));
  if (rc) return rc;
  if (T > 0) HIPCHK(ctx, hipMemcpyAsync(ctx->r_tris.p, triangles, sizeof(int32_t) * 3 * (size_t)T, hipMemcpyHostToDevice, ctx->stream));
  if (foreign) ctx->tris.uploaded_foreign(tri_valid || vtx_valid);
  else ctx->tris.uploaded(T, ctx->topo, tri_valid || vtx_valid);
  uint8_t* d_tv = nullptr;
  uint8_t* d_vv = nullptr;
  if (tri_valid && T > 0) {
    d_tv = (uint8_t*)ctx->r_valid.p;
    HIPCHK(ctx, hipMemcpyAsync(d_tv, tri_valid, (size_t)T, hipMemcpyHostToDevice, ctx->stream));
  }
  if (vtx_valid && V > 0) {
    d_vv = (uint8_t*)ctx->r_valid.p + (size_t)T;
    HIPCHK(ctx, hipMemcpyAsync(d_vv, vtx_valid, (size_t)V, hipMemcpyHostToDevice, ctx->stream));
  }
  LAUNCHCHK(ctx, launch_interpolate_mesh(T, (const int32_t*)ctx->r_tris.p, d_vtx, d_val, value_scale, d_vv, d_tv,
                                         (unsigned long long*)ctx->r_keys.p, (float*)ctx->r_img.p, (int*)ctx->r_cov.p,
                                         rows, cols, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(out, ctx->r_img.p, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
  int cov = 0;
  HIPCHK(ctx, hipMemcpyAsync(&cov, ctx->r_cov.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, wait_solver_stream(ctx));
  if (coverage) *coverage = cov;
  return FLAME_NLTGV2_OK;
}

// interpolate_mesh on the side stream (see flame_nltgv2.h): the canonical pos / x are read there while the solver already runs again
// on its packed state; the next unpack waits for ev_raster_done (ensure_canon), so do the kernels of a prepared sync that reuse them.
int flame_nltgv2_interpolate_mesh_begin(flame_nltgv2_ctx* ctx, const int32_t* triangles, int32_t T, const uint8_t* tri_valid,
                                        int rows, int cols, float graph_scale) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_interpolate_mesh_begin");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_graph) return fail(ctx, FLAME_NLTGV2_ERR_NO_GRAPH);
  const int32_t V = ctx->L.V;
  if (T < 0 || rows <= 0 || cols <= 0 || (T > 0 && !triangles)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (!triangles_in_range(triangles, T, V)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const size_t n = (size_t)rows * (size_t)cols;
  hipStream_t rs = ctx->raster_stream;
  const bool trace = std::getenv("FLAME_NLTGV2_TRACE") != nullptr;
  const auto tr0 = std::chrono::steady_clock::now();
  auto tr_us = [&]() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tr0).count(); };
  double tr_a = 0, tr_b = 0, tr_c = 0, tr_d = 0;
  bool replaced = false;
  rc = open_stage(ctx, ctx->h_img, sizeof(float) * (n + 16), &replaced);  // pinned: the map | the coverage count
  if (replaced) ctx->img_pending_rows = ctx->img_pending_cols = 0;
  if (rc) return rc;
  // the caller's triangles go up first (pageable memory: the copy holds the host), while the solver still runs ...
  rc = ensure(ctx, ctx->r_tris, sizeof(int32_t) * 3 * (size_t)T);
  if (!rc) rc = ensure(ctx, ctx->r_tvalid, (size_t)T + 16);  // (its own buffer: project_graph writes r_valid on the context's stream)
  if (!rc) rc = ensure(ctx, ctx->r_keys, sizeof(unsigned long long) * n);
  if (!rc) rc = ensure(ctx, ctx->r_img, sizeof(float) * n);
  if (!rc) rc = ensure(ctx, ctx->r_cov, sizeof(int));
  if (rc) return rc;
  if (T > 0) HIPCHK(ctx, hipMemcpyAsync(ctx->r_tris.p, triangles, sizeof(int32_t) * 3 * (size_t)T, hipMemcpyHostToDevice, rs));
  ctx->tris.uploaded(T, ctx->topo, tri_valid != nullptr);  // (what mesh_outputs_begin(triangles = NULL) and the debug stages refer to)
  uint8_t* d_tv = nullptr;
  if (tri_valid && T > 0) {
    d_tv = (uint8_t*)ctx->r_tvalid.p;
    HIPCHK(ctx, hipMemcpyAsync(d_tv, tri_valid, (size_t)T, hipMemcpyHostToDevice, rs));
  }
  tr_a = tr_us();
  rc = mesh_state_on(ctx, rs);  // ... it stops here, and may go on as soon as the caller enqueues the next run
  if (rc) return rc;
  tr_b = tr_us();
  LAUNCHCHK(ctx, launch_interpolate_mesh(T, (const int32_t*)ctx->r_tris.p, ctx->c.pos, ctx->c.x, graph_scale, nullptr, d_tv,
                                         (unsigned long long*)ctx->r_keys.p, (float*)ctx->r_img.p, (int*)ctx->r_cov.p, rows, cols, rs));
  tr_c = tr_us();
  rc = side_kernels_read_last(ctx);
  if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->h_img.p, ctx->r_img.p, sizeof(float) * n, hipMemcpyDeviceToHost, rs));
  HIPCHK(ctx, hipMemcpyAsync(ctx->h_img.p + sizeof(float) * n, ctx->r_cov.p, sizeof(int), hipMemcpyDeviceToHost, rs));
  ctx->map_rows = rows, ctx->map_cols = cols;
  ctx->img_pending_rows = rows, ctx->img_pending_cols = cols;  // (what _end describes: a synchronous interpolate_mesh in between changes map_rows)
  tr_d = tr_us();
  if (trace)
    std::fprintf(stderr, "[flame_nltgv2] interpolate_mesh_begin: checks + triangles up %.1f us, solver settled + unpack enqueued %.1f, rasteriser enqueued %.1f, copies out enqueued %.1f\n",
                 tr_a, tr_b - tr_a, tr_c - tr_b, tr_d - tr_c);
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_interpolate_mesh_end(flame_nltgv2_ctx* ctx, const float** map_out, int32_t* coverage_out) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_interpolate_mesh_end");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->h_img.p || ctx->img_pending_rows == 0) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  HIPCHK(ctx, hipStreamSynchronize(ctx->raster_stream));
  const size_t n = (size_t)ctx->img_pending_rows * (size_t)ctx->img_pending_cols;
  if (map_out) *map_out = (const float*)ctx->h_img.p;
  if (coverage_out) std::memcpy(coverage_out, ctx->h_img.p + sizeof(float) * n, sizeof(int32_t));
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_interpolate_mesh(flame_nltgv2_ctx* ctx, const int32_t* triangles, int32_t T, const uint8_t* tri_valid,
                                  int rows, int cols, float graph_scale, float* idepthmap_out, int32_t* coverage_out) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_interpolate_mesh");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_graph) return fail(ctx, FLAME_NLTGV2_ERR_NO_GRAPH);
  rc = ensure_canon(ctx);
  if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->raster_stream));  // (r_img may still be on its way out for an interpolate_mesh_begin)
  rc = interpolate_common(ctx, triangles, T, ctx->L.V, false, nullptr, tri_valid, ctx->c.pos, ctx->c.x, graph_scale, rows,
                          cols, idepthmap_out, coverage_out);
  if (!rc) ctx->map_rows = rows, ctx->map_cols = cols;  // (the map stays on the device: flame_nltgv2_sync_input.init_from_map)
  else ctx->tris.none_resident();
  return rc;
}

int flame_nltgv2_interpolate_mesh_arrays(flame_nltgv2_ctx* ctx, const int32_t* triangles, int32_t T, const float* vertices_xy,
                                         const float* values, int32_t V, const uint8_t* vtx_valid,
                                         const uint8_t* tri_valid, int rows, int cols, float* img_out,
                                         int32_t* coverage_out) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_interpolate_mesh_arrays");
  int rc = enter(ctx);
  if (rc) return rc;
  if (V < 0 || (V > 0 && (!vertices_xy || !values))) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  rc = ensure(ctx, ctx->r_vtx, sizeof(float) * 2 * (size_t)V);
  if (!rc) rc = ensure(ctx, ctx->r_val, sizeof(float) * (size_t)V);
  if (rc) return rc;
  if (V > 0) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->r_vtx.p, vertices_xy, sizeof(float) * 2 * (size_t)V, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->r_val.p, values, sizeof(float) * (size_t)V, hipMemcpyHostToDevice, ctx->stream));
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->raster_stream));
  ctx->map_rows = ctx->map_cols = 0;  // (r_img will hold an image of the caller's arrays, not the graph's map)
  ctx->tris.none_resident();          // (... and r_tris triangles of those arrays)
  return interpolate_common(ctx, triangles, T, V, true, vtx_valid, tri_valid, (const float2*)ctx->r_vtx.p,
                            (const float*)ctx->r_val.p, 1.0f, rows, cols, img_out, coverage_out);
}

void flame_nltgv2_default_mesh_filter_params(flame_nltgv2_mesh_filter_params* p) {
  if (!p) return;
  // params.h:69-85
  p->do_oblique_triangle_filter = 1;
  p->oblique_normal_thresh = 1.39626f;
  p->oblique_idepth_diff_factor = 0.35f;
  p->oblique_idepth_diff_abs = 0.1f;
  p->do_edge_length_filter = 1;
  p->edge_length_thresh = 0.333f;
  p->do_idepth_triangle_filter = 1;
  p->min_triangle_idepth = 0.01f;
}

// Floats in their numeric order as integers: ord(a) < ord(b) <=> a < b (no NaNs; -0 just below +0).
static int64_t float_ord(float f) {
  uint32_t u;
  std::memcpy(&u, &f, sizeof(u));
  return (u & 0x80000000u) ? -(int64_t)(u & 0x7fffffffu) - 1 : (int64_t)u;
}
static float ord_float(int64_t o) {
  const uint32_t u = o < 0 ? (uint32_t)(-(o + 1)) | 0x80000000u : (uint32_t)o;
  float f;
  std::memcpy(&f, &u, sizeof(f));
  return f;
}

float flame_nltgv2_oblique_cos_bound(float thresh) {
  // accepted(d) := (float)acos((double)d) <= thresh is monotone in d (the arc cosine falls): find the smallest accepted float of [-1, 1]
  auto accepted = [thresh](float d) { return (float)std::acos((double)d) <= thresh; };
  if (!(thresh == thresh)) return -1.0f;  // a NaN threshold: `angle > thresh` is never true
  if (accepted(-1.0f)) return -1.0f;      // thresh >= pi
  if (!accepted(1.0f)) return HUGE_VALF;  // thresh < 0
  int64_t lo = float_ord(-1.0f), hi = float_ord(1.0f);  // accepted(hi), !accepted(lo)
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (accepted(ord_float(mid))) hi = mid; else lo = mid;
  }
  return ord_float(hi);
}

// The mesh outputs on the side stream (see flame_nltgv2.h).
int flame_nltgv2_mesh_outputs_begin(flame_nltgv2_ctx* ctx, const int32_t* triangles, int32_t T, const float* Kinv,
                                    const flame_nltgv2_mesh_filter_params* filter, int rows, int cols, float graph_scale,
                                    int want_filtered_map) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_mesh_outputs_begin");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_graph) return fail(ctx, FLAME_NLTGV2_ERR_NO_GRAPH);
  const int32_t V = ctx->L.V;
  if (T < 0 || rows <= 0 || cols <= 0 || !Kinv || !filter) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (!triangles && !ctx->tris.matches(T, ctx->topo)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (triangles && !triangles_in_range(triangles, T, V)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const size_t n = want_filtered_map ? (size_t)rows * (size_t)cols : 0;
  hipStream_t rs = ctx->raster_stream;
  flame_nltgv2_ctx::MeshPending mp;
  mp.V = V, mp.T = T, mp.rows = want_filtered_map ? rows : 0, mp.cols = want_filtered_map ? cols : 0;
  mp.at = mesh_layout(V, T, rows, cols, want_filtered_map != 0);
  rc = open_stage(ctx, ctx->mesh, mp.at.total);
  if (rc) return rc;
  const size_t fV = sizeof(float) * (size_t)V;
  rc = ensure(ctx, ctx->m_P, 4 * fV);
  if (!rc) rc = ensure(ctx, ctx->m_idepth, fV);
  if (!rc) rc = ensure(ctx, ctx->m_normals, 3 * fV);
  if (!rc) rc = ensure(ctx, ctx->m_tvalid, (size_t)T + 16);
  if (!rc) rc = ensure(ctx, ctx->m_nvalid, sizeof(int));
  if (!rc) rc = ensure(ctx, ctx->m_tnormal, sizeof(float4) * (size_t)T);
  if (!rc) rc = ensure(ctx, ctx->m_offset, sizeof(int) * ((size_t)V + 1));
  if (!rc) rc = ensure(ctx, ctx->m_cursor, sizeof(int) * (size_t)V);
  if (!rc) rc = ensure(ctx, ctx->m_incident, sizeof(int32_t) * 3 * (size_t)T);
  if (!rc && triangles) rc = ensure(ctx, ctx->r_tris, sizeof(int32_t) * 3 * (size_t)T);
  if (!rc && want_filtered_map) {
    ctx->fmap_rows = ctx->fmap_cols = 0;  // (m_img is about to be rewritten: flame_nltgv2_metric_outputs_begin, use_filtered_map)
    rc = ensure(ctx, ctx->m_keys, sizeof(unsigned long long) * n);
    if (!rc) rc = ensure(ctx, ctx->m_img, sizeof(float) * n);
    if (!rc) rc = ensure(ctx, ctx->m_cov, sizeof(int));
  }
  if (rc) return rc;
  ctx->mesh.active = false;  // (from here on the pinned outputs are being rewritten)
  if (triangles) {
    if (T > 0) HIPCHK(ctx, hipMemcpyAsync(ctx->r_tris.p, triangles, sizeof(int32_t) * 3 * (size_t)T, hipMemcpyHostToDevice, rs));
    ctx->tris.uploaded_unrasterised(T, ctx->topo);  // (r_keys no longer speaks of r_tris)
  }
  flame_hip::MeshFilter mf;
  std::memcpy(mf.Kinv, Kinv, sizeof(mf.Kinv));
  mf.do_oblique = filter->do_oblique_triangle_filter != 0;
  mf.do_edge_length = filter->do_edge_length_filter != 0;
  mf.do_idepth = filter->do_idepth_triangle_filter != 0;
  mf.cos_bound = flame_nltgv2_oblique_cos_bound(filter->oblique_normal_thresh);
  mf.diff_factor = filter->oblique_idepth_diff_factor, mf.diff_abs = filter->oblique_idepth_diff_abs;
  float dist_thresh2 = filter->edge_length_thresh * (float)cols;  // flame.cc:2297-2298
  dist_thresh2 *= dist_thresh2;
  mf.edge_thresh2 = dist_thresh2;
  mf.min_idepth = filter->min_triangle_idepth;
  flame_hip::MeshBuffers mb;
  mb.P = (float4*)ctx->m_P.p, mb.vtx_idepth = (float*)ctx->m_idepth.p, mb.normals = (float*)ctx->m_normals.p;
  mb.tri_valid = (uint8_t*)ctx->m_tvalid.p, mb.n_valid = (int*)ctx->m_nvalid.p, mb.tri_normal = (float4*)ctx->m_tnormal.p;
  mb.offset = (int*)ctx->m_offset.p, mb.cursor = (int*)ctx->m_cursor.p, mb.incident = (int32_t*)ctx->m_incident.p;
  ctx->tris.validity_written();  // (flame_nltgv2_debug_wireframe_begin, validity == 2)
  rc = mesh_state_on(ctx, rs);
  if (rc) return rc;
  HIPCHK(ctx, hipEventRecord(ctx->mesh.ev0, rs));
  LAUNCHCHK(ctx, flame_hip::launch_mesh_outputs(V, T, ctx->c.pos, ctx->c.x, graph_scale, (const int32_t*)ctx->r_tris.p, mf, mb, rs));
  // the filtered map: the rasteriser of interpolate_mesh over the idepths and the validity this stage has just left on the device
  if (want_filtered_map) {
    LAUNCHCHK(ctx, launch_interpolate_mesh(T, (const int32_t*)ctx->r_tris.p, ctx->c.pos, mb.vtx_idepth, 1.0f, nullptr, mb.tri_valid,
                                           (unsigned long long*)ctx->m_keys.p, (float*)ctx->m_img.p, (int*)ctx->m_cov.p, rows, cols, rs));
    ctx->fmap_rows = rows, ctx->fmap_cols = cols;
  }
  rc = side_kernels_read_last(ctx);  // (of the canonical pos / x)
  if (rc) return rc;
  char* h = ctx->mesh.h.p;
  HIPCHK(ctx, hipMemcpyAsync(h + mp.at.normals, mb.normals, 3 * fV, hipMemcpyDeviceToHost, rs));
  HIPCHK(ctx, hipMemcpyAsync(h + mp.at.idepth, mb.vtx_idepth, fV, hipMemcpyDeviceToHost, rs));
  HIPCHK(ctx, hipMemcpyAsync(h + mp.at.counts, mb.n_valid, sizeof(int), hipMemcpyDeviceToHost, rs));
  if (T > 0) HIPCHK(ctx, hipMemcpyAsync(h + mp.at.valid, mb.tri_valid, (size_t)T, hipMemcpyDeviceToHost, rs));
  if (want_filtered_map) {
    HIPCHK(ctx, hipMemcpyAsync(h + mp.at.map, ctx->m_img.p, sizeof(float) * n, hipMemcpyDeviceToHost, rs));
    HIPCHK(ctx, hipMemcpyAsync(h + mp.at.counts + sizeof(int32_t), ctx->m_cov.p, sizeof(int), hipMemcpyDeviceToHost, rs));
  }
  ctx->mesh_pending = mp;
  return close_stage(ctx, ctx->mesh);
}

int flame_nltgv2_mesh_outputs_end(flame_nltgv2_ctx* ctx, flame_nltgv2_mesh_outputs_view* out) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_mesh_outputs_end");
  int rc = enter(ctx);
  if (rc) return rc;
  const flame_nltgv2_ctx::MeshPending& mp = ctx->mesh_pending;
  if (!out || !ctx->mesh.h.p || !ctx->mesh.active) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  HIPCHK(ctx, hipStreamSynchronize(ctx->raster_stream));
  const char* h = ctx->mesh.h.p;
  int32_t counts[2];
  std::memcpy(counts, h + mp.at.counts, sizeof(counts));
  out->V = mp.V, out->T = mp.T;
  out->tri_valid = (const uint8_t*)(h + mp.at.valid);
  out->normals = (const float*)(h + mp.at.normals);
  out->vtx_idepth = (const float*)(h + mp.at.idepth);
  out->n_valid = counts[0];
  out->rows = mp.rows, out->cols = mp.cols;
  out->filtered_map = mp.rows > 0 ? (const float*)(h + mp.at.map) : nullptr;
  out->filtered_coverage = mp.rows > 0 ? counts[1] : 0;
  out->device_ms = stage_ms(ctx->mesh);
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_mesh_outputs(flame_nltgv2_ctx* ctx, const int32_t* triangles, int32_t T, const float* Kinv,
                              const flame_nltgv2_mesh_filter_params* filter, int rows, int cols, float graph_scale,
                              uint8_t* tri_valid_out, float* normals_out, float* vtx_idepth_out, int32_t* n_valid_out,
                              float* filtered_map_out, int32_t* filtered_coverage_out) {
  int rc = flame_nltgv2_mesh_outputs_begin(ctx, triangles, T, Kinv, filter, rows, cols, graph_scale,
                                           filtered_map_out != nullptr || filtered_coverage_out != nullptr);
  if (rc) return rc;
  flame_nltgv2_mesh_outputs_view v;
  rc = flame_nltgv2_mesh_outputs_end(ctx, &v);
  if (rc) return rc;
  if (tri_valid_out && v.T > 0) std::memcpy(tri_valid_out, v.tri_valid, (size_t)v.T);
  if (normals_out) std::memcpy(normals_out, v.normals, sizeof(float) * 3 * (size_t)v.V);
  if (vtx_idepth_out) std::memcpy(vtx_idepth_out, v.vtx_idepth, sizeof(float) * (size_t)v.V);
  if (n_valid_out) *n_valid_out = v.n_valid;
  if (filtered_map_out) std::memcpy(filtered_map_out, v.filtered_map, sizeof(float) * (size_t)v.rows * (size_t)v.cols);
  if (filtered_coverage_out) *filtered_coverage_out = v.filtered_coverage;
  return FLAME_NLTGV2_OK;
}

void flame_nltgv2_default_metric_params(flame_nltgv2_metric_params* p) {
  if (!p) return;
  p->min_depth = 0.0f, p->max_depth = HUGE_VALF;
  p->use_filtered_map = 0;
  p->want_depth = p->want_depth_mm = p->want_organized = p->want_cloud = 1;
  p->want_mesh = 0;
  p->copy_out = 1;
  p->reserved = 0;
  p->map_device = nullptr;
}

// The metric outputs on the side stream (see flame_nltgv2.h).  The stage reads what the other stages left on the device, in the
// order of that stream, and nothing of the canonical arrays: no mesh_state_on, no side_kernels_read_last.
int flame_nltgv2_metric_outputs_begin(flame_nltgv2_ctx* ctx, const float* Kinv, const float* T_world_cam,
                                      const flame_nltgv2_metric_params* params, int rows, int cols) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_metric_outputs_begin");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_graph) return fail(ctx, FLAME_NLTGV2_ERR_NO_GRAPH);
  if (!Kinv || !params || rows <= 0 || cols <= 0 || (uint64_t)rows * (uint64_t)cols >= (1ull << 31)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  MetricWants w;
  w.depth = params->want_depth != 0, w.depth_mm = params->want_depth_mm != 0, w.organized = params->want_organized != 0;
  w.cloud = params->want_cloud != 0, w.mesh = params->want_mesh != 0, w.copy_out = params->copy_out != 0;
  const bool want_pixels = w.depth || w.depth_mm || w.organized || w.cloud;
  if (!want_pixels && !w.mesh) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const float* map = nullptr;
  rc = want_pixels ? resident_map(ctx, params->map_device, params->use_filtered_map, rows, cols, &map) : FLAME_NLTGV2_OK;
  if (rc) return rc;
  if (w.mesh && !ctx->tris.validity_current(ctx->topo)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const int32_t V = w.mesh ? ctx->L.V : 0, T = w.mesh ? ctx->tris.T() : 0;
  const size_t n = (size_t)rows * (size_t)cols, f = sizeof(float);
  hipStream_t rs = ctx->raster_stream;
  flame_nltgv2_ctx::MetricPending mp;
  mp.rows = rows, mp.cols = cols, mp.V = V, mp.T = T, mp.want = w;
  mp.at = metric_layout(rows, cols, V, T, w);
  rc = open_stage(ctx, ctx->metric, mp.at.total);
  if (rc) return rc;
  rc = ensure(ctx, ctx->x_counts, 2 * sizeof(int));
  if (!rc && w.depth) rc = ensure(ctx, ctx->x_depth, f * n);
  if (!rc && w.depth_mm) rc = ensure(ctx, ctx->x_mm, sizeof(uint16_t) * n + 16);
  if (!rc && w.organized) rc = ensure(ctx, ctx->x_org, 3 * f * n);
  if (!rc && w.cloud) {
    rc = ensure(ctx, ctx->x_cloud, 3 * f * n);
    if (!rc) rc = ensure(ctx, ctx->x_pix, sizeof(uint32_t) * n);
    if (!rc) rc = ensure(ctx, ctx->x_blocks, sizeof(int) * (size_t)flame_hip::metric_blocks((long)n));
  }
  if (!rc && w.mesh) {
    rc = ensure(ctx, ctx->x_verts, 3 * f * (size_t)V + 16);
    if (!rc) rc = ensure(ctx, ctx->x_norms, 3 * f * (size_t)V + 16);
    if (!rc) rc = ensure(ctx, ctx->x_tris, 3 * sizeof(int32_t) * (size_t)T + 16);
    if (!rc) rc = ensure(ctx, ctx->x_tblocks, sizeof(int) * (size_t)flame_hip::metric_blocks(T) + 16);
  }
  if (rc) return rc;
  ctx->metric.active = false;  // (from here on the pinned outputs are being rewritten)
  flame_hip::MetricArgs a;
  a.rows = rows, a.cols = cols;
  std::memcpy(a.Kinv, Kinv, sizeof(a.Kinv));
  a.has_pose = T_world_cam != nullptr;
  if (T_world_cam) std::memcpy(a.pose, T_world_cam, sizeof(a.pose));
  else std::memset(a.pose, 0, sizeof(a.pose));
  a.min_depth = params->min_depth, a.max_depth = params->max_depth;
  int* counts = (int*)ctx->x_counts.p;
  HIPCHK(ctx, hipEventRecord(ctx->metric.ev0, rs));
  HIPCHK(ctx, hipMemsetAsync(counts, 0, 2 * sizeof(int), rs));
  if (want_pixels) {
    LAUNCHCHK(ctx, flame_hip::launch_metric_pixels(a, map, w.depth ? (float*)ctx->x_depth.p : nullptr, w.depth_mm ? (uint16_t*)ctx->x_mm.p : nullptr,
                                                   w.organized ? (float*)ctx->x_org.p : nullptr, w.cloud ? (int*)ctx->x_blocks.p : nullptr, rs));
    if (w.cloud)
      LAUNCHCHK(ctx, flame_hip::launch_metric_cloud(a, map, (int*)ctx->x_blocks.p, counts, (float*)ctx->x_cloud.p, (uint32_t*)ctx->x_pix.p, rs));
  }
  if (w.mesh) {
    LAUNCHCHK(ctx, flame_hip::launch_metric_vertices(a, V, (const float4*)ctx->m_P.p, (const float*)ctx->m_normals.p, (float*)ctx->x_verts.p,
                                                     (float*)ctx->x_norms.p, rs));
    LAUNCHCHK(ctx, flame_hip::launch_metric_triangles(T, (const int32_t*)ctx->r_tris.p, (const uint8_t*)ctx->m_tvalid.p, (int*)ctx->x_tblocks.p,
                                                      counts + 1, (int32_t*)ctx->x_tris.p, rs));
  }
  char* h = ctx->metric.h.p;
  HIPCHK(ctx, hipMemcpyAsync(h + mp.at.counts, counts, 2 * sizeof(int), hipMemcpyDeviceToHost, rs));
  if (w.copy_out) {  // (the dense cloud: in _end, n_points points of it)
    if (w.depth) HIPCHK(ctx, hipMemcpyAsync(h + mp.at.depth, ctx->x_depth.p, f * n, hipMemcpyDeviceToHost, rs));
    if (w.depth_mm) HIPCHK(ctx, hipMemcpyAsync(h + mp.at.depth_mm, ctx->x_mm.p, sizeof(uint16_t) * n, hipMemcpyDeviceToHost, rs));
    if (w.organized) HIPCHK(ctx, hipMemcpyAsync(h + mp.at.organized, ctx->x_org.p, 3 * f * n, hipMemcpyDeviceToHost, rs));
    if (w.mesh && V > 0) {
      HIPCHK(ctx, hipMemcpyAsync(h + mp.at.vertices, ctx->x_verts.p, 3 * f * (size_t)V, hipMemcpyDeviceToHost, rs));
      HIPCHK(ctx, hipMemcpyAsync(h + mp.at.normals, ctx->x_norms.p, 3 * f * (size_t)V, hipMemcpyDeviceToHost, rs));
    }
    if (w.mesh && T > 0) HIPCHK(ctx, hipMemcpyAsync(h + mp.at.triangles, ctx->x_tris.p, 3 * sizeof(int32_t) * (size_t)T, hipMemcpyDeviceToHost, rs));
  }
  ctx->metric_pending = mp;
  return close_stage(ctx, ctx->metric);
}

int flame_nltgv2_metric_outputs_end(flame_nltgv2_ctx* ctx, flame_nltgv2_metric_outputs_view* out) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_metric_outputs_end");
  int rc = enter(ctx);
  if (rc) return rc;
  flame_nltgv2_ctx::MetricPending& mp = ctx->metric_pending;
  if (!out || !ctx->metric.h.p || !ctx->metric.active) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  hipStream_t rs = ctx->raster_stream;
  HIPCHK(ctx, hipStreamSynchronize(rs));
  char* h = ctx->metric.h.p;
  int32_t counts[2];
  std::memcpy(counts, h + mp.at.counts, sizeof(counts));
  const MetricWants& w = mp.want;
  if (w.cloud && w.copy_out && !mp.cloud_fetched) {
    if (counts[0] > 0) {
      HIPCHK(ctx, hipMemcpyAsync(h + mp.at.cloud, ctx->x_cloud.p, 3 * sizeof(float) * (size_t)counts[0], hipMemcpyDeviceToHost, rs));
      HIPCHK(ctx, hipMemcpyAsync(h + mp.at.cloud_pixel, ctx->x_pix.p, sizeof(uint32_t) * (size_t)counts[0], hipMemcpyDeviceToHost, rs));
      HIPCHK(ctx, hipStreamSynchronize(rs));
    }
    mp.cloud_fetched = true;
  }
  const bool host = w.copy_out;
  out->rows = mp.rows, out->cols = mp.cols, out->V = mp.V, out->T = mp.T;
  out->n_points = counts[0], out->n_valid = counts[1];
  out->depth = host && w.depth ? (const float*)(h + mp.at.depth) : nullptr;
  out->depth_device = w.depth ? ctx->x_depth.p : nullptr;
  out->depth_mm = host && w.depth_mm ? (const uint16_t*)(h + mp.at.depth_mm) : nullptr;
  out->depth_mm_device = w.depth_mm ? ctx->x_mm.p : nullptr;
  out->organized = host && w.organized ? (const float*)(h + mp.at.organized) : nullptr;
  out->organized_device = w.organized ? ctx->x_org.p : nullptr;
  out->cloud = host && w.cloud ? (const float*)(h + mp.at.cloud) : nullptr;
  out->cloud_device = w.cloud ? ctx->x_cloud.p : nullptr;
  out->cloud_pixel = host && w.cloud ? (const uint32_t*)(h + mp.at.cloud_pixel) : nullptr;
  out->cloud_pixel_device = w.cloud ? ctx->x_pix.p : nullptr;
  out->mesh_vertices = host && w.mesh ? (const float*)(h + mp.at.vertices) : nullptr;
  out->mesh_vertices_device = w.mesh ? ctx->x_verts.p : nullptr;
  out->mesh_normals = host && w.mesh ? (const float*)(h + mp.at.normals) : nullptr;
  out->mesh_normals_device = w.mesh ? ctx->x_norms.p : nullptr;
  out->mesh_triangles = host && w.mesh ? (const int32_t*)(h + mp.at.triangles) : nullptr;
  out->mesh_triangles_device = w.mesh ? ctx->x_tris.p : nullptr;
  out->device_ms = stage_ms(ctx->metric);
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_metric_outputs(flame_nltgv2_ctx* ctx, const float* Kinv, const float* T_world_cam,
                                const flame_nltgv2_metric_params* params, int rows, int cols, float* depth_out, uint16_t* depth_mm_out,
                                float* organized_out, float* cloud_out, uint32_t* cloud_pixel_out, int32_t* n_points_out,
                                float* mesh_vertices_out, float* mesh_normals_out, int32_t* mesh_triangles_out, int32_t* n_valid_out) {
  flame_nltgv2_metric_params p;
  flame_nltgv2_default_metric_params(&p);
  if (params) p = *params;
  p.want_depth = depth_out != nullptr, p.want_depth_mm = depth_mm_out != nullptr, p.want_organized = organized_out != nullptr;
  p.want_cloud = cloud_out != nullptr || cloud_pixel_out != nullptr || n_points_out != nullptr;
  p.want_mesh = mesh_vertices_out != nullptr || mesh_normals_out != nullptr || mesh_triangles_out != nullptr || n_valid_out != nullptr;
  p.copy_out = 1;
  int rc = flame_nltgv2_metric_outputs_begin(ctx, Kinv, T_world_cam, params ? &p : nullptr, rows, cols);
  if (rc) return rc;
  flame_nltgv2_metric_outputs_view v;
  rc = flame_nltgv2_metric_outputs_end(ctx, &v);
  if (rc) return rc;
  const size_t n = (size_t)v.rows * (size_t)v.cols, f = sizeof(float);
  if (depth_out) std::memcpy(depth_out, v.depth, f * n);
  if (depth_mm_out) std::memcpy(depth_mm_out, v.depth_mm, sizeof(uint16_t) * n);
  if (organized_out) std::memcpy(organized_out, v.organized, 3 * f * n);
  if (cloud_out) std::memcpy(cloud_out, v.cloud, 3 * f * (size_t)v.n_points);
  if (cloud_pixel_out) std::memcpy(cloud_pixel_out, v.cloud_pixel, sizeof(uint32_t) * (size_t)v.n_points);
  if (n_points_out) *n_points_out = v.n_points;
  if (mesh_vertices_out) std::memcpy(mesh_vertices_out, v.mesh_vertices, 3 * f * (size_t)v.V);
  if (mesh_normals_out) std::memcpy(mesh_normals_out, v.mesh_normals, 3 * f * (size_t)v.V);
  if (mesh_triangles_out) std::memcpy(mesh_triangles_out, v.mesh_triangles, 3 * sizeof(int32_t) * (size_t)v.n_valid);
  if (n_valid_out) *n_valid_out = v.n_valid;
  return FLAME_NLTGV2_OK;
}

void flame_nltgv2_default_map_error_params(flame_nltgv2_map_error_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->KRKinv[0] = p->KRKinv[4] = p->KRKinv[8] = 1.0f;
  p->source = FLAME_NLTGV2_MAP_ERROR_PHOTO;
  p->border = 3;
  p->relative = 1;
  p->ptile_num = 99, p->ptile_den = 100;
  p->max_error = 32.0f;
  p->want_stats = p->want_error_map = p->copy_out = 1;
}

// The map error on the side stream (see flame_nltgv2.h).  Like the metric outputs it reads what the other stages left on the device, in
// the order of that stream, and nothing of the canonical arrays: no mesh_state_on, no side_kernels_read_last.
int flame_nltgv2_map_error_begin(flame_nltgv2_ctx* ctx, const flame_nltgv2_map_error_params* params, int rows, int cols) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_map_error_begin");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_graph) return fail(ctx, FLAME_NLTGV2_ERR_NO_GRAPH);
  if (!params || rows <= 0 || cols <= 0 || (uint64_t)rows * (uint64_t)cols >= (1ull << 31)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const flame_nltgv2_map_error_params& p = *params;
  const bool photo = p.source == FLAME_NLTGV2_MAP_ERROR_PHOTO;
  if (!photo && p.source != FLAME_NLTGV2_MAP_ERROR_TRUTH) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  MapErrorWants w;
  w.stats = p.want_stats != 0, w.error_map = p.want_error_map != 0, w.image = p.want_image != 0, w.copy_out = p.copy_out != 0;
  w.host_truth = !photo && p.truth_host != nullptr;
  w.host_gray = !photo && w.image && p.gray_host != nullptr;
  if (!w.stats && !w.error_map && !w.image) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const float* map = nullptr;
  rc = resident_map(ctx, p.map_device, p.use_filtered_map, rows, cols, &map);
  if (rc) return rc;
  flame_hip::MapErrorPhoto ph{};
  bool ctx_images = false;
  if (photo) {
    if (p.border < 1) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
    if (p.ref_device || p.cmp_device) {
      if (!p.ref_device || !p.cmp_device || p.image_step_bytes < cols) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
      ph.ref = (const uint8_t*)p.ref_device, ph.cmp = (const uint8_t*)p.cmp_device, ph.step = p.image_step_bytes;
    } else {
      if (ctx->img_rows != rows || ctx->img_cols != cols || !ctx->img_ref.p) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
      ph.ref = (const uint8_t*)ctx->img_ref.p, ph.cmp = (const uint8_t*)ctx->img_cmp.p, ph.step = ctx->img_step;
      ctx_images = true;
    }
    std::memcpy(ph.geo.KRKinv, p.KRKinv, sizeof(ph.geo.KRKinv));
    std::memcpy(ph.geo.Kt, p.Kt, sizeof(ph.geo.Kt));
    ph.border = p.border;
  } else {
    if ((p.truth_host != nullptr) == (p.truth_device != nullptr)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  }
  const int win = map_error_window(p.win_size, cols, flame_hip::kMapErrorMaxWin);
  if (win == 0) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  float hist_scale = p.hist_scale;
  if (hist_scale == 0.0f) hist_scale = photo ? 1.0f : 1000.0f;
  if (!(hist_scale > 0.0f) || !(hist_scale <= 3.402823466e+38f)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (p.ptile_den <= 0 || p.ptile_num < 0 || p.ptile_num > p.ptile_den) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (w.image) {
    if (!(p.max_error > 0.0f)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
    if (!photo && ((p.gray_host != nullptr) == (p.gray_device != nullptr) || p.gray_step_bytes < cols)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  }
  const size_t n = (size_t)rows * (size_t)cols, f = sizeof(float);
  hipStream_t rs = ctx->raster_stream;
  flame_nltgv2_ctx::MapErrorPending mp;
  mp.rows = rows, mp.cols = cols, mp.source = p.source, mp.win_size = win, mp.hist_scale = hist_scale, mp.want = w;
  mp.at = map_error_layout(rows, cols, w);
  rc = open_stage(ctx, ctx->merr, mp.at.total);
  if (rc) return rc;
  rc = ensure(ctx, ctx->e_err, f * n);
  if (!rc && win > 1) rc = ensure(ctx, ctx->e_smooth, f * n);
  if (!rc && w.stats) rc = ensure(ctx, ctx->e_stats, sizeof(flame_hip::MapErrorStats));
  if (!rc && w.stats) rc = ensure(ctx, ctx->e_partials, sizeof(double) * (size_t)flame_hip::map_error_chunks((long)n));
  if (!rc && w.image) rc = ensure(ctx, ctx->e_img, 3 * n + 16);
  if (!rc && w.host_truth) rc = ensure(ctx, ctx->e_truth, f * n);
  if (!rc && w.host_gray) rc = ensure(ctx, ctx->e_gray, n + 16);
  if (rc) return rc;
  ctx->merr.active = false;  // (from here on the pinned outputs are being rewritten)
  char* h = ctx->merr.h.p;
  const float* truth = (const float*)p.truth_device;
  if (w.host_truth) {  // through pinned memory: the caller's array is free when this returns
    std::memcpy(h + mp.at.truth, p.truth_host, f * n);
    HIPCHK(ctx, hipMemcpyAsync(ctx->e_truth.p, h + mp.at.truth, f * n, hipMemcpyHostToDevice, rs));
    truth = (const float*)ctx->e_truth.p;
  }
  const uint8_t* gray = ph.ref;
  int gray_step = ph.step;
  if (!photo && w.image) {
    rc = stage_gray(ctx, p.gray_host, p.gray_device, p.gray_step_bytes, rows, cols, h + mp.at.gray, ctx->e_gray, &gray, &gray_step);
    if (rc) return rc;
  }
  HIPCHK(ctx, hipEventRecord(ctx->merr.ev0, rs));
  float* err = (float*)ctx->e_err.p;
  if (photo) LAUNCHCHK(ctx, flame_hip::launch_map_error_photo(rows, cols, ph, map, err, rs));
  else LAUNCHCHK(ctx, flame_hip::launch_map_error_truth(rows, cols, map, truth, p.relative != 0, err, rs));
  ctx->merr_reads_images = ctx_images;
  if (win > 1) {
    LAUNCHCHK(ctx, flame_hip::launch_map_error_box(rows, cols, win, err, (float*)ctx->e_smooth.p, rs));
    err = (float*)ctx->e_smooth.p;
  }
  if (w.stats)
    LAUNCHCHK(ctx, flame_hip::launch_map_error_stats((long)n, err, hist_scale, p.ptile_num, p.ptile_den, (double*)ctx->e_partials.p,
                                                     (flame_hip::MapErrorStats*)ctx->e_stats.p, rs));
  if (w.image) LAUNCHCHK(ctx, flame_hip::launch_map_error_picture(rows, cols, gray, gray_step, err, p.max_error, p.flip != 0, (uint8_t*)ctx->e_img.p, rs));
  if (w.stats) HIPCHK(ctx, hipMemcpyAsync(h + mp.at.stats, ctx->e_stats.p, sizeof(flame_hip::MapErrorStats), hipMemcpyDeviceToHost, rs));
  if (w.copy_out) {
    if (w.error_map) HIPCHK(ctx, hipMemcpyAsync(h + mp.at.error_map, err, f * n, hipMemcpyDeviceToHost, rs));
    if (w.image) HIPCHK(ctx, hipMemcpyAsync(h + mp.at.image, ctx->e_img.p, 3 * n, hipMemcpyDeviceToHost, rs));
  }
  mp.err_device = err;
  ctx->merr_pending = mp;
  return close_stage(ctx, ctx->merr);
}

int flame_nltgv2_map_error_end(flame_nltgv2_ctx* ctx, flame_nltgv2_map_error_view* out) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_map_error_end");
  int rc = enter(ctx);
  if (rc) return rc;
  const flame_nltgv2_ctx::MapErrorPending& mp = ctx->merr_pending;
  if (!out || !ctx->merr.h.p || !ctx->merr.active) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  HIPCHK(ctx, hipStreamSynchronize(ctx->raster_stream));
  ctx->merr_reads_images = false;
  const char* h = ctx->merr.h.p;
  const MapErrorWants& w = mp.want;
  out->rows = mp.rows, out->cols = mp.cols, out->source = mp.source, out->win_size = mp.win_size;
  out->hist_scale = mp.hist_scale;
  out->device_ms = stage_ms(ctx->merr);
  out->stats = w.stats ? (const flame_nltgv2_map_error_stats*)(h + mp.at.stats) : nullptr;
  out->stats_device = w.stats ? ctx->e_stats.p : nullptr;
  out->error_map = w.copy_out && w.error_map ? (const float*)(h + mp.at.error_map) : nullptr;
  out->error_map_device = w.error_map ? mp.err_device : nullptr;
  out->image = w.copy_out && w.image ? (const uint8_t*)(h + mp.at.image) : nullptr;
  out->image_device = w.image ? ctx->e_img.p : nullptr;
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_map_error(flame_nltgv2_ctx* ctx, const flame_nltgv2_map_error_params* params, int rows, int cols, float* error_map_out,
                           uint8_t* image_out, flame_nltgv2_map_error_stats* stats_out) {
  flame_nltgv2_map_error_params p;
  flame_nltgv2_default_map_error_params(&p);
  if (params) p = *params;
  p.want_error_map = error_map_out != nullptr, p.want_image = image_out != nullptr, p.want_stats = stats_out != nullptr;
  p.copy_out = 1;
  int rc = flame_nltgv2_map_error_begin(ctx, params ? &p : nullptr, rows, cols);
  if (rc) return rc;
  flame_nltgv2_map_error_view v;
  rc = flame_nltgv2_map_error_end(ctx, &v);
  if (rc) return rc;
  const size_t n = (size_t)v.rows * (size_t)v.cols;
  if (error_map_out) std::memcpy(error_map_out, v.error_map, sizeof(float) * n);
  if (image_out) std::memcpy(image_out, v.image, 3 * n);
  if (stats_out) *stats_out = *v.stats;
  return FLAME_NLTGV2_OK;
}

void flame_nltgv2_default_view_params(flame_nltgv2_view_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->Kinv_src[0] = p->Kinv_src[4] = p->Kinv_src[8] = 1.0f;
  p->K_dst[0] = p->K_dst[4] = p->K_dst[8] = 1.0f;
  p->R[0] = p->R[4] = p->R[8] = 1.0f;
  p->want_map = p->want_tri_index = p->copy_out = 1;
}

// The three host arrays of the _arrays form, which go up into buffers of the stage.
struct ViewMesh { const int32_t* host_tris; const float *host_xy, *host_id; };

// What begin and the _arrays form share, behind their argument checks: open_stage, the stage's buffers, everything enqueued on the
// side stream, close_stage.  The mesh of V vertices and T triangles: own's arrays, or (own == NULL) the graph's live mesh at graph_scale
// with p.validity 0 or 2; host_valid: the validity array of validity == 1.
static int view_enqueue(flame_nltgv2_ctx* ctx, const flame_nltgv2_view_params& p, int32_t V, int32_t T, float graph_scale, const uint8_t* host_valid,
                        const ViewMesh* own, int rows, int cols) {
  const size_t n = (size_t)rows * (size_t)cols;
  hipStream_t rs = ctx->raster_stream;
  flame_nltgv2_ctx::ViewPending vp;
  vp.rows = rows, vp.cols = cols, vp.T = T;
  vp.want.map = p.want_map != 0, vp.want.tri_index = p.want_tri_index != 0, vp.want.copy_out = p.copy_out != 0;
  vp.at = view_layout(rows, cols, vp.want);
  int rc = open_stage(ctx, ctx->view, vp.at.total);
  if (rc) return rc;
  rc = ensure(ctx, ctx->v_vtx, sizeof(flame_hip::ViewVertex) * (size_t)V + 16);
  if (!rc) rc = ensure(ctx, ctx->v_keys, sizeof(unsigned long long) * n);
  if (!rc) rc = ensure(ctx, ctx->v_counts, sizeof(flame_hip::ViewCounts));
  if (!rc) rc = ensure(ctx, ctx->v_big, sizeof(int) * (2 * (size_t)T + 2));
  if (!rc && vp.want.map) rc = ensure(ctx, ctx->v_map, sizeof(float) * n);
  if (!rc && vp.want.tri_index) rc = ensure(ctx, ctx->v_tri, sizeof(int32_t) * n);
  if (!rc && host_valid) rc = ensure(ctx, ctx->v_tvalid, (size_t)T + 16);
  if (!rc && own) rc = ensure(ctx, ctx->v_atris, sizeof(int32_t) * 3 * (size_t)T + 16);
  if (!rc && own) rc = ensure(ctx, ctx->v_apos, sizeof(float) * 2 * (size_t)V + 16);
  if (!rc && own) rc = ensure(ctx, ctx->v_aid, sizeof(float) * (size_t)V + 16);
  if (rc) return rc;
  ctx->view.active = false;  // (from here on the pinned outputs are being rewritten)
  flame_hip::FuseSource src = own ? arrays_source(ctx) : live_source(ctx, p.validity, graph_scale);
  src.cam = view_camera(p.Kinv_src, p.K_dst, p.R, p.t, p.near_depth);
  // (pageable memory: each copy holds the host until the bytes have left the caller's array)
  if (host_valid && T > 0) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->v_tvalid.p, host_valid, (size_t)T, hipMemcpyHostToDevice, rs));
    src.tri_valid = (const uint8_t*)ctx->v_tvalid.p;
  }
  if (own && T > 0) HIPCHK(ctx, hipMemcpyAsync(ctx->v_atris.p, own->host_tris, sizeof(int32_t) * 3 * (size_t)T, hipMemcpyHostToDevice, rs));
  if (own && V > 0) {
    HIPCHK(ctx, hipMemcpyAsync(ctx->v_apos.p, own->host_xy, sizeof(float) * 2 * (size_t)V, hipMemcpyHostToDevice, rs));
    HIPCHK(ctx, hipMemcpyAsync(ctx->v_aid.p, own->host_id, sizeof(float) * (size_t)V, hipMemcpyHostToDevice, rs));
  }
  flame_hip::ViewVertex* vtx = (flame_hip::ViewVertex*)ctx->v_vtx.p;
  unsigned long long* keys = (unsigned long long*)ctx->v_keys.p;
  flame_hip::ViewCounts* counts = (flame_hip::ViewCounts*)ctx->v_counts.p;
  int* big = (int*)ctx->v_big.p;
  rc = enqueue_projection(ctx, ctx->view, !own,
                          [&] { return flame_hip::launch_view_vertices(src, V, vtx, rs); },
                          [&] { return flame_hip::launch_view_clear((long)n, keys, counts, big, rs); },
                          [&] { return flame_hip::launch_view_raster(src, T, vtx, keys, counts, big, rows, cols, rs); });
  if (rc) return rc;
  LAUNCHCHK(ctx, flame_hip::launch_view_resolve((long)n, keys, vp.want.map ? (float*)ctx->v_map.p : nullptr,
                                                vp.want.tri_index ? (int32_t*)ctx->v_tri.p : nullptr, counts, rs));
  char* h = ctx->view.h.p;
  HIPCHK(ctx, hipMemcpyAsync(h + vp.at.counts, counts, sizeof(flame_hip::ViewCounts), hipMemcpyDeviceToHost, rs));
  if (vp.want.copy_out) {
    if (vp.want.map) HIPCHK(ctx, hipMemcpyAsync(h + vp.at.map, ctx->v_map.p, sizeof(float) * n, hipMemcpyDeviceToHost, rs));
    if (vp.want.tri_index) HIPCHK(ctx, hipMemcpyAsync(h + vp.at.tri_index, ctx->v_tri.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, rs));
  }
  ctx->view_pending = vp;
  return close_stage(ctx, ctx->view);
}

static bool view_size_ok(int rows, int cols) { return rows >= 1 && cols >= 1 && rows <= 32767 && cols <= 32767; }

// The view renderer on the side stream (see flame_nltgv2.h).
int flame_nltgv2_render_view_begin(flame_nltgv2_ctx* ctx, const flame_nltgv2_view_params* params, const uint8_t* tri_valid, int rows, int cols,
                                   float graph_scale) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_render_view_begin");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_graph) return fail(ctx, FLAME_NLTGV2_ERR_NO_GRAPH);
  if (!params || !view_size_ok(rows, cols)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (!ctx->tris.current(ctx->topo)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (params->validity < 0 || params->validity > 2 || (tri_valid != nullptr) != (params->validity == 1)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (params->validity == 2 && !ctx->tris.validity_current(ctx->topo)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  return view_enqueue(ctx, *params, ctx->L.V, ctx->tris.T(), graph_scale, tri_valid, nullptr, rows, cols);
}

int flame_nltgv2_render_view_end(flame_nltgv2_ctx* ctx, flame_nltgv2_view_outputs_view* out) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_render_view_end");
  int rc = enter(ctx);
  if (rc) return rc;
  const flame_nltgv2_ctx::ViewPending& vp = ctx->view_pending;
  if (!out || !ctx->view.h.p || !ctx->view.active) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  HIPCHK(ctx, hipStreamSynchronize(ctx->raster_stream));
  const char* h = ctx->view.h.p;
  const bool host = vp.want.copy_out;
  out->rows = vp.rows, out->cols = vp.cols, out->T = vp.T;
  std::memcpy(&out->counts, h + vp.at.counts, sizeof(out->counts));
  out->device_ms = stage_ms(ctx->view);
  out->map = host && vp.want.map ? (const float*)(h + vp.at.map) : nullptr;
  out->map_device = vp.want.map ? ctx->v_map.p : nullptr;
  out->tri_index = host && vp.want.tri_index ? (const int32_t*)(h + vp.at.tri_index) : nullptr;
  out->tri_index_device = vp.want.tri_index ? ctx->v_tri.p : nullptr;
  return FLAME_NLTGV2_OK;
}

// _end and the copies into the caller's arrays: the tail of the two synchronous forms
static int view_finish(flame_nltgv2_ctx* ctx, float* map_out, int32_t* tri_index_out, flame_nltgv2_view_counts* counts_out) {
  flame_nltgv2_view_outputs_view v;
  const int rc = flame_nltgv2_render_view_end(ctx, &v);
  if (rc) return rc;
  const size_t n = (size_t)v.rows * (size_t)v.cols;
  if (map_out) std::memcpy(map_out, v.map, sizeof(float) * n);
  if (tri_index_out) std::memcpy(tri_index_out, v.tri_index, sizeof(int32_t) * n);
  if (counts_out) *counts_out = v.counts;
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_render_view(flame_nltgv2_ctx* ctx, const flame_nltgv2_view_params* params, const uint8_t* tri_valid, int rows, int cols,
                             float graph_scale, float* map_out, int32_t* tri_index_out, flame_nltgv2_view_counts* counts_out) {
  flame_nltgv2_view_params p;
  flame_nltgv2_default_view_params(&p);
  if (params) p = *params;
  p.want_map = map_out != nullptr, p.want_tri_index = tri_index_out != nullptr, p.copy_out = 1;
  const int rc = flame_nltgv2_render_view_begin(ctx, params ? &p : nullptr, tri_valid, rows, cols, graph_scale);
  if (rc) return rc;
  return view_finish(ctx, map_out, tri_index_out, counts_out);
}

int flame_nltgv2_render_view_arrays(flame_nltgv2_ctx* ctx, const flame_nltgv2_view_params* params, const int32_t* triangles, int32_t T,
                                    const float* vertices_xy, const float* idepths, int32_t V, const uint8_t* tri_valid, int rows, int cols,
                                    float* map_out, int32_t* tri_index_out, flame_nltgv2_view_counts* counts_out) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_render_view_arrays");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!params || !view_size_ok(rows, cols) || T < 0 || V < 0 || (T > 0 && !triangles) || (V > 0 && (!vertices_xy || !idepths)))
    return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (params->validity < 0 || params->validity > 1 || (tri_valid != nullptr) != (params->validity == 1)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (!triangles_in_range(triangles, T, V)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  flame_nltgv2_view_params p = *params;
  p.want_map = map_out != nullptr, p.want_tri_index = tri_index_out != nullptr, p.copy_out = 1;
  const ViewMesh own{triangles, vertices_xy, idepths};
  rc = view_enqueue(ctx, p, V, T, 1.0f, tri_valid, &own, rows, cols);
  if (rc) return rc;
  return view_finish(ctx, map_out, tri_index_out, counts_out);
}

// ---- the kept meshes (see flame_nltgv2.h) ----------------------------------------------------------------------------------------------
static bool slot_ok(int32_t slot) { return slot >= 0 && slot < FLAME_NLTGV2_KEPT_MESHES; }

// The slot's buffers hold V vertices and T triangles.  The side stream may still hold a fusion that reads the slot, or a snapshot that
// writes it.  A buffer that is large enough is reused, and stream order covers both.  A buffer that must grow is replaced by ensure(),
// which releases the old one with hipFree: hipFree returns only after the device has finished all work enqueued before it, on every
// stream (ensure asks an open run to stop first, so that the wait is short).  That guarantee is the one relied on here; the slot keeps
// no event of its own.
static int kept_reserve(flame_nltgv2_ctx* ctx, flame_nltgv2_ctx::KeptMesh& k, int32_t V, int32_t T, bool valid) {
  int rc = ensure(ctx, k.pos, sizeof(float) * 2 * (size_t)V + 16);
  if (!rc) rc = ensure(ctx, k.id, sizeof(float) * (size_t)V + 16);
  if (!rc) rc = ensure(ctx, k.tris, sizeof(int32_t) * 3 * (size_t)T + 16);
  if (!rc && valid) rc = ensure(ctx, k.valid, (size_t)T + 16);
  return rc;
}

int flame_nltgv2_keep_mesh(flame_nltgv2_ctx* ctx, int32_t slot, float graph_scale, int32_t validity) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_keep_mesh");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!slot_ok(slot)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (!ctx->have_graph) return fail(ctx, FLAME_NLTGV2_ERR_NO_GRAPH);
  if (!ctx->tris.current(ctx->topo)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (validity != 0 && validity != 2) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (validity == 2 && !ctx->tris.validity_current(ctx->topo)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const int32_t V = ctx->L.V, T = ctx->tris.T();
  flame_nltgv2_ctx::KeptMesh& k = ctx->kept[slot];
  k.V = k.T = -1, k.has_valid = false;  // (from here on the slot is being rewritten: empty until everything is enqueued)
  rc = kept_reserve(ctx, k, V, T, validity == 2);
  if (rc) return rc;
  hipStream_t rs = ctx->raster_stream;
  rc = mesh_state_on(ctx, rs);
  if (rc) return rc;
  LAUNCHCHK(ctx, flame_hip::launch_keep_vertices(V, ctx->c.pos, ctx->c.x, graph_scale, (float2*)k.pos.p, (float*)k.id.p, rs));
  rc = side_kernels_read_last(ctx);  // the snapshot kernel is the last reader of the canonical pos / x
  if (rc) return rc;
  if (T > 0) HIPCHK(ctx, hipMemcpyAsync(k.tris.p, ctx->r_tris.p, sizeof(int32_t) * 3 * (size_t)T, hipMemcpyDeviceToDevice, rs));
  if (validity == 2 && T > 0) HIPCHK(ctx, hipMemcpyAsync(k.valid.p, ctx->m_tvalid.p, (size_t)T, hipMemcpyDeviceToDevice, rs));
  k.V = V, k.T = T, k.has_valid = validity == 2;
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_keep_mesh_arrays(flame_nltgv2_ctx* ctx, int32_t slot, const int32_t* triangles, int32_t T, const float* vertices_xy,
                                  const float* idepths, int32_t V, const uint8_t* tri_valid) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_keep_mesh_arrays");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!slot_ok(slot) || T < 0 || V < 0 || (T > 0 && !triangles) || (V > 0 && (!vertices_xy || !idepths))) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (!triangles_in_range(triangles, T, V)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  flame_nltgv2_ctx::KeptMesh& k = ctx->kept[slot];
  k.V = k.T = -1, k.has_valid = false;
  rc = kept_reserve(ctx, k, V, T, tri_valid != nullptr);
  if (rc) return rc;
  hipStream_t rs = ctx->raster_stream;
  // (pageable memory: each copy holds the host until the bytes have left the caller's array)
  if (V > 0) {
    HIPCHK(ctx, hipMemcpyAsync(k.pos.p, vertices_xy, sizeof(float) * 2 * (size_t)V, hipMemcpyHostToDevice, rs));
    HIPCHK(ctx, hipMemcpyAsync(k.id.p, idepths, sizeof(float) * (size_t)V, hipMemcpyHostToDevice, rs));
  }
  if (T > 0) {
    HIPCHK(ctx, hipMemcpyAsync(k.tris.p, triangles, sizeof(int32_t) * 3 * (size_t)T, hipMemcpyHostToDevice, rs));
    if (tri_valid) HIPCHK(ctx, hipMemcpyAsync(k.valid.p, tri_valid, (size_t)T, hipMemcpyHostToDevice, rs));
  }
  k.V = V, k.T = T, k.has_valid = tri_valid != nullptr;
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_drop_mesh(flame_nltgv2_ctx* ctx, int32_t slot) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (!slot_ok(slot)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  ctx->kept[slot].V = ctx->kept[slot].T = -1, ctx->kept[slot].has_valid = false;  // (a fusion still in flight reads the buffers, which stay)
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_kept_mesh_info(flame_nltgv2_ctx* ctx, int32_t slot, int32_t* V, int32_t* T, int32_t* has_validity) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (!slot_ok(slot)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const flame_nltgv2_ctx::KeptMesh& k = ctx->kept[slot];
  if (V) *V = k.V;
  if (T) *T = k.T;
  if (has_validity) *has_validity = k.has_valid ? 1 : 0;
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_get_kept_mesh(flame_nltgv2_ctx* ctx, int32_t slot, float* vertices_xy, float* idepths, int32_t* triangles, uint8_t* tri_valid) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (!slot_ok(slot) || ctx->kept[slot].V < 0 || (tri_valid && !ctx->kept[slot].has_valid)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const flame_nltgv2_ctx::KeptMesh& k = ctx->kept[slot];
  hipStream_t rs = ctx->raster_stream;
  if (vertices_xy && k.V > 0) HIPCHK(ctx, hipMemcpyAsync(vertices_xy, k.pos.p, sizeof(float) * 2 * (size_t)k.V, hipMemcpyDeviceToHost, rs));
  if (idepths && k.V > 0) HIPCHK(ctx, hipMemcpyAsync(idepths, k.id.p, sizeof(float) * (size_t)k.V, hipMemcpyDeviceToHost, rs));
  if (triangles && k.T > 0) HIPCHK(ctx, hipMemcpyAsync(triangles, k.tris.p, sizeof(int32_t) * 3 * (size_t)k.T, hipMemcpyDeviceToHost, rs));
  if (tri_valid && k.T > 0) HIPCHK(ctx, hipMemcpyAsync(tri_valid, k.valid.p, (size_t)k.T, hipMemcpyDeviceToHost, rs));
  HIPCHK(ctx, hipStreamSynchronize(rs));
  return FLAME_NLTGV2_OK;
}

// ---- the fusion of views (see flame_nltgv2.h) --------------------------------------------------------------------------------------------
void flame_nltgv2_default_fuse_params(flame_nltgv2_fuse_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->n_sources = 1;
  for (flame_nltgv2_fuse_source& s : p->sources) {
    s.slot = -1, s.graph_scale = 1.0f, s.weight = 1.0f;
    s.Kinv_src[0] = s.Kinv_src[4] = s.Kinv_src[8] = 1.0f;
    s.R[0] = s.R[4] = s.R[8] = 1.0f;
  }
  p->K_dst[0] = p->K_dst[4] = p->K_dst[8] = 1.0f;
  p->rel_tol = 0.05f;
  p->min_support = 1;
  p->want_fused = p->want_masks = p->want_spread = p->copy_out = 1;
}

int flame_nltgv2_fuse_views_begin(flame_nltgv2_ctx* ctx, const flame_nltgv2_fuse_params* params, int rows, int cols) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_fuse_views_begin");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!params || !view_size_ok(rows, cols)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const flame_nltgv2_fuse_params& p = *params;
  const int N = p.n_sources;
  if (N < 1 || N > FLAME_NLTGV2_FUSE_SOURCES) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (!std::isfinite(p.rel_tol) || p.rel_tol < 0.0f || p.min_support < 1 || p.min_support > N) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  int live = -1;
  for (int s = 0; s < N; ++s) {
    const flame_nltgv2_fuse_source& src = p.sources[s];
    if (!(std::isfinite(src.weight) && src.weight > 0.0f)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
    if (src.slot == -1) {
      if (live >= 0) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
      live = s;
      if (!ctx->have_graph) return fail(ctx, FLAME_NLTGV2_ERR_NO_GRAPH);
      if (!ctx->tris.current(ctx->topo)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
      if (src.validity != 0 && src.validity != 2) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
      if (src.validity == 2 && !ctx->tris.validity_current(ctx->topo)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
    } else if (!slot_ok(src.slot) || ctx->kept[src.slot].V < 0) {
      return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
    }
  }
  // the source table: cameras, device meshes, prefix sums of V and T
  flame_hip::FuseTable tab;
  std::memset(&tab, 0, sizeof(tab));
  tab.n = N;
  int64_t v_sum = 0, t_sum = 0;
  for (int s = 0; s < N; ++s) {
    const flame_nltgv2_fuse_source& src = p.sources[s];
    flame_hip::FuseSource& o = tab.s[s];
    o = s == live ? live_source(ctx, src.validity, src.graph_scale) : kept_source(ctx->kept[src.slot]);
    o.cam = view_camera(src.Kinv_src, p.K_dst, src.R, src.t, p.near_depth);
    o.weight = src.weight;
    o.v0 = (int32_t)v_sum, o.t0 = (int32_t)t_sum;
    v_sum += s == live ? ctx->L.V : ctx->kept[src.slot].V, t_sum += s == live ? ctx->tris.T() : ctx->kept[src.slot].T;
    if (v_sum > INT32_MAX / 4 || t_sum > INT32_MAX / 4) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);  // (3 t and 2 + 2 t stay ints)
  }
  tab.v_end = (int32_t)v_sum, tab.t_end = (int32_t)t_sum;

  const size_t n = (size_t)rows * (size_t)cols;
  hipStream_t rs = ctx->raster_stream;
  flame_nltgv2_ctx::FusePending fp;
  fp.rows = rows, fp.cols = cols, fp.n_sources = N;
  fp.want.fused = p.want_fused != 0, fp.want.masks = p.want_masks != 0, fp.want.spread = p.want_spread != 0;
  fp.want.layers = p.want_layers != 0, fp.want.copy_out = p.copy_out != 0;
  fp.at = fuse_layout(rows, cols, N, fp.want);
  rc = open_stage(ctx, ctx->fuse, fp.at.total);
  if (rc) return rc;
  rc = ensure(ctx, ctx->f_vtx, sizeof(flame_hip::ViewVertex) * (size_t)tab.v_end + 16);
  if (!rc) rc = ensure(ctx, ctx->f_keys, sizeof(unsigned long long) * n * (size_t)N);
  if (!rc) rc = ensure(ctx, ctx->f_counts, sizeof(flame_hip::FuseCounts));
  if (!rc) rc = ensure(ctx, ctx->f_big, sizeof(int) * (2 * (size_t)tab.t_end + 2));
  if (!rc && fp.want.fused) rc = ensure(ctx, ctx->f_fused, sizeof(float) * n);
  if (!rc && fp.want.masks) rc = ensure(ctx, ctx->f_pmask, n);
  if (!rc && fp.want.masks) rc = ensure(ctx, ctx->f_imask, n);
  if (!rc && fp.want.spread) rc = ensure(ctx, ctx->f_spread, sizeof(float) * n);
  if (!rc && fp.want.layers) rc = ensure(ctx, ctx->f_layers, sizeof(float) * n * (size_t)N);
  if (rc) return rc;
  ctx->fuse.active = false;  // (from here on the pinned outputs are being rewritten)
  flame_hip::ViewVertex* vtx = (flame_hip::ViewVertex*)ctx->f_vtx.p;
  unsigned long long* keys = (unsigned long long*)ctx->f_keys.p;
  flame_hip::FuseCounts* counts = (flame_hip::FuseCounts*)ctx->f_counts.p;
  int* big = (int*)ctx->f_big.p;
  rc = enqueue_projection(ctx, ctx->fuse, live >= 0,
                          [&] { return flame_hip::launch_fuse_vertices(tab, vtx, rs); },
                          [&] { return flame_hip::launch_fuse_clear((long)(n * (size_t)N), keys, counts, big, rs); },
                          [&] { return flame_hip::launch_fuse_raster(tab, vtx, keys, counts, big, rows, cols, rs); });
  if (rc) return rc;
  flame_hip::FuseOutputs out;
  out.fused = fp.want.fused ? (float*)ctx->f_fused.p : nullptr;
  out.present_mask = fp.want.masks ? (uint8_t*)ctx->f_pmask.p : nullptr;
  out.inlier_mask = fp.want.masks ? (uint8_t*)ctx->f_imask.p : nullptr;
  out.spread = fp.want.spread ? (float*)ctx->f_spread.p : nullptr;
  out.layers = fp.want.layers ? (float*)ctx->f_layers.p : nullptr;
  LAUNCHCHK(ctx, flame_hip::launch_fuse_vote(tab, (long)n, keys, p.rel_tol, p.min_support, out, counts, rs));
  char* h = ctx->fuse.h.p;
  HIPCHK(ctx, hipMemcpyAsync(h + fp.at.counts, counts, sizeof(flame_hip::FuseCounts), hipMemcpyDeviceToHost, rs));
  if (fp.want.copy_out) {
    if (fp.want.fused) HIPCHK(ctx, hipMemcpyAsync(h + fp.at.fused, out.fused, sizeof(float) * n, hipMemcpyDeviceToHost, rs));
    if (fp.want.masks) {
      HIPCHK(ctx, hipMemcpyAsync(h + fp.at.present, out.present_mask, n, hipMemcpyDeviceToHost, rs));
      HIPCHK(ctx, hipMemcpyAsync(h + fp.at.inlier, out.inlier_mask, n, hipMemcpyDeviceToHost, rs));
    }
    if (fp.want.spread) HIPCHK(ctx, hipMemcpyAsync(h + fp.at.spread, out.spread, sizeof(float) * n, hipMemcpyDeviceToHost, rs));
    if (fp.want.layers) HIPCHK(ctx, hipMemcpyAsync(h + fp.at.layers, out.layers, sizeof(float) * n * (size_t)N, hipMemcpyDeviceToHost, rs));
  }
  ctx->fuse_pending = fp;
  return close_stage(ctx, ctx->fuse);
}

int flame_nltgv2_fuse_views_end(flame_nltgv2_ctx* ctx, flame_nltgv2_fuse_outputs_view* out) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_fuse_views_end");
  int rc = enter(ctx);
  if (rc) return rc;
  const flame_nltgv2_ctx::FusePending& fp = ctx->fuse_pending;
  if (!out || !ctx->fuse.h.p || !ctx->fuse.active) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  HIPCHK(ctx, hipStreamSynchronize(ctx->raster_stream));
  const char* h = ctx->fuse.h.p;
  const bool host = fp.want.copy_out;
  out->rows = fp.rows, out->cols = fp.cols, out->n_sources = fp.n_sources;
  std::memcpy(&out->counts, h + fp.at.counts, sizeof(out->counts));
  out->device_ms = stage_ms(ctx->fuse);
  out->fused = host && fp.want.fused ? (const float*)(h + fp.at.fused) : nullptr;
  out->fused_device = fp.want.fused ? ctx->f_fused.p : nullptr;
  out->present_mask = host && fp.want.masks ? (const uint8_t*)(h + fp.at.present) : nullptr;
  out->present_mask_device = fp.want.masks ? ctx->f_pmask.p : nullptr;
  out->inlier_mask = host && fp.want.masks ? (const uint8_t*)(h + fp.at.inlier) : nullptr;
  out->inlier_mask_device = fp.want.masks ? ctx->f_imask.p : nullptr;
  out->spread = host && fp.want.spread ? (const float*)(h + fp.at.spread) : nullptr;
  out->spread_device = fp.want.spread ? ctx->f_spread.p : nullptr;
  out->layers = host && fp.want.layers ? (const float*)(h + fp.at.layers) : nullptr;
  out->layers_device = fp.want.layers ? ctx->f_layers.p : nullptr;
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_fuse_views(flame_nltgv2_ctx* ctx, const flame_nltgv2_fuse_params* params, int rows, int cols, float* fused_out,
                            uint8_t* present_mask_out, uint8_t* inlier_mask_out, float* spread_out, float* layers_out,
                            flame_nltgv2_fuse_counts* counts_out) {
  flame_nltgv2_fuse_params p;
  flame_nltgv2_default_fuse_params(&p);
  if (params) p = *params;
  p.want_fused = fused_out != nullptr, p.want_masks = present_mask_out != nullptr || inlier_mask_out != nullptr;
  p.want_spread = spread_out != nullptr, p.want_layers = layers_out != nullptr, p.copy_out = 1;
  int rc = flame_nltgv2_fuse_views_begin(ctx, params ? &p : nullptr, rows, cols);
  if (rc) return rc;
  flame_nltgv2_fuse_outputs_view v;
  rc = flame_nltgv2_fuse_views_end(ctx, &v);
  if (rc) return rc;
  const size_t n = (size_t)v.rows * (size_t)v.cols;
  if (fused_out) std::memcpy(fused_out, v.fused, sizeof(float) * n);
  if (present_mask_out) std::memcpy(present_mask_out, v.present_mask, n);
  if (inlier_mask_out) std::memcpy(inlier_mask_out, v.inlier_mask, n);
  if (spread_out) std::memcpy(spread_out, v.spread, sizeof(float) * n);
  if (layers_out) std::memcpy(layers_out, v.layers, sizeof(float) * n * (size_t)v.n_sources);
  if (counts_out) *counts_out = v.counts;
  return FLAME_NLTGV2_OK;
}

// ---- the volumetric map (see flame_nltgv2.h) ---------------------------------------------------------------------------------------------
void flame_nltgv2_default_volume_params(flame_nltgv2_volume_params* p) {
  if (!p) return;
  p->nx = p->ny = p->nz = 64;
  p->voxel_size = 0.05f;
  p->origin[0] = p->origin[1] = p->origin[2] = 0.0f;
  p->trunc = 0.15f;
  p->max_weight = 64.0f;
}

void flame_nltgv2_default_integrate_params(flame_nltgv2_integrate_params* p) {
  if (!p) return;
  p->weight = 1.0f;
  p->near_depth = 0.0f;
  p->min_depth = 0.0f, p->max_depth = HUGE_VALF;
  p->use_filtered_map = 0, p->reserved = 0;
  p->map_device = nullptr;
}

void flame_nltgv2_default_raycast_params(flame_nltgv2_raycast_params* p) {
  if (!p) return;
  p->z_near = 0.1f, p->dz = 0.05f;
  p->n_steps = 64;
  p->copy_out = 1;
}

static bool finite_positive(float v) { return std::isfinite(v) && v > 0.0f; }

static flame_hip::VolumeGrid volume_grid(const flame_nltgv2_ctx* ctx) {
  const flame_nltgv2_volume_params& p = ctx->vol_params;
  flame_hip::VolumeGrid g;
  g.nx = p.nx, g.ny = p.ny, g.nz = p.nz;
  g.voxel_size = p.voxel_size;
  std::memcpy(g.origin, p.origin, sizeof(g.origin));
  g.trunc = p.trunc, g.max_weight = p.max_weight;
  for (int a = 0; a < 3; ++a) g.base[a] = ctx->vol_base[a];
  return g;
}
static size_t volume_count(const flame_nltgv2_ctx* ctx) {
  return (size_t)volume_voxels(ctx->vol_params.nx, ctx->vol_params.ny, ctx->vol_params.nz);
}

// The side stream may still hold an integration that writes the volume or a raycast that reads it: it is waited for, then the memory
// goes back (hipFree waits for the device: an open run is asked to stop first, as in ensure()).
static int volume_release(flame_nltgv2_ctx* ctx) {
  ctx->have_volume = false;
  if (!ctx->vol.p) return FLAME_NLTGV2_OK;
  HIPCHK(ctx, hipStreamSynchronize(ctx->raster_stream));
  request_open_stop(ctx);
  HIPCHK(ctx, hipFree(ctx->vol.p));
  ctx->device_bytes -= ctx->vol.cap;
  ctx->vol.p = nullptr, ctx->vol.cap = 0;
  if (ctx->vol2.p) {  // the shift's second buffer goes with it
    HIPCHK(ctx, hipFree(ctx->vol2.p));
    ctx->device_bytes -= ctx->vol2.cap;
    ctx->vol2.p = nullptr, ctx->vol2.cap = 0;
  }
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_volume_create(flame_nltgv2_ctx* ctx, const flame_nltgv2_volume_params* params) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_volume_create");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!params || volume_voxels(params->nx, params->ny, params->nz) == 0) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (!finite_positive(params->voxel_size) || !finite_positive(params->trunc) || !finite_positive(params->max_weight))
    return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(params->origin[a])) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  // exactly the bytes of the volume (ensure() would take half as much again: up to a GiB for nothing)
  const size_t bytes = sizeof(flame_hip::Voxel) * (size_t)volume_voxels(params->nx, params->ny, params->nz);
  if (ctx->vol.cap != bytes) {
    rc = volume_release(ctx);
    if (rc) return rc;
    const hipError_t e = hipMalloc(&ctx->vol.p, bytes);
    if (e != hipSuccess) {
      ctx->last_hip = (int)e;
      ctx->vol.p = nullptr;
      return fail(ctx, e == hipErrorOutOfMemory ? FLAME_NLTGV2_ERR_OOM : FLAME_NLTGV2_ERR_HIP);
    }
    ctx->vol.cap = bytes;
    ctx->device_bytes += bytes;
  }
  ctx->vol_params = *params;
  ctx->vol_base[0] = ctx->vol_base[1] = ctx->vol_base[2] = 0;
  ctx->have_volume = true;
  LAUNCHCHK(ctx, flame_hip::launch_volume_fill(volume_grid(ctx), (flame_hip::Voxel*)ctx->vol.p, ctx->raster_stream));
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_volume_reset(flame_nltgv2_ctx* ctx) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_volume_reset");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_volume) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  LAUNCHCHK(ctx, flame_hip::launch_volume_fill(volume_grid(ctx), (flame_hip::Voxel*)ctx->vol.p, ctx->raster_stream));
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_volume_destroy(flame_nltgv2_ctx* ctx) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_volume_destroy");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_volume) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  return volume_release(ctx);
}

int flame_nltgv2_volume_info(flame_nltgv2_ctx* ctx, flame_nltgv2_volume_params* params_out, int64_t* device_bytes_out) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_volume) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (params_out) *params_out = ctx->vol_params;
  if (device_bytes_out) *device_bytes_out = (int64_t)(ctx->vol.cap + ctx->vol2.cap);
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_volume_download(flame_nltgv2_ctx* ctx, float* tsdf_out, float* weight_out) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_volume_download");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_volume) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const size_t n = volume_count(ctx);
  std::vector<flame_hip::Voxel> h(n);
  HIPCHK(ctx, hipMemcpyAsync(h.data(), ctx->vol.p, sizeof(flame_hip::Voxel) * n, hipMemcpyDeviceToHost, ctx->raster_stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->raster_stream));
  for (size_t i = 0; i < n; ++i) {
    if (tsdf_out) tsdf_out[i] = h[i].tsdf;
    if (weight_out) weight_out[i] = h[i].weight;
  }
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_volume_upload(flame_nltgv2_ctx* ctx, const float* tsdf, const float* weight) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_volume_upload");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_volume || !tsdf || !weight) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const size_t n = volume_count(ctx);
  std::vector<flame_hip::Voxel> h(n);
  for (size_t i = 0; i < n; ++i) {
    if (!(weight[i] >= 0.0f)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
    h[i].tsdf = tsdf[i], h[i].weight = weight[i];
  }
  HIPCHK(ctx, hipMemcpyAsync(ctx->vol.p, h.data(), sizeof(flame_hip::Voxel) * n, hipMemcpyHostToDevice, ctx->raster_stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->raster_stream));  // (h leaves scope)
  return FLAME_NLTGV2_OK;
}

// The integration on the side stream.  Like the metric stage it reads what the other stages left on the device, in the order of that
// stream, and nothing of the canonical arrays: no mesh_state_on, no side_kernels_read_last.
int flame_nltgv2_volume_integrate_begin(flame_nltgv2_ctx* ctx, const float* K, const float* T_cam_world,
                                        const flame_nltgv2_integrate_params* params, int rows, int cols) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_volume_integrate_begin");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_volume) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (!K || !T_cam_world || !params || rows <= 0 || cols <= 0 || (uint64_t)rows * (uint64_t)cols >= (1ull << 31)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (!finite_positive(params->weight)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const float* map = nullptr;
  if (!params->map_device && !ctx->have_graph) return fail(ctx, FLAME_NLTGV2_ERR_NO_GRAPH);
  rc = resident_map(ctx, params->map_device, params->use_filtered_map, rows, cols, &map);
  if (rc) return rc;
  hipStream_t rs = ctx->raster_stream;
  flame_nltgv2_ctx::IntegratePending ip;
  ip.rows = rows, ip.cols = cols;
  ip.at = integrate_layout();
  rc = open_stage(ctx, ctx->vint, ip.at.total);
  if (rc) return rc;
  rc = ensure(ctx, ctx->vi_counts, kCountSetsBytes);
  if (rc) return rc;
  ctx->vint.active = false;  // (from here on the pinned outputs are being rewritten)
  flame_hip::IntegrateArgs a;
  std::memcpy(a.K, K, sizeof(a.K));
  std::memcpy(a.pose, T_cam_world, sizeof(a.pose));
  a.rows = rows, a.cols = cols;
  a.weight = params->weight, a.near_depth = params->near_depth, a.min_depth = params->min_depth, a.max_depth = params->max_depth;
  int* counts = (int*)ctx->vi_counts.p;
  HIPCHK(ctx, hipEventRecord(ctx->vint.ev0, rs));
  LAUNCHCHK(ctx, flame_hip::launch_volume_integrate(volume_grid(ctx), a, map, (flame_hip::Voxel*)ctx->vol.p, counts, rs));
  HIPCHK(ctx, hipMemcpyAsync(ctx->vint.h.p + ip.at.counts, counts, kCountSetsBytes, hipMemcpyDeviceToHost, rs));
  ctx->vint_pending = ip;
  return close_stage(ctx, ctx->vint);
}

int flame_nltgv2_volume_integrate_end(flame_nltgv2_ctx* ctx, flame_nltgv2_integrate_view* out) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_volume_integrate_end");
  int rc = enter(ctx);
  if (rc) return rc;
  const flame_nltgv2_ctx::IntegratePending& ip = ctx->vint_pending;
  if (!out || !ctx->vint.h.p || !ctx->vint.active) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  HIPCHK(ctx, hipStreamSynchronize(ctx->raster_stream));
  out->rows = ip.rows, out->cols = ip.cols;
  out->device_ms = stage_ms(ctx->vint);
  out->reserved = 0;
  sum_count_slots((const int32_t*)(ctx->vint.h.p + ip.at.counts), (int)(sizeof(out->counts) / sizeof(int32_t)), (int32_t*)&out->counts);
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_volume_integrate(flame_nltgv2_ctx* ctx, const float* K, const float* T_cam_world,
                                  const flame_nltgv2_integrate_params* params, int rows, int cols, flame_nltgv2_integrate_counts* counts_out) {
  int rc = flame_nltgv2_volume_integrate_begin(ctx, K, T_cam_world, params, rows, cols);
  if (rc) return rc;
  flame_nltgv2_integrate_view v;
  rc = flame_nltgv2_volume_integrate_end(ctx, &v);
  if (rc) return rc;
  if (counts_out) *counts_out = v.counts;
  return FLAME_NLTGV2_OK;
}

// The raycast on the side stream: it reads the volume alone.
int flame_nltgv2_volume_raycast_begin(flame_nltgv2_ctx* ctx, const float* Kinv, const float* T_world_cam,
                                      const flame_nltgv2_raycast_params* params, int rows, int cols) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_volume_raycast_begin");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_volume) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (!Kinv || !T_world_cam || !params || !view_size_ok(rows, cols)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (!std::isfinite(params->z_near) || !finite_positive(params->dz) || params->n_steps < 1 || params->n_steps > 4096)
    return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const size_t n = (size_t)rows * (size_t)cols;
  hipStream_t rs = ctx->raster_stream;
  flame_nltgv2_ctx::RaycastPending rp;
  rp.rows = rows, rp.cols = cols, rp.copy_out = params->copy_out != 0;
  rp.at = raycast_layout(rows, cols, rp.copy_out);
  rc = open_stage(ctx, ctx->vray, rp.at.total);
  if (rc) return rc;
  rc = ensure(ctx, ctx->y_map, sizeof(float) * n);
  if (!rc) rc = ensure(ctx, ctx->y_counts, kCountSetsBytes);
  if (rc) return rc;
  ctx->vray.active = false;  // (from here on the pinned outputs are being rewritten)
  flame_hip::RaycastArgs a;
  std::memcpy(a.Kinv, Kinv, sizeof(a.Kinv));
  std::memcpy(a.pose, T_world_cam, sizeof(a.pose));
  a.rows = rows, a.cols = cols;
  a.z_near = params->z_near, a.dz = params->dz, a.n_steps = params->n_steps;
  int* counts = (int*)ctx->y_counts.p;
  HIPCHK(ctx, hipEventRecord(ctx->vray.ev0, rs));
  LAUNCHCHK(ctx, flame_hip::launch_volume_raycast(volume_grid(ctx), a, (const flame_hip::Voxel*)ctx->vol.p, (float*)ctx->y_map.p, counts, rs));
  char* h = ctx->vray.h.p;
  HIPCHK(ctx, hipMemcpyAsync(h + rp.at.counts, counts, kCountSetsBytes, hipMemcpyDeviceToHost, rs));
  if (rp.copy_out) HIPCHK(ctx, hipMemcpyAsync(h + rp.at.map, ctx->y_map.p, sizeof(float) * n, hipMemcpyDeviceToHost, rs));
  ctx->vray_pending = rp;
  return close_stage(ctx, ctx->vray);
}

int flame_nltgv2_volume_raycast_end(flame_nltgv2_ctx* ctx, flame_nltgv2_raycast_view* out) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_volume_raycast_end");
  int rc = enter(ctx);
  if (rc) return rc;
  const flame_nltgv2_ctx::RaycastPending& rp = ctx->vray_pending;
  if (!out || !ctx->vray.h.p || !ctx->vray.active) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  HIPCHK(ctx, hipStreamSynchronize(ctx->raster_stream));
  const char* h = ctx->vray.h.p;
  out->rows = rp.rows, out->cols = rp.cols;
  out->device_ms = stage_ms(ctx->vray);
  out->reserved = 0;
  sum_count_slots((const int32_t*)(h + rp.at.counts), (int)(sizeof(out->counts) / sizeof(int32_t)), (int32_t*)&out->counts);
  out->map = rp.copy_out ? (const float*)(h + rp.at.map) : nullptr;
  out->map_device = ctx->y_map.p;
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_volume_raycast(flame_nltgv2_ctx* ctx, const float* Kinv, const float* T_world_cam,
                                const flame_nltgv2_raycast_params* params, int rows, int cols, float* map_out,
                                flame_nltgv2_raycast_counts* counts_out) {
  flame_nltgv2_raycast_params p;
  flame_nltgv2_default_raycast_params(&p);
  if (params) p = *params;
  p.copy_out = 1;
  int rc = flame_nltgv2_volume_raycast_begin(ctx, Kinv, T_world_cam, params ? &p : nullptr, rows, cols);
  if (rc) return rc;
  flame_nltgv2_raycast_view v;
  rc = flame_nltgv2_volume_raycast_end(ctx, &v);
  if (rc) return rc;
  if (map_out) std::memcpy(map_out, v.map, sizeof(float) * (size_t)v.rows * (size_t)v.cols);
  if (counts_out) *counts_out = v.counts;
  return FLAME_NLTGV2_OK;
}

// ---- the window that follows the camera (see flame_nltgv2.h) ---------------------------------------------------------------------------
void flame_nltgv2_default_follow_params(flame_nltgv2_follow_params* p) {
  if (!p) return;
  p->focus_depth = 0.0f;
  p->step = 8;
}

int flame_nltgv2_volume_window(flame_nltgv2_ctx* ctx, int32_t base_out[3]) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_volume || !base_out) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  std::memcpy(base_out, ctx->vol_base, sizeof(ctx->vol_base));
  return FLAME_NLTGV2_OK;
}

// The shift on the side stream: out of place from vol into vol2, then the two change names.  Whatever was enqueued before reads or
// writes the old vol ahead of the kernel, whatever comes later the new one behind it: the stream's order is the whole synchronisation.
int flame_nltgv2_volume_shift_begin(flame_nltgv2_ctx* ctx, const int32_t shift[3]) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_volume_shift_begin");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_volume || !shift) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const int32_t dims[3] = {ctx->vol_params.nx, ctx->vol_params.ny, ctx->vol_params.nz};
  flame_nltgv2_ctx::ShiftPending sp;
  if (!shifted_base(ctx->vol_base, shift, sp.base)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  std::memcpy(sp.shift, shift, sizeof(sp.shift));
  int s[3];
  const bool moves = clamped_shift(dims, shift, s);
  if (moves && !ctx->vol2.p) {  // exactly the bytes of the volume, as flame_nltgv2_volume_create takes them
    const hipError_t e = hipMalloc(&ctx->vol2.p, ctx->vol.cap);
    if (e != hipSuccess) {
      ctx->last_hip = (int)e;
      ctx->vol2.p = nullptr;
      (void)hipGetLastError();
      return fail(ctx, e == hipErrorOutOfMemory ? FLAME_NLTGV2_ERR_OOM : FLAME_NLTGV2_ERR_HIP);
    }
    ctx->vol2.cap = ctx->vol.cap;
    ctx->device_bytes += ctx->vol2.cap;
  }
  hipStream_t rs = ctx->raster_stream;
  sp.at = integrate_layout();
  rc = open_stage(ctx, ctx->vshift, sp.at.total);
  if (rc) return rc;
  rc = ensure(ctx, ctx->vs_counts, kCountSetsBytes);
  if (rc) return rc;
  ctx->vshift.active = false;  // (from here on the pinned outputs are being rewritten)
  int* counts = (int*)ctx->vs_counts.p;
  HIPCHK(ctx, hipEventRecord(ctx->vshift.ev0, rs));
  LAUNCHCHK(ctx, flame_hip::launch_volume_shift(volume_grid(ctx), s, (const flame_hip::Voxel*)ctx->vol.p, moves ? (flame_hip::Voxel*)ctx->vol2.p : nullptr,
                                                counts, &sp.record_bytes, rs));
  HIPCHK(ctx, hipMemcpyAsync(ctx->vshift.h.p + sp.at.counts, counts, kCountSetsBytes, hipMemcpyDeviceToHost, rs));
  if (moves) {
    std::swap(ctx->vol.p, ctx->vol2.p);
    std::memcpy(ctx->vol_base, sp.base, sizeof(ctx->vol_base));
  } else {
    sp.record_bytes = 0;
  }
  ctx->vshift_pending = sp;
  return close_stage(ctx, ctx->vshift);
}

int flame_nltgv2_volume_shift_end(flame_nltgv2_ctx* ctx, flame_nltgv2_shift_view* out) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_volume_shift_end");
  int rc = enter(ctx);
  if (rc) return rc;
  const flame_nltgv2_ctx::ShiftPending& sp = ctx->vshift_pending;
  if (!out || !ctx->vshift.h.p || !ctx->vshift.active) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  HIPCHK(ctx, hipStreamSynchronize(ctx->raster_stream));
  std::memcpy(out->shift, sp.shift, sizeof(out->shift));
  std::memcpy(out->base, sp.base, sizeof(out->base));
  out->device_ms = stage_ms(ctx->vshift);
  out->record_bytes = sp.record_bytes;
  sum_count_slots((const int32_t*)(ctx->vshift.h.p + sp.at.counts), (int)(sizeof(out->counts) / sizeof(int32_t)), (int32_t*)&out->counts);
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_volume_shift(flame_nltgv2_ctx* ctx, const int32_t shift[3], flame_nltgv2_shift_counts* counts_out) {
  int rc = flame_nltgv2_volume_shift_begin(ctx, shift);
  if (rc) return rc;
  flame_nltgv2_shift_view v;
  rc = flame_nltgv2_volume_shift_end(ctx, &v);
  if (rc) return rc;
  if (counts_out) *counts_out = v.counts;
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_volume_follow(flame_nltgv2_ctx* ctx, const float* T_world_cam, const flame_nltgv2_follow_params* params,
                               flame_nltgv2_follow_plan* plan_out) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_volume || !T_world_cam || !params || !plan_out) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const flame_nltgv2_volume_params& vp = ctx->vol_params;
  const int32_t dims[3] = {vp.nx, vp.ny, vp.nz};
  int32_t shift[3];
  if (!follow_shift(T_world_cam, params->focus_depth, params->step, vp.origin, vp.voxel_size, ctx->vol_base, dims, shift))
    return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  WindowPlan plan;
  window_plan(dims, shift, &plan);
  std::memcpy(plan_out, &plan, sizeof(plan));
  return FLAME_NLTGV2_OK;
}

void flame_nltgv2_default_volume_mesh_params(flame_nltgv2_volume_mesh_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->want_normals = p->copy_out = 1;
}

// The surface extraction on the side stream: it reads the volume alone.  The counts are known only on the device when the emit pass
// runs, so the arrays have room for the caller's capacities (capped by what the box can give) and _end fetches what was written.
int flame_nltgv2_volume_mesh_begin(flame_nltgv2_ctx* ctx, const flame_nltgv2_volume_mesh_params* params) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_volume_mesh_begin");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_volume || !params) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (params->max_vertices < 0 || params->max_triangles < 0) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const int32_t dims[3] = {ctx->vol_params.nx, ctx->vol_params.ny, ctx->vol_params.nz};
  flame_hip::MeshBox box;
  const uint64_t n_box = mesh_box_voxels(dims, params->lo, params->hi, box.lo, box.n);
  if (n_box == 0) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const size_t v_room = (size_t)mesh_vertex_room(n_box, params->max_vertices), t_room = (size_t)mesh_triangle_room(n_box, params->max_triangles);
  const size_t blocks = (size_t)flame_hip::mesh_blocks((long)n_box);
  hipStream_t rs = ctx->raster_stream;
  flame_nltgv2_ctx::VolumeMeshPending mp;
  mp.want_normals = params->want_normals != 0, mp.copy_out = params->copy_out != 0;
  mp.v_room = (int32_t)v_room, mp.t_room = (int32_t)t_room;
  mp.at = volume_mesh_layout((int64_t)v_room, (int64_t)t_room, mp.want_normals, mp.copy_out);
  rc = open_stage(ctx, ctx->vmesh, mp.at.total);
  if (rc) return rc;
  rc = ensure(ctx, ctx->z_cls, n_box);
  if (!rc) rc = ensure(ctx, ctx->z_emask, n_box);
  if (!rc) rc = ensure(ctx, ctx->z_vloc, sizeof(uint16_t) * n_box);
  if (!rc) rc = ensure(ctx, ctx->z_tloc, sizeof(uint16_t) * n_box);
  if (!rc) rc = ensure(ctx, ctx->z_bv, sizeof(int) * blocks);
  if (!rc) rc = ensure(ctx, ctx->z_bt, sizeof(int) * blocks);
  if (!rc) rc = ensure(ctx, ctx->z_counts, kCountSetsBytes);
  if (!rc) rc = ensure(ctx, ctx->z_totals, kMeshTotalsBytes);
  if (!rc) rc = ensure(ctx, ctx->z_verts, 3 * sizeof(float) * v_room);
  if (!rc && mp.want_normals) rc = ensure(ctx, ctx->z_norms, 3 * sizeof(float) * v_room);
  if (!rc) rc = ensure(ctx, ctx->z_tris, 3 * sizeof(int32_t) * t_room);
  if (rc) return rc;
  ctx->vmesh.active = false;  // (from here on the pinned outputs are being rewritten)
  flame_hip::MeshScratch sc;
  sc.cls = (uint8_t*)ctx->z_cls.p, sc.emask = (uint8_t*)ctx->z_emask.p;
  sc.vloc = (uint16_t*)ctx->z_vloc.p, sc.tloc = (uint16_t*)ctx->z_tloc.p;
  sc.block_v = (int*)ctx->z_bv.p, sc.block_t = (int*)ctx->z_bt.p;
  flame_hip::MeshOut mo;
  mo.vertices = (float*)ctx->z_verts.p, mo.normals = mp.want_normals ? (float*)ctx->z_norms.p : nullptr, mo.triangles = (int32_t*)ctx->z_tris.p;
  int* counts = (int*)ctx->z_counts.p;
  HIPCHK(ctx, hipEventRecord(ctx->vmesh.ev0, rs));
  LAUNCHCHK(ctx, flame_hip::launch_volume_mesh(volume_grid(ctx), box, (const flame_hip::Voxel*)ctx->vol.p, sc, counts, (flame_hip::MeshTotals*)ctx->z_totals.p,
                                               (int)v_room, (int)t_room, mo, ctx->z_pass, rs));
  char* h = ctx->vmesh.h.p;
  HIPCHK(ctx, hipMemcpyAsync(h + mp.at.counts, counts, kCountSetsBytes, hipMemcpyDeviceToHost, rs));
  HIPCHK(ctx, hipMemcpyAsync(h + mp.at.totals, ctx->z_totals.p, kMeshTotalsBytes, hipMemcpyDeviceToHost, rs));
  ctx->vmesh_pending = mp;
  return close_stage(ctx, ctx->vmesh);
}

int flame_nltgv2_volume_mesh_end(flame_nltgv2_ctx* ctx, flame_nltgv2_volume_mesh_view* out) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_volume_mesh_end");
  int rc = enter(ctx);
  if (rc) return rc;
  flame_nltgv2_ctx::VolumeMeshPending& mp = ctx->vmesh_pending;
  if (!out || !ctx->vmesh.h.p || !ctx->vmesh.active) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  hipStream_t rs = ctx->raster_stream;
  HIPCHK(ctx, hipStreamSynchronize(rs));
  char* h = ctx->vmesh.h.p;
  flame_hip::MeshTotals tot;
  std::memcpy(&tot, h + mp.at.totals, sizeof(tot));
  int32_t cubes[flame_hip::kMeshCubeCounters];
  sum_count_slots((const int32_t*)(h + mp.at.counts), flame_hip::kMeshCubeCounters, cubes);
  const bool overflow = tot.n_vertices > mp.v_room || tot.n_triangles > mp.t_room;  // (the emit pass's own test)
  const bool host = mp.copy_out && !overflow;
  if (host && !mp.fetched) {  // exactly what was written, as metric_outputs_end fetches the dense cloud
    const size_t vb = 3 * sizeof(float) * (size_t)tot.n_vertices, tb = 3 * sizeof(int32_t) * (size_t)tot.n_triangles;
    if (vb) HIPCHK(ctx, hipMemcpyAsync(h + mp.at.vertices, ctx->z_verts.p, vb, hipMemcpyDeviceToHost, rs));
    if (vb && mp.want_normals) HIPCHK(ctx, hipMemcpyAsync(h + mp.at.normals, ctx->z_norms.p, vb, hipMemcpyDeviceToHost, rs));
    if (tb) HIPCHK(ctx, hipMemcpyAsync(h + mp.at.triangles, ctx->z_tris.p, tb, hipMemcpyDeviceToHost, rs));
    if (vb || tb) HIPCHK(ctx, hipStreamSynchronize(rs));
    mp.fetched = true;
  }
  std::memset(out, 0, sizeof(*out));
  out->counts.n_vertices = tot.n_vertices, out->counts.n_triangles = tot.n_triangles;
  out->counts.live_cubes = cubes[0], out->counts.surface_cubes = cubes[1];
  out->counts.overflow = overflow ? 1 : 0;
  out->device_ms = stage_ms(ctx->vmesh);
  const hipEvent_t marks[flame_hip::kMeshPasses + 1] = {ctx->vmesh.ev0, ctx->z_pass[0], ctx->z_pass[1], ctx->z_pass[2], ctx->vmesh.ev1};
  for (int p = 0; p < flame_hip::kMeshPasses; ++p)
    if (hipEventElapsedTime(&out->pass_ms[p], marks[p], marks[p + 1]) != hipSuccess) (void)hipGetLastError(), out->pass_ms[p] = 0.0f;
  out->vertices = host ? (const float*)(h + mp.at.vertices) : nullptr;
  out->normals = host && mp.want_normals ? (const float*)(h + mp.at.normals) : nullptr;
  out->triangles = host ? (const int32_t*)(h + mp.at.triangles) : nullptr;
  out->vertices_device = ctx->z_verts.p;
  out->normals_device = mp.want_normals ? ctx->z_norms.p : nullptr;
  out->triangles_device = ctx->z_tris.p;
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_volume_mesh(flame_nltgv2_ctx* ctx, const flame_nltgv2_volume_mesh_params* params, float* vertices_out, float* normals_out,
                             int32_t* triangles_out, flame_nltgv2_volume_mesh_counts* counts_out) {
  flame_nltgv2_volume_mesh_params p;
  flame_nltgv2_default_volume_mesh_params(&p);
  if (params) p = *params;
  p.copy_out = 1, p.want_normals = normals_out != nullptr;
  int rc = flame_nltgv2_volume_mesh_begin(ctx, params ? &p : nullptr);
  if (rc) return rc;
  flame_nltgv2_volume_mesh_view v;
  rc = flame_nltgv2_volume_mesh_end(ctx, &v);
  if (rc) return rc;
  if (counts_out) *counts_out = v.counts;
  if (v.counts.overflow) return FLAME_NLTGV2_OK;
  const size_t vb = 3 * sizeof(float) * (size_t)v.counts.n_vertices;
  if (vertices_out && vb) std::memcpy(vertices_out, v.vertices, vb);
  if (normals_out && vb) std::memcpy(normals_out, v.normals, vb);
  if (triangles_out && v.counts.n_triangles) std::memcpy(triangles_out, v.triangles, 3 * sizeof(int32_t) * (size_t)v.counts.n_triangles);
  return FLAME_NLTGV2_OK;
}

void flame_nltgv2_default_debug_image_params(flame_nltgv2_debug_image_params* p) {
  if (!p) return;
  p->scene_color_scale = 1.0f;  // params.h:109
  p->flip = 0;
  p->want_idepthmap = 1;
  p->want_normals = 1;
}

// The debug images on the side stream (see flame_nltgv2.h).
int flame_nltgv2_debug_images_begin(flame_nltgv2_ctx* ctx, const uint8_t* img_host, const void* img_device, int step_bytes,
                                    const float* K, const flame_nltgv2_debug_image_params* params, int rows, int cols) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_debug_images_begin");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_graph) return fail(ctx, FLAME_NLTGV2_ERR_NO_GRAPH);
  if (rows <= 0 || cols <= 0) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const float* map = nullptr;
  rc = resident_map(ctx, nullptr, 0, rows, cols, &map);
  if (rc) return rc;
  if (!ctx->tris.current(ctx->topo)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if ((img_host != nullptr) == (img_device != nullptr) || step_bytes < cols || !K || !params) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const int32_t T = ctx->tris.T();
  const size_t n = (size_t)rows * (size_t)cols;
  const bool want_id = params->want_idepthmap != 0, want_n = params->want_normals != 0;
  hipStream_t rs = ctx->raster_stream;
  flame_nltgv2_ctx::DebugPending dp;
  dp.rows = rows, dp.cols = cols, dp.want_idepth = want_id, dp.want_normals = want_n;
  dp.at = debug_layout(rows, cols, want_id, want_n, img_host != nullptr);
  rc = open_stage(ctx, ctx->dbg, dp.at.total);
  if (rc) return rc;
  // r_keys names the winners of an all-valid rasterisation of r_tris: w1 / w2 are looked up there.  Otherwise (a map rasterised with
  // tri_valid, triangles re-uploaded by mesh_outputs_begin) the stage rasterises them itself
  const bool from_keys = ctx->tris.keys_name_winners();
  if (img_host) rc = ensure(ctx, ctx->d_gray, n + 16);
  if (!rc && want_id) rc = ensure(ctx, ctx->d_idimg, 3 * n + 16);
  if (!rc && want_n) {
    rc = ensure(ctx, ctx->d_nimg, 3 * n + 16);
    if (!rc) rc = ensure(ctx, ctx->d_w1map, sizeof(float) * n);
    if (!rc) rc = ensure(ctx, ctx->d_w2map, sizeof(float) * n);
    if (!rc && !from_keys) rc = ensure(ctx, ctx->d_keys, sizeof(unsigned long long) * n);
    if (!rc && !from_keys) rc = ensure(ctx, ctx->d_cov, sizeof(int));
  }
  if (rc) return rc;
  ctx->dbg.active = false;  // (from here on the pinned outputs are being rewritten)
  char* h = ctx->dbg.h.p;
  flame_hip::DebugImageArgs a;
  a.rows = rows, a.cols = cols;
  a.scene_color_scale = params->scene_color_scale, a.flip = params->flip != 0;
  a.k00 = K[0], a.k11 = K[4];
  rc = stage_gray(ctx, img_host, img_device, step_bytes, rows, cols, h + dp.at.gray, ctx->d_gray, &a.gray, &a.gray_step);
  if (rc) return rc;
  if (want_n) {  // (w1 / w2 of the state mesh_state_on selects; the idepth image needs the resident map alone)
    rc = mesh_state_on(ctx, rs);
    if (rc) return rc;
  }
  HIPCHK(ctx, hipEventRecord(ctx->dbg.ev0, rs));
  if (want_n) {
    if (from_keys) {
      LAUNCHCHK(ctx, flame_hip::launch_debug_wmaps((const unsigned long long*)ctx->r_keys.p, (const int32_t*)ctx->r_tris.p, ctx->c.pos,
                                                   ctx->c.w1, ctx->c.w2, (float*)ctx->d_w1map.p, (float*)ctx->d_w2map.p, rows, cols, rs));
    } else {  // the resident map was rasterised with a validity mask: the rasteriser itself, twice, into buffers of this stage
      LAUNCHCHK(ctx, launch_interpolate_mesh(T, (const int32_t*)ctx->r_tris.p, ctx->c.pos, ctx->c.w1, 1.0f, nullptr, nullptr,
                                             (unsigned long long*)ctx->d_keys.p, (float*)ctx->d_w1map.p, (int*)ctx->d_cov.p, rows, cols, rs));
      LAUNCHCHK(ctx, launch_interpolate_mesh(T, (const int32_t*)ctx->r_tris.p, ctx->c.pos, ctx->c.w2, 1.0f, nullptr, nullptr,
                                             (unsigned long long*)ctx->d_keys.p, (float*)ctx->d_w2map.p, (int*)ctx->d_cov.p, rows, cols, rs));
    }
    rc = side_kernels_read_last(ctx);  // (of the canonical pos / w1 / w2)
    if (rc) return rc;
  }
  LAUNCHCHK(ctx, flame_hip::launch_debug_images(a, map, (const float*)ctx->d_w1map.p, (const float*)ctx->d_w2map.p,
                                                want_id ? (uint8_t*)ctx->d_idimg.p : nullptr, want_n ? (uint8_t*)ctx->d_nimg.p : nullptr, rs));
  if (want_id) HIPCHK(ctx, hipMemcpyAsync(h + dp.at.idimg, ctx->d_idimg.p, 3 * n, hipMemcpyDeviceToHost, rs));
  if (want_n) {
    HIPCHK(ctx, hipMemcpyAsync(h + dp.at.nimg, ctx->d_nimg.p, 3 * n, hipMemcpyDeviceToHost, rs));
    HIPCHK(ctx, hipMemcpyAsync(h + dp.at.w1, ctx->d_w1map.p, sizeof(float) * n, hipMemcpyDeviceToHost, rs));
    HIPCHK(ctx, hipMemcpyAsync(h + dp.at.w2, ctx->d_w2map.p, sizeof(float) * n, hipMemcpyDeviceToHost, rs));
  }
  ctx->debug_pending = dp;
  return close_stage(ctx, ctx->dbg);
}

int flame_nltgv2_debug_images_end(flame_nltgv2_ctx* ctx, flame_nltgv2_debug_images_view* out) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_debug_images_end");
  int rc = enter(ctx);
  if (rc) return rc;
  const flame_nltgv2_ctx::DebugPending& dp = ctx->debug_pending;
  if (!out || !ctx->dbg.h.p || !ctx->dbg.active) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  HIPCHK(ctx, hipStreamSynchronize(ctx->raster_stream));
  const char* h = ctx->dbg.h.p;
  out->rows = dp.rows, out->cols = dp.cols;
  out->idepthmap_img = dp.want_idepth ? (const uint8_t*)(h + dp.at.idimg) : nullptr;
  out->normals_img = dp.want_normals ? (const uint8_t*)(h + dp.at.nimg) : nullptr;
  out->w1_map = dp.want_normals ? (const float*)(h + dp.at.w1) : nullptr;
  out->w2_map = dp.want_normals ? (const float*)(h + dp.at.w2) : nullptr;
  out->device_ms = stage_ms(ctx->dbg);
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_debug_images(flame_nltgv2_ctx* ctx, const uint8_t* img_host, const void* img_device, int step_bytes, const float* K,
                              const flame_nltgv2_debug_image_params* params, int rows, int cols, uint8_t* idepthmap_img_out,
                              uint8_t* normals_img_out, float* w1_map_out, float* w2_map_out) {
  int rc = flame_nltgv2_debug_images_begin(ctx, img_host, img_device, step_bytes, K, params, rows, cols);
  if (rc) return rc;
  flame_nltgv2_debug_images_view v;
  rc = flame_nltgv2_debug_images_end(ctx, &v);
  if (rc) return rc;
  const size_t n = (size_t)v.rows * (size_t)v.cols;
  if (idepthmap_img_out && v.idepthmap_img) std::memcpy(idepthmap_img_out, v.idepthmap_img, 3 * n);
  if (normals_img_out && v.normals_img) std::memcpy(normals_img_out, v.normals_img, 3 * n);
  if (w1_map_out && v.w1_map) std::memcpy(w1_map_out, v.w1_map, sizeof(float) * n);
  if (w2_map_out && v.w2_map) std::memcpy(w2_map_out, v.w2_map, sizeof(float) * n);
  return FLAME_NLTGV2_OK;
}

void flame_nltgv2_default_wireframe_params(flame_nltgv2_wireframe_params* p) {
  if (!p) return;
  p->scene_color_scale = 1.0f;  // params.h:109
  p->flip = 0;
  p->validity = 0;
}

// fill + fold + the picture's way out, on the side stream: the second half of a wireframe call, which _end repeats with a larger
// entry buffer where the entries did not fit
static int wireframe_second_half(flame_nltgv2_ctx* ctx, const flame_nltgv2_ctx::WirePending& wp) {
  flame_hip::WireImageArgs a;
  a.rows = wp.rows, a.cols = wp.cols, a.gray = wp.gray, a.gray_step = wp.gray_step;
  a.scene_color_scale = wp.scene_color_scale, a.flip = wp.flip;
  hipStream_t rs = ctx->raster_stream;
  LAUNCHCHK(ctx, flame_hip::launch_wireframe_paint(wp.T, wire_buffers(ctx), a, (uint8_t*)ctx->w_img.p, rs));
  HIPCHK(ctx, hipMemcpyAsync(ctx->wire.h.p + wp.at.img, ctx->w_img.p, 3 * (size_t)wp.rows * (size_t)wp.cols, hipMemcpyDeviceToHost, rs));
  return FLAME_NLTGV2_OK;
}

// The wireframe image on the side stream (see flame_nltgv2.h).
int flame_nltgv2_debug_wireframe_begin(flame_nltgv2_ctx* ctx, const uint8_t* img_host, const void* img_device, int step_bytes,
                                       const uint8_t* tri_valid, const flame_nltgv2_wireframe_params* params, int rows, int cols,
                                       float graph_scale) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_debug_wireframe_begin");
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_graph) return fail(ctx, FLAME_NLTGV2_ERR_NO_GRAPH);
  if (rows <= 0 || cols <= 0 || rows > 32767 || cols > 32767) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);  // (int16 endpoints)
  if (!ctx->tris.current(ctx->topo)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if ((img_host != nullptr) == (img_device != nullptr) || step_bytes < cols || !params) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (params->validity < 0 || params->validity > 2 || (tri_valid != nullptr) != (params->validity == 1)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const int32_t T = ctx->tris.T();
  if (params->validity == 2 && !ctx->tris.validity_current(ctx->topo)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  // every draw visits at most max(rows, cols) pixels: the entries, their offsets and the draw ids are 32-bit
  if ((uint64_t)3 * (uint64_t)T * (uint64_t)(rows > cols ? rows : cols) >= (1ull << 31)) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  const size_t n = (size_t)rows * (size_t)cols;
  hipStream_t rs = ctx->raster_stream;
  flame_nltgv2_ctx::WirePending wp;
  wp.rows = rows, wp.cols = cols, wp.flip = params->flip != 0, wp.T = T, wp.scene_color_scale = params->scene_color_scale;
  wp.at = wire_layout(rows, cols, img_host != nullptr);
  rc = open_stage(ctx, ctx->wire, wp.at.total);
  if (rc) return rc;
  size_t want = 2 * n, grown = ctx->w_last_total + ctx->w_last_total / 4 + 1;
  if (grown > want) want = grown;
  if (want < ctx->w_cap) want = ctx->w_cap;  // (never shrinks)
  if (want > 0xffffffffull) want = 0xffffffffull;
  rc = ensure(ctx, ctx->w_draws, sizeof(flame_hip::WireDraw) * 3 * (size_t)T);
  if (!rc) rc = ensure(ctx, ctx->w_cnt, sizeof(uint32_t) * n);
  if (!rc) rc = ensure(ctx, ctx->w_off, sizeof(uint32_t) * n);
  if (!rc) rc = ensure(ctx, ctx->w_fill, sizeof(uint32_t) * n);
  if (!rc) rc = ensure(ctx, ctx->w_entries, sizeof(uint64_t) * want);
  if (!rc) rc = ensure(ctx, ctx->w_counts, flame_hip::kWireCounts * sizeof(int));
  if (!rc) rc = ensure(ctx, ctx->w_img, 3 * n + 16);
  if (!rc && img_host) rc = ensure(ctx, ctx->w_gray, n + 16);
  if (!rc && tri_valid) rc = ensure(ctx, ctx->w_tvalid, (size_t)T + 16);
  if (rc) return rc;
  ctx->w_cap = want;
  ctx->wire.active = false;  // (from here on the pinned outputs are being rewritten)
  char* h = ctx->wire.h.p;
  rc = stage_gray(ctx, img_host, img_device, step_bytes, rows, cols, h + wp.at.gray, ctx->w_gray, &wp.gray, &wp.gray_step);
  if (rc) return rc;
  const uint8_t* d_tv = nullptr;
  if (params->validity == 1 && T > 0) {  // (pageable memory: the copy holds the host until the bytes have left the caller's array)
    HIPCHK(ctx, hipMemcpyAsync(ctx->w_tvalid.p, tri_valid, (size_t)T, hipMemcpyHostToDevice, rs));
    d_tv = (const uint8_t*)ctx->w_tvalid.p;
  } else if (params->validity == 2) {
    d_tv = (const uint8_t*)ctx->m_tvalid.p;
  }
  rc = mesh_state_on(ctx, rs);
  if (rc) return rc;
  HIPCHK(ctx, hipEventRecord(ctx->wire.ev0, rs));
  // the setup kernel is the last reader of the canonical pos / x (see interpolate_mesh_begin): ev_raster_done goes right behind it
  LAUNCHCHK(ctx, flame_hip::launch_wireframe_lists(T, (const int32_t*)ctx->r_tris.p, ctx->c.pos, ctx->c.x, graph_scale, d_tv, wire_buffers(ctx), rows,
                                                   cols, ctx->ev_raster_done, rs));
  ctx->raster_inflight = true;
  HIPCHK(ctx, hipMemcpyAsync(h + wp.at.counts, ctx->w_counts.p, flame_hip::kWireCounts * sizeof(int), hipMemcpyDeviceToHost, rs));
  rc = wireframe_second_half(ctx, wp);
  if (rc) return rc;
  ctx->wire_pending = wp;
  return close_stage(ctx, ctx->wire);
}

int flame_nltgv2_debug_wireframe_end(flame_nltgv2_ctx* ctx, flame_nltgv2_wireframe_view* out) {
  flame_hip::RoctxRange roctx_range_("flame_nltgv2_debug_wireframe_end");
  int rc = enter(ctx);
  if (rc) return rc;
  const flame_nltgv2_ctx::WirePending wp = ctx->wire_pending;
  if (!out || !ctx->wire.h.p || !ctx->wire.active) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  HIPCHK(ctx, hipStreamSynchronize(ctx->raster_stream));
  int32_t counts[flame_hip::kWireCounts];
  std::memcpy(counts, ctx->wire.h.p + wp.at.counts, sizeof(counts));
  const size_t total = (size_t)(uint32_t)counts[flame_hip::kWireTotal];
  out->device_ms = stage_ms(ctx->wire);
  out->refilled = 0;
  if (total > ctx->w_cap) {  // the entries did not fit: a larger buffer, then fill and fold once more (the records, cnt and offsets stand)
    const size_t want = total + total / 4 + 1;
    rc = ensure(ctx, ctx->w_entries, sizeof(uint64_t) * want);
    if (rc) return rc;
    ctx->w_cap = want;
    HIPCHK(ctx, hipEventRecord(ctx->wire.ev0, ctx->raster_stream));
    rc = wireframe_second_half(ctx, wp);
    if (rc) return rc;
    HIPCHK(ctx, hipEventRecord(ctx->wire.ev1, ctx->raster_stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->raster_stream));
    out->device_ms += stage_ms(ctx->wire);
    out->refilled = 1;
  }
  ctx->w_last_total = total;
  out->rows = wp.rows, out->cols = wp.cols;
  out->wireframe_img = (const uint8_t*)(ctx->wire.h.p + wp.at.img);
  out->lines_drawn = counts[flame_hip::kWireDrawn], out->lines_skipped = counts[flame_hip::kWireSkipped];
  out->entries = (int64_t)total;
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_debug_wireframe(flame_nltgv2_ctx* ctx, const uint8_t* img_host, const void* img_device, int step_bytes,
                                 const uint8_t* tri_valid, const flame_nltgv2_wireframe_params* params, int rows, int cols,
                                 float graph_scale, uint8_t* wireframe_img_out, int32_t* lines_drawn_out, int32_t* lines_skipped_out) {
  int rc = flame_nltgv2_debug_wireframe_begin(ctx, img_host, img_device, step_bytes, tri_valid, params, rows, cols, graph_scale);
  if (rc) return rc;
  flame_nltgv2_wireframe_view v;
  rc = flame_nltgv2_debug_wireframe_end(ctx, &v);
  if (rc) return rc;
  if (wireframe_img_out) std::memcpy(wireframe_img_out, v.wireframe_img, 3 * (size_t)v.rows * (size_t)v.cols);
  if (lines_drawn_out) *lines_drawn_out = v.lines_drawn;
  if (lines_skipped_out) *lines_skipped_out = v.lines_skipped;
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_photo_set_images(flame_nltgv2_ctx* ctx, const uint8_t* ref, const uint8_t* cmp, int rows, int cols,
                                  int step_bytes) {
  int rc = enter(ctx);
  if (rc) return rc;
  PhotoStale stale_{ctx};  // (photo_err no longer describes what this call leaves)
  if (!ref || !cmp || rows < 2 || cols < 2 || step_bytes < cols) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  // the last row ends at its cols-th byte: the caller's buffer need not hold that row's padding
  const size_t bytes = (size_t)(rows - 1) * (size_t)step_bytes + (size_t)cols;
  if (ctx->merr_reads_images) {  // (a map_error_begin without its _end may still read the images that are about to be replaced)
    HIPCHK(ctx, hipStreamSynchronize(ctx->raster_stream));
    ctx->merr_reads_images = false;
  }
  HIPCHK(ctx, wait_solver_stream(ctx));
  rc = ensure(ctx, ctx->img_ref, bytes + 16);
  if (!rc) rc = ensure(ctx, ctx->img_cmp, bytes + 16);
  if (rc) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->img_ref.p, ref, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(ctx->img_cmp.p, cmp, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, wait_solver_stream(ctx));
  ctx->img_rows = rows, ctx->img_cols = cols, ctx->img_step = step_bytes;
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_photo_residual(flame_nltgv2_ctx* ctx, const float* KRKinv, const float* Kt, float graph_scale,
                                int border, float* err_out) {
  int rc = enter(ctx);
  if (rc) return rc;
  PhotoStale stale_{ctx};  // (it writes photo_err with the caller's target, not the standing one)
  if (!ctx->have_graph) return fail(ctx, FLAME_NLTGV2_ERR_NO_GRAPH);
  if (!KRKinv || !Kt || !err_out || border < 1 || ctx->img_rows == 0) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  rc = ensure_canon(ctx);
  if (rc) return rc;
  const size_t fV = sizeof(float) * (size_t)ctx->L.V;
  rc = ensure(ctx, ctx->photo_err, fV);
  if (rc) return rc;
  PhotoGeometry geo;
  std::memcpy(geo.KRKinv, KRKinv, sizeof(geo.KRKinv));
  std::memcpy(geo.Kt, Kt, sizeof(geo.Kt));
  LAUNCHCHK(ctx, launch_photo_residual(ctx->c, graph_scale, geo, (const uint8_t*)ctx->img_ref.p,
                                       (const uint8_t*)ctx->img_cmp.p, ctx->img_rows, ctx->img_cols, ctx->img_step,
                                       border, (float*)ctx->photo_err.p, ctx->stream));
  if (fV) HIPCHK(ctx, hipMemcpyAsync(err_out, ctx->photo_err.p, fV, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, wait_solver_stream(ctx));
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_photo_fuse(flame_nltgv2_ctx* ctx, const float* KRKinv, const float* Kt, float graph_scale, int border,
                            int enable) {
  int rc = enter(ctx);
  if (rc) return rc;
  PhotoStale stale_{ctx};  // (photo_err no longer describes what this call leaves)
  if (!enable) {
    ctx->photo_fused = false;
    return FLAME_NLTGV2_OK;
  }
  if (!ctx->have_graph) return fail(ctx, FLAME_NLTGV2_ERR_NO_GRAPH);
  if (!KRKinv || !Kt || border < 1 || ctx->img_rows == 0) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  HIPCHK(ctx, wait_solver_stream(ctx));
  rc = ensure(ctx, ctx->photo_err, sizeof(float) * (size_t)ctx->L.V);
  if (rc) return rc;
  std::memcpy(ctx->photo_geo.KRKinv, KRKinv, sizeof(ctx->photo_geo.KRKinv));
  std::memcpy(ctx->photo_geo.Kt, Kt, sizeof(ctx->photo_geo.Kt));
  ctx->photo_scale = graph_scale, ctx->photo_border = border;
  ctx->photo_fused = true;
  return FLAME_NLTGV2_OK;
}

int flame_nltgv2_photo_residual_last(flame_nltgv2_ctx* ctx, float* err_out) {
  int rc = enter(ctx);
  if (rc) return rc;
  if (!ctx->have_graph) return fail(ctx, FLAME_NLTGV2_ERR_NO_GRAPH);
  if (!ctx->photo_fused || !err_out) return fail(ctx, FLAME_NLTGV2_ERR_INVALID_ARG);
  if (ctx->pending.active) {
    rc = finish(ctx);
    if (rc) return rc;
  }
  if (!ctx->photo_fresh) {  // no run since the graph, the state, the images or the target changed: the stand-alone sweep, never stale values
    rc = ensure_canon(ctx);
    if (!rc) rc = enqueue_photo_sweep(ctx, false);
    if (rc) return rc;
  }
  const size_t fV = sizeof(float) * (size_t)ctx->L.V;
  if (fV) HIPCHK(ctx, hipMemcpyAsync(err_out, ctx->photo_err.p, fV, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, wait_solver_stream(ctx));
  return FLAME_NLTGV2_OK;
}


}  // extern "C"
