/*
 * flame_nltgv2.h -- C-ABI of libflame_nltgv2_hip.so: the MI355X (gfx950) implementation of FLaME's
 * NLTGV2-L1 primal-dual graph regularizer.
 *
 * This is the drop-in boundary for ONE path of robustrobotics/flame:
 *   src/flame/optimizers/nltgv2_l1_graph_regularizer.{h,cc}   (namespace
 *   flame::optimizers::nltgv2_l1_graph_regularizer), called from src/flame/flame.cc:104 (solver
 *   thread) and flame.cc:2172-2173 (cost statistics).
 * Every entry point below names the reference interface it replaces.  Plain pointers and sizes
 * only; no C++/torch types.  All pointers are HOST memory unless the name says "device".
 *
 * Conventions
 *   - All functions return 0 (FLAME_NLTGV2_OK) on success or a negative flame_nltgv2_status.
 *     Nothing here aborts or throws (the reference's FLAME_ASSERT calls exit(1), assert.h:111).
 *   - A context is NOT thread-safe; use one per solver thread.  The caller provides the
 *     graph_mtx_-equivalent (flame.h:539; lock sites flame.cc:103, 302, 309, 329, 365).
 *   - Edge k is directed src[k] -> dst[k] == (boost::source, boost::target) of the k-th edge of
 *     boost::edges(graph) (nltgv2...cc:91-96).  Orientation is semantic (the operator uses the
 *     SOURCE vertex's w_bar only, cc:100-101,129-133); edge order fixes the floating-point
 *     accumulation order of primalStep (cc:120-142) and is honoured exactly.
 *   - There is no CPU fallback: every compute entry point fails with
 *     FLAME_NLTGV2_ERR_NO_DEVICE / _HIP when no gfx950 device is usable.
 */
#ifndef FLAME_NLTGV2_H_
#define FLAME_NLTGV2_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLAME_NLTGV2_ABI_VERSION 7 /* 7: flame_nltgv2_run_open, flame_nltgv2_iterations, FLAME_NLTGV2_OPT_MESH_STATE; 6: the region-per-workgroup form left the library (FLAME_NLTGV2_OPT_PERSISTENT = 7 is an invalid argument, last_run_path 8 never occurs, the two info words it used are reserved; the struct's layout is unchanged); 5: flame_nltgv2_info grew (last_run_waves_per_cu, ..., replays_per_step); flame_nltgv2_stream_wait_run, _runs_in_flight */

typedef struct flame_nltgv2_ctx flame_nltgv2_ctx;

typedef enum flame_nltgv2_status {
  FLAME_NLTGV2_OK = 0,
  FLAME_NLTGV2_ERR_INVALID_ARG = -1, /* NULL pointer, negative size, index out of range, self loop */
  FLAME_NLTGV2_ERR_NO_DEVICE = -2,   /* no HIP device / wrong device ordinal */
  FLAME_NLTGV2_ERR_HIP = -3,         /* a HIP runtime call failed (see flame_nltgv2_last_hip_error) */
  FLAME_NLTGV2_ERR_NO_GRAPH = -4,    /* compute call before flame_nltgv2_upload_graph */
  FLAME_NLTGV2_ERR_NAN = -5,         /* a dual variable became NaN/Inf: the condition on which the
                                        reference's FLAME_ASSERT(!std::isnan(new_q)) fires
                                        (nltgv2...h:174).  Reported once by the call that finds it; the state
                                        stays readable (q was clamped to +-1 where it happened) and usable. */
  FLAME_NLTGV2_ERR_OOM = -6,
  FLAME_NLTGV2_ERR_TIMEOUT = -7,     /* persistent run: a bounded neighbour wait expired.  run()/sync() normally hide
                                        this: the run's results go to second copies of the state, so the state is
                                        rolled back and the steps are redone with one launch per step (get_info:
                                        timeouts_recovered); runs chained with run_async() are covered too (the chain's
                                        starting state is copied aside once, the chain replayed).  Returned only if that
                                        recovery itself is impossible */
  FLAME_NLTGV2_ERR_ASSERT = -8       /* flame_stereo.h: an input on which the reference's FLAME_ASSERT would
                                        exit(1) (assert.h:111) */
} flame_nltgv2_status;

/* == struct Params, nltgv2_l1_graph_regularizer.h:121-129 (same fields, order and defaults). */
typedef struct flame_nltgv2_params {
  float data_factor; /* 0.1   lambda */
  float step_x;      /* 0.001 primal step tau */
  float step_q;      /* 125   dual step sigma */
  float theta;       /* 0.25  extra-gradient step */
  float x_min;       /* 0     feasible set */
  float x_max;       /* 10 */
} flame_nltgv2_params;

/* Flat (structure-of-arrays) image of a reference Graph (h:107-112): VertexData (h:74-90) and
 * EdgeData (h:95-102; `valid` is syncGraph bookkeeping, flame.cc:2080-2118, and has no image here).
 * Used read-only by upload and write-only by download; in a download any pointer may be NULL to
 * skip that array. */
typedef struct flame_nltgv2_graph {
  int32_t V, E;
  float* pos; /* 2*V floats, (x,y) interleaved: VertexData::pos */
  float *x, *w1, *w2;
  float *x_bar, *w1_bar, *w2_bar;
  float *x_prev, *w1_prev, *w2_prev; /* upload: may be NULL (step() overwrites them, cc:35-42) */
  float *data_term, *data_weight;
  int32_t *src, *dst;
  float *alpha, *beta;
  float *q1, *q2, *q3;
} flame_nltgv2_graph;

void flame_nltgv2_default_params(flame_nltgv2_params* p);

/* Context lifetime.  `device` is the HIP device ordinal (one process / one context per GPU).
 * Replaces: the Graph object owned by Flame (flame.h:536) as the holder of solver state. */
int flame_nltgv2_create(flame_nltgv2_ctx** out, int device);
int flame_nltgv2_destroy(flame_nltgv2_ctx* ctx);

/* Run all subsequent work of this context on the caller's hipStream_t (pass NULL to return to the
 * context's own stream).  Lets a host framework time / order the solver with its own events. */
int flame_nltgv2_set_stream(flame_nltgv2_ctx* ctx, void* hip_stream);

/* Topology + weights + state -> device.  Replaces the graph (re)construction of
 * Flame::syncGraph (flame.cc:2030-2121: add_vertex / add_edge / remove_*), after which the packed
 * device layout is rebuilt.  Buffers are reused and grown geometrically across calls. */
int flame_nltgv2_upload_graph(flame_nltgv2_ctx* ctx, const flame_nltgv2_graph* g);

/* Per-frame graph synchronisation with WARM START: the graph-edit part of Flame::syncGraph
 * (flame.cc:1985-2121) and the vertex removal of Flame::projectGraph (flame.cc:1923-1931).  The caller
 * passes the vertex set of the new frame (stable feature ids, positions, data terms) and the edges of its
 * new triangulation; vertices/edges that survive keep their primal/dual state (an edge also keeps its old
 * orientation, as boost::edge(u,v) finds it either way, flame.cc:2094-2100), new ones start as the
 * reference initialises them.  Order of the resulting edge list: surviving edges in their previous
 * relative order, then new edges in triangulator order -- what boost::edges() yields after the
 * reference's erase/add_edge sequence.  (The reference's VERTEX order is BGL hash order and therefore
 * unspecified; here it is the caller's.)  Feature ids default to the vertex index after upload_graph. */
typedef struct flame_nltgv2_sync_input {
  int32_t V;
  const int32_t* feat_id;   /* [V] unique, >= 0, stable across frames (Flame::feat_to_vtx_, flame.h:542-543) */
  const float* pos;         /* [2V] positions in the new frame (after projectGraph re-projection) */
  const float* data_term;   /* [V] feat.idepth_mu / graph_scale */
  const float* data_weight; /* [V] */
  const float* init_x;      /* [V] x of NEW vertices (flame.cc:2160-2162); NULL = data_term */
  int32_t E;
  const int32_t* edges;     /* [2E] triangulator->edges(): pairs of indices into the new vertex list */
  int32_t check_sticky_obstacles; /* params.check_sticky_obstacles, flame.cc:2011 */
  float sticky_threshold;         /* 0.25f in the reference */
  float init_graph_scale;         /* > 0: a NEW vertex whose init_x is NaN (no valid prediction) starts at the mean of
                                   * x*scale over its neighbours with data_weight > 0, / scale -- all means formed from
                                   * the neighbours' values as they stand after the vertex pass (survivors: their x; new:
                                   * init_x, or data_term where that is NaN too), neighbours in ascending edge id --, or at
                                   * data_term when it has none (init_with_prediction, flame.cc:2133-2158).  0: init_x is
                                   * taken as it is. */
  int32_t edges_unique;           /* != 0: the caller vouches that `edges` lists every vertex pair at most once (what
                                   * flame_delaunay_triangulate -- and the reference's Triangle -- return): the search for
                                   * duplicates among the new edges is skipped.  0 (default): pairs that repeat are dropped as
                                   * boost::edge() / add_edge do it in the reference (flame.cc:2094-2100), the first one stays */
  int32_t init_from_map;          /* != 0 (init_x must be NULL, init_graph_scale > 0): a NEW vertex starts at the prediction the
                                   * reference reads from its dense map, idepthmap(pos.y + 0.5f, pos.x + 0.5f) / graph_scale
                                   * (init_with_prediction, flame.cc:2131) -- looked up ON THE DEVICE in the map the context's last
                                   * flame_nltgv2_interpolate_mesh[_begin] left there (no map yet, or a position outside it: NaN, i.e.
                                   * the neighbours' mean as above).  Saves the host gather and the upload of init_x every frame */
} flame_nltgv2_sync_input;
int flame_nltgv2_sync_graph(flame_nltgv2_ctx* ctx, const flame_nltgv2_sync_input* in);
/* The same sync in two halves, so that the solver keeps iterating while the frame's graph is prepared (the reference's solver thread
 * stands still through all of Flame::syncGraph: it holds graph_mtx_, flame.cc:103, 309-318):
 *   prepare  checks the inputs (same errors as sync_graph), copies them, and enqueues the construction of the new topology on a
 *            side stream -- it only READS the live graph; returns at once.  The caller's arrays are free on return.
 *   commit   waits for that construction, settles the runs enqueued meanwhile, swaps the new topology in and moves the state
 *            (what sync_graph does after its index maps).  sync_graph == prepare; commit.  Whatever of this does not need the solver
 *            stopped is enqueued beside or behind the runs still in flight (the new graph's per-slot and per-lane tables on the side
 *            stream into spare buffers; the state's unpack and its gather into spare arrays behind the runs): the solver's stream
 *            stands empty for ~50 us at 640x480.
 * Between the two only run / run_async / sync and read-outs (download_state, export, get_info) may be called; upload_graph,
 * sync_graph, set_feature_ids or another prepare cancel the prepared sync (commit then returns FLAME_NLTGV2_ERR_INVALID_ARG). */
int flame_nltgv2_sync_prepare(flame_nltgv2_ctx* ctx, const flame_nltgv2_sync_input* in);
int flame_nltgv2_sync_commit(flame_nltgv2_ctx* ctx);
/* Declares the feature ids of the vertices of a graph brought in with flame_nltgv2_upload_graph (V ints,
 * unique): Flame::vtx_to_feat_ (flame.h:542-543). */
int flame_nltgv2_set_feature_ids(flame_nltgv2_ctx* ctx, const int32_t* feat_id);
/* Current edge list / feature ids (E, E, V ints; any pointer may be NULL). */
int flame_nltgv2_get_topology(flame_nltgv2_ctx* ctx, int32_t* src, int32_t* dst, int32_t* feat_id);
/* Vertex and edge count of the current graph (after a sync: V as passed, E = surviving + new edges). */
int flame_nltgv2_graph_size(flame_nltgv2_ctx* ctx, int32_t* V, int32_t* E);

/* Flame::projectGraph (flame.cc:1888-1905) on the device state: every vertex is re-projected into the new
 * frame with EpipolarGeometry::project(pos, x*graph_scale, &u_new, &idepth_new)
 * (stereo/epipolar_geometry.h:152-180); pos and x = idepth_new/graph_scale are written back; keep_out[v] = 0
 * where the reference would remove the vertex (outside the valid region, cv::Rect_<float>::contains, or
 * idepth_new < 0; flame.cc:1902-1906).  pos_out (2V floats, may be NULL) receives the new positions for the
 * host's re-triangulation.  Removal itself happens in the following flame_nltgv2_sync_graph, as in the
 * reference (projectGraph is always followed by syncGraph, flame.cc:301-318).
 * All matrices row-major 3x3 as EpipolarGeometry holds them; q = (w,x,y,z). */
typedef struct flame_nltgv2_projection {
  float K[9], Kinv[9], KRKinv[9];
  float q_ref_to_cmp[4];
  float t_ref_to_cmp[3];
  float region_x, region_y, region_w, region_h; /* valid_region, flame.cc:1881-1884 */
} flame_nltgv2_projection;
int flame_nltgv2_project_graph(flame_nltgv2_ctx* ctx, const flame_nltgv2_projection* pr, float graph_scale,
                               uint8_t* keep_out, float* pos_out);
/* The rescale_data block of Flame::update (flame.cc:328-351): new_scale = mean(data_term*graph_scale);
 * x, x_bar, x_prev, data_term *= graph_scale/new_scale; params->data_factor *= new_scale/graph_scale.
 * (The reference forms the mean over a hash set, i.e. in an unspecified order; here in a fixed order -- 1024 strided partial sums
 * combined pairwise -- that the checker restates: oracle/photometric_oracle.c strided_tree_sum.) */
int flame_nltgv2_rescale_data(flame_nltgv2_ctx* ctx, float graph_scale, float* new_graph_scale, flame_nltgv2_params* params);

/* Per-frame refresh of data_term/data_weight for an unchanged topology (flame.cc:1985-2018). */
int flame_nltgv2_update_data(flame_nltgv2_ctx* ctx, const float* data_term, const float* data_weight);

/* State only (x,w,x_bar,w_bar,q; NULL members are left untouched) for an unchanged topology,
 * e.g. after projectGraph re-projected x (flame.cc:1898-1900) or rescale_data (flame.cc:328-351). */
int flame_nltgv2_upload_state(flame_nltgv2_ctx* ctx, const flame_nltgv2_graph* state);

/* n_iters x step(params, graph) (nltgv2...cc:33-49), state resident on the device; returns after
 * the work has completed.  Replaces the body of the solver thread loop, flame.cc:101-107. */
int flame_nltgv2_run(flame_nltgv2_ctx* ctx, const flame_nltgv2_params* p, int n_iters);
/* Same, but only enqueues; flame_nltgv2_sync waits and reports the NaN flag. */
int flame_nltgv2_run_async(flame_nltgv2_ctx* ctx, const flame_nltgv2_params* p, int n_iters);
int flame_nltgv2_sync(flame_nltgv2_ctx* ctx);
/* Same as run, additionally returns the device time of the n_iters steps measured with HIP events
 * on the stream the kernels run on (what bench.py reports). */
int flame_nltgv2_run_timed(flame_nltgv2_ctx* ctx, const flame_nltgv2_params* p, int n_iters, float* elapsed_ms);

/* The individually callable pieces of a step, each one kernel sweep over the canonical SoA state:
 *   save_prev           step()'s x_prev/w_prev copy                 cc:35-42
 *   dual_step           internal::dualStep                          cc:89-114
 *   primal_step         internal::primalStep (+ proxL1)             cc:116-154
 *   extragradient_step  internal::extraGradientStep                 cc:156-174
 * step == save_prev; dual; primal; extragradient == flame_nltgv2_run(ctx,p,1). */
int flame_nltgv2_save_prev(flame_nltgv2_ctx* ctx);
int flame_nltgv2_dual_step(flame_nltgv2_ctx* ctx, const flame_nltgv2_params* p);
int flame_nltgv2_primal_step(flame_nltgv2_ctx* ctx, const flame_nltgv2_params* p);
int flame_nltgv2_extragradient_step(flame_nltgv2_ctx* ctx, const flame_nltgv2_params* p);
int flame_nltgv2_step(flame_nltgv2_ctx* ctx, const flame_nltgv2_params* p);

/* smoothnessCost (cc:51-71) and dataCost (cc:73-85); cost() (h:149-151) is their sum.  The device forms the
 * addends exactly as the reference does, the host adds them sequentially in float in edge / vertex order: the
 * results equal the reference's to the last bit (for the caller's vertex order; the reference's is BGL hash order). */
int flame_nltgv2_costs(flame_nltgv2_ctx* ctx, const flame_nltgv2_params* p, float* smoothness, float* data);

/* Device -> host copy of the solver state in the caller's original vertex/edge order.  Replaces
 * the read-back loop flame.cc:372-380 (and is the checkpoint format). */
int flame_nltgv2_download_state(flame_nltgv2_ctx* ctx, flame_nltgv2_graph* out);

/* Writes scale * x[v] (original vertex order, V floats) into DEVICE memory `dst_device`, on the
 * context's stream: the `vtx.x * graph_scale_` of flame.cc:377, kept on the GPU so that a
 * multi-GPU host can hand the buffer straight to an RCCL gather. */
int flame_nltgv2_export_idepth_device(flame_nltgv2_ctx* ctx, void* dst_device, float scale);
/* Same, enqueue only: ordered on the context's stream (see flame_nltgv2_set_stream), no host wait -- a
 * collective enqueued on the same stream afterwards reads the finished buffer. */
int flame_nltgv2_export_idepth_device_async(flame_nltgv2_ctx* ctx, void* dst_device, float scale);
/* Standing export target: while `dst_device` is set (NULL = off), every run()/run_async() also leaves
 * scale * x[v] there (V floats, original vertex order) as part of the same launch -- the persistent kernels write
 * it in their epilogue, so a per-step result gather needs no extra kernel between two runs. */
int flame_nltgv2_set_export_target(flame_nltgv2_ctx* ctx, void* dst_device, float scale);
/* Makes another stream of the caller (`hip_stream`, a hipStream_t; not the context's own) wait for everything enqueued on the context's
 * stream so far -- the consumer side of the standing export target (the read-back of flame.cc:372-380 left on the device): a collective
 * on `hip_stream` then reads the finished row.  No
 * host wait.  Called right behind run_async() it costs the solver's stream nothing: the run's launch carries the event as its own
 * completion signal, where an event recorded by the caller is one more operation between two solver launches on an in-order queue
 * (5 us each at 640x480).  FLAME_NLTGV2_ERR_INVALID_ARG for a null stream or the context's own. */
int flame_nltgv2_stream_wait_run(flame_nltgv2_ctx* ctx, void* hip_stream);
/* How many of the last two runs enqueued with run_async() the device has not finished yet (0, 1 or 2): what a free-running solver
 * thread (flame.cc:99-112) paces itself by -- it keeps two runs in flight, so that the device never waits for the host between two of them, without ever
 * blocking in the context (include/flame_hip/solver_loop.hpp, device mode).  Does not wait, does not check the runs' results (sync()
 * does), and costs the solver's stream nothing where the launch carries the event. */
int flame_nltgv2_runs_in_flight(flame_nltgv2_ctx* ctx, int32_t* n_out);
/* A run that goes on until the caller needs the state -- the reference's solver thread is `while (true) step()` (flame.cc:99-112), and a
 * frame loop that enqueues rounds of N iterations pays each round's start-up and the gap between two launches (12 us per round at 640x480)
 * and waits for up to two rounds whenever it needs the state.  run_open enqueues ONE launch of at most max_iters (even) iterations; the next
 * call that needs the solver settled (sync, download_state, project_graph, sync_commit, a further run, ...) asks it to stop: one patch reads the
 * request and publishes the iteration every patch leaves at (~0.15 ms later at 640x480).  *opened = 0: not applicable here (a graph beyond ONE
 * launch of the patch-per-wave or the two-half-edges form at <= 20 / 14 patches per CU, record verification or the probe on) -- NOTHING was
 * enqueued and nothing waited for, use run_async.  How many iterations an open run did is known once it is settled: flame_nltgv2_iterations.  An expired open run is taken back
 * and redone like any other.  flame_nltgv2_stream_wait_run / _runs_in_flight see it like a run_async (in flight until it has been stopped). */
int flame_nltgv2_run_open(flame_nltgv2_ctx* ctx, const flame_nltgv2_params* p, int max_iters, int32_t* opened);
/* Iterations applied to the state by all runs of this context so far (run, run_async: counted when enqueued; an open run: when settled --
 * *open_in_flight = 1 says one is not yet counted).  Never waits. */
int flame_nltgv2_iterations(flame_nltgv2_ctx* ctx, int64_t* total, int32_t* open_in_flight);

/* Mesh -> dense inverse-depth map, the step right after the solver each frame:
 * utils::interpolateMesh (utils/image_utils.cc:373-396) over utils::DrawShadedTriangleBarycentric
 * (utils/rasterization.cc:164-246), as called at flame.cc:409-415, plus the coverage count of
 * flame.cc:428-437.  `triangles`: T index triples in the reference triangulator's order and winding
 * (utils::Delaunay::triangles()); later triangles win on shared pixels, exactly like the reference's
 * sequential loop.  Output: rows*cols floats, NaN where no triangle covers the pixel.
 *   interpolate_mesh         vertices = the context's graph: pos and x*graph_scale straight from the device
 *                            state (flame.cc:372-380 without the host round trip)
 *   interpolate_mesh_arrays  the reference signature: explicit vertices / values / validity arrays */
int flame_nltgv2_interpolate_mesh(flame_nltgv2_ctx* ctx, const int32_t* triangles, int32_t T, const uint8_t* tri_valid,
                                  int rows, int cols, float graph_scale, float* idepthmap_out, int32_t* coverage_out);
/* interpolate_mesh in two halves, so that the solver iterates while the map is rasterised and copied out: begin settles the runs,
 * brings the state to its canonical arrays and enqueues rasteriser + device-to-host copy on a side stream, returning at once (the
 * caller goes on with run_async); end waits for that stream.  *map_out points at the context's pinned rows*cols floats (valid
 * until the next begin); the map also stays on the device for flame_nltgv2_sync_input.init_from_map.  A begin that runs out of
 * pinned memory (FLAME_NLTGV2_ERR_OOM) leaves the map of an earlier begin, and its pending end, as they are. */
int flame_nltgv2_interpolate_mesh_begin(flame_nltgv2_ctx* ctx, const int32_t* triangles, int32_t T, const uint8_t* tri_valid,
                                        int rows, int cols, float graph_scale);
int flame_nltgv2_interpolate_mesh_end(flame_nltgv2_ctx* ctx, const float** map_out, int32_t* coverage_out);
int flame_nltgv2_interpolate_mesh_arrays(flame_nltgv2_ctx* ctx, const int32_t* triangles, int32_t T,
                                         const float* vertices_xy, const float* values, int32_t V,
                                         const uint8_t* vtx_valid, const uint8_t* tri_valid, int rows, int cols,
                                         float* img_out, int32_t* coverage_out);

/* Mesh outputs: what Flame::update() makes of the graph between the solver and its getters (flame.cc:372-415; getters
 * flame.h:207-250) -- vtx_idepths_ (flame.cc:377), getVertexNormals (the triangle-based overload, flame.cc:2554-2641), tri_validity_ from
 * obliqueTriangleFilter / edgeLengthFilter / idepthTriangleFilter (flame.cc:2207-2361, applied in that order, flame.cc:389-407) and the
 * FILTERED dense map (getFilteredInverseDepthMap, flame.h:217-228: interpolateMesh with tri_validity_) -- from the resident state, on the
 * context's side stream, beside the running solver.  The arithmetic is the reference's scalar float code operation for operation
 * (tests/mesh_ref.py restates it; device and checker agree bit for bit).  Pinned down here, since Eigen is not part of this tree:
 *   - P = (Kinv * (pos.x, pos.y, 1)) / idepth: the full 3x3 product, then three divisions; every sum of three products -- matrix rows,
 *     dot products, squared norms -- is taken left to right, (a + b) + c, as everywhere else in this library (flame_nltgv2_project_graph);
 *   - normalize() leaves a vector whose squared norm is not > 0 unchanged (Eigen >= 3.3), so a degenerate triangle has a zero normal;
 *   - every comparison with a NaN is false: a NaN never clears validity; idepth == 0 gives infinite points and plain IEEE results;
 *     the reference's FLAME_ASSERT(max_id >= min_id) (flame.cc:2263) is not reproduced: nothing aborts;
 *   - the angle test `fabs(acos(d)) > oblique_normal_thresh` (flame.cc:2252-2253) is made on d itself: no arc cosine runs on the device
 *     (see flame_nltgv2_oblique_cos_bound);
 *   - a vertex normal is the reference's SEQUENTIAL running mean over its triangles in ascending triangle index,
 *     n = normalize((count * n + normal_t) / (count + 1)) (flame.cc:2614-2630), triangles with a corner idepth <= 0 skipped
 *     (flame.cc:2585); a vertex without a contributing triangle has the normal (0, 0, 0).  Normals are OUTWARD (delta2 x delta1,
 *     flame.cc:2611); the filter's normal is the inward one (flame.cc:2244).
 *
 * == the mesh filter fields of struct Params, params.h:69-85 (same defaults). */
typedef struct flame_nltgv2_mesh_filter_params {
  int32_t do_oblique_triangle_filter; /* 1        params.h:70 */
  float oblique_normal_thresh;        /* 1.39626  params.h:71  angle between inward normal and viewing ray, radians (80 deg) */
  float oblique_idepth_diff_factor;   /* 0.35     params.h:73  (max_id - min_id) / max_id, flame.cc:2265 */
  float oblique_idepth_diff_abs;      /* 0.1      params.h:76  max_id - min_id, flame.cc:2269 */
  int32_t do_edge_length_filter;      /* 1        params.h:80 */
  float edge_length_thresh;           /* 0.333    params.h:81  fraction of the map WIDTH: thresh2 = (thresh * cols)^2, flame.cc:2297-2298 */
  int32_t do_idepth_triangle_filter;  /* 1        params.h:84 */
  float min_triangle_idepth;          /* 0.01     params.h:85  mean corner idepth, flame.cc:2346-2347 */
} flame_nltgv2_mesh_filter_params;
void flame_nltgv2_default_mesh_filter_params(flame_nltgv2_mesh_filter_params* p);

/* The smallest float D in [-1, 1] with (float)acos((double)D) <= thresh, found by bisection over the floats (HOST code, double libm, no
 * context, no GPU).  The reference rejects a triangle when fabs(acos(d)) > thresh (flame.cc:2252-2253); the arc cosine is monotone, so
 * that is `d >= -1 && d <= 1 && d < D` -- for |d| > 1 or a NaN the reference's angle is a NaN, which rejects nothing.  A device arc cosine
 * differs from the host's in the last ulps and would flip triangles at the threshold; this comparison cannot.  thresh >= pi: -1 (rejects
 * nothing); thresh < 0: +infinity (rejects every d in [-1, 1]); a NaN threshold: -1.  Default threshold 1.39626: 0.17365146f. */
float flame_nltgv2_oblique_cos_bound(float oblique_normal_thresh);

/* Pointers into pinned memory of the context, valid until the next flame_nltgv2_mesh_outputs_begin. */
typedef struct flame_nltgv2_mesh_outputs_view {
  int32_t V, T;
  const uint8_t* tri_valid;   /* [T] tri_validity_, flame.cc:389-407 */
  const float* normals;       /* [3V] vtx_normals_, (x, y, z) interleaved, caller's vertex order */
  const float* vtx_idepth;    /* [V] vtx_idepths_ = x * graph_scale, flame.cc:377 */
  int32_t n_valid;            /* number of non-zero tri_valid */
  int32_t rows, cols;         /* of the filtered map (0, 0: not asked for) */
  const float* filtered_map;  /* [rows * cols] getFilteredInverseDepthMap, NaN where no VALID triangle covers the pixel; NULL: not asked for */
  int32_t filtered_coverage;  /* its non-NaN pixels */
  float device_ms;            /* measurement aid: HIP-event time of the stage on the side stream, kernels and copies out */
} flame_nltgv2_mesh_outputs_view;

/* begin  checks the arguments -- an error (no graph, T < 0, an index outside [0, V), rows / cols <= 0, Kinv or filter NULL, triangles NULL
 *        without resident triangles or with another T) is reported before anything is enqueued and leaves the outputs of an earlier begin
 *        as they are --, then enqueues everything on the context's side stream and returns.  WHICH STATE it describes is decided exactly as
 *        in flame_nltgv2_interpolate_mesh_begin (the runs are settled and the canonical arrays read; with FLAME_NLTGV2_OPT_MESH_STATE = 1
 *        and runs in flight: the state the last settle left, nothing waited for), so a mesh_outputs_begin right behind an
 *        interpolate_mesh_begin describes the state of that map.
 *        triangles == NULL: the T triangles the last flame_nltgv2_interpolate_mesh[_begin] of this context left on the device for the
 *        current topology (the frame loop calls both on one triangulation: no second upload).
 *        Kinv: 9 floats row-major (Flame::Kinv_).  rows / cols: the map's size; cols also scales edge_length_thresh.
 *        want_filtered_map != 0: the filtered map is rasterised as well, into buffers OF ITS OWN: the resident unfiltered map
 *        (flame_nltgv2_sync_input.init_from_map) and the pinned map of interpolate_mesh_end stay what they were.  The validity goes from
 *        the filter kernel to the rasteriser on the device.
 * end    waits for the side stream and fills *out.
 * flame_nltgv2_mesh_outputs == begin; end; copies into the caller's arrays (each may be NULL).
 * getInverseDepthMesh (flame.h:233-249) = the caller's positions + vtx_idepth + normals + the caller's triangles + tri_valid. */
int flame_nltgv2_mesh_outputs_begin(flame_nltgv2_ctx* ctx, const int32_t* triangles, int32_t T, const float* Kinv,
                                    const flame_nltgv2_mesh_filter_params* filter, int rows, int cols, float graph_scale,
                                    int want_filtered_map);
int flame_nltgv2_mesh_outputs_end(flame_nltgv2_ctx* ctx, flame_nltgv2_mesh_outputs_view* out);
int flame_nltgv2_mesh_outputs(flame_nltgv2_ctx* ctx, const int32_t* triangles, int32_t T, const float* Kinv,
                              const flame_nltgv2_mesh_filter_params* filter, int rows, int cols, float graph_scale,
                              uint8_t* tri_valid_out, float* normals_out, float* vtx_idepth_out, int32_t* n_valid_out,
                              float* filtered_map_out, int32_t* filtered_coverage_out);

/* ---- Metric outputs: what a consumer of the library reads -- a depth image, a point cloud, a 3-D mesh -------------------------------
 * A planner, a TSDF fuser or a ROS front-end does not read inverse depth on a pixel grid.  This stage makes, from the maps and the mesh
 * buffers that already stand on the device, on the context's side stream, beside the running solver: the depth image in metres, the
 * 16-bit millimetre image, the organised and the dense point cloud in the camera or the world frame, and the mesh with 3-D vertices,
 * normals and only the triangles that survived the filters.  Nothing of this has a counterpart in the reference; the conventions are the
 * ones stated for flame_nltgv2_mesh_outputs above.  tests/metric_ref.py restates the operations in numpy float32 and is the checker:
 * device and checker agree bit for bit.
 *
 * PER PIXEL (row, col) with map value v:
 *   q = Kinv * (col, row, 1): the full 3x3 product, every sum of three products left to right, no FMA;
 *   P = q / v: three divisions;  z = P.z;
 *   the pixel is VALID iff v > 0.0f && z > min_depth && z < max_depth.  Every comparison with a NaN is false, so with the defaults
 *   (min_depth = 0, max_depth = +infinity) a NaN, zero, negative or infinite v and an overflowing z are all holes.
 * WORLD FRAME: with a pose T_world_cam (12 floats, row-major [R | t]) P_w = ((r0 * x + r1 * y) + r2 * z) + t, row by row; with NULL
 *   the camera-frame P is written untouched.  A valid pixel's point is written with plain IEEE results.
 * OUTPUTS, each chosen by its want_* flag:
 *   depth          [rows * cols] float     z where the pixel is valid, the quiet NaN 0x7fc00000 on holes (z is the CAMERA-frame depth,
 *                                          with a pose too)
 *   depth_mm       [rows * cols] uint16    rintf(z * 1000.0f), ties to even; written if it lies in [1, 65535], else 0; 0 on holes
 *   organized      [rows * cols * 3] float P or P_w; three quiet NaNs 0x7fc00000 on holes
 *   cloud          [n_points * 3] float, cloud_pixel [n_points] uint32: the valid pixels' points and linear pixel indices
 *                                          row * cols + col in ascending row-major order.  Deterministic: count / scan / scatter, a
 *                                          lane's rank from the scan and the wave's 64-bit ballot, no counter that lanes race for.
 *   mesh_vertices  [3V] float              the vertices flame_nltgv2_mesh_outputs_begin back-projected, P = (Kinv * (pos, 1)) /
 *                                          (x * graph_scale) with ITS Kinv and graph_scale, then posed; every vertex is written, with
 *                                          plain IEEE results (x == 0: infinite points)
 *   mesh_normals   [3V] float              R * the vertex normals of that call ((r0 * nx + r1 * ny) + r2 * nz); without a pose copies
 *   mesh_triangles [3 * n_valid] int32     the index triples of the triangles with non-zero validity of that call, in ascending triangle
 *                                          index; n_valid is the n_valid it reported.  The vertices are not compacted or re-indexed.
 * WHICH MAP: map_device != NULL: a map of the caller's own in device memory (a torch tensor, another library's output), read in
 *   place of the resident ones by the same kernels; nothing is uploaded.  Its rules, since the library knows nothing about it:
 *     - it holds rows * cols floats, row-major, rows of cols floats without padding, on the context's device.  The size cannot be
 *       checked: rows and cols are taken on trust, and a smaller buffer is read out of bounds;
 *     - it is read on the context's SIDE stream, which waits for no stream of the caller's: whatever writes the map must have
 *       completed before begin is called (a stream or device synchronise of the caller's), and the map must stay allocated and
 *       unchanged until _end has returned;
 *     - use_filtered_map is ignored, no resident map is needed and none is touched; a graph is still required
 *       (FLAME_NLTGV2_ERR_NO_GRAPH), as for every stage of this context, and want_mesh keeps its own conditions.
 *   Otherwise use_filtered_map == 0: the resident unfiltered map of the last flame_nltgv2_interpolate_mesh[_begin];
 *   use_filtered_map != 0: the filtered map of the last flame_nltgv2_mesh_outputs_begin(want_filtered_map != 0).
 * The mesh outputs need the validity, the normals and the vertices of a flame_nltgv2_mesh_outputs_begin for the current topology and
 * the current triangle upload (the rule of flame_nltgv2_wireframe_params.validity == 2). */
typedef struct flame_nltgv2_metric_params {
  float   min_depth;         /* 0.0        metres, exclusive */
  float   max_depth;         /* +infinity  metres, exclusive */
  int32_t use_filtered_map;  /* 0 */
  int32_t want_depth;        /* 1 */
  int32_t want_depth_mm;     /* 1 */
  int32_t want_organized;    /* 1 */
  int32_t want_cloud;        /* 1 */
  int32_t want_mesh;         /* 0  mesh_vertices + mesh_normals + mesh_triangles */
  int32_t copy_out;          /* 1  0: the outputs stay on the device; only the two counters travel */
  int32_t reserved;          /* 0 */
  const void* map_device;    /* NULL       a caller's own device map: see WHICH MAP above for its rules */
} flame_nltgv2_metric_params;
void flame_nltgv2_default_metric_params(flame_nltgv2_metric_params* p);

/* Pointers into pinned memory of the context and, beside each, the device pointer of the same array; all valid until the next
 * flame_nltgv2_metric_outputs_begin.  An output that was not asked for has two NULLs; with copy_out == 0 every host pointer is NULL. */
typedef struct flame_nltgv2_metric_outputs_view {
  int32_t rows, cols, V, T;
  int32_t n_points;                  /* valid pixels (0 without want_cloud) */
  int32_t n_valid;                   /* valid triangles (0 without want_mesh) */
  const float* depth;                const void* depth_device;
  const uint16_t* depth_mm;          const void* depth_mm_device;
  const float* organized;            const void* organized_device;
  const float* cloud;                const void* cloud_device;
  const uint32_t* cloud_pixel;       const void* cloud_pixel_device;
  const float* mesh_vertices;        const void* mesh_vertices_device;
  const float* mesh_normals;         const void* mesh_normals_device;
  const int32_t* mesh_triangles;     const void* mesh_triangles_device;
  float device_ms;                   /* measurement aid: HIP-event time of what begin enqueued on the side stream, kernels and copies out
                                        (the n_points points of `cloud` travel in _end, once their number is known: not in it) */
} flame_nltgv2_metric_outputs_view;

/* begin  checks the arguments -- an error (no graph; Kinv or params NULL; rows / cols <= 0 or rows * cols >= 2^31; no resident map of
 *        the kind asked for, or one of another size than rows x cols; want_mesh without current mesh buffers; nothing wanted) is reported
 *        before anything is enqueued and leaves the outputs of an earlier begin, and its pending _end, as they are --, then enqueues
 *        everything on the context's side stream and returns.  The stage only READS the buffers of the other stages, in the order of
 *        that stream: a metric_outputs_begin right behind interpolate_mesh_begin + mesh_outputs_begin describes their state, whatever
 *        the solver does meanwhile.
 *        Kinv: 9 floats row-major (Flame::Kinv_).  T_world_cam: 12 floats or NULL.
 * end    waits for the side stream, brings the n_points points of the dense cloud to the host (copy_out) and fills *out.
 * flame_nltgv2_metric_outputs == begin (with copy_out forced to 1 and the want_* flags replaced by: the array is not NULL; mesh: any of
 *        the three); end; copies into the caller's arrays.  cloud_out / cloud_pixel_out must hold rows * cols points,
 *        mesh_triangles_out 3T indices. */
int flame_nltgv2_metric_outputs_begin(flame_nltgv2_ctx* ctx, const float* Kinv, const float* T_world_cam,
                                      const flame_nltgv2_metric_params* params, int rows, int cols);
int flame_nltgv2_metric_outputs_end(flame_nltgv2_ctx* ctx, flame_nltgv2_metric_outputs_view* out);
int flame_nltgv2_metric_outputs(flame_nltgv2_ctx* ctx, const float* Kinv, const float* T_world_cam,
                                const flame_nltgv2_metric_params* params, int rows, int cols, float* depth_out, uint16_t* depth_mm_out,
                                float* organized_out, float* cloud_out, uint32_t* cloud_pixel_out, int32_t* n_points_out,
                                float* mesh_vertices_out, float* mesh_normals_out, int32_t* mesh_triangles_out, int32_t* n_valid_out);

/* ---- Map error: how good the dense inverse-depth map is -- photometrically, or against a true map ---------------------------------------
 * The reference was built around this measurement: getPoseFrame picks a comparison pose-frame (photo_error_num_pfs), DetectionData::cmp
 * carries it, Flame::photo_error_ is handed to detectFeatures, Params::debug_draw_photo_error exists and update() takes idepths_true "for
 * debugging" -- but the code that used all of it is the commented-out block flame.cc:854-984: the per-pixel error, a box mean, a 256-bin
 * histogram with median and 99th percentile, total_photo_error / avg_photo_error.  This stage computes that block's quantities on the
 * context's side stream, beside the running solver, from live, test-pinned pieces.  Nothing of the dead block is pinned by a reference
 * test, and three of its rules are replaced on purpose (marked UNPINNED below).  tests/map_error_ref.py restates every rule in numpy
 * float32 (no FMA) and is the checker: device and checker agree bit for bit.  The stage only READS other stages' buffers.
 *
 * WHICH MAP: as flame_nltgv2_metric_params: map_device (under the rules stated there), else use_filtered_map, else the resident
 *   unfiltered map; a resident map must be rows x cols.
 * 1. ERROR IMAGE, rows * cols floats, NaN = "no error defined here".
 *   source == FLAME_NLTGV2_MAP_ERROR_PHOTO: for pixel (row, col) with map value v the per-vertex residual of flame_nltgv2_photo_residual
 *     at u = (col, row): |I_cmp(project(u, v)) - I_ref(u)| with KRKinv (9 floats) and Kt (3 floats) as there.  NaN where v is NaN or
 *     negative, where u or the projection lies outside [border, size - border) in x or y, or where the projection is NaN; v == 0 uses the
 *     infinite-depth projection.  border >= 1.  The images: ref_device / cmp_device, two u8 images in device memory with rows of
 *     image_step_bytes (>= cols) bytes each, read in place (two frames resident in the stereo context: flame_stereo_frame_image_device;
 *     the rules of map_device hold for them), or, both NULL, the images of flame_nltgv2_photo_set_images, whose size must be rows x cols
 *     (they must not be replaced before _end; flame_nltgv2_photo_set_images waits for a pending stage).  It equals the checker's
 *     oracle.capi.photo_residual on the pixel grid bit for bit.
 *   source == FLAME_NLTGV2_MAP_ERROR_TRUTH: with a true inverse-depth map t of the same size (truth_host: rows * cols floats, staged
 *     through pinned memory, free when begin returns; or truth_device, under the rules of map_device; exactly one of the two) a pixel
 *     is valid iff !(v != v) && t > 0.0f -- a NaN, zero or negative t is a hole --, err = fabsf(v - t), with relative != 0
 *     err = fabsf(v - t) / t (an IEEE division); infinite operands whose result is a NaN (inf - inf, inf / inf) give a hole.  Every hole
 *     of either source is the quiet NaN 0x7fc00000.  This is update()'s idepths_true.
 * 2. BOX MEAN, win_size odd in [1, 31]; 1: none; 0: the reference's choice, 11, or 5 when cols < 640.  h = win_size / 2.  A pixel whose
 *   own error is NaN stays NaN.  Every other pixel gets sum / (float)count over the window [row - h, row + h] x [col - h, col + h]:
 *   count = the non-NaN errors in the window (>= 1: the pixel itself); sum is taken separably in float32 in a fixed order: for every row
 *   of the window a horizontal sum that starts from +0.0f and goes left to right over the window's columns, then, over the window's
 *   rows top to bottom, the sum of those horizontal sums, again from +0.0f.  A NaN or a position outside the image contributes +0.0f
 *   (adding it or skipping it gives the same bits).  The kernel's tiling does not show.
 *   UNPINNED, deviates from the dead block, which box-sums an integral image with NaN set to 0, divides by win * win -- diluting
 *   errors at the edge of coverage and turning holes into zeros -- and has a first-row / first-column bug (flame.cc:903).
 * 3. STATISTICS over the non-NaN pixels of the (smoothed) error image (want_stats):
 *   n_valid     their number.
 *   hist[256]   s = err * hist_scale (a float multiply); bin = s >= 255.0f ? 255 : (int)(s + 0.5f): the clamp comes before the
 *               conversion, so +inf lands in bin 255.  hist_scale == 0 selects the default: 1.0 for PHOTO (the bins are the reference's
 *               fast_roundf(err) grey levels), 1000.0 for TRUTH (relative: bins 0.1 % wide up to 25.5 %); otherwise it must be finite
 *               and > 0.
 *   median_bin  the smallest m with 2 * cum[m] > n_valid, cum[m] = hist[0] + ... + hist[m].
 *   ptile_bin   the smallest m with ptile_den * cum[m] > ptile_num * n_valid, in 64-bit integers (default 99 / 100; 0 <= ptile_num <=
 *               ptile_den, ptile_den > 0; ptile_num == ptile_den: no such m, -1).  Both are -1 when n_valid == 0.
 *               UNPINNED: replaces the dead block's float comparison and its `else if`, which cannot find both ranks in one bin.
 *   sum, mean   the reference's total_photo_error / avg_photo_error: sum is a double, mean = (float)(sum / n_valid), 0 when n_valid
 *               == 0.  The order of the sum is part of the definition and independent of the launch: the float errors are converted to
 *               double, holes are +0.0; every block of 1024 consecutive linear pixel indices (the last one padded with +0.0) is reduced
 *               pairwise, p[t] += p[t + s] for s = 512, 256, ..., 1; the block partials b[0 .. B) are combined as
 *               flame_nltgv2_rescale_data's sum: q[t] = b[t] + b[t + 1024] + ... in turn from +0.0, t < 1024, then q pairwise in the same
 *               way.  No floating-point atomics anywhere: two calls give the same bytes.
 * 4. PICTURE (want_image), rows * cols * 3 bytes: the grey reference image (cvtColor(GRAY2RGB)) with every non-NaN error pixel replaced
 *   by jet(err, 0, max_error) (utils/visualization.h:142-167; max_error > 0), flip as in flame_nltgv2_debug_image_params; no text.
 *   PHOTO: the grey image is the reference image of the call.  TRUTH: gray_host or gray_device with gray_step_bytes, exactly one, as in
 *   flame_nltgv2_debug_images_begin; without one the picture cannot be requested.
 * 5. want_stats, want_error_map, want_image, copy_out as in the metric stage: with copy_out == 0 the error map and the picture stay on
 *   the device and only the statistics travel (1048 bytes). */
#define FLAME_NLTGV2_MAP_ERROR_PHOTO 0
#define FLAME_NLTGV2_MAP_ERROR_TRUTH 1
typedef struct flame_nltgv2_map_error_params {
  const void*    map_device;        /* NULL */
  const void*    ref_device;        /* NULL     PHOTO */
  const void*    cmp_device;        /* NULL     PHOTO */
  const float*   truth_host;        /* NULL     TRUTH */
  const void*    truth_device;      /* NULL     TRUTH */
  const uint8_t* gray_host;         /* NULL     TRUTH with want_image */
  const void*    gray_device;       /* NULL     TRUTH with want_image */
  float   KRKinv[9];                /* identity PHOTO */
  float   Kt[3];                    /* 0        PHOTO */
  int32_t source;                   /* FLAME_NLTGV2_MAP_ERROR_PHOTO */
  int32_t use_filtered_map;         /* 0 */
  int32_t image_step_bytes;         /* 0        of ref_device and cmp_device */
  int32_t border;                   /* 3        PHOTO */
  int32_t relative;                 /* 1        TRUTH */
  int32_t win_size;                 /* 0        the reference's choice */
  float   hist_scale;               /* 0        the default of the source */
  int32_t ptile_num;                /* 99 */
  int32_t ptile_den;                /* 100 */
  int32_t gray_step_bytes;          /* 0 */
  float   max_error;                /* 32.0     the error painted in the last colour of the picture */
  int32_t flip;                     /* 0 */
  int32_t want_stats;               /* 1 */
  int32_t want_error_map;           /* 1 */
  int32_t want_image;               /* 0 */
  int32_t copy_out;                 /* 1 */
} flame_nltgv2_map_error_params;
void flame_nltgv2_default_map_error_params(flame_nltgv2_map_error_params* p);

/* The statistics, as they lie on the device and in pinned memory. */
typedef struct flame_nltgv2_map_error_stats {
  int32_t hist[256];
  int32_t n_valid, median_bin, ptile_bin;
  float   mean;
  double  sum;
} flame_nltgv2_map_error_stats;

/* Pointers into pinned memory of the context and the device pointers of the same arrays; all valid until the next
 * flame_nltgv2_map_error_begin.  What was not asked for is NULL; with copy_out == 0 error_map and image are NULL. */
typedef struct flame_nltgv2_map_error_view {
  int32_t rows, cols, source, win_size;  /* win_size: the one that was used */
  float   hist_scale;                    /* the one that was used */
  float   device_ms;                     /* measurement aid: HIP-event time of what begin enqueued on the side stream */
  const flame_nltgv2_map_error_stats* stats;  const void* stats_device;
  const float* error_map;                     const void* error_map_device;
  const uint8_t* image;                       const void* image_device;
} flame_nltgv2_map_error_view;

/* begin  checks the arguments -- an error (no graph; params NULL; rows / cols <= 0 or rows * cols >= 2^31; an unknown source; no resident
 *        map of the kind asked for or one of another size; PHOTO: border < 1, one of ref_device / cmp_device without the other or with
 *        image_step_bytes < cols, neither and no images of flame_nltgv2_photo_set_images or images of another size; TRUTH: not exactly one
 *        true map; win_size even, negative or above 31; hist_scale negative, NaN or infinite; ptile_den <= 0, ptile_num < 0 or
 *        ptile_num > ptile_den; want_image with max_error not > 0, or in TRUTH mode without exactly one grey image of gray_step_bytes
 *        >= cols; nothing wanted) is reported before anything is enqueued and leaves the outputs of an earlier begin, and its pending
 *        _end, as they are --, then enqueues everything on the context's side stream and returns.
 * end    waits for the side stream and fills *out.
 * flame_nltgv2_map_error == begin (with copy_out forced to 1 and the want_* flags replaced by: the array is not NULL); end; copies into
 *        the caller's arrays: error_map_out rows * cols floats, image_out rows * cols * 3 bytes, *stats_out. */
int flame_nltgv2_map_error_begin(flame_nltgv2_ctx* ctx, const flame_nltgv2_map_error_params* params, int rows, int cols);
int flame_nltgv2_map_error_end(flame_nltgv2_ctx* ctx, flame_nltgv2_map_error_view* out);
int flame_nltgv2_map_error(flame_nltgv2_ctx* ctx, const flame_nltgv2_map_error_params* params, int rows, int cols,
                           float* error_map_out, uint8_t* image_out, flame_nltgv2_map_error_stats* stats_out);

/* ---- The mesh rendered into another camera ------------------------------------------------------------------------------------------------
 * Every other output is tied to the camera and the instant of the frame the solver works on.  This stage looks at the mesh -- a 3-D
 * surface -- from anywhere else: depth registered to a second camera with its own intrinsics and size, the map predicted at a newer
 * pose, or the current mesh in the previous pose-frame's view, whose difference to the map that pose-frame kept
 * (flame_nltgv2_map_error_begin, TRUTH, truth_device) measures consistency where there is no true map.  The reference has no
 * counterpart, so the rules are stated here in full; tests/view_ref.py restates them in numpy float32 and Python integers and is the
 * checker: device and checker agree bit for bit.  It is not the rasteriser of flame_nltgv2_interpolate_mesh: in its own view the mesh
 * never overlaps itself and "the later triangle wins" on whole-pixel vertices; from another viewpoint the surface folds over itself,
 * so here the NEAREST wins and vertices keep 1/16 pixel.
 *
 * All arithmetic is float32 without FMA; every sum of three products is taken left to right, (a + b) + c.
 * Inputs: vertices pos[v] in source pixels; id[v] = x[v] * graph_scale (the _arrays form: the caller's idepths); triangles (a, b, c)
 * with optional validity; Kinv_src, K_dst, R (9 floats each, row-major) and t (3 floats) with P_dst = R * P_src + t; a target of
 * rows x cols pixels, each in 1 .. 32767, which need not be the source's size; near_depth.
 *   1 vertex      q = Kinv_src * (pos.x, pos.y, 1); P = q / id (three divisions); P' = R * P, then + t per component; h = K_dst * P';
 *                 u = h.x / h.z, w = h.y / h.z; sx = u * 16.0f, sy = w * 16.0f.  The vertex is USABLE iff id > 0.0f, P'.z > near_depth,
 *                 fabsf(sx) <= 1048576.0f and fabsf(sy) <= 1048576.0f (every comparison with a NaN is false), and its source position
 *                 keeps the same bound: fabsf(pos.x * 16.0f), fabsf(pos.y * 16.0f) <= 1048576.0f.  Then X = (int)rintf(sx),
 *                 Y = (int)rintf(sy), Xs = (int)rintf(pos.x * 16.0f), Ys = (int)rintf(pos.y * 16.0f) -- ties to even, positions in 1/16
 *                 pixel -- and id' = 1.0f / P'.z.
 *   2 triangle    drawn iff its validity byte is non-zero (where validity is in force), all three vertices are usable, and the doubled
 *                 signed areas A = (Xb - Xa)(Yc - Ya) - (Yb - Ya)(Xc - Xa) and As, the same on Xs, Ys, both exact in int64, are both
 *                 non-zero and of the same sign: a triangle whose orientation flipped is seen from behind and culled.  No clipping: a
 *                 triangle with an unusable vertex is dropped whole.
 *   3 coverage    pixel centres lie at integer pixel coordinates, (16 col, 16 row).  s = sign(A); w_a = s * E(b, c), w_b = s * E(c, a),
 *                 w_c = s * E(a, b) with E(i, j) = (Xj - Xi)(16 row - Yi) - (Yj - Yi)(16 col - Xi) in int64.  A pixel inside the image
 *                 is covered iff all three weights are >= 0, edges and corners included.  Nothing outside the image is touched.
 *   4 value       val = (id'_a * (float)w_a + (id'_b * (float)w_b + id'_c * (float)w_c)) / (float)|A|, every int64 -> float conversion
 *                 rounding to nearest even.  A covered pixel is a CANDIDATE iff val > 0.0f && val < +infinity.
 *   5 depth test  the candidate with the largest val owns the pixel (the nearest surface); among equal bit patterns the larger triangle
 *                 index.  One 64-bit integer maximum over {bits(val) << 32 | (t + 1)}; the key image is cleared per call, and the
 *                 result does not depend on scheduling: two calls give the same bytes.
 *   6 outputs     map: rows * cols floats, the owner's val, the quiet NaN 0x7fc00000 on holes.  tri_index: rows * cols int32, the
 *                 owner's triangle index, -1 on holes (a consumer interpolates colour or normals in the target view with it).  The
 *                 counters: coverage = the non-hole pixels; tris_drawn, tris_culled_vertex (a vertex not usable), tris_culled_facing
 *                 (zero area in either view, or flipped) -- a triangle whose validity byte is zero is in none of the three.
 * want_map, want_tri_index, copy_out as in the metric stage: with copy_out == 0 only the counters travel (16 bytes) and map_device /
 * tri_index_device of the view serve flame_nltgv2_metric_params.map_device, flame_nltgv2_map_error_params.map_device / truth_device.
 * Not done: clipping against the near plane, anti-aliasing, lens distortion of the target camera. */
typedef struct flame_nltgv2_view_params {
  float   Kinv_src[9];     /* identity  the source camera's inverse intrinsics (Flame::Kinv_) */
  float   K_dst[9];        /* identity  the target camera's intrinsics */
  float   R[9];            /* identity  P_dst = R * P_src + t */
  float   t[3];            /* 0 */
  float   near_depth;      /* 0.0       a vertex at or below this depth in the target camera is not usable */
  int32_t validity;        /* 0: every triangle is valid (tri_valid must be NULL); 1: tri_valid is a host array of T bytes;
                              2: the validity the last flame_nltgv2_mesh_outputs_begin left on the device for the resident
                                 triangles (tri_valid must be NULL; an error if there is none for the current triangles and topology;
                                 an error in the _arrays form) */
  int32_t want_map;        /* 1 */
  int32_t want_tri_index;  /* 1 */
  int32_t copy_out;        /* 1  0: the outputs stay on the device; only the counters travel */
} flame_nltgv2_view_params;
void flame_nltgv2_default_view_params(flame_nltgv2_view_params* p);

/* The counters, as they lie on the device and in pinned memory. */
typedef struct flame_nltgv2_view_counts {
  int32_t coverage, tris_drawn, tris_culled_vertex, tris_culled_facing;
} flame_nltgv2_view_counts;

/* Pointers into pinned memory of the context and the device pointers of the same arrays; all valid until the next
 * flame_nltgv2_render_view_begin or flame_nltgv2_render_view_arrays.  What was not asked for has two NULLs; with copy_out == 0 every
 * host pointer is NULL. */
typedef struct flame_nltgv2_view_outputs_view {
  int32_t rows, cols, T;
  flame_nltgv2_view_counts counts;
  float   device_ms;                 /* measurement aid: HIP-event time of what begin enqueued on the side stream, kernels and copies out */
  const float* map;                  const void* map_device;        /* [rows * cols] */
  const int32_t* tri_index;          const void* tri_index_device;  /* [rows * cols] */
} flame_nltgv2_view_outputs_view;

/* begin  checks the arguments -- an error (no graph; params NULL; rows or cols outside 1 .. 32767; no resident triangles for the current
 *        topology; validity outside 0 .. 2; a tri_valid pointer with validity != 1 or none with validity == 1; validity == 2 without a
 *        matching flame_nltgv2_mesh_outputs_begin) is reported before anything is enqueued and leaves the outputs of an earlier begin,
 *        and its pending _end, as they are --, then enqueues everything on the context's side stream, beside a running solver, and
 *        returns.  The triangles are the ones the last flame_nltgv2_interpolate_mesh[_begin] or flame_nltgv2_mesh_outputs_begin left on
 *        the device; pos and x are read from the state flame_nltgv2_interpolate_mesh_begin would read (FLAME_NLTGV2_OPT_MESH_STATE
 *        decides in the same way).  Only the vertex kernel reads pos / x: whoever rewrites them waits for that kernel, not for the
 *        picture.  The stage only READS the buffers of the other stages, and they leave this stage's alone.
 * end    waits for the side stream and fills *out.
 * flame_nltgv2_render_view == begin (with copy_out forced to 1 and the want_* flags replaced by: the array is not NULL); end; copies into
 *        the caller's arrays: map_out rows * cols floats, tri_index_out rows * cols int32, *counts_out (each may be NULL).
 * flame_nltgv2_render_view_arrays  the same for a mesh of the caller's, synchronously: T triangles that index V vertices_xy (2V floats,
 *        source pixels) with V idepths -- a pose-frame's stored mesh, curr_pf_->tris / vtx / vtx_idepths --, tri_valid NULL or T bytes
 *        (params->validity must say 0 or 1 accordingly).  An error (also: T or V negative, a missing array, an index outside 0 .. V - 1)
 *        is reported before anything is enqueued.  It needs no graph and uses this stage's buffers only: the resident triangles, the
 *        rasteriser's key image and the resident maps stay as they are; what a pending flame_nltgv2_render_view_end would have returned
 *        is replaced by this call's outputs. */
int flame_nltgv2_render_view_begin(flame_nltgv2_ctx* ctx, const flame_nltgv2_view_params* params, const uint8_t* tri_valid, int rows,
                                   int cols, float graph_scale);
int flame_nltgv2_render_view_end(flame_nltgv2_ctx* ctx, flame_nltgv2_view_outputs_view* out);
int flame_nltgv2_render_view(flame_nltgv2_ctx* ctx, const flame_nltgv2_view_params* params, const uint8_t* tri_valid, int rows, int cols,
                             float graph_scale, float* map_out, int32_t* tri_index_out, flame_nltgv2_view_counts* counts_out);
int flame_nltgv2_render_view_arrays(flame_nltgv2_ctx* ctx, const flame_nltgv2_view_params* params, const int32_t* triangles, int32_t T,
                                    const float* vertices_xy, const float* idepths, int32_t V, const uint8_t* tri_valid, int rows,
                                    int cols, float* map_out, int32_t* tri_index_out, flame_nltgv2_view_counts* counts_out);

/* ---- Kept meshes: the mesh a pose-frame keeps (flame.cc:417-426, curr_pf_->tris / vtx / vtx_idepths) -----------------------------------
 * Slots 0 .. FLAME_NLTGV2_KEPT_MESHES - 1 of the context, each empty or holding on the device V positions (source pixels), V inverse
 * depths, T triangles and, optionally, T validity bytes.  A kept mesh survives flame_nltgv2_upload_graph, flame_nltgv2_sync_graph /
 * _sync_commit and any change of topology: that is its purpose.  Slots are written and read on the context's side stream only, so
 * stream order covers every hazard between a snapshot, a fusion that reads it and the next snapshot into the same slot.
 *
 * flame_nltgv2_keep_mesh         snapshots the resident mesh into `slot`, device to device, enqueued on the side stream beside a running
 *        solver: the resident triangles (of the last flame_nltgv2_interpolate_mesh[_begin] or flame_nltgv2_mesh_outputs_begin), pos, and
 *        id[v] = x[v] * graph_scale -- one float32 multiply, no FMA -- with pos / x read from the state flame_nltgv2_render_view_begin
 *        would read (FLAME_NLTGV2_OPT_MESH_STATE decides in the same way).  validity: 0 = none is kept (every triangle is valid), 2 = the
 *        validity the last flame_nltgv2_mesh_outputs_begin left for the resident triangles.  Rendering the slot later gives the bytes
 *        flame_nltgv2_render_view_begin on the live mesh would have given at the moment of the snapshot (id * 1.0f == id).
 *        Errors, reported before anything is enqueued, the slot left as it was: slot out of range; no graph; no resident triangles for
 *        the current topology; validity not 0 or 2, or 2 without a matching flame_nltgv2_mesh_outputs_begin.  (A failure behind these
 *        checks -- no memory for a slot that must grow -- leaves the slot empty.)
 * flame_nltgv2_keep_mesh_arrays  uploads a mesh of the caller's into `slot`: the arguments and their checks are those of
 *        flame_nltgv2_render_view_arrays (T or V negative, a missing array, an index outside 0 .. V - 1); tri_valid NULL or T bytes.  It
 *        needs no graph.  The caller's arrays are free when it returns.
 * flame_nltgv2_drop_mesh         empties a slot (prunePoseFrames); dropping an empty slot is OK.  The memory stays with the context.
 * flame_nltgv2_kept_mesh_info    *V = *T = -1 and *has_validity = 0 for an empty slot (each pointer may be NULL).
 * flame_nltgv2_get_kept_mesh     downloads a slot, synchronously (for tests, and for callers that persist meshes): 2V floats, V floats,
 *        3T int32, T bytes; each pointer may be NULL; an error for an empty slot, and for tri_valid where the slot keeps none. */
#define FLAME_NLTGV2_KEPT_MESHES 16
int flame_nltgv2_keep_mesh(flame_nltgv2_ctx* ctx, int32_t slot, float graph_scale, int32_t validity);
int flame_nltgv2_keep_mesh_arrays(flame_nltgv2_ctx* ctx, int32_t slot, const int32_t* triangles, int32_t T, const float* vertices_xy,
                                  const float* idepths, int32_t V, const uint8_t* tri_valid);
int flame_nltgv2_drop_mesh(flame_nltgv2_ctx* ctx, int32_t slot);
int flame_nltgv2_kept_mesh_info(flame_nltgv2_ctx* ctx, int32_t slot, int32_t* V, int32_t* T, int32_t* has_validity);
int flame_nltgv2_get_kept_mesh(flame_nltgv2_ctx* ctx, int32_t slot, float* vertices_xy, float* idepths, int32_t* triangles, uint8_t* tri_valid);

/* ---- Several meshes fused in one view --------------------------------------------------------------------------------------------------
 * Up to FLAME_NLTGV2_FUSE_SOURCES meshes -- kept slots and, optionally, the live resident mesh -- rendered into ONE target camera in a
 * single batch of launches, then a vote per pixel: where enough pose-frames agree on the surface the pixel gets their weighted mean,
 * and the masks name who saw it and who disagreed.  Cross-view agreement removes the sliver triangles and mismatched features the
 * single-view triangle filters only guess at.  The reference has no counterpart, so the rules are stated here in full;
 * tests/fuse_ref.py restates them in numpy float32 and Python integers over tests/view_ref.py and is the checker: device and checker
 * agree bit for bit.  All arithmetic is float32 without FMA.
 *   A layers       layer s is exactly what rules 1 - 5 of flame_nltgv2_render_view_begin give for source s (its mesh, its Kinv_src, R, t)
 *                  into the target (K_dst, near_depth, rows x cols), the 64-bit key {bits(val) << 32 | t + 1} and its tie rule included;
 *                  holes are the quiet NaN 0x7fc00000.  A kept slot renders with the validity it keeps, if any; the live mesh as its
 *                  `validity` says (0 or 2).
 *   B present      source s is present at a pixel iff layer s is no hole there; n = the number present.
 *   C reference    the present values ordered ascending by (bits(v_s), s) -- positive floats order as their bits do, equal bit patterns
 *                  by source index --; m = the value at index n / 2 (integer division): the UPPER median, which of two sources that
 *                  disagree is the larger inverse depth, the NEARER surface.  For navigation the conservative choice is the nearer one:
 *                  an obstacle one pose-frame saw must not be voted away by one that saw through it.
 *   D inliers      a present s is an inlier iff fabsf(v_s - m) <= rel_tol * m (one subtraction, one multiplication, one comparison);
 *                  support = the number of inliers; the owner of m is always one of them.
 *   E fused value  the pixel is fused iff support >= min_support; then num = ((v_a * w_a) + v_b * w_b) + ... and den = (w_a + w_b) + ...
 *                  over the inliers in ascending source index, left to right, and fused = num / den; otherwise the pixel is a hole.
 *   F outputs      fused: rows * cols floats.  present_mask, inlier_mask: rows * cols uint8, bit s for source s, written for every pixel,
 *                  fused or not: present & ~inlier names the pose-frames that disagree here.  spread: rows * cols floats, the largest
 *                  inlier minus the smallest (one subtraction), the quiet NaN where n == 0.  layers: n_sources * rows * cols floats,
 *                  only with want_layers.  The counters (flame_nltgv2_fuse_counts, 32 int32): coverage = the fused pixels;
 *                  support_hist[k] = the pixels with support k -- every pixel of the target falls in exactly one bin, n == 0 in bin 0 --;
 *                  present[s], inlier[s] = the pixels where source s is; tris_drawn summed over the sources; the rest reserved, zero.
 *   G transfers    with copy_out == 0 only the counters travel (128 bytes); the view carries the device pointers beside the host ones.
 *                  fused_device serves flame_nltgv2_metric_params.map_device and flame_nltgv2_map_error_params.map_device /
 *                  truth_device (under the rules stated there), and is what a volumetric integrator would consume.
 * No floating-point atomics anywhere: two calls give the same bytes.
 * Not done: clipping at the near plane, anti-aliasing, per-pixel confidence weights, fusing colour or normals. */
#define FLAME_NLTGV2_FUSE_SOURCES 8
typedef struct flame_nltgv2_fuse_source {
  int32_t slot;            /* -1        a kept slot, or -1: the live resident mesh (at most one source of a call) */
  int32_t validity;        /* 0         the live mesh only: 0 every triangle is valid, 2 the validity of the last mesh_outputs_begin */
  float   graph_scale;     /* 1.0       the live mesh only: id[v] = x[v] * graph_scale */
  float   weight;          /* 1.0       finite and > 0 */
  float   Kinv_src[9];     /* identity  this source's inverse intrinsics */
  float   R[9];            /* identity  P_dst = R * P_src + t */
  float   t[3];            /* 0 */
} flame_nltgv2_fuse_source;

typedef struct flame_nltgv2_fuse_params {
  int32_t n_sources;       /* 1         1 .. FLAME_NLTGV2_FUSE_SOURCES */
  flame_nltgv2_fuse_source sources[FLAME_NLTGV2_FUSE_SOURCES];
  float   K_dst[9];        /* identity  the target camera's intrinsics */
  float   near_depth;      /* 0.0 */
  float   rel_tol;         /* 0.05      finite and >= 0 */
  int32_t min_support;     /* 1         1 .. n_sources */
  int32_t want_fused;      /* 1 */
  int32_t want_masks;      /* 1 */
  int32_t want_spread;     /* 1 */
  int32_t want_layers;     /* 0 */
  int32_t copy_out;        /* 1  0: the outputs stay on the device; only the counters travel */
} flame_nltgv2_fuse_params;
void flame_nltgv2_default_fuse_params(flame_nltgv2_fuse_params* p);

/* The counters, as they lie on the device and in pinned memory: 32 words. */
typedef struct flame_nltgv2_fuse_counts {
  int32_t coverage;
  int32_t support_hist[FLAME_NLTGV2_FUSE_SOURCES + 1];
  int32_t present[FLAME_NLTGV2_FUSE_SOURCES];
  int32_t inlier[FLAME_NLTGV2_FUSE_SOURCES];
  int32_t tris_drawn;
  int32_t reserved[5];
} flame_nltgv2_fuse_counts;

/* Pointers into pinned memory of the context and the device pointers of the same arrays; all valid until the next
 * flame_nltgv2_fuse_views_begin.  What was not asked for has two NULLs; with copy_out == 0 every host pointer is NULL. */
typedef struct flame_nltgv2_fuse_outputs_view {
  int32_t rows, cols, n_sources;
  float   device_ms;                 /* measurement aid: HIP-event time of what begin enqueued on the side stream, kernels and copies out */
  flame_nltgv2_fuse_counts counts;
  const float*   fused;              const void* fused_device;         /* [rows * cols] */
  const uint8_t* present_mask;       const void* present_mask_device;  /* [rows * cols] */
  const uint8_t* inlier_mask;        const void* inlier_mask_device;   /* [rows * cols] */
  const float*   spread;             const void* spread_device;        /* [rows * cols] */
  const float*   layers;             const void* layers_device;        /* [n_sources * rows * cols] */
} flame_nltgv2_fuse_outputs_view;

/* begin  checks the arguments -- an error (params NULL; n_sources, rows or cols out of range (rows, cols in 1 .. 32767); a slot out of
 *        range or empty; two live sources; a live source without a graph, without resident triangles for the current topology, with a
 *        validity other than 0 or 2, or 2 without a matching flame_nltgv2_mesh_outputs_begin; a weight that is not finite and > 0;
 *        rel_tol not finite or < 0; min_support outside 1 .. n_sources) is reported before anything is enqueued and leaves the outputs
 *        of an earlier begin, and its pending _end, as they are --, then enqueues everything on the context's side stream and returns.
 *        One vertex launch, one count launch, one raster launch and one launch for large boxes serve ALL sources; the vote reads the
 *        key layers directly.  A live source's pos / x are read as flame_nltgv2_render_view_begin reads them, by the vertex kernel
 *        alone.  The stage only READS the buffers of the other stages and the kept slots; its key layers, vertices and lists are its
 *        own, so a pending flame_nltgv2_render_view_end is not disturbed by it, nor the other way round.  The same slot may be named
 *        twice.
 * end    waits for the side stream and fills *out.
 * flame_nltgv2_fuse_views == begin (with copy_out forced to 1 and the want_* flags replaced by: the array is not NULL; the masks are
 *        made if either is asked for); end; copies into the caller's arrays (each may be NULL). */
int flame_nltgv2_fuse_views_begin(flame_nltgv2_ctx* ctx, const flame_nltgv2_fuse_params* params, int rows, int cols);
int flame_nltgv2_fuse_views_end(flame_nltgv2_ctx* ctx, flame_nltgv2_fuse_outputs_view* out);
int flame_nltgv2_fuse_views(flame_nltgv2_ctx* ctx, const flame_nltgv2_fuse_params* params, int rows, int cols, float* fused_out,
                            uint8_t* present_mask_out, uint8_t* inlier_mask_out, float* spread_out, float* layers_out,
                            flame_nltgv2_fuse_counts* counts_out);

/* ---- Volumetric map: integrate depth maps, raycast a view -------------------------------------------------------------------------------
 * One truncated-signed-distance volume per context, resident on the device: the map that keeps what pruned pose-frames saw.  Two stages
 * on the side stream work on it beside a running solver: flame_nltgv2_volume_integrate_begin folds one inverse-depth map, seen from one
 * pose, into it; flame_nltgv2_volume_raycast_begin renders it into any pinhole camera as a dense inverse-depth map on the device, which
 * serves flame_stereo_align_frame as idepthmap_device (frame-to-model tracking), flame_nltgv2_map_error_params.truth_device (consistency
 * against everything seen so far) and flame_nltgv2_metric_params.map_device.  The reference has no counterpart, so the rules are stated
 * here in full (UNPINNED); tests/volume_ref.py restates them in numpy float32 and is the checker: device and checker agree bit for bit.
 * All arithmetic is float32 without FMA, every sum of three products left to right, divisions correctly rounded.
 *
 * THE STORE.  nx, ny, nz each in 1 .. 1024 with nx * ny * nz <= 2^28; voxel_size, trunc, max_weight finite and > 0; origin (finite) is
 *   the world position of the CENTRE of voxel (0, 0, 0).  A voxel is the record {float tsdf; float weight} at linear index
 *   (k * ny + j) * nx + i, x fastest; a fresh or reset voxel is {1.0f, 0.0f}.  The volume survives flame_nltgv2_upload_graph,
 *   flame_nltgv2_sync_graph / _sync_commit and every change of topology, as the kept meshes do; it is written and read on the context's
 *   side stream only, so stream order covers every hazard between the calls below.
 *   flame_nltgv2_volume_create    makes the volume, every voxel {1, 0}; on a context that already has one it replaces it.  An error in
 *                                 the parameters leaves an existing volume as it is.
 *   flame_nltgv2_volume_reset     every voxel {1, 0} again.
 *   flame_nltgv2_volume_destroy   frees it (flame_nltgv2_destroy does too).
 *   flame_nltgv2_volume_info      the parameters it was created with and the bytes it takes on the device (each pointer may be NULL).
 *   flame_nltgv2_volume_download  synchronous: nx * ny * nz floats each, in the linear order above (each pointer may be NULL).
 *   flame_nltgv2_volume_upload    synchronous, both arrays required: it exists so that a raycast can be tested on voxel values an
 *                                 integration would never produce, and checks weight >= 0 for every voxel (a NaN is not) and nothing else.
 *   Every call but create on a context without a volume answers FLAME_NLTGV2_ERR_INVALID_ARG.
 * THE WINDOW.  The volume is a window of nx x ny x nz voxels on one infinite grid: it has an int32 base[3], (0, 0, 0) after
 *   flame_nltgv2_volume_create, which flame_nltgv2_volume_reset and _upload leave unchanged, and LOCAL voxel (i, j, k) -- the index of
 *   the store, of _download / _upload and of the mesh's boxes -- is GLOBAL voxel (base.x + i, base.y + j, base.z + k).  origin is the
 *   world position of the centre of GLOBAL voxel (0, 0, 0) and never changes: flame_nltgv2_volume_shift_begin (below this block) moves
 *   base, not origin, so a voxel's centre keeps its float32 bits for as long as the voxel stays in the window, integration into a moving
 *   window equals, bit for bit, a crop of integration into a larger fixed volume, and a mesh vertex of a kept cube keeps its bytes
 *   across a shift.  With base == (0, 0, 0) every rule below is what it was before the window existed, bit for bit.  After any shift
 *   |base[a]| <= 2^22 on every axis.  flame_nltgv2_volume_window returns the base.
 *
 * INTEGRATION, per voxel (i, j, k), with K (9 floats row-major) and T_cam_world (12 floats, row-major [R | t]):
 *   1 centre     p = origin + (float)(base + index) * voxel_size, per axis, the sum taken in integers before the conversion; P = ((r0 * p.x + r1 * p.y) + r2 * p.z) + t, row by row.
 *   2 front      the voxel is skipped unless P.z > near_depth.                                               counter `front`
 *   3 projection q = K * P, the full 3x3 product; u = q.x / q.z, v = q.y / q.z.
 *   4 in image   iff u >= -0.5f && u < (float)cols - 0.5f && v >= -0.5f && v < (float)rows - 0.5f.  The test comes first, so that no
 *                NaN or huge value reaches a conversion.                                                     counter `in_image`
 *   5 pixel      col = (int)floorf(u + 0.5f), row = (int)floorf(v + 0.5f), both clamped to the image: the NEAREST pixel, no
 *                interpolation -- a hole must not bleed.
 *   6 validity   d = map[row * cols + col]; zm = 1.0f / d; valid iff d > 0.0f && zm > min_depth && zm < max_depth: the rule of the
 *                metric outputs, so a NaN, zero, negative or infinite d is a hole.                           counter `valid`
 *   7 distance   sdf = zm - P.z: projective, along the optical axis.  A voxel with sdf < -trunc is left alone.   counter `behind`
 *   8 truncation s = fminf(sdf / trunc, 1.0f).
 *   9 update     W = w_old + weight; tsdf = ((tsdf_old * w_old) + (s * weight)) / W; w = fminf(W, max_weight).  counter `updated`;
 *                `saturated` counts the updated voxels with W > max_weight.
 *   The counters nest: updated = valid - behind <= valid <= in_image <= front.  A voxel that is not updated is not written, and its
 *   record is not loaded either: the tests of 2 - 7 come before the load.  Each voxel has one owner; there are no floating-point
 *   atomics: the same calls in the same order give the same bytes.  Integration is not commutative in float32: the order of the
 *   calls is part of the result.  Only the counters come down (2 KiB: sixteen partial sets, which _end sums).
 *   WHICH MAP: exactly as flame_nltgv2_metric_params: map_device (rows * cols floats on the context's device, taken on trust; read on
 *   the side stream, which waits for no stream of the caller's: its writer must have completed before begin, and it must stay allocated
 *   and unchanged until _end has returned), else use_filtered_map != 0: the filtered map of the last
 *   flame_nltgv2_mesh_outputs_begin(want_filtered_map != 0), else the resident unfiltered map of the last
 *   flame_nltgv2_interpolate_mesh[_begin]; a resident map must have the size rows x cols.  Unlike the metric stage a graph is needed
 *   only when a resident map is read (FLAME_NLTGV2_ERR_NO_GRAPH).
 *
 * RAYCAST, per pixel (row, col), with Kinv (9 floats) and T_world_cam (12 floats); rows, cols in 1 .. 32767; z_near, dz finite, dz > 0;
 * n_steps in 1 .. 4096:
 *   q = Kinv * (col, row, 1), as in the metric outputs.  For n = 0 .. n_steps - 1:
 *     z_n = z_near + (float)n * dz: a product, not a running sum;  Pc = q * z_n, componentwise;  p = T_world_cam applied as in rule 1;
 *     g = (p - origin) / voxel_size, per axis: a GLOBAL coordinate;
 *     the sample is VALID iff, per axis, g >= (float)base && g <= (float)(base + n_axis - 1), and all eight voxels around it have
 *     weight > 0; an axis with n_axis == 1 has no valid sample;
 *     ig = min((int)floorf(g), base + n_axis - 2), the local cell index is ig - base, f = g - (float)ig, so g == base + n_axis - 1
 *     gives f == 1;
 *     the value is trilinear with lerp(a, b, t) = a + t * (b - a), along x, then y, then z.
 *   The ray ENDS at the first valid sample with value <= 0.  It is a HIT iff the sample of step n - 1 was valid and > 0: then
 *   z* = z_{n-1} + dz * (f_prev / (f_prev - f_cur)) with the two values, and the pixel is 1.0f / (z* * q.z).  Otherwise the surface was
 *   met from inside or behind: the pixel is a hole, counted in `back`.  A ray that never ends is a hole, counted in `empty` if it had
 *   no valid sample at all.  Holes are the quiet NaN 0x7fc00000.
 *   The view follows the other stages: the host pointer, the device pointer beside it, device_ms; all valid until the next
 *   flame_nltgv2_volume_raycast_begin.  With copy_out == 0 only the counters travel (2 KiB, as above) and the host pointer is NULL.
 *
 * begin  (both stages) checks the arguments -- an error (no volume; a NULL matrix or params; rows / cols out of range; integration:
 *        weight not finite or <= 0, no map of the kind asked for or one of another size; raycast: z_near or dz not finite, dz <= 0,
 *        n_steps out of range) is reported before anything is enqueued and leaves the volume, the outputs of an earlier begin and its
 *        pending _end as they are --, then enqueues everything on the context's side stream and returns.
 * end    waits for the side stream and fills *out.
 * flame_nltgv2_volume_integrate / flame_nltgv2_volume_raycast == begin (the raycast with copy_out forced to 1); end; copies into the
 *        caller's arrays (each may be NULL).
 * (The surface as a triangle mesh with normals: flame_nltgv2_volume_mesh_begin, below this block.)
 * (The window that follows the camera: flame_nltgv2_volume_shift_begin and flame_nltgv2_volume_follow, below the mesh.)
 * Not done: colour, a sparse or hashed volume. */
typedef struct flame_nltgv2_volume_params {
  int32_t nx, ny, nz;      /* 64, 64, 64 */
  float   voxel_size;      /* 0.05       metres */
  float   origin[3];       /* 0          the world position of the centre of GLOBAL voxel (0, 0, 0): THE WINDOW */
  float   trunc;           /* 0.15       metres */
  float   max_weight;      /* 64.0 */
} flame_nltgv2_volume_params;
void flame_nltgv2_default_volume_params(flame_nltgv2_volume_params* p);

typedef struct flame_nltgv2_integrate_params {
  float   weight;            /* 1.0        finite and > 0 */
  float   near_depth;        /* 0.0        metres, exclusive */
  float   min_depth;         /* 0.0        metres, exclusive */
  float   max_depth;         /* +infinity  metres, exclusive */
  int32_t use_filtered_map;  /* 0 */
  int32_t reserved;          /* 0 */
  const void* map_device;    /* NULL       a caller's own device map: see WHICH MAP above for its rules */
} flame_nltgv2_integrate_params;
void flame_nltgv2_default_integrate_params(flame_nltgv2_integrate_params* p);

/* The counters, as they lie on the device and in pinned memory: 8 words. */
typedef struct flame_nltgv2_integrate_counts {
  int32_t front, in_image, valid, behind, updated, saturated;
  int32_t reserved[2];
} flame_nltgv2_integrate_counts;

typedef struct flame_nltgv2_integrate_view {
  int32_t rows, cols;
  float   device_ms;       /* measurement aid: HIP-event time of what begin enqueued on the side stream */
  int32_t reserved;
  flame_nltgv2_integrate_counts counts;
} flame_nltgv2_integrate_view;

typedef struct flame_nltgv2_raycast_params {
  float   z_near;          /* 0.1        metres: the depth of the first sample along the optical axis */
  float   dz;              /* 0.05       metres, > 0 */
  int32_t n_steps;         /* 64         1 .. 4096 */
  int32_t copy_out;        /* 1  0: the map stays on the device; only the counters travel */
} flame_nltgv2_raycast_params;
void flame_nltgv2_default_raycast_params(flame_nltgv2_raycast_params* p);

typedef struct flame_nltgv2_raycast_counts {
  int32_t hits, back, empty, reserved;
} flame_nltgv2_raycast_counts;

/* map: pinned memory of the context (NULL with copy_out == 0); map_device: the same array on the device; both valid until the next
 * flame_nltgv2_volume_raycast_begin. */
typedef struct flame_nltgv2_raycast_view {
  int32_t rows, cols;
  float   device_ms;       /* measurement aid: HIP-event time of what begin enqueued on the side stream, kernel and copies out */
  int32_t reserved;
  flame_nltgv2_raycast_counts counts;
  const float* map;        const void* map_device;   /* [rows * cols] inverse depths */
} flame_nltgv2_raycast_view;

int flame_nltgv2_volume_create(flame_nltgv2_ctx* ctx, const flame_nltgv2_volume_params* params);
int flame_nltgv2_volume_reset(flame_nltgv2_ctx* ctx);
int flame_nltgv2_volume_destroy(flame_nltgv2_ctx* ctx);
int flame_nltgv2_volume_info(flame_nltgv2_ctx* ctx, flame_nltgv2_volume_params* params_out, int64_t* device_bytes_out);
int flame_nltgv2_volume_download(flame_nltgv2_ctx* ctx, float* tsdf_out, float* weight_out);
int flame_nltgv2_volume_upload(flame_nltgv2_ctx* ctx, const float* tsdf, const float* weight);
int flame_nltgv2_volume_integrate_begin(flame_nltgv2_ctx* ctx, const float* K, const float* T_cam_world,
                                        const flame_nltgv2_integrate_params* params, int rows, int cols);
int flame_nltgv2_volume_integrate_end(flame_nltgv2_ctx* ctx, flame_nltgv2_integrate_view* out);
int flame_nltgv2_volume_integrate(flame_nltgv2_ctx* ctx, const float* K, const float* T_cam_world,
                                  const flame_nltgv2_integrate_params* params, int rows, int cols, flame_nltgv2_integrate_counts* counts_out);
int flame_nltgv2_volume_raycast_begin(flame_nltgv2_ctx* ctx, const float* Kinv, const float* T_world_cam,
                                      const flame_nltgv2_raycast_params* params, int rows, int cols);
int flame_nltgv2_volume_raycast_end(flame_nltgv2_ctx* ctx, flame_nltgv2_raycast_view* out);
int flame_nltgv2_volume_raycast(flame_nltgv2_ctx* ctx, const float* Kinv, const float* T_world_cam,
                                const flame_nltgv2_raycast_params* params, int rows, int cols, float* map_out,
                                flame_nltgv2_raycast_counts* counts_out);

/* ---- Volumetric map: the surface as a triangle mesh --------------------------------------------------------------------------------------
 * flame_nltgv2_volume_mesh_begin turns a box of the volume into a triangle mesh with vertex normals on the device, on the side stream
 * beside a running solver; the volume is read only.  The reference has no counterpart: the rules are stated here in full (UNPINNED);
 * tests/volume_mesh_ref.py restates them in numpy float32 and is the checker: device and checker agree bit for bit.  All arithmetic is
 * float32 without FMA, with correctly rounded division and sqrtf.  Marching TETRAHEDRA, not marching cubes: no 256-case table, no
 * ambiguous faces, a surface that is watertight by construction.
 *
 * THE BOX.  A call works on the voxels lo[a] <= index < hi[a] per axis; all-zero hi means the whole volume.  0 <= lo < hi <= n_axis, and
 *   a box holds at most 2^26 voxels, so that 7 vertices and 12 triangles per voxel never pass int32.  A larger volume is meshed in several
 *   calls: boxes that overlap by one voxel layer tile it -- their triangles are disjoint, their union is the whole extraction, and a
 *   vertex both have has the same key, position and normal in both.
 * CUBES.  Cube (i, j, k) has its lower corner at voxel (i, j, k) and all eight corners inside the box.  It is LIVE iff all eight weights
 *   are > 0 (the raycast's rule).  A box with an axis of one voxel has no cube.
 * INSIDE.  A voxel is inside iff tsdf <= 0.0f: a NaN is outside, -0.0f inside (the raycast's "ends at the first sample <= 0").
 * TETS.  Each live cube is cut into six tetrahedra, one per permutation (a, b, c) of the axes, in the order xyz, xzy, yxz, yzx, zxy, zyx,
 *   with the corners A = c, B = c + e_a, C = c + e_a + e_b, D = c + (1, 1, 1) (Kuhn's decomposition: the face diagonals of neighbouring
 *   cubes agree, which closes the surface).
 * EDGES AND KEYS.  Every tet edge runs from a voxel, its owner, to the voxel at offset E[e],
 *   E = [(1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1)].  Its key is voxel_linear_index * 7 + e (64 bits) with the volume's
 *   linear index (k * ny + j) * nx + i: boxes agree on keys.  Keys are LOCAL to the window: they are not stable across a
 *   flame_nltgv2_volume_shift, but positions are (THE WINDOW); welding across shifts is left to the caller.
 * TRIANGLES OF A TET.  From the 4-bit mask of inside corners, bit 0 = A .. bit 3 = D.  Masks 0 and 15: none.  One corner P alone on its
 *   side, the others Q < R < S by letter: the triangle (PQ, PR, PS).  Two inside P < Q and two outside R < S: the quad PR, PS, QS, QR, split
 *   along PR - QS into (PR, PS, QS) and (PR, QS, QR).  The second and third corners are swapped where needed so that
 *   det(b - a, c - a, O - a) > 0, with a, b, c the midpoints of the three edges and O the lowest-lettered outside corner (everything doubled:
 *   exact integers): counter-clockwise seen from the outside (positive tsdf, free space).  The 6 x 16 table is generated from this rule by
 *   the checker; the device reads flame_amd/csrc/volume_mesh_table.h, written by that generator.
 * VERTICES.  One for exactly the keys that at least one triangle names: an edge with a sign change but no live cube of the box around it
 *   has none.  t = f0 / (f0 - f1) with f0 the owner's tsdf and f1 the far end's, whichever is inside; position p0 + t * (p1 - p0) per
 *   axis with p = origin + (float)(base + index) * voxel_size as in integration rule 1.  f1 == 0 puts a vertex on a corner and may give zero-area
 *   triangles: they are kept.  Non-finite tsdf values go through the arithmetic as they are.
 * NORMALS (want_normals).  The gradient at a voxel, per axis, over the neighbours inside the VOLUME (not the box) with weight > 0: both:
 *   (f+ - f-) * 0.5f; one: f+ - f0 or f0 - f-; none: 0.0f.  At a vertex n = g0 + t * (g1 - g0) per component,
 *   len = sqrtf((nx * nx + ny * ny) + nz * nz), n / len per component where len > 0, else (0, 0, 0).  It points where tsdf grows: into free
 *   space, the side the triangles face.
 * ORDER.  Vertices in ascending key order; triangles by (the cube's linear index in the volume, tet 0 .. 5, triangle 0 .. 1); a triangle's
 *   corner is the rank of its key among the vertices.  Count, scan, scatter with every element placed by rank: no counter is raced for,
 *   no floating-point atomics, two calls give the same bytes.
 * CAPACITY.  max_vertices and max_triangles, both >= 0.  The counts are always returned; the arrays are written only if BOTH fit,
 *   otherwise overflow = 1, nothing is promised about the arrays, and the caller asks again with the counts it was given
 *   (max_* = 0 is a pure count query).  The device arrays, and with copy_out the pinned ones, take room for
 *   min(max_vertices, 7 * box voxels) vertices and min(max_triangles, 12 * box voxels) triangles; between the passes the stage keeps
 *   6 bytes per voxel of the box.
 *
 * begin  checks every argument -- no volume; NULL params; a box out of range, empty or over 2^26 voxels; a negative capacity: reported
 *        before anything is enqueued, leaving the volume, an earlier view and a pending _end as they are --, then enqueues everything on
 *        the side stream.
 * end    waits, reads the counts and, with copy_out and no overflow, fetches exactly n_vertices / n_triangles elements.  The host
 *        pointers (NULL with copy_out == 0, on overflow, the normals without want_normals) and the device pointers beside them are valid
 *        until the next flame_nltgv2_volume_mesh_begin.  With copy_out == 0 only the counters travel.
 * flame_nltgv2_volume_mesh == begin with copy_out forced to 1 and want_normals = (normals_out != NULL); end; copies into the caller's
 *        arrays (each may be NULL), which hold max_vertices / max_triangles elements; nothing is copied on overflow.
 * Not done: colour, vertex welding across calls or shifts, decimation, a sparse or hashed volume. */
typedef struct flame_nltgv2_volume_mesh_params {
  int32_t lo[3];           /* 0, 0, 0 */
  int32_t hi[3];           /* 0, 0, 0    all zero: the whole volume */
  int32_t max_vertices;    /* 0 */
  int32_t max_triangles;   /* 0 */
  int32_t want_normals;    /* 1 */
  int32_t copy_out;        /* 1  0: the arrays stay on the device; only the counters travel */
} flame_nltgv2_volume_mesh_params;
void flame_nltgv2_default_volume_mesh_params(flame_nltgv2_volume_mesh_params* p);

/* 8 words.  surface_cubes: live cubes with at least one triangle. */
typedef struct flame_nltgv2_volume_mesh_counts {
  int32_t n_vertices, n_triangles, live_cubes, surface_cubes, overflow;
  int32_t reserved[3];
} flame_nltgv2_volume_mesh_counts;

typedef struct flame_nltgv2_volume_mesh_view {
  flame_nltgv2_volume_mesh_counts counts;
  float   device_ms;       /* measurement aid: HIP-event time of what begin enqueued on the side stream */
  float   pass_ms[4];      /* ... of its passes: classify, count, scan, emit (with the copies out of the counters) */
  int32_t reserved[3];
  const float*   vertices;   const void* vertices_device;    /* [3 * n_vertices] world frame */
  const float*   normals;    const void* normals_device;     /* [3 * n_vertices] */
  const int32_t* triangles;  const void* triangles_device;   /* [3 * n_triangles] */
} flame_nltgv2_volume_mesh_view;

int flame_nltgv2_volume_mesh_begin(flame_nltgv2_ctx* ctx, const flame_nltgv2_volume_mesh_params* params);
int flame_nltgv2_volume_mesh_end(flame_nltgv2_ctx* ctx, flame_nltgv2_volume_mesh_view* out);
int flame_nltgv2_volume_mesh(flame_nltgv2_ctx* ctx, const flame_nltgv2_volume_mesh_params* params, float* vertices_out, float* normals_out,
                             int32_t* triangles_out, flame_nltgv2_volume_mesh_counts* counts_out);

/* ---- Volumetric map: a window that follows the camera ------------------------------------------------------------------------------------
 * flame_nltgv2_volume_shift_begin moves THE WINDOW (above) by shift[3] voxels, any int32 triple, on the side stream beside a running
 * solver; flame_nltgv2_volume_follow says by how much, from a camera pose.  The reference has no counterpart: the rules are stated here
 * in full (UNPINNED); tests/volume_window_ref.py restates them in numpy and is the checker: device and checker agree bit for bit.
 *
 * THE SHIFT.  base' = base + shift.  Destination local voxel (i, j, k) receives the record of source local voxel
 *   (i + s.x, j + s.y, k + s.z) if that lies inside the window -- copied as 8 bytes: NaNs, -0 and payloads survive --, otherwise the
 *   fresh record {1.0f, 0.0f}.  |s_a| >= n_a on any axis clears everything: that is also how a caller jumps the window far away.
 *   |base'[a]| > 2^22 on any axis is FLAME_NLTGV2_ERR_INVALID_ARG and nothing changes.
 *   Out of place: the context keeps a second buffer of the volume's size, allocated at the first shift that moves anything (from then on
 *   flame_nltgv2_volume_info reports both buffers), writes it from the first and swaps the two behind the enqueue; every later stage is
 *   enqueued on the same side stream, so stream order covers the hazard.  Every source record is read exactly once and every destination
 *   record has exactly one writer; no floating-point atomics, no counter raced for a place: two calls give the same bytes.  The kernel
 *   moves two records per access (16 bytes) where nx and the linear displacement (s.z * ny + s.y) * nx + s.x are even and one (8 bytes)
 *   otherwise; both give the same bytes, and record_bytes says which ran.
 *   A zero shift moves nothing, allocates nothing and swaps nothing (record_bytes == 0): only the read-only count behind kept_seen is
 *   enqueued.
 * COUNTERS (8 words, summed in _end from sixteen partial sets as in the other volume stages; integer adds only).  kept: records moved;
 *   kept_seen: records moved with weight > 0; lost_seen: records with weight > 0 that left; entered: fresh records.
 *   kept + entered == nx * ny * nz, and kept_seen + lost_seen == the voxels with weight > 0 before the call.
 * begin  checks the arguments -- no volume; NULL shift; a base past the limit; no memory for the second buffer (FLAME_NLTGV2_ERR_OOM):
 *        reported before anything is enqueued, leaving the volume, the window, an earlier view and a pending _end as they are --, then
 *        enqueues everything on the side stream; the window has moved when it returns: a later begin of any volume stage sees base'.
 * end    waits for the side stream and fills *out.
 * flame_nltgv2_volume_shift == begin; end; copies the counters (counts_out may be NULL).
 *
 * FOLLOW (host arithmetic only, float32, no FMA; nothing is enqueued and nothing shifts).  With T_world_cam (12 floats, row-major
 *   [R | t]), focus_depth (the point followed lies that far along the optical axis; 0: the camera centre) and step >= 1, per axis a:
 *     c_a = t_a + focus_depth * R[a][2];  g_a = (c_a - origin_a) / voxel_size;  m_a = base_a + n_a / 2 (integer division);
 *     q_a = (int)truncf((g_a - (float)m_a) / (float)step);  shift_a = q_a * step.
 *   So the window moves in whole steps and only once the point is a whole step off the middle voxel: hysteresis.  A non-finite c_a, a
 *   quotient outside +-2^22 or a product outside int32 is FLAME_NLTGV2_ERR_INVALID_ARG, as are no volume, a NULL argument, a non-finite
 *   focus_depth and step < 1.  The base limit is flame_nltgv2_volume_shift_begin's to answer.
 *   THE PLAN.  shift[3]; the KEPT box: the voxels that stay, max(0, s_a) <= index < min(n_a, n_a + s_a) in pre-shift local indices
 *   (has_kept == 0 and all zeros if nothing stays); and n_leaving <= 3 LEAVING boxes, pre-shift local indices, the slabs in this order:
 *   the leaving x-slab over all j, k; the leaving y-slab over the kept i range and all k; the leaving z-slab over the kept i and j ranges
 *   -- each extended by one voxel layer towards the kept side.  Together with the kept box they tile the window in the sense of THE BOX:
 *   flame_nltgv2_volume_mesh of each gives disjoint triangles whose union is the whole extraction.  If anything leaves entirely
 *   (|s_a| >= n_a on an axis) the plan is one leaving box, the whole window.  The intended loop per frame: follow; volume_mesh of each
 *   leaving box (the map streamed out); volume_shift; integrate; raycast. */
typedef struct flame_nltgv2_shift_counts {
  int32_t kept, kept_seen, lost_seen, entered;
  int32_t reserved[4];
} flame_nltgv2_shift_counts;

typedef struct flame_nltgv2_shift_view {
  int32_t shift[3];        /* what begin was given */
  float   device_ms;       /* measurement aid: HIP-event time of what begin enqueued on the side stream */
  int32_t base[3];         /* the window after the shift */
  int32_t record_bytes;    /* 16 or 8: the path the kernel took; 0: a zero shift, nothing moved */
  flame_nltgv2_shift_counts counts;
} flame_nltgv2_shift_view;

typedef struct flame_nltgv2_follow_params {
  float   focus_depth;     /* 0.0   metres along the optical axis; 0: the camera centre */
  int32_t step;            /* 8     voxels, >= 1 */
} flame_nltgv2_follow_params;
void flame_nltgv2_default_follow_params(flame_nltgv2_follow_params* p);

/* 32 words.  Boxes as flame_nltgv2_volume_mesh_params takes them: lo <= index < hi, pre-shift local indices. */
typedef struct flame_nltgv2_follow_plan {
  int32_t shift[3];
  int32_t n_leaving;       /* 0 .. 3 */
  int32_t has_kept;        /* 1: kept_lo / kept_hi name a box; 0: nothing stays */
  int32_t kept_lo[3], kept_hi[3];
  int32_t leaving_lo[3][3], leaving_hi[3][3];   /* [box][axis] */
  int32_t reserved[3];
} flame_nltgv2_follow_plan;

int flame_nltgv2_volume_window(flame_nltgv2_ctx* ctx, int32_t base_out[3]);
int flame_nltgv2_volume_shift_begin(flame_nltgv2_ctx* ctx, const int32_t shift[3]);
int flame_nltgv2_volume_shift_end(flame_nltgv2_ctx* ctx, flame_nltgv2_shift_view* out);
int flame_nltgv2_volume_shift(flame_nltgv2_ctx* ctx, const int32_t shift[3], flame_nltgv2_shift_counts* counts_out);
int flame_nltgv2_volume_follow(flame_nltgv2_ctx* ctx, const float* T_world_cam, const flame_nltgv2_follow_params* params,
                               flame_nltgv2_follow_plan* plan_out);

/* ---- The debug images of Flame::update()'s last block, "Draw stuff" (flame.cc:490-511) -------------------------------------------------
 * getDebugImageInverseDepthMap and getDebugImageNormals (flame.h:294-306) from what already stands on the device: the resident dense map,
 * the rasteriser's key image, the canonical w1 / w2 and the frame's grey image.  (getDebugImageFeatures: flame_stereo_draw_features,
 * flame_stereo.h.)  Every byte is meant to equal the reference's; tests/debug_ref.py restates the operations and is the checker.
 *
 * (getDebugImageWireframe: flame_nltgv2_debug_wireframe_begin, below this block.)
 *
 * NOT covered, on purpose:
 *   cv::putText        debug_draw_text_overlay is treated as false.
 * (debug_draw_photo_error feeds on commented-out code in the reference, flame.cc:854-984; what that block computed, and a picture of
 * it, is flame_nltgv2_map_error_begin above, with its unpinned parts marked there.)
 * (getDebugImageMatches, debug_draw_matches: live code too; flame_stereo_draw_matches, flame_stereo.h.  getDebugImageDetections,
 * drawDetections, whose `score` is written at flame.cc:1249: flame_stereo_draw_detections, flame_stereo.h.  With them every
 * getDebugImage* getter of flame.h has a counterpart.)
 *
 * Pixel bytes are the reference's cv::Vec3b c[0], c[1], c[2] in that order; cvtColor(GRAY2RGB) is three equal bytes.
 *   idepth image   drawInverseDepthMap, flame.cc:2699-2719: a NaN of the map leaves the grey pixel, every other value v gives
 *                  jet(v * scene_color_scale, 0, 2) (utils/visualization.h:142-167) with C++'s promotions as written there: the first
 *                  branch is float arithmetic, the other three go through double (their 0.25 * dv, 0.5 * dv, 0.75 * dv literals); the
 *                  result is truncated to uint8_t.
 *   w1 / w2 maps   w1_map_ / w2_map_, flame.cc:498-503: interpolateMesh(triangles, vtx, vtx_w1 [vtx_w2], all valid, all valid), NaN where
 *                  no triangle covers the pixel.  The winning triangle of a pixel is the same for every attribute and its index stands in
 *                  the rasteriser's key image, so they cost no second and third rasterisation -- unless the resident map was rasterised
 *                  with a validity mask (tri_valid != NULL): then the rasteriser runs twice into buffers of this stage.  Same values.
 *   normals image  drawNormals, flame.cc:2667-2697: planeParamToNormal (flame.cc:2643-2663) at u = (col, row), evaluated AS WRITTEN, its
 *                  quirks included: K(0,0) and K(1,1) stand where one would expect the principal point.  Float subexpressions stay
 *                  float; a, b, d, nx, ny, nz are double; the normal is cast to float, normalised (a no-op unless the squared norm is
 *                  > 0, sums left to right: the conventions of flame_nltgv2_mesh_outputs) and negated.  normalMap
 *                  (utils/visualization.h:119-130) is painted only where normal(2) > 0.0f; a NaN anywhere leaves the grey pixel.
 *   flip           debug_flip_images, cv::flip(img, img, -1): the unflipped image in reversed linear pixel order.  The w maps are not
 *                  images and are never flipped. */
typedef struct flame_nltgv2_debug_image_params {
  float   scene_color_scale;  /* 1.0  params.h:109 */
  int32_t flip;               /* 0    debug_flip_images */
  int32_t want_idepthmap;     /* 1    drawInverseDepthMap, flame.cc:2699-2719 */
  int32_t want_normals;       /* 1    flame.cc:497-506 + drawNormals, flame.cc:2667-2697 */
} flame_nltgv2_debug_image_params;
void flame_nltgv2_default_debug_image_params(flame_nltgv2_debug_image_params* p);

/* Pointers into pinned memory of the context, valid until the next flame_nltgv2_debug_images_begin. */
typedef struct flame_nltgv2_debug_images_view {
  int32_t rows, cols;
  const uint8_t* idepthmap_img;  /* [rows * cols * 3] debug_img_idepthmap_; NULL: not asked for */
  const uint8_t* normals_img;    /* [rows * cols * 3] debug_img_normals_; NULL: not asked for */
  const float* w1_map;           /* [rows * cols] w1_map_, NaN where uncovered; NULL without want_normals */
  const float* w2_map;           /* [rows * cols] w2_map_ */
  float device_ms;               /* measurement aid: HIP-event time of the stage on the side stream, kernels and copies out */
} flame_nltgv2_debug_images_view;

/* begin  checks the arguments -- an error (no graph; no resident map, or one of another size than rows x cols; no resident triangles for
 *        the current topology; both or neither image pointer; step_bytes < cols; K or params NULL) is reported before anything is enqueued
 *        and leaves the outputs of an earlier begin as they are --, then enqueues everything on the context's side stream, beside a running
 *        solver, and returns.
 *        The grey image is fnew_->img[0]: rows of cols bytes, step_bytes apart, in host memory (img_host: staged through pinned memory;
 *        the caller's buffer is free when begin returns) or in device memory (img_device, e.g. flame_stereo_frame_image_device: nothing
 *        is uploaded; it must stay valid until _end).  Exactly one of the two is non-NULL.  K: 9 floats row-major (Flame::K_).
 *        WHICH MAP AND WHICH STATE: the inverse-depth map is the resident unfiltered map the last flame_nltgv2_interpolate_mesh[_begin]
 *        left on the device, the triangles are the ones that call left there (as flame_nltgv2_mesh_outputs_begin(triangles = NULL) uses
 *        them), and w1 / w2 are read from the state flame_nltgv2_interpolate_mesh_begin would read (FLAME_NLTGV2_OPT_MESH_STATE decides
 *        in the same way) -- so a debug_images_begin right behind an interpolate_mesh_begin describes the state of that map.
 *        The resident map, the pinned map of interpolate_mesh_end, the buffers of mesh_outputs and the key image are only read.
 * end    waits for the side stream and fills *out.
 * flame_nltgv2_debug_images == begin; end; copies into the caller's arrays (each may be NULL). */
int flame_nltgv2_debug_images_begin(flame_nltgv2_ctx* ctx, const uint8_t* img_host, const void* img_device, int step_bytes,
                                    const float* K, const flame_nltgv2_debug_image_params* params, int rows, int cols);
int flame_nltgv2_debug_images_end(flame_nltgv2_ctx* ctx, flame_nltgv2_debug_images_view* out);
int flame_nltgv2_debug_images(flame_nltgv2_ctx* ctx, const uint8_t* img_host, const void* img_device, int step_bytes, const float* K,
                              const flame_nltgv2_debug_image_params* params, int rows, int cols, uint8_t* idepthmap_img_out,
                              uint8_t* normals_img_out, float* w1_map_out, float* w2_map_out);

/* ---- getDebugImageWireframe (flame.h, drawWireframe flame.cc:2414-2457 at its call site flame.cc:491-494) ---------------------------------
 * drawColorMappedWireframe (utils/image_utils.h:693-719) over applyColorMapLine (utils/visualization.h:235-260), from the resident
 * triangles, the canonical pos / x and the frame's grey image.  The reference draws SEQUENTIALLY and blends: a pixel's final value
 * depends on every draw that touched it, in draw order.  OpenCV is not part of this tree, so the rule is stated here in full; every byte
 * follows from it, and tests/wireframe_ref.py restates it sequentially and is the checker.
 *   1 endpoints   cv::Point2f -> cv::Point is cvRound, round half to even (2.5 -> 2, 3.5 -> 4), per coordinate, as the rasteriser does it.
 *   2 the walk    cv::LineIterator(img, pt1, pt2), OpenCV 3.2, connectivity 8, starting AT pt1 (not left to right), restated -- UNPINNED:
 *                 dx = x2 - x1, dy = y2 - y1; sx, sy their signs; dx, dy their absolute values; if dy > dx (strict) y is the major axis
 *                 and dx, dy are swapped; err = dx - 2 dy; count = dx + 1.  After visiting a pixel: m = err < 0;
 *                 err += -2 dy + (m ? 2 dx : 0); one pixel along the major axis and, if m, also one along the minor axis.
 *                 (0,0)->(2,1) visits (0,0) (1,0) (2,1); (2,1)->(0,0) visits (2,1) (1,1) (0,0): direction matters.
 *   3 value       slope0 = (B_val - A_val) / (float)count; pixel ii (0 .. count - 1) has val = A_val + (float)ii * slope0, in float
 *                 without FMA (B's value is never reached); its colour is jet(val * scene_color_scale, 0, 2) exactly as in the idepth
 *                 image above, the NaN colour (0, 0, 255) included (UNPINNED).  A_val, B_val are x * graph_scale (vtx_idepths_).
 *   4 blend       alpha = 0.5 (flame.cc:2432): color * 0.5f + old * 0.5f is exact in float and the store into a uchar truncates, so per
 *                 channel new = (color + old) >> 1.  A pixel starts at its grey value and folds its draws in increasing draw id,
 *                 id = 3 * triangle + k, k = 0: v0 -> v1, k = 1: v1 -> v2, k = 2: v0 -> v2.  One draw visits a pixel at most once.
 *   5 validity    a triangle is drawn iff its tri_valid byte is non-zero (the reference's vtx_validity is all true).
 *   6 outside     DEVIATES from the reference, which clips with cv::clipLine -- UNPINNED; the pipeline never needs it (projectGraph drops
 *                 out-of-image vertices, flame.cc:1922).  Here a line with a non-finite endpoint coordinate, or a ROUNDED endpoint outside
 *                 [0, cols - 1] x [0, rows - 1], is not drawn at all and counted in lines_skipped; the other lines of its triangle are
 *                 drawn.  Nothing is written outside the image for any input.
 *   7 flip        cv::flip(img, img, -1): the finished picture in reversed linear pixel order.  No text overlay.
 * == scene_color_scale params.h:109, debug_flip_images, and where the triangle validity comes from. */
typedef struct flame_nltgv2_wireframe_params {
  float   scene_color_scale;  /* 1.0 */
  int32_t flip;               /* 0 */
  int32_t validity;           /* 0: every triangle is valid (tri_valid must be NULL); 1: tri_valid is a host array of T bytes;
                                 2: the validity the last flame_nltgv2_mesh_outputs_begin left on the device for the resident
                                    triangles (tri_valid must be NULL; an error if there is none for the current triangles and topology) */
} flame_nltgv2_wireframe_params;
void flame_nltgv2_default_wireframe_params(flame_nltgv2_wireframe_params* p);

/* Pointers into pinned memory of the context, valid until the next flame_nltgv2_debug_wireframe_begin. */
typedef struct flame_nltgv2_wireframe_view {
  int32_t rows, cols;
  const uint8_t* wireframe_img;  /* [rows * cols * 3] debug_img_wireframe_ */
  int32_t lines_drawn;           /* lines of valid triangles that were walked */
  int32_t lines_skipped;         /* lines of valid triangles left out by rule 6; drawn + skipped = 3 * valid triangles */
  int64_t entries;               /* pixel visits of all draws together */
  int32_t refilled;              /* 1: the entries did not fit the stage's buffer, and _end grew it and repeated the second half */
  float device_ms;               /* measurement aid: HIP-event time of the stage on the side stream, kernels and copy out */
} flame_nltgv2_wireframe_view;

/* begin  checks the arguments -- an error (no graph; no resident triangles for the current topology; rows / cols <= 0 or > 32767, or more
 *        than 2^31 possible pixel visits; both or neither image pointer; step_bytes < cols; params NULL; validity outside 0..2; a tri_valid
 *        pointer with validity != 1 or none with validity == 1; validity == 2 without a matching flame_nltgv2_mesh_outputs_begin) is
 *        reported before anything is enqueued and leaves the outputs of an earlier begin as they are --, then enqueues everything on the
 *        context's side stream, beside a running solver, and returns.  The triangles are the ones the last
 *        flame_nltgv2_interpolate_mesh[_begin] or flame_nltgv2_mesh_outputs_begin left on the device; pos and x are read from the state
 *        flame_nltgv2_interpolate_mesh_begin would read.  The grey image is given as in flame_nltgv2_debug_images_begin (a device image
 *        must stay valid until _end).  rows x cols need not be the resident map's size: the map is not read.  The buffers, pinned outputs
 *        and pending _end of flame_nltgv2_mesh_outputs_begin and flame_nltgv2_debug_images_begin are left alone, and they leave this
 *        stage's alone.  Only the first kernel reads pos / x: whoever rewrites them waits for that kernel, not for the picture.
 * end    waits for the side stream and fills *out.  The entry buffer holds max(2 * rows * cols, 1.25 * the last call's entries) and never
 *        shrinks; where a call's entries exceed it, _end grows it, repeats fill and fold, waits again and sets refilled: the picture
 *        is exact either way, and begin never waits for a count.
 * flame_nltgv2_debug_wireframe == begin; end; copies into the caller's array and counters (each may be NULL). */
int flame_nltgv2_debug_wireframe_begin(flame_nltgv2_ctx* ctx, const uint8_t* img_host, const void* img_device, int step_bytes,
                                       const uint8_t* tri_valid, const flame_nltgv2_wireframe_params* params, int rows, int cols,
                                       float graph_scale);
int flame_nltgv2_debug_wireframe_end(flame_nltgv2_ctx* ctx, flame_nltgv2_wireframe_view* out);
int flame_nltgv2_debug_wireframe(flame_nltgv2_ctx* ctx, const uint8_t* img_host, const void* img_device, int step_bytes,
                                 const uint8_t* tri_valid, const flame_nltgv2_wireframe_params* params, int rows, int cols,
                                 float graph_scale, uint8_t* wireframe_img_out, int32_t* lines_drawn_out, int32_t* lines_skipped_out);

/* 2-D Delaunay triangulation of float32 points: the counterpart of utils::Delaunay
 * (src/flame/utils/delaunay.{h,cc}, a wrapper of the vendored Shewchuk Triangle called with "zneQB",
 * delaunay.cc:66-68) that feeds Flame::syncGraph its edge list (flame.cc:2073-2104) and interpolateMesh its
 * triangles.  HOST code, like the reference's; exact predicates, so a point set in
 * general position yields the same set of triangles as Triangle.  Triangles are counter-clockwise in
 * x-right / y-up coordinates (Triangle's convention); edges are unique undirected pairs.  Pass NULL for
 * `triangles` / `edges` to query the counts (Euler: T <= 2n - 5, E <= 3n - 6).  Needs no context, no GPU. */
int flame_delaunay_triangulate(const float* xy, int32_t n, int32_t* triangles, int32_t tri_capacity,
                               int32_t* n_triangles, int32_t* edges, int32_t edge_capacity, int32_t* n_edges);

/* Per-vertex photometric residual (BASELINE config 5).  No live reference counterpart: the only
 * occurrence is the commented-out block flame.cc:854-893; built from the live pieces
 * EpipolarGeometry::project (stereo/epipolar_geometry.h:127-143) and utils::bilinearInterp<uint8_t,float>
 * (utils/image_utils.h:230-255).  err[v] = |I_cmp(project(pos_v, x_v*graph_scale)) - I_ref(pos_v)|, NaN
 * where either pixel is outside [border, size-border).  An epilogue: it never modifies x.
 * KRKinv: 9 floats row-major, Kt: 3 floats (EpipolarGeometry::loadGeometry, h:88-93).
 * Images: rows of cols bytes, step_bytes >= cols apart; (rows - 1) * step_bytes + cols bytes are read. */
int flame_nltgv2_photo_set_images(flame_nltgv2_ctx* ctx, const uint8_t* ref, const uint8_t* cmp, int rows, int cols,
                                  int step_bytes);
int flame_nltgv2_photo_residual(flame_nltgv2_ctx* ctx, const float* KRKinv, const float* Kt, float graph_scale,
                                int border, float* err_out);
/* Standing form of the same residual, computed as part of the solver's own launch (BASELINE config 5: "photometric
 * data-term residual fused into the primal step"): while enabled, every run()/run_async() leaves the residual of its
 * final x in a device buffer -- the persistent kernels evaluate it in their epilogue, right after the last primal
 * step, from the registers that hold x; the one-launch-per-step path appends one sweep.  It never feeds back into x.
 * flame_nltgv2_photo_residual_last copies that buffer out (V floats, caller's vertex order; no kernel is launched) --
 * unless the graph, the state, the images or the target changed after the last run (upload, sync, projection, rescale,
 * single solver steps, new images, photo_fuse again) or flame_nltgv2_photo_residual used the buffer for its own target:
 * then it computes the residual of the current pos and x for the standing target with the stand-alone sweep first.  The images are those of flame_nltgv2_photo_set_images; enable = 0 switches it off. */
int flame_nltgv2_photo_fuse(flame_nltgv2_ctx* ctx, const float* KRKinv, const float* Kt, float graph_scale, int border,
                            int enable);
int flame_nltgv2_photo_residual_last(flame_nltgv2_ctx* ctx, float* err_out);

/* Options (flame_nltgv2_set_option).  These are the stable surface; a caller never needs any of them -- every default is the
 * measured best.  (Tuning knobs and test hooks of the current kernels, numbers 100 and up, live in a test-only header.) */
enum {
  FLAME_NLTGV2_OPT_SOLVER = 1,       /* 0 = fused / persistent kernels (default), 1 = the reference's four loops one by one
                                        (save_prev / dual / primal / extragradient sweeps on the canonical arrays) */
  FLAME_NLTGV2_OPT_USE_HIPGRAPH = 2, /* 1 (default) = the one-launch-per-step path replays its launches from a hipGraph */
  FLAME_NLTGV2_OPT_PERSISTENT = 5,   /* 1 (default) = run() uses ONE persistent launch for all n_iters steps when the graph
                                        fits on the chip, picking the form by size; 3 = the vertex-per-lane form by name,
                                        4 = the patch-per-wave form by name, 6 = the patch-per-wave form with two half-edges
                                        per lane by name -- each only if it fits; 0 = always one launch per step.  (2 was round 1's
                                        lane-per-half-edge form, retired in round 3; 7 was round 5's region-per-workgroup form, measured
                                        15 % slower than the patch-per-wave form at every BASELINE size -- profiles/r05_wg_region.txt --
                                        and taken out in round 6; 2, 5 and 7: invalid argument) */
  FLAME_NLTGV2_OPT_PROBE = 12,       /* 1 = the patch-per-wave kernel records a per-patch, per-step cycle probe (8 words:
                                        HW id, XCC id, wait cycles, compute cycles, poll rounds, step start, 100 MHz clock,
                                        0), read with flame_nltgv2_read_probe; 0 (default) = off */
  FLAME_NLTGV2_OPT_VERIFY_RECORDS = 14, /* persistent kernels: 1 = after a neighbour record's tag matched, read the 16 bytes
                                        once more and compare all four dwords (the exchange relies on an aligned 16-byte
                                        access never being torn between payload and tag; this checks it at run time, at the
                                        price of one more load round trip per step); a difference takes the run back like a
                                        timeout and counts in flame_nltgv2_info.torn_records_detected.  2 = the same plus a
                                        test hook that corrupts one re-read.  0 (default) = off */
  FLAME_NLTGV2_OPT_PLACEMENT = 16,   /* patch-per-wave form on all eight XCDs: 1 (default) = the records another XCD reads are
                                        placed on memory pages whose home channel suits that pair of XCDs (a hand-off across
                                        XCDs takes 0.39-0.66 us depending on the page; measured once per context, ~3 ms at
                                        the first such run), 0 = every record at its linear place.  Addresses only: results
                                        are bit-identical either way */

  FLAME_NLTGV2_OPT_SYNC_PATH = 17,   /* flame_nltgv2_sync_graph: 0 (default) = index maps and the new graph's layout tables are built on the
                                        device wherever that applies (a duplicate-free edge list -- edges_unique --, no vertex of more than 64
                                        edges; feature ids of any magnitude), on the host otherwise; 1 = always on the host; 2 = on the device or
                                        FLAME_NLTGV2_ERR_INVALID_ARG.  Same result either way */

  FLAME_NLTGV2_OPT_COST_SUM = 18,    /* flame_nltgv2_costs: 0 (default) = the addends are summed sequentially in float, in the reference's edge
                                        order and the caller's vertex order, on the host: smoothnessCost equals the reference's to the last
                                        bit; 1 = both sums on the device in a fixed strided / pairwise order (a few microseconds, no copy of
                                        2E + V floats; agrees with the sequential sums to ~1e-6 relative) */

  FLAME_NLTGV2_OPT_MESH_STATE = 19,  /* flame_nltgv2_interpolate_mesh_begin with runs enqueued since the last call that settled the solver:
                                        0 (default) = waits for them and rasterises the state they leave; 1 = rasterises the state that
                                        call left (the canonical arrays as they have stood since: a run works on its packed copies) and
                                        waits for nothing -- the runs in flight go on beside the rasteriser.  The reference's
                                        interpolateMesh reads whatever iterate its solver thread has reached (flame.cc:372-380 under
                                        graph_mtx_): the state right after syncGraph is one of them.  What a frame loop gains: it can
                                        enqueue the next round BEFORE it prepares the mesh (SolverLoop::withDevice(f, g)) */

  FLAME_NLTGV2_OPT_EXPERIMENTAL = 100 /* option numbers from here on are tuning knobs and test hooks of the current kernels: declared in
                                         flame_amd/csrc/flame_nltgv2_test_options.h (tests and tools only), not part of this surface */
};
int flame_nltgv2_set_option(flame_nltgv2_ctx* ctx, int option, int value);

typedef struct flame_nltgv2_info {
  int32_t abi_version;
  int32_t device;
  int32_t V, E;
  int32_t n_slices;        /* 64-vertex slices of the packed (SELL-64) layout */
  int32_t max_degree;
  int64_t padded_half_edges; /* slots in the packed half-edge arrays (>= 2*E) */
  int64_t device_bytes;    /* device memory held by the context */
  int64_t algorithmic_bytes_per_iter; /* 64*V + 40*E, SURVEY.md section 8(d) */
  int32_t compute_units;
  char device_name[64];
  char gcn_arch[32];
  int32_t last_run_path; /* 0 none, 1 persistent launch (lane per half-edge), 2 one launch per step
                            (hipGraph), 3 one launch per step (eager), 4 four canonical sweeps per step,
                            5 persistent launch (vertex per lane), 6 persistent launch (patch per wave),
                            7 persistent launch (patch per wave, two half-edges per lane)  (8 was the region-per-workgroup
                            form of ABI 5) */
  int32_t he_waves;      /* always 0 (the lane-per-half-edge form, retired in round 3; kept for the layout of the struct) */
  int32_t tv_waves;      /* waves of the vertex-per-lane persistent form (0: not applicable) */
  int32_t tv_wave_capacity; /* vertex-per-lane waves the device keeps resident */
  int32_t last_run_groups;  /* persistent launches the last run was split into (groups of whole components) */
  int32_t timeouts_recovered; /* persistent runs whose wait expired: state rolled back, steps redone one launch per step */
  int32_t patches;       /* waves (patches of ~10 vertices) of the patch-per-wave persistent form (0: not applicable) */
  int32_t torn_records_detected; /* persistent runs stopped by FLAME_NLTGV2_OPT_VERIFY_RECORDS (a record whose second
                                    read differed from the first): rolled back and redone the same way */
  int32_t last_sync_path; /* flame_nltgv2_sync_graph: 0 none yet, 1 index maps + layout tables on the host, 2 on the device */
  int32_t last_run_waves_per_cu; /* waves per compute unit of the last persistent run's largest launch (0: none) */
  int32_t reserved0, reserved1; /* always 0 (ABI 5: regions, region_depth of the region-per-workgroup form; kept for the layout of the struct) */
  int32_t replays_per_step; /* expired chains whose persistent replay (reduced residency) expired too: redone one launch per step */
} flame_nltgv2_info;
int flame_nltgv2_get_info(flame_nltgv2_ctx* ctx, flame_nltgv2_info* info);

/* Error reporting. */
int flame_nltgv2_last_error(flame_nltgv2_ctx* ctx);     /* last non-OK status of this context */
int flame_nltgv2_last_hip_error(flame_nltgv2_ctx* ctx); /* raw hipError_t of the last HIP failure */
const char* flame_nltgv2_status_string(int status);
int flame_nltgv2_abi_version(void);

/* Measurement aid: copies out the cycle probe the last patch-per-wave run recorded (FLAME_NLTGV2_OPT_PROBE):
 * [patch][step][8] words; *n_words = words available.  Not part of the reference's surface. */
int flame_nltgv2_read_probe(flame_nltgv2_ctx* ctx, uint32_t* out, int64_t max_words, int64_t* n_words);

/* Measurement aid: the record placement (FLAME_NLTGV2_OPT_PLACEMENT).  *state: 1 = the page ranking of the device is known (measured
 * once per device and process, when the first context is created), 0 = not yet (the measurement did not complete then: the first run
 * that can use it tries again), -1 = unavailable (it did not complete then either; records keep their linear places).
 * *placed_records = records of the current topology that were given a place in the pool (per step parity);
 * us[0..2] = one-way hand-off by choice of page as the calibration measured it, mean over the XCD pairs: the best page,
 * the mean page, the worst page.  Any output pointer may be NULL.  Not part of the reference's surface. */
int flame_nltgv2_placement_info(flame_nltgv2_ctx* ctx, int32_t* state, int32_t* placed_records, float* us);

/* Test hook: the layout arrays the device expanded for the current topology (nltgv2_layout.hip) compared word for word
 * with the host builders (nltgv2_pack.hpp); *mismatches = number of differing words -- plus, when records are placed, the
 * number of placed offsets that are misaligned, out of the pool or given out twice. */
int flame_nltgv2_layout_selftest(flame_nltgv2_ctx* ctx, int64_t* mismatches);
/* Host-only packing probe (no device needed; used by the CPU test-suite): builds the packed
 * SELL-64 layout the fused sweep runs on and copies it out.  Any output pointer may be NULL.
 *   perm[n_slices*64]       packed slot -> original vertex id (-1 = padding lane)
 *   slice_row[n_slices+1]   first 64-wide row of each slice in the half-edge arrays
 *   rec_nbr[rows*64]        packed neighbour index | role<<31 (role 1: this vertex is the TARGET)
 *   rec_edge[rows*64]       original edge id of the slot (-1 = empty)
 * Returns n_slices (>= 0) or a negative status; *rows_out receives the number of 64-wide rows. */
int flame_nltgv2_pack_probe(const flame_nltgv2_graph* g, int32_t* perm, int32_t* slice_row,
                            int32_t* rec_nbr, int32_t* rec_edge, int64_t capacity_rows, int64_t* rows_out);

#ifdef __cplusplus
}
#endif
#endif /* FLAME_NLTGV2_H_ */
