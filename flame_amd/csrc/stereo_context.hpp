// stereo_context.hpp -- the context behind include/flame_stereo.h and what its entry points share (stereo_capi.hip,
// stereo_front_capi.hip, stereo_debug_align_capi.hip): buffers that own themselves and how they grow, the resident frames and their
// spare buffer sets, SCHK / enter, the timed launch and the decode of a stage's error words.  The pure part is stereo_host.hpp.
#ifndef FLAME_AMD_STEREO_CONTEXT_HPP_
#define FLAME_AMD_STEREO_CONTEXT_HPP_

#include <hip/hip_runtime.h>

#include <unordered_map>
#include <utility>
#include <vector>

#include "flame_stereo.h"
#include "stereo_kernels.h"
#include "feature_kernels.h"
#include "align_kernels.h"
#include "stereo_host.hpp"

namespace flame_hip {

// `cap` elements of device memory, or with kPinned of pinned host memory, freed with the array; reads as its pointer.  Allocated
// once, or grown by grow() / grow_keep().
template <typename T, bool kPinned = false>
struct Array {
  T* p = nullptr;
  size_t cap = 0;
  Array() = default;
  Array(const Array&) = delete;
  Array& operator=(const Array&) = delete;
  ~Array() { (void)release(); }
  operator T*() const { return p; }
  hipError_t alloc(size_t count) {  // (of an empty array)
    const size_t bytes = count * sizeof(T);
    const hipError_t e = kPinned ? hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) : hipMalloc((void**)&p, bytes);
    if (e == hipSuccess) cap = count;
    return e;
  }
  hipError_t release() {
    const hipError_t e = !p ? hipSuccess : kPinned ? hipHostFree(p) : hipFree(p);
    if (e == hipSuccess) p = nullptr, cap = 0;
    return e;
  }
  void swap(Array& o) { std::swap(p, o.p), std::swap(cap, o.cap); }
};

// The buffer set of a resident frame: a plain record, released by free_frame() alone, so that a set can move into
// flame_stereo_ctx::spare and back without a hipFree.
struct Frame {
  uint8_t* img_pad = nullptr;
  float* gx_pad = nullptr;
  float* gy_pad = nullptr;
  uint8_t* pyr = nullptr;  // levels >= 1 (align_host.hpp, place_levels), allocated by the first build_pyramid; travels with the set
  int pyr_levels = 0;      // n_levels of the last build_pyramid; 0: none since the frame was added
};

// The stream and the two events: a base of the context, so that they outlive its arrays (flame_stereo_destroy: release, then these).
struct StereoStreams {
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  ~StereoStreams() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (own_stream) (void)hipStreamDestroy(own_stream);
  }
};

}  // namespace flame_hip

struct flame_stereo_ctx : flame_hip::StereoStreams {
  template <typename T> using Dev = flame_hip::Array<T>;
  template <typename T> using Pinned = flame_hip::Array<T, true>;
  using StereoFeature = flame_hip::StereoFeature;

  int device = 0;
  bool timed = false;
  int last_hip = 0;
  bool have_camera = false;
  flame_hip::StereoCamera cam{};
  std::unordered_map<uint32_t, flame_hip::Frame> frames;
  // buffers of dropped frames, reused by the next add_frame: hipFree waits for every stream of the device, also for a solver that runs
  // beside the tracker (tools/frame_loop.py --pipelined: 0.5 ms per frame).  At most kSpareFrames of them (release_frame).
  std::vector<flame_hip::Frame> spare;
  Dev<uint8_t> d_raw;  // staging of the unpadded upload; the rectified grey image of add_raw_frame
  // add_raw_frame (input_kernels.hip)
  bool have_input = false;  // set_input since the last set_camera
  flame_stereo_input_params input{};
  Dev<uint8_t> d_rawsrc;  // staging of a raw frame that comes from the host
  Dev<int> d_istats; Pinned<int> h_istats;  // kInputWords ints each
  Dev<flame_hip::StereoPoseEntry> d_poses; Pinned<flame_hip::StereoPoseEntry> h_poses;
  Dev<StereoFeature> d_feats;
  Dev<int> d_stats; Pinned<int> h_stats;  // kStatWords ints each
  Dev<StereoFeature> d_res;  // the resident feature set (flame_stereo_set_features)
  int n_res = 0;
  int lanes_per_feature = 0;  // 0 = by feature count (pick_lanes)
  // projectFeatures / detectFeatures (feature_kernels.hip)
  Dev<StereoFeature> d_res_alt;          // the other buffer of the resident set's ping-pong pair
  Dev<StereoFeature> d_proj, d_proj_alt;  // the projected set (Flame::feats_in_curr_) and its other buffer
  int n_proj = 0;
  Dev<StereoFeature> d_proj_tmp;  // one projected record per resident feature
  Dev<uint8_t> d_keep;
  Dev<int> d_groups;  // per-workgroup counts of the compactions
  Dev<flame_hip::ProjectPoseEntry> d_ppose;
  Dev<uint32_t> d_keep_ids;  // prune_pose_frames: the ids of the kept pose-frames
  Dev<unsigned long long> d_cell_key;
  Dev<uint8_t> d_blocked;
  Dev<float> d_map;   // a host idepth map, uploaded
  Dev<float> d_mask;  // a host mask, uploaded
  Dev<int> d_fstats; Pinned<int> h_fstats;  // kFrontWords ints each
  // select_graph_features (feature_kernels.hip)
  bool aligned = false;  // the resident and the projected set are index-aligned (set by project_features)
  Dev<flame_hip::SelectPoseEntry> d_spose;
  Dev<int> d_sel; Pinned<int> h_sel;  // the output block: kFrontWords stats words + 6 words per record
  int graph_copy = 0;  // FLAME_STEREO_OPT_GRAPH_COPY
  // draw_features (debug_kernels.hip): per-pixel owner words + the two counters behind them, and the image;
  // draw_detections (detections_kernels.hip) keeps its kDetWords stats words in d_owner and paints into d_draw too
  Dev<uint32_t> d_owner;
  Dev<uint8_t> d_draw;
  // draw_matches (matches_kernels.hip): the draw records of the last update, and the lists of the fold
  int record_matches = 0;  // FLAME_STEREO_OPT_RECORD_MATCHES
  Dev<flame_hip::MatchRecord> d_match;
  bool match_stand = false;  // records of an enqueued update stand (whether it hit an assert shows in h_stats once the stream is idle)
  int match_n = 0;
  uint32_t match_frame = 0;
  Dev<uint32_t> d_mlist;  // cnt, offset, fill (one word per pixel each) and the kMatchCounts counters behind them
  Dev<uint64_t> d_mentries;
  size_t match_last_total = 0;
  // align_linearize / align_frame (align_kernels.hip)
  Dev<double> d_apart;  // [kAlignSums][chunks] partials
  Dev<flame_hip::AlignSystem> d_asys; Pinned<flame_hip::AlignSystem> h_asys;  // allocated by the first alignment
};

namespace flame_hip {

#define SCHK(ctx, expr)                  \
  do {                                   \
    hipError_t _e = (expr);              \
    if (_e != hipSuccess) {              \
      (ctx)->last_hip = (int)_e;         \
      return _e == hipErrorOutOfMemory ? FLAME_NLTGV2_ERR_OOM : FLAME_NLTGV2_ERR_HIP; \
    }                                    \
  } while (0)

inline int enter(flame_stereo_ctx* ctx) {
  if (!ctx) return FLAME_NLTGV2_ERR_INVALID_ARG;
  SCHK(ctx, hipSetDevice(ctx->device));
  return 0;
}

inline void free_frame(Frame& f) {
  for (void* p : {(void*)f.img_pad, (void*)f.gx_pad, (void*)f.gy_pad, (void*)f.pyr})
    if (p) (void)hipFree(p);
  f = Frame{};
}

inline void drop_all_frames(flame_stereo_ctx* ctx) {
  for (auto& kv : ctx->frames) free_frame(kv.second);
  ctx->frames.clear();
  for (Frame& f : ctx->spare) free_frame(f);  // (the camera changes: another padded size)
  ctx->spare.clear();
}

// The buffers of a frame that leaves go to `spare` for the next add_frame, up to kSpareFrames sets; the rest is freed
// (hipFree waits for the device).  4 covers the steady state of a front-end that drops one non-pose frame per frame and
// prunes one or two pose-frames every few frames, and bounds the idle memory at 4 x 3 padded planes (72 MB at 1080p).
constexpr size_t kSpareFrames = 4;
inline void release_frame(flame_stereo_ctx* ctx, std::unordered_map<uint32_t, Frame>::iterator it) {
  it->second.pyr_levels = 0;  // (the levels go with the frame; their buffer stays with the set)
  if (ctx->spare.size() < kSpareFrames) ctx->spare.push_back(it->second); else free_frame(it->second);
  ctx->frames.erase(it);
}

inline size_t padded_pixels(const StereoCamera& c) { return (size_t)(c.width + 2 * c.border) * (size_t)(c.height + 2 * c.border); }
inline int padded_pitch(const StereoCamera& c) { return c.width + 2 * c.border; }
// Pixel (0, 0) of a frame's padded plane; its rows are padded_pitch() apart.
template <typename T>
T* interior(const StereoCamera& c, T* plane) { return plane + host::interior_offset(c.border, padded_pitch(c)); }

// The buffer set of frame `frame_id` for add_frame / add_raw_frame to fill: the one the id has (adding an existing id replaces
// it), else one from `spare`, else a new one.  On failure the id is not resident.
inline int acquire_frame(flame_stereo_ctx* ctx, uint32_t frame_id, Frame** out) {
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
      SCHK(ctx, e);
    }
  }
  f.pyr_levels = 0;  // (a replaced frame's levels describe the old image)
  *out = &f;
  return 0;
}

// Room for `count` elements; what the array held is lost.  Frees before it allocates.
template <typename T, bool kPinned>
int grow(flame_stereo_ctx* ctx, Array<T, kPinned>& a, size_t count) {
  if (a.cap >= count) return 0;
  SCHK(ctx, a.release());
  SCHK(ctx, a.alloc(kPinned ? host::grown_pinned(count) : host::grown(count)));
  return 0;
}

// grow() for the resident set when it is appended to: the first `keep` records move to the new buffer, which is allocated and
// filled before the old one is freed.
template <typename T>
int grow_keep(flame_stereo_ctx* ctx, Array<T>& a, size_t count, size_t keep) {
  if (a.cap >= count) return 0;
  Array<T> next;
  SCHK(ctx, next.alloc(host::grown(count)));
  if (keep > 0) {
    hipError_t e = hipMemcpyAsync(next.p, a.p, keep * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
      ctx->last_hip = (int)e;
      return FLAME_NLTGV2_ERR_HIP;  // (`next` frees itself)
    }
  }
  SCHK(ctx, a.release());
  a.swap(next);
  return 0;
}

// Enqueues what `enqueue` enqueues between the two events flame_stereo_last_kernel_ms reads.  `enqueue` returns the first error.
template <typename F>
int timed(flame_stereo_ctx* ctx, F&& enqueue) {
  SCHK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  SCHK(ctx, (hipError_t)enqueue());
  SCHK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  ctx->timed = true;
  return 0;
}

// The status of a stage whose kernels left `assert_idx` and `bad_frame_idx`; on an error *error_index (if given) names the record.
inline int decode_error(int assert_idx, int bad_frame_idx, host::ErrorRule rule, int* error_index) {
  const host::FirstError e = host::first_error(assert_idx, bad_frame_idx, rule);
  if (e.kind == host::ErrorKind::kNone) return 0;
  if (error_index) *error_index = e.index;
  return e.kind == host::ErrorKind::kAssert ? FLAME_NLTGV2_ERR_ASSERT : FLAME_NLTGV2_ERR_INVALID_ARG;
}

}  // namespace flame_hip

#endif  // FLAME_AMD_STEREO_CONTEXT_HPP_
