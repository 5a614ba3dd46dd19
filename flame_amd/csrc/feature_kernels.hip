// feature_kernels.hip -- gfx950 kernels of the two stages that create and remove features of the resident set
// (include/flame_stereo.h: flame_stereo_project_features, flame_stereo_detect_features).
//
// projectFeatures (src/flame/flame.cc:1754-1860 of the reference):
//   k_project_flag     one lane per feature: pose-frame lookup, EpipolarGeometry::project(u, idepth, &u_cur,
//                      &idepth_cur), the valid-region test, the projected record into a scratch array, a keep flag
//                      and the number kept per workgroup of 256.
//   k_project_scatter  one lane per feature: its rank = the counts of the workgroups before it (each workgroup sums
//                      them; there are n / 256) + a ballot prefix inside the workgroup; a stable scatter of the kept
//                      resident records and their projected records into the other buffer of each ping-pong pair (the
//                      host swaps the pairs only when no feature asserted).
//
// detectFeatures, live single-pass part (flame.cc:1000-1058) + the detection loop's initialisation (flame.cc:736-757):
//   k_detect_mask      one lane per mask point: clears the cell the point falls in (idempotent stores).
//   k_detect_cells     one wave per cell: the lanes walk the cell's pixels (a 16-wide cell puts each pixel row of the
//                      cell in one 16-lane row of the wave, so the gradient reads are 64-byte rows), score every
//                      candidate with referenceEpiline and reduce the packed key (bits(epigrad^2) << 32 | row-major
//                      pixel index) to its maximum over the wave.  epigrad^2 >= +0, so the float bits order like the
//                      values and the largest key is the reference's winner, ties to the LAST pixel in scan order
//                      (its `>=`), with no atomics at all.
//   k_detect_count     one lane per cell: the cells with a score > 0 that are not masked, counted per workgroup of 256.
//   k_detect_emit      one lane per cell: the same ranking as k_project_scatter, in row-major cell order, and the
//                      initialised 40-byte records at n_res + rank.
//
// prunePoseFrames (flame.cc:554-706), the two feature loops (flame.cc:608-700):
//   k_prune_move       one lane per feature: the kept-id lookup; a feature of a kept pose-frame is left alone.  Any
//                      other feature is looked up in the table of dropped pose-frames (geometry towards the target
//                      pose-frame), run through inverse_depth_filter::predict and rewritten into a scratch record;
//                      a flag byte per feature (kPruneKeep | kPruneRewritten | kPruneMoved | kPruneInvalidated) and
//                      three counts per workgroup (kept, moved, invalidated; three arrays).
//   k_prune_commit     one lane per feature, after k_prune_move on the same stream: does nothing when an error index
//                      was raised.  When every record is kept, the rewritten records go back IN PLACE; otherwise the
//                      kept records are compacted stably into the other buffer (group_base / group_rank).  Writes
//                      the totals.
//   What the reference's loops do, kept literally:
//    1. the target is pruned_pfs.crbegin() of a std::map: the kept pose-frame with the LARGEST id (the host passes it);
//    2. `valid` is not tested: invalid features of a dropped frame are moved too; `valid` is only ever cleared;
//    3. records [0, first_new) (feats_) get frame_id, xy, idepth_mu, idepth_var overwritten BEFORE the success test,
//       also when the move fails (idepth_mu = the 0 predict returns, xy = the projected point);
//    4. idepth_var *= (idepth_pf / old_idepth)^4 as two squarings, 1 when double(idepth_pf) < 1e-6 (the NEW value);
//       predict's var_pred is discarded, so process_var_factor has no effect;
//    5. the region is an integer cv::Rect against a Point2f that is rounded to nearest-even first (rect_contains of
//       stereo_geometry.hpp, the update kernel's rule; unpinned: OpenCV is not available to check it).  A NaN
//       coordinate is outside;
//    6. where EpipolarGeometry::project asserts (negative or NaN idepth_mu, a zero third coordinate): the lowest
//       such index in stats[kFrontAssert], nothing is committed;
//    7. records [first_new, n) (new_feats_) that fail are REMOVED, never rewritten; failing feats_ records are kept
//       with valid = 0;
//    8. (the `pruned_pfs.size() == 0 -> clear()` branch is unreachable once the current pose-frame was found.)
//
// syncGraph's preprocessing (flame.cc:1954-1980, and the data-term lines 2001-2004, 2041-2044):
//   k_select_flag      one lane per record: FLAME_ASSERT(idepth >= 0) and pfs.at(frame_id) for EVERY record (the lowest
//                      failing index of each by atomicMin), the height of the RESIDENT record's point in the world, its
//                      class (selected, or the first failing test: invalid, variance, height) as a byte, and four counts
//                      per workgroup (four arrays).
//   k_select_scatter   one lane per record, after k_select_flag on the same stream: does nothing when an error index was
//                      raised.  The selected records are compacted stably (group_base / group_rank) into the output
//                      block: feat_id from the resident record, pos / data_term / data_weight from the PROJECTED record
//                      at the same index, and the index itself.  Writes the totals.
//   The output block is kFrontWords stats words, then five sections S words apart (pos: 2 S): S = the record count when
//   the host copies the whole block down in one piece, or the selected count (every workgroup sums it itself) when the
//   host copies the stats first and then 6 V words.
//
// Arithmetic keeps the reference's expression order and width; the build has -ffp-contract=off and correctly rounded
// division and sqrt, so results are bit-identical to the reference's scalar float code.  Nothing depends on the order
// in which atomics arrive: the only atomics are atomicMin of an error index.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "feature_kernels.h"
#include "stereo_geometry.hpp"

namespace flame_hip {
namespace {

constexpr int kGroup = 256;  // items per workgroup of the counting and scattering kernels (4 waves)

// The exclusive offset of workgroup b's flagged items: the sum of the counts of the workgroups before it.  There are at
// most a few hundred groups (n / 256), so every workgroup sums them itself instead of waiting for a scan launch.
__device__ int group_base(const int* __restrict__ counts, int b) {
  __shared__ int part[kGroup / 64];
  int s = 0;
  for (int k = threadIdx.x; k < b; k += kGroup) s += counts[k];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

// The exclusive rank of this lane's flag among the workgroup's flagged lanes (ballot + popcount per wave, the waves'
// totals through LDS); *count = the workgroup's total.
__device__ int group_rank(bool flag, int* count) {
  __shared__ int wave_total[kGroup / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  if (lane == 0) wave_total[wave] = __popcll(m);
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wave; ++w) before += wave_total[w];
  *count = (wave_total[0] + wave_total[1]) + (wave_total[2] + wave_total[3]);
  return before + __popcll(m & ((1ull << lane) - 1ull));
}

// ---- projectFeatures --------------------------------------------------------------------------------------------

// One feature: the keep flag, the projected record into proj[i], and the lowest-index error words.
__device__ bool project_one(const StereoCamera& cam, const ProjectRegion& R, int n_poses,
                            const ProjectPoseEntry* __restrict__ poses, uint32_t cur_frame_id, int i,
                            const StereoFeature* __restrict__ feats, StereoFeature* __restrict__ proj, int* __restrict__ stats) {
  const StereoFeature f = feats[i];
  int k = 0;
  while (k < n_poses && poses[k].frame_id != f.frame_id) ++k;
  if (k == n_poses) {  // pfs.at() throws before the `valid` test (flame.cc:1784)
    atomicMin(&stats[kFrontBadFrame], i);
    return false;
  }
  if (!f.valid) return false;
  V2 xy;
  float idepth_cur;
  if (!project_idepth(poses[k].geo, cam, V2{f.x, f.y}, f.idepth_mu, &xy, &idepth_cur)) {
    atomicMin(&stats[kFrontAssert], i);
    return false;
  }
  // cv::Rect_<float>::contains: x <= p.x < x + width, y <= p.y < y + height (all float)
  const bool inside = R.x <= xy.x && xy.x < R.x + R.w && R.y <= xy.y && xy.y < R.y + R.h;
  if (!inside || idepth_cur < 0.0f) return false;
  if (!(xy.x >= 0) || !(xy.x < (float)cam.width) || !(xy.y >= 0) || !(xy.y < (float)cam.height)) {  // flame.cc:1809-1812
    atomicMin(&stats[kFrontAssert], i);
    return false;
  }
  StereoFeature c;
  c.id = f.id;
  c.frame_id = cur_frame_id;
  c.x = xy.x, c.y = xy.y;
  c.idepth_mu = idepth_cur;
  float v4 = c.idepth_mu / f.idepth_mu;
  v4 *= v4;
  v4 *= v4;
  if ((double)f.idepth_mu < 1e-6) v4 = 1;
  c.idepth_var = v4 * f.idepth_var;
  c.valid = 1;
  c.reserved_[0] = c.reserved_[1] = c.reserved_[2] = 0;
  c.num_updates = f.num_updates;
  c.num_dropouts = 0;  // the reference leaves whatever feats_in_curr held at this index (never read downstream)
  c.search_status = 0;
  proj[i] = c;
  return true;
}

__global__ __launch_bounds__(kGroup) void k_project_flag(const StereoCamera cam, const ProjectRegion R, const int n_poses,
                                                         const ProjectPoseEntry* __restrict__ poses,
                                                         const uint32_t cur_frame_id, const int n,
                                                         const StereoFeature* __restrict__ feats,
                                                         StereoFeature* __restrict__ proj, uint8_t* __restrict__ keep,
                                                         int* __restrict__ counts, int* __restrict__ stats) {
  const int i = blockIdx.x * kGroup + threadIdx.x;
  bool k = false;
  if (i < n) {
    k = project_one(cam, R, n_poses, poses, cur_frame_id, i, feats, proj, stats);
    keep[i] = k ? 1 : 0;
  }
  const int c = __syncthreads_count(k);
  if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// Stable compaction: the kept resident records and their projected records at the same rank in both outputs.
__global__ __launch_bounds__(kGroup) void k_project_scatter(const int n, const uint8_t* __restrict__ keep,
                                                            const int* __restrict__ counts,
                                                            const StereoFeature* __restrict__ feats,
                                                            const StereoFeature* __restrict__ proj,
                                                            StereoFeature* __restrict__ feats_out,
                                                            StereoFeature* __restrict__ proj_out, int* __restrict__ stats) {
  const int i = blockIdx.x * kGroup + threadIdx.x;
  const bool k = i < n && keep[i];
  const int base = group_base(counts, blockIdx.x);
  int total;
  const int at = base + group_rank(k, &total);
  if (k) {
    feats_out[at] = feats[i];
    proj_out[at] = proj[i];
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) stats[kFrontCount] = base + total;
}

// ---- prunePoseFrames --------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kGroup) void k_prune_move(const StereoCamera cam, const PruneRegion R, const int n_keep,
                                                       const uint32_t* __restrict__ keep_ids, const int n_dropped,
                                                       const ProjectPoseEntry* __restrict__ dropped,
                                                       const uint32_t target_frame_id, const int first_new, const int n,
                                                       const StereoFeature* __restrict__ feats,
                                                       StereoFeature* __restrict__ moved, uint8_t* __restrict__ flags,
                                                       int* __restrict__ counts, int* __restrict__ stats) {
  const int i = blockIdx.x * kGroup + threadIdx.x;
  uint8_t fl = 0;
  if (i < n) {
    fl = kPruneKeep;
    StereoFeature f = feats[i];
    int k = 0;
    while (k < n_keep && keep_ids[k] != f.frame_id) ++k;
    if (k == n_keep) {  // pruned_pfs.count(feat.frame_id) == 0
      int d = 0;
      while (d < n_dropped && dropped[d].frame_id != f.frame_id) ++d;
      V2 u_pf;
      float idepth_pf;
      if (d == n_dropped) {  // pfs_[feat.frame_id] of a frame that is not there
        atomicMin(&stats[kFrontBadFrame], i);
      } else if (!project_idepth(dropped[d].geo, cam, V2{f.x, f.y}, f.idepth_mu, &u_pf, &idepth_pf)) {
        atomicMin(&stats[kFrontAssert], i);
      } else {
        bool move_success = true;  // inverse_depth_filter::predict (inverse_depth_filter.cc:41-47)
        if (idepth_pf < 0.0f) {
          idepth_pf = 0.0f;
          move_success = false;
        }
        const bool ok = move_success && rect_contains(R.x, R.y, R.w, R.h, u_pf);
        if (!ok && i >= first_new) {
          fl = 0;  // new_feats_: removed, not rewritten (flame.cc:675-678)
        } else {
          f.frame_id = target_frame_id;
          f.x = u_pf.x, f.y = u_pf.y;
          const float old_idepth = f.idepth_mu;
          f.idepth_mu = idepth_pf;
          float v4 = idepth_pf / old_idepth;
          v4 *= v4;
          v4 *= v4;
          if ((double)idepth_pf < 1e-6) v4 = 1;
          f.idepth_var *= v4;
          if (!ok) f.valid = 0;  // feats_: kept, marked (flame.cc:643-647)
          moved[i] = f;
          fl = kPruneKeep | kPruneRewritten | (ok ? kPruneMoved : kPruneInvalidated);
        }
      }
    }
    flags[i] = fl;
  }
  const int c_keep = __syncthreads_count(fl & kPruneKeep);
  const int c_moved = __syncthreads_count(fl & kPruneMoved);
  const int c_inval = __syncthreads_count(fl & kPruneInvalidated);
  if (threadIdx.x == 0) {
    counts[blockIdx.x] = c_keep;
    counts[gridDim.x + blockIdx.x] = c_moved;
    counts[2 * gridDim.x + blockIdx.x] = c_inval;
  }
}

__global__ __launch_bounds__(kGroup) void k_prune_commit(const int n, const uint8_t* __restrict__ flags,
                                                         const int* __restrict__ counts,
                                                         StereoFeature* __restrict__ feats,
                                                         const StereoFeature* __restrict__ moved,
                                                         StereoFeature* __restrict__ feats_out, int* __restrict__ stats) {
  if (stats[kFrontAssert] != INT_MAX || stats[kFrontBadFrame] != INT_MAX) return;  // (uniform: written by k_prune_move only)
  const int i = blockIdx.x * kGroup + threadIdx.x;
  const int groups = gridDim.x;
  const int kept = group_base(counts, groups);  // the kept counts of all workgroups
  const uint8_t fl = i < n ? flags[i] : 0;
  if (kept == n) {  // nothing removed: in place, only the rewritten records are stored
    if (fl & kPruneRewritten) feats[i] = moved[i];
  } else {
    __syncthreads();  // (group_base's LDS words are reused)
    const int base = group_base(counts, blockIdx.x);
    int total;
    const int at = base + group_rank(fl & kPruneKeep, &total);
    if (fl & kPruneKeep) feats_out[at] = (fl & kPruneRewritten) ? moved[i] : feats[i];
  }
  if (blockIdx.x == 0) {
    __syncthreads();
    const int n_moved = group_base(counts + groups, groups);
    __syncthreads();
    const int n_inval = group_base(counts + 2 * groups, groups);
    if (threadIdx.x == 0) {
      stats[kFrontCount] = kept;
      stats[kPruneStatMoved] = n_moved;
      stats[kPruneStatInvalidated] = n_inval;
    }
  }
}

// ---- syncGraph's preprocessing ----------------------------------------------------------------------------------

// The class of one record: selected, or the first of the reference's tests that fails (flame.cc:1976-1977).
__device__ uint8_t select_one(const StereoCamera& cam, const SelectRule& rule, int n_poses,
                              const SelectPoseEntry* __restrict__ poses, int i, const StereoFeature& f,
                              int* __restrict__ stats) {
  const float idepth = f.idepth_mu;
  bool error = false;
  if (!(idepth >= 0.0f)) {  // FLAME_ASSERT(idepth >= 0.0f) (flame.cc:1968): every record, valid or not; NaN fails
    atomicMin(&stats[kFrontAssert], i);
    error = true;
  }
  int k = 0;
  while (k < n_poses && poses[k].frame_id != f.frame_id) ++k;
  if (k == n_poses) {  // pfs.at(feat.frame_id) (flame.cc:1974): every record
    atomicMin(&stats[kFrontBadFrame], i);
    error = true;
  }
  if (error) return kSelectNone;
  // pix /= idepth: three true divisions (Eigen >= 3.3); Kinv * pix: the full product, each row (a + b) + c
  const float px = f.x / idepth, py = f.y / idepth, pz = 1.0f / idepth;
  const float X = (cam.Kinv[0] * px + cam.Kinv[1] * py) + cam.Kinv[2] * pz;
  const float Y = (cam.Kinv[3] * px + cam.Kinv[4] * py) + cam.Kinv[5] * pz;
  const float Z = (cam.Kinv[6] * px + cam.Kinv[7] * py) + cam.Kinv[8] * pz;
  const SelectPoseEntry P = poses[k];
  const float wy = ((P.r10 * X + P.r11 * Y) + P.r12 * Z) + P.ty;
  const float h = -wy;
  if (!f.valid) return kSelectInvalid;
  if (!(f.idepth_var < rule.idepth_var_max_graph)) return kSelectFailVar;
  if (!(h >= rule.min_height && h <= rule.max_height)) return kSelectFailHeight;
  if (f.id > (uint32_t)INT_MAX) atomicMin(&stats[kSelectBadId], i);  // the sync's feat_id is int32_t >= 0
  return kSelectTaken;
}

__global__ __launch_bounds__(kGroup) void k_select_flag(const StereoCamera cam, const SelectRule rule, const int n_poses,
                                                        const SelectPoseEntry* __restrict__ poses, const int n,
                                                        const StereoFeature* __restrict__ feats, uint8_t* __restrict__ cls,
                                                        int* __restrict__ counts, int* __restrict__ stats) {
  const int i = blockIdx.x * kGroup + threadIdx.x;
  uint8_t c = kSelectNone;
  if (i < n) {
    c = select_one(cam, rule, n_poses, poses, i, feats[i], stats);
    cls[i] = c;
  }
  const int c_taken = __syncthreads_count(c == kSelectTaken);
  const int c_invalid = __syncthreads_count(c == kSelectInvalid);
  const int c_var = __syncthreads_count(c == kSelectFailVar);
  const int c_height = __syncthreads_count(c == kSelectFailHeight);
  if (threadIdx.x == 0) {
    counts[blockIdx.x] = c_taken;
    counts[gridDim.x + blockIdx.x] = c_invalid;
    counts[2 * gridDim.x + blockIdx.x] = c_var;
    counts[3 * gridDim.x + blockIdx.x] = c_height;
  }
}

// `out`: kFrontWords stats words (k_select_flag's `stats`), then the five sections, `section` words apart (pos: twice
// that); section <= 0 = the selected count.
__global__ __launch_bounds__(kGroup) void k_select_scatter(const SelectRule rule, const int n, const uint8_t* __restrict__ cls,
                                                           const int* __restrict__ counts,
                                                           const StereoFeature* __restrict__ feats,
                                                           const StereoFeature* __restrict__ proj, const int section,
                                                           int* __restrict__ out) {
  if (out[kFrontAssert] != INT_MAX || out[kFrontBadFrame] != INT_MAX || out[kSelectBadId] != INT_MAX) return;  // (uniform)
  const int i = blockIdx.x * kGroup + threadIdx.x;
  const int groups = gridDim.x;
  const int taken_all = group_base(counts, groups);
  __syncthreads();  // (group_base's LDS words are reused)
  const int base = group_base(counts, blockIdx.x);
  const bool taken = i < n && cls[i] == kSelectTaken;
  int total;
  const int at = base + group_rank(taken, &total);
  if (taken) {
    const size_t S = (size_t)(section > 0 ? section : taken_all);
    int* body = out + kFrontWords;
    const StereoFeature c = proj[i];  // feats_in_curr[feat_id_to_idx[id]]: neither its `valid` nor its `id` is read
    body[at] = (int)feats[i].id;
    float* pos = (float*)(body + S);
    pos[2 * (size_t)at] = c.x, pos[2 * (size_t)at + 1] = c.y;
    ((float*)(body + 3 * S))[at] = c.idepth_mu / rule.graph_scale;
    ((float*)(body + 4 * S))[at] = rule.adaptive_data_weights ? 1.0f / c.idepth_var : 1.0f;
    (body + 5 * S)[at] = i;
  }
  if (blockIdx.x == 0) {
    __syncthreads();
    const int n_invalid = group_base(counts + groups, groups);
    __syncthreads();
    const int n_var = group_base(counts + 2 * groups, groups);
    __syncthreads();
    const int n_height = group_base(counts + 3 * groups, groups);
    if (threadIdx.x == 0) {
      out[kFrontCount] = taken_all;
      out[kSelectStatInvalid] = n_invalid;
      out[kSelectStatFailVar] = n_var;
      out[kSelectStatFailHeight] = n_height;
    }
  }
}

// ---- detectFeatures ---------------------------------------------------------------------------------------------

// A mask point (x, y) clears cell (uint(y / win), uint(x / win)) (flame.cc:1006-1010); `stride` floats between points.
__global__ __launch_bounds__(256) void k_detect_mask(const int n, const float* __restrict__ xy, const int stride,
                                                     const int win, const int hc, const int wc,
                                                     uint8_t* __restrict__ blocked) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = xy[(size_t)i * stride], y = xy[(size_t)i * stride + 1];
  if (!(x >= 0.0f) || !(y >= 0.0f)) return;  // (the host rejects such points; the projected set has none)
  const uint32_t cx = (uint32_t)(x / (float)win), cy = (uint32_t)(y / (float)win);
  if (cx < (uint32_t)wc && cy < (uint32_t)hc) blocked[(size_t)cy * wc + cx] = 1;
}

// The candidate pixels are rows [r_lo, r_hi) x cols [c_lo, c_hi).  A pixel's cell is int(float(ii) / win): for
// ii < 2^14 that is the integer quotient (float(ii) / win is at least 1/win below the next integer, far more than
// its rounding error), so the cell's pixels are the integer block [cy * win, cy * win + win) of rows.
__global__ __launch_bounds__(256) void k_detect_cells(const DetectGrid G, const Geo geo, const StereoCamera cam,
                                                      const float* __restrict__ gx_pad, const float* __restrict__ gy_pad,
                                                      unsigned long long* __restrict__ cell_key, int* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int cell = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  if (cell >= G.hc * G.wc) return;
  const int cy = cell / G.wc, cx = cell - cy * G.wc;
  const int win = G.win, pw = cam.width + 2 * cam.border;
  unsigned long long best = 0;
  for (int k = lane; k < win * win; k += 64) {
    const int lr = k / win, ii = cy * win + lr, jj = cx * win + (k - lr * win);
    if (ii < G.r_lo || ii >= G.r_hi || jj < G.c_lo || jj >= G.c_hi) continue;
    const size_t o = (size_t)(ii + cam.border) * pw + (jj + cam.border);
    const float gx = gx_pad[o], gy = gy_pad[o];
    const float gmag2 = gx * gx + gy * gy;
    if (gmag2 < G.g2) continue;
    V2 epi;
    if (!reference_epiline(geo, cam, V2{(float)ii, (float)jj}, &epi)) {  // (row, col) as (x, y), as flame.cc:1029
      atomicMin(&stats[kFrontAssert], ii * cam.width + jj);
      continue;
    }
    const float epigrad = gx * epi.x + gy * epi.y;
    const float epigrad2 = epigrad * epigrad;
    if (epigrad2 < G.g2) continue;
    if (!(epigrad2 >= 0.0f)) continue;  // NaN never passes the reference's `epigrad2 >= best`
    const unsigned long long key =
        ((unsigned long long)__float_as_uint(epigrad2) << 32) | (unsigned long long)(uint32_t)(ii * cam.width + jj);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = __shfl_xor(best, d, 64);
    best = o > best ? o : best;
  }
  if (lane == 0) cell_key[cell] = best;
}

// A cell is emitted iff cmask > 0 and best_gradsc > 0 (flame.cc:1052): a positive float has nonzero bits.
__device__ __forceinline__ bool emitted(int c, int n_cells, const unsigned long long* __restrict__ cell_key,
                                        const uint8_t* __restrict__ blocked) {
  return c < n_cells && !blocked[c] && (cell_key[c] >> 32) != 0;
}

__global__ __launch_bounds__(kGroup) void k_detect_count(const int n_cells, const unsigned long long* __restrict__ cell_key,
                                                         const uint8_t* __restrict__ blocked, int* __restrict__ counts) {
  const int c = __syncthreads_count(emitted(blockIdx.x * kGroup + threadIdx.x, n_cells, cell_key, blocked));
  if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// The new features in row-major cell order, initialised as the detection loop does (flame.cc:739-753).
__global__ __launch_bounds__(kGroup) void k_detect_emit(const int n_cells, const int width,
                                                        const unsigned long long* __restrict__ cell_key,
                                                        const uint8_t* __restrict__ blocked, const int* __restrict__ counts,
                                                        const DetectInit I, const float* __restrict__ idepthmap,
                                                        StereoFeature* __restrict__ out, int* __restrict__ stats) {
  const int c = blockIdx.x * kGroup + threadIdx.x;
  const bool e = emitted(c, n_cells, cell_key, blocked);
  const int base = group_base(counts, blockIdx.x);
  int total;
  const int at = base + group_rank(e, &total);
  if (e) {
    const uint32_t px = (uint32_t)(cell_key[c] & 0xffffffffull);
    const int ii = (int)(px / (uint32_t)width), jj = (int)(px - (uint32_t)ii * (uint32_t)width);
    StereoFeature f;
    f.id = I.first_id + (uint32_t)at;  // feat_count_++ (flame.cc:741)
    f.frame_id = I.ref_frame_id;
    f.x = (float)jj, f.y = (float)ii;
    f.idepth_var = I.idepth_var_init;
    f.valid = 1;
    f.reserved_[0] = f.reserved_[1] = f.reserved_[2] = 0;
    f.num_updates = 0;
    f.num_dropouts = 0;
    f.search_status = 0;
    // idepthmap(fast_roundf(y), fast_roundf(x)) of integer coordinates (flame.cc:749-753)
    f.idepth_mu = I.idepth_init;
    if (idepthmap) {
      const float d = idepthmap[(size_t)ii * width + jj];
      if (!isnan(d)) f.idepth_mu = d;
    }
    out[at] = f;
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) stats[kFrontCount] = base + total;
}

}  // namespace

hipError_t launch_project_features(const StereoCamera& cam, const ProjectRegion& region, int n_poses,
                                   const ProjectPoseEntry* poses, uint32_t cur_frame_id, int n, const StereoFeature* feats,
                                   StereoFeature* proj_tmp, uint8_t* keep, int* counts, StereoFeature* feats_out,
                                   StereoFeature* proj_out, int* stats, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const int groups = (n + kGroup - 1) / kGroup;
  hipLaunchKernelGGL(k_project_flag, dim3(groups), dim3(kGroup), 0, stream, cam, region, n_poses, poses, cur_frame_id, n, feats,
                     proj_tmp, keep, counts, stats);
  hipLaunchKernelGGL(k_project_scatter, dim3(groups), dim3(kGroup), 0, stream, n, keep, counts, feats, proj_tmp, feats_out,
                     proj_out, stats);
  return hipGetLastError();
}

hipError_t launch_detect_features(const DetectGrid& grid, const Geo& geo, const StereoCamera& cam, const float* gx_pad,
                                  const float* gy_pad, int n_mask, const float* mask_xy, int mask_stride, uint8_t* blocked,
                                  unsigned long long* cell_key, int* counts, const DetectInit& init, const float* idepthmap,
                                  StereoFeature* out, int* stats, hipStream_t stream) {
  const int n_cells = grid.hc * grid.wc;
  if (n_cells <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(blocked, 0, (size_t)n_cells, stream);
  if (e != hipSuccess) return e;
  if (n_mask > 0)
    hipLaunchKernelGGL(k_detect_mask, dim3((n_mask + 255) / 256), dim3(256), 0, stream, n_mask, mask_xy, mask_stride, grid.win,
                       grid.hc, grid.wc, blocked);
  hipLaunchKernelGGL(k_detect_cells, dim3((n_cells + 3) / 4), dim3(256), 0, stream, grid, geo, cam, gx_pad, gy_pad, cell_key,
                     stats);
  const int groups = (n_cells + kGroup - 1) / kGroup;
  hipLaunchKernelGGL(k_detect_count, dim3(groups), dim3(kGroup), 0, stream, n_cells, cell_key, blocked, counts);
  hipLaunchKernelGGL(k_detect_emit, dim3(groups), dim3(kGroup), 0, stream, n_cells, cam.width, cell_key, blocked, counts, init,
                     idepthmap, out, stats);
  return hipGetLastError();
}

hipError_t launch_prune_features(const StereoCamera& cam, const PruneRegion& region, int n_keep, const uint32_t* keep_ids,
                                 int n_dropped, const ProjectPoseEntry* dropped, uint32_t target_frame_id, int first_new, int n,
                                 StereoFeature* feats, StereoFeature* moved, uint8_t* flags, int* counts,
                                 StereoFeature* feats_out, int* stats, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const int groups = (n + kGroup - 1) / kGroup;
  hipLaunchKernelGGL(k_prune_move, dim3(groups), dim3(kGroup), 0, stream, cam, region, n_keep, keep_ids, n_dropped, dropped,
                     target_frame_id, first_new, n, feats, moved, flags, counts, stats);
  hipLaunchKernelGGL(k_prune_commit, dim3(groups), dim3(kGroup), 0, stream, n, flags, counts, feats, moved, feats_out, stats);
  return hipGetLastError();
}

SelectPoseEntry select_pose_entry(uint32_t frame_id, const float q[4], const float t[3]) {
  // row 1 of Eigen's Quaternion::toRotationMatrix() (w, x, y, z), in float: the host build is uncontracted like the device's
  const float w = q[0], x = q[1], y = q[2], z = q[3];
  const float tx = 2.0f * x, ty = 2.0f * y, tz = 2.0f * z;
  const float twx = tx * w, twz = tz * w, txx = tx * x, txy = tx * y, tyz = ty * z, tzz = tz * z;
  SelectPoseEntry e;
  e.frame_id = frame_id;
  e.r10 = txy + twz;
  e.r11 = 1.0f - (txx + tzz);
  e.r12 = tyz - twx;
  e.ty = t[1];
  return e;
}

hipError_t launch_select_graph_features(const StereoCamera& cam, const SelectRule& rule, int n_poses,
                                        const SelectPoseEntry* poses, int n, const StereoFeature* feats,
                                        const StereoFeature* proj, uint8_t* cls, int* counts, int section, int* out,
                                        hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  const int groups = (n + kGroup - 1) / kGroup;
  hipLaunchKernelGGL(k_select_flag, dim3(groups), dim3(kGroup), 0, stream, cam, rule, n_poses, poses, n, feats, cls, counts, out);
  hipLaunchKernelGGL(k_select_scatter, dim3(groups), dim3(kGroup), 0, stream, rule, n, cls, counts, feats, proj, section, out);
  return hipGetLastError();
}

}  // namespace flame_hip
