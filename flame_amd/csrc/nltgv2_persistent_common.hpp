// nltgv2_persistent_common.hpp -- what the persistent kernels share, once: the patch rows' meta bits, the wait report, the open
// run's stop decision, the vertex update, the record verification, the give-up epilogue and the write-back of a run's state.
// Included by nltgv2_persistent.hip (k_persistent_pv), nltgv2_persistent_lean.hip (k_persistent_pv_lean), nltgv2_persistent_pv2.hip (k_persistent_pv2) and nltgv2_persistent_tv.hip
// (k_persistent_tv).  The protocol these pieces belong to is described at the top of nltgv2_persistent.hip; the step bodies (the
// poll statements, the DPP accumulations, the dual updates, the two-step loops) are what differs and stay with their kernels.
// Everything here is inlined: the compiler's scheduling of these kernels is sensitive to how code is factored, so a change is
// checked against the instruction streams of the kernels as built (profiles/persistent_common.txt), not assumed.
#ifndef FLAME_AMD_NLTGV2_PERSISTENT_COMMON_HPP_
#define FLAME_AMD_NLTGV2_PERSISTENT_COMMON_HPP_

#include "nltgv2_device.hpp"

namespace flame_hip {
namespace {

// meta word of a lane of a patch row (nltgv2_pack.hpp, layouts (E) and (E2))
constexpr unsigned kWgActiveBit = 1u << 25, kWgValidBit = 1u << 26, kWgPublishBit = 1u << 27, kWgHeadBit = 1u << 28;
typedef float v2f_t __attribute__((ext_vector_type(2)));
typedef float v4f_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void lds_wave_sync() {  // LDS operations of one wave are processed in issue order
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
__device__ __forceinline__ unsigned read_hw_id() {
  unsigned v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(v));
  return v;
}

// Which wait of a persistent run expired, for the host's trace (FLAME_NLTGV2_TRACE) and flame_nltgv2_info: the first wave
// to give up leaves {which wait, patch, step, lanes still waiting, the foreign record of the first of them, tag seen / wanted,
// XCC and HW ids} in err[1..10] (err[0] stays the flag word).  which: 1 rotation word, 2 XCC table, 3 a step's records.
__device__ __forceinline__ void report_expired(int* err, int which, int wg, int it, unsigned long long pend, int frid, unsigned seen,
                                               unsigned want) {
  if (atomicCAS(&err[1], 0, which) == 0) {
    err[2] = wg, err[3] = it, err[4] = (int)(unsigned)pend, err[5] = (int)(unsigned)(pend >> 32), err[6] = frid;
    err[7] = (int)seen, err[8] = (int)want, err[9] = (int)read_xcc_id(), err[10] = (int)read_hw_id();
  }
}

// A wave that gives up (one lane of it): every other wave leaves through the abort flag, the host reads the flag word --
// 2: a wait expired, 4: a torn record -- takes the run back and redoes it per step.
__device__ __forceinline__ void give_up(int* abort_flag, int* err, bool torn) {
  __hip_atomic_store(abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  atomicOr(err, torn ? 4 : 2);
}

// OPEN (round 6): a run that goes on until the host needs the state (the OPEN instances of the two patch kernels).  n_iters is then
// an upper bound; ONE patch (the middle one of the launch) looks at a word the host sets to this run's tag0 (a 4-byte copy on a
// stream of its own; a request for an earlier run means nothing, so the word is never cleared) every kOpenCheck iterations and, when
// it says so, publishes the iteration every patch leaves at -- its own plus kOpenMargin, more than any patch can be ahead of it (a
// patch is ahead of another by at most their distance in the patch graph) -- in err[12] as tag0 + iteration (tags grow from run to
// run: a stale word of an earlier run is below this run's tag0 and means nothing).  Every patch reads that word every kOpenCheck
// iterations.  A patch that saw the word too late has no neighbours left to wait for: its wait expires and the run is taken back
// and redone like any other (nltgv2_run.hip finish()).  The patch that decides leaves the number of iterations done in err[13]
// (tag0 + n) on its way out.
constexpr unsigned kOpenMargin = 128u, kOpenCheck = 64u;  // (both even: an open run does an even number of iterations)

// The stop decision at a check iteration (it % kOpenCheck == 0 -- all patches at the same ones: the network runs in lock step, so
// the ~0.5 us this load takes are spent by everybody at once, 1-2 % of the time): the deciding patch first looks at the host's
// request, everybody at the word.  stop_at: tag0 + the iteration to leave at, 0 while that is not known (updated in place: returned
// by value it changed three times as many lines of the OPEN instances, profiles/persistent_common.txt).
// (Asked for every trip and looked at a trip later it cost 17 %: the compiler waits for the publish stores in front of the
//  load, and the step's polls never wait for vmcnt, so nothing hides it.)
__device__ __forceinline__ void open_run_check(unsigned& stop_at, const bool decides, const unsigned* const stop_req, unsigned* const stop_word,
                                               const unsigned tag0, const int it, const int n_iters, const int lane) {
  if (decides && stop_at == 0u && stop_req &&
      (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(stop_req, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == tag0) {
    stop_at = tag0 + (unsigned)it + kOpenMargin;
    if (lane == 0) {
      __hip_atomic_store(stop_word, stop_at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      // (taken: tags start over with every topology, the next graph's first run has this tag0 again)
      __hip_atomic_store(const_cast<unsigned*>(stop_req), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (stop_at == 0u) {
    const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(stop_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (w > tag0 && w - tag0 <= (unsigned)n_iters + kOpenMargin) stop_at = w;  // (a word of an earlier run is below this run's tag0)
  }
}

// Record verification (FLAME_NLTGV2_OPT_VERIFY_RECORDS) of the patch kernels: every fetch lane reads its foreign record once more,
// with an ordinary load, and compares all four dwords with what the LDS-DMA left in its slot: a record is final once its tag is
// visible, so a difference means a torn 16-byte access (memory side or LDS side) -- reported, the run is taken back and redone
// per step.  The test hook (verify & 2) makes the second read of one lane of the launch's first patch differ, in step 2.  (The hook's
// ingredients are passed one by one: as one bool evaluated by the caller the VERIFY instances came out ~1000 lines different.)
__device__ __forceinline__ bool fetch_record_torn(const int frid, const char* const src, const float4* const lds_slot, const unsigned s,
                                                  const int verify, const int it, const int wg, const int wg_begin, const int lane) {
  v4i_t g2 = {0, 0, 0, 0};
  if (frid >= 0) {
    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(g2) : "v"(src) : "memory");
  }
  const float4 l4 = *lds_slot;
  if ((verify & 2) && it == 2 && wg == wg_begin && lane == 0) g2.x ^= 0x00400000;  // test hook
  return frid >= 0 && (g2.x != __float_as_int(l4.x) || g2.y != __float_as_int(l4.y) || g2.z != __float_as_int(l4.z) ||
                       (unsigned)g2.w != s || __float_as_uint(l4.w) != s);
}

// Vertex update of the patch kernels: proxL1 (cc:147-151, h:179-197), extragradient (cc:160-171), from the accumulated (X, Wa) and
// the state (x, w12) of the step before.  Both shifted values up front and two selects (the same result as prox_l1 of
// nltgv2_device.hpp: as branches this was three exec-masked blocks in the hand-off path).
struct VertexNext {
  float xn, nb;  // the new x and x_bar
  v2f_t wbn;     // the new (w1_bar, w2_bar); the new (w1, w2) are Wa themselves
};
__device__ __forceinline__ VertexNext vertex_update(const SolverParams& p, const float X, const v2f_t Wa, const float x, const v2f_t w12,
                                                    const float data, const float thr) {
  VertexNext n;
  const float diff = X - data, x_dn = X - thr, x_up = X + thr;
  float xn = (diff < -thr) ? x_up : data;
  xn = (diff > thr) ? x_dn : xn;
  xn = (xn < p.x_min) ? p.x_min : xn;
  xn = (xn > p.x_max) ? p.x_max : xn;
  float nb = xn + p.theta * (xn - x);
  nb = (nb < p.x_min) ? p.x_min : nb;
  nb = (nb > p.x_max) ? p.x_max : nb;
  n.xn = xn, n.nb = nb;
  n.wbn = Wa + p.theta * (Wa - w12);
  return n;
}

// End of a run, the lane that holds vertex pv's state: into the OTHER copies of the state arrays (the run is transactional: the
// host swaps the roles once it knows that the run succeeded), the caller's export array and, when a standing target is set, the
// photometric residual of the final x (nltgv2_device.hpp) as part of the solver's own launch.
__device__ __forceinline__ void write_back_vertex(const int pv, const float x, const v2f_t w12, const float xb, const v2f_t wb12,
                                                  const float x_prev, const v2f_t w_prev, const float data, float4* vstate_out,
                                                  float4* bar_out, float4* vprev, const int32_t* __restrict__ perm,
                                                  const RunTail* __restrict__ tail) {
  vstate_out[pv] = make_float4(x, w12.x, w12.y, data);
  bar_out[pv] = make_float4(xb, wb12.x, wb12.y, 0.0f);
  vprev[pv] = make_float4(x_prev, w_prev.x, w_prev.y, 0.0f);
  float* const export_out = tail->export_out;
  float* const photo_err = tail->photo.err;
  if (export_out || photo_err) {
    const int o = perm[pv];  // the caller's vertex index
    if (o >= 0 && export_out) export_out[o] = x * tail->export_scale;
    if (o >= 0 && photo_err) {
      const PhotoFuse& photo = tail->photo;
      photo_err[o] = photo_residual_at(photo.pos[o], x * photo.graph_scale, photo.geo, photo.ref, photo.cmp, photo.rows,
                                       photo.cols, photo.step, photo.border);
    }
  }
}

}  // namespace
}  // namespace flame_hip

#endif  // FLAME_AMD_NLTGV2_PERSISTENT_COMMON_HPP_
