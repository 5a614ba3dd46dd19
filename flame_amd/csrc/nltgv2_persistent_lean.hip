// nltgv2_persistent_lean.hip -- k_persistent_pv_lean: the patch-per-wave persistent kernel (k_persistent_pv, nltgv2_persistent.hip: the
// protocol, the LDS map, the tables and what every term means are described there) for the regime the headline runs in -- few patches
// per CU, unpaced narrowed polls, the same-XCD copy on, no vertex of more than 16 edges, no probe, no verification, not an open run.
// Arguments, prologue and epilogue are the general kernel's; what differs is the loop: between a record arriving and the next one
// leaving a lone wave issues one instruction per ~5 cycles, needed or not, and the general kernel's body pays there for what it can also
// do (register copies that line up packed pairs, moves that assemble the record, pads, EXEC bookkeeping, a taken branch over the code
// of larger degrees).  The compiler cannot be steered there (profiles/r06_hot_path_ab.txt), so ONE statement holds the step from its
// first poll to the record in LDS, written by hand with fixed temporaries: the same IEEE operations in the same order as the general
// kernel's (no contraction -- the one fma is the exact (source - target) of the dual update, as there --, the compare-and-select clamps
// of x, nothing re-associated), which is what keeps the result bit-identical.
// Compiled with -ffp-contract=off like the other kernels; counts of both kernels as built: profiles/pv_lean_path.txt.
// NOT EXERCISED: the wait's bounded fallback (64 rounds without all tags: abort flag, spin budget, report_expired) is the general
// kernel's logic written once more inside the statement, and no test reaches it -- the fault-injection hook, which is how the suite
// makes a wait expire, sends a run to the general kernel (pv_lean_applies).  It was checked by reading the ISA as built only.
#include "nltgv2_persistent_common.hpp"

namespace flame_hip {

namespace {

// The step statement's fixed registers (clobbered; nothing else lives there while it runs):
//   v64 tag of the neighbour's record   v65 tag of this lane's fetch slot   v66 | v[68:69] the neighbour's x_bar | (w1_bar, w2_bar)
//   v67 | v[70:71] this vertex's x_bar | (w1_bar, w2_bar)   v[72:73] d12, K23   v[74:75] wbi, m12   v76 d0, K1   v77 cx   v[78:79] u23
//   v[80:81] M2, a12   v[82:83] b12   v84 X   v85 diff, x_bar'   v[86:87] the w sums   v[88:89] theta * (W - w)   v90, v91 x_up, x_dn, x'
//   v[92:95] the record {x_bar', w1_bar', w2_bar', tag + 1}: built where the stores read it   v96 | v[98:99] q1r | q23r (the NaN check)
//   v[100:101] the clamped (q2, q3)
// Packed pairs must be even-aligned, which a 16-byte LDS read cannot give (x, w1 | w2, tag): the records are read as b32 + read2_b32
// after their tag word (a tag that matches vouches for what is read after it, as in the general kernel).
#define PVL_CLOBBERS                                                                                                                   \
  "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79", "v80", "v81", "v82",  \
      "v83", "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", "v96", "v97", "v98", "v99", "v100",  \
      "v101", "vcc", "scc", "memory"

// shift J of the ordered accumulation (nltgv2_persistent.hip, "step"): X += cx, W1 += a1, W2 += a2, W1 += b1, W2 += b2 of lane + J
#define PVL_ADDS(J)                                                           \
  "v_add_f32_dpp v84, v77, v84 row_shl:" #J " row_mask:0xf bank_mask:0xf\n\t" \
  "v_add_f32_dpp v86, v80, v86 row_shl:" #J " row_mask:0xf bank_mask:0xf\n\t" \
  "v_add_f32_dpp v87, v81, v87 row_shl:" #J " row_mask:0xf bank_mask:0xf\n\t" \
  "v_add_f32_dpp v86, v82, v86 row_shl:" #J " row_mask:0xf bank_mask:0xf\n\t" \
  "v_add_f32_dpp v87, v83, v87 row_shl:" #J " row_mask:0xf bank_mask:0xf\n\t"
#define PVL_RM(J, M) "s_mov_b64 exec, %[" #M "]\n\t" PVL_ADDS(J)

__global__ void __launch_bounds__(64)
k_persistent_pv_lean(const int wg_begin, const int n_wgs, const int wgs_per_xcd, const int lcap, const int slab_slots,
                     const int32_t* __restrict__ wg_slot, const int32_t* __restrict__ wg_vid,
                     const uint32_t* __restrict__ wg_meta, const int32_t* __restrict__ wg_nbr,
                     const int32_t* __restrict__ wg_fetch, const int32_t* __restrict__ wg_info, const int4* hrec,
                     const float4* hq, const float4* vstate,
                     float4* hq_out, float4* vstate_out, const float2* vaux, const float4* bar_in, float4* bar_out, float4* vprev,
                     void* xbuf, const int rec_bytes, const int dual_arg, const unsigned tag0, const int n_iters,
                     const unsigned max_spins_arg, const int poll_gap_arg, const SolverParams p,
                     int* __restrict__ err, int* __restrict__ abort_flag, const int32_t* __restrict__ perm,
                     const RunTail* __restrict__ tail, unsigned* __restrict__ probe, char* place_pool,
                     const int32_t* __restrict__ rec_off, const int rec_off_stride, unsigned* rot_word) {
  extern __shared__ float4 lds[];
  constexpr int T = 64;
  (void)dual_arg, (void)poll_gap_arg, (void)probe;  // (folded: same-XCD copy on, no pause, narrowed re-loads, no pre-sleep; no probe)
  const unsigned max_spins = max_spins_arg & 0x7fffffffu;
  const int lane = (int)threadIdx.x;
  int b = blockIdx.x;
  if (rot_word) {  // (the rotation of the grid: nltgv2_persistent.hip)
    const unsigned want = (tag0 & 0x0fffffffu) << 4;
    if (b == 0 && lane == 0) __hip_atomic_store(rot_word, want | read_xcc_id(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned v = 0;
    for (unsigned spins = 0;; ++spins) {
      v = __builtin_amdgcn_readfirstlane(__hip_atomic_load(rot_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      if ((v & ~15u) == want) break;
      if (spins > (max_spins_arg & 0x7fffffffu)) {
        if (lane == 0) {
          give_up(abort_flag, err, false);
          report_expired(err, 1, (int)blockIdx.x, -1, 0ull, -1, v, want);
        }
        return;
      }
      __builtin_amdgcn_s_sleep(2);
    }
    b += (int)(v & 7u);
    if (b >= (int)gridDim.x) b -= (int)gridDim.x;
  }
  const int xcd = b & 7, idx = b >> 3;
  if (idx >= wgs_per_xcd) return;
  if (xcd * wgs_per_xcd + idx >= n_wgs) return;
  const int wg = wg_begin + xcd * wgs_per_xcd + idx;  // this launch covers patches [wg_begin, +n_wgs)
  const int rid_base = wg_info[4 * wg], n_fetch = wg_info[4 * wg + 1];
  const int count_flags = wg_info[4 * wg + 2];
  if ((count_flags & 0xffff) == 0) return;                 // (a patch without a vertex: nothing to do)
  if (unsigned* const pg = tail->progress) {               // (trace runs only) when this patch started, in us of the 100 MHz clock
    if (lane == 0) pg[n_wgs + (wg - wg_begin)] = (unsigned)(wall_clock64() / 100u) | 1u;
  }
  const int stride = wg_info[4 * wg + 3];  // the patch's largest degree (at most 16 here: the planner sends other graphs to the general kernel)
  // LDS map, float4 units: [rec area 0: lcap local + 64 fetch slots | rec area 1 | slab_slots (unused: 0) | spare 64]
  const int rec_stride = lcap + T;
  const int o_ovfA = 2 * rec_stride + slab_slots;
  const __amdgpu_buffer_rsrc_t rx = make_rsrc(xbuf);
  constexpr int kPar = 2;
  const int S = rec_bytes, par = 2 * rec_bytes, tab_off = kPar * par;
  const unsigned xcc_want = (tag0 & 0x0fffffffu) << 4;
  const unsigned p0 = tag0 & 1u;  // parity of the first step: its records live in area p0

  const size_t hl = (size_t)wg * T + lane;
  const unsigned meta = wg_meta[hl];
  const int slot = wg_slot[hl];
  const int pv = wg_vid[hl];
  const int nbr_code = wg_nbr[hl];
  const int frid = (lane < n_fetch) ? wg_fetch[hl] : -1;  // the foreign record this lane fetches
  const int loc = (int)((meta >> 13) & 2047u);
  const bool active = (meta & kWgActiveBit) != 0u;
  const bool valid = (meta & kWgValidBit) != 0u, publishes = (meta & kWgPublishBit) != 0u;
  const bool state_lane = (meta & kWgHeadBit) != 0u;
  const unsigned degx = (meta & kWgHeadBit) ? ((meta >> 6) & 127u) : (active ? 255u : 0u);
  const unsigned long long rm1 = __ballot(degx > 1u), rm2 = __ballot(degx > 2u), rm3 = __ballot(degx > 3u), rm4 = __ballot(degx > 4u),
                           rm5 = __ballot(degx > 5u), rm6 = __ballot(degx > 6u), rm7 = __ballot(degx > 7u), rm8 = __ballot(degx > 8u);
  const int nbr_idx = active ? ((nbr_code < 0) ? lcap + (nbr_code & 0x7fffffff) : nbr_code) : (valid ? loc : 0);

  int4 rec = make_int4(0, 0, 0, 0);
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (active) {
    rec = hrec[slot];
    q = hq[slot];
  }
  const bool is_target = rec.x < 0;
  const float alpha = __int_as_float(rec.y), dx = __int_as_float(rec.z), dy = __int_as_float(rec.w);
  const float beta = q.w;
  float q1 = q.x;
  v2f_t q23 = {q.y, q.z};
  // signed per-lane constants: the per-role selects of the primal contributions folded in (nltgv2_persistent.hip, "step")
  const float ac = is_target ? alpha : -alpha;
  const float sg = is_target ? -1.0f : 1.0f;  // the dual update takes (source - target): this lane's own record enters with this sign
  const v2f_t P12 = {alpha * dx, alpha * dy};
  const v2f_t C2 = !active ? v2f_t{0.0f, 0.0f} : is_target ? v2f_t{beta, beta} : v2f_t{-dx, -dy};
  const float nbeta = -beta;
  const v2f_t beta2 = {beta, beta}, nbeta2 = {nbeta, nbeta}, sg2 = {sg, sg};

  float4 st = make_float4(0.f, 0.f, 0.f, 0.f), bs4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float2 aux = make_float2(0.f, 0.f);
  if (valid) {
    st = vstate[pv];
    aux = vaux[pv];
    bs4 = bar_in[pv];
  }
  const float data = st.w;
  const float thr = p.step_x * (p.data_factor * aux.x);
  float x = st.x;
  v2f_t w12 = {st.y, st.z};
  float xb = bs4.x;
  v2f_t wb12 = {bs4.y, bs4.z};
  float x_prev = x;
  v2f_t w_prev = w12;
  bool timed_out = n_fetch > T;  // (the host never launches such a layout in this form)

  const int my_off = (rid_base + loc) << 4;
  // (a lane without a vertex writes its record to a spare entry of its own, which nobody reads)
  const int rec_w = valid ? loc : o_ovfA + lane, rec_wstride = valid ? rec_stride : 0;

  // fetch slots: tag 0 is never a live tag
  lds[lcap + lane] = make_float4(0.f, 0.f, 0.f, 0.f);
  lds[rec_stride + lcap + lane] = make_float4(0.f, 0.f, 0.f, 0.f);

  // ---- where this lane's polls read: the remote copy of its foreign record, or the copy in this XCD's L2 ------------
  int off0 = (frid >= 0) ? (frid << 4) : 0;
  bool fetch_remote = frid >= 0;
  {  // (the XCC-table exchange of the general kernel, word for word)
    const unsigned my_xcc = read_xcc_id();
    if (state_lane && publishes)
      __builtin_amdgcn_raw_buffer_store_b32((int)(xcc_want | my_xcc), rx, tab_off + (my_off >> 2), 0, kAuxSc1);
    if (n_fetch > 0 && !timed_out) {
      bool pend = frid >= 0;
      unsigned g0 = 0, spins = 0;
      for (;;) {
        if (pend) {
          int o = tab_off + (frid << 2);
          asm volatile("" : "+v"(o)::"memory");
          g0 = (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rx, o, 0, kAuxSc1);
          pend = ((g0 & ~15u) != xcc_want);
        }
        if (!__any(pend)) break;
        if (++spins > max_spins) {
          timed_out = true;
          const unsigned long long pm = __ballot(pend);
          const int fl = __ffsll((long long)pm) - 1;
          const int ff = __shfl(frid, fl, 64);
          const unsigned gs = (unsigned)__shfl((int)g0, fl, 64);
          if (lane == 0) report_expired(err, 2, wg, -1, pm, ff, gs, xcc_want);
          break;
        }
        __builtin_amdgcn_s_sleep(2);
      }
      if (!timed_out && frid >= 0 && (g0 & 15u) == my_xcc) off0 += S, fetch_remote = false;
    }
  }
  const unsigned long long fetch_mask = __ballot(frid >= 0);  // the lanes with a fetch duty (the wave runs with all 64 lanes)
  const bool pub_lane = state_lane && publishes;
  const char* const xb_base = static_cast<const char*>(xbuf);
  const bool placed = place_pool != nullptr;
  int pub0 = -1, pub1 = -1;
  const char* src0 = xb_base + off0;
  const char* src1 = xb_base + off0 + par;
  if (placed) {
    if (pub_lane) pub0 = rec_off[rid_base + loc], pub1 = rec_off[rec_off_stride + rid_base + loc];
    if (fetch_remote) {
      const int o0 = rec_off[frid], o1 = rec_off[rec_off_stride + frid];
      if (o0 >= 0) src0 = place_pool + o0;
      if (o1 >= 0) src1 = place_pool + o1;
    }
  }
  // where the two copies of this lane's record go, by parity: the remote one (its place in the pool, or the linear one) and the
  // one for readers on this XCD (a plain store: it stays in this XCD's L2)
  char* const xb_w = static_cast<char*>(xbuf);
  char* const pa0 = pub0 >= 0 ? place_pool + pub0 : xb_w + my_off;
  char* const pa1 = pub1 >= 0 ? place_pool + pub1 : xb_w + my_off + par;
  char* const la0 = xb_w + my_off + S;
  char* const la1 = xb_w + my_off + S + par;
  {
    lds[(p0 ? rec_wstride : 0) + rec_w] = make_float4(xb, wb12.x, wb12.y, __uint_as_float(tag0));  // area A
    if (pub_lane) {
      v4i_t o;
      o.x = __float_as_int(xb), o.y = __float_as_int(wb12.x), o.z = __float_as_int(wb12.y), o.w = (int)tag0;
      asm volatile("global_store_dwordx4 %0, %1, off sc1\n\t"
                   "global_store_dwordx4 %2, %1, off" ::"v"(p0 ? pa1 : pa0), "v"(o), "v"(p0 ? la1 : la0) : "memory");
    }
  }
  lds_wave_sync();
  const unsigned lds_addr0 = (unsigned)(size_t)(lds);  // LDS byte address of the dynamic array

  // what the statement reads from scalar registers
  const unsigned long long it_mask = __ballot(is_target), pub_mask = __ballot(pub_lane), rec_mask = __ballot(state_lane || !valid);
  const unsigned u_sq = __float_as_uint(p.step_q), u_sx = __float_as_uint(p.step_x), u_th = __float_as_uint(p.theta);
  const unsigned long long sq2 = ((unsigned long long)u_sq << 32) | u_sq, sx2 = ((unsigned long long)u_sx << 32) | u_sx,
                           th2 = ((unsigned long long)u_th << 32) | u_th;  // (the packed halves: both lanes of a pair take the same scalar)
  const float x_min_v = p.x_min, x_max_v = p.x_max;  // (the selects of the clamps take their constant from a vector register)
  const float neg_zero = -0.0f;
  unsigned ok_lane = 1u;  // stays 1 while this lane's (q1r, q2r, q3r) are finite in every step: the reference's FLAME_ASSERT h:174

  // One step: tag s.  rd_nbr: LDS byte address of the neighbour's record; dst: LDS byte address of the step's fetch slots; src: this
  // lane's poll address; rd_own / wr_own: LDS byte addresses of this vertex's record of step s / of step s + 1; pub_r, pub_l: where
  // the two copies of the record of step s + 1 go.
  auto step = [&](const unsigned s, const unsigned rd_nbr, const unsigned dst, const unsigned rd_own, const unsigned wr_own, const int it,
                  const char* const src, char* const pub_r, char* const pub_l) {
    const unsigned own_slot = dst + 16u * (unsigned)lane;
    const unsigned s_next = s + 1u;
    {
      unsigned cnt, keep, pend_lo, tag_seen, outer, ab;
      unsigned long long pnarrow, exec_saved, t64a, t64b;
      // The statement: this vertex's (x_bar, w_bar) from the record its head left in LDS and the tag of the record to come (both
      // ahead of the wait); up to 64 poll rounds -- one LDS-DMA load per fetch lane that still waits, then every lane's neighbour
      // record from LDS, tag first -- at issue priority 0; from the wait's exit at priority 3: dual update, contributions, ordered sum,
      // vertex update, the record, both stores; then priority 0 again, the record into LDS, and what the publish did not need (the NaN
      // check, the state for the next step, step()'s prev copy -- the register copies among these sit in the two wait states between a
      // v_cmp and the v_cndmask that reads VCC, which the packed w arithmetic fills first).  64 rounds without all tags: the bounded
      // fallback of the general kernel -- the abort flag, the spin budget, 64 more rounds -- inside the statement as well (a loop
      // around it would copy the step's whole state in front of every wait); it leaves with pend_lo != 0 and nothing done.  The code of
      // a patch with a vertex of 9-16 edges stands in front of the statement's entry: the common case falls through from shift 7
      // into the vertex update.
      asm volatile("s_branch 0f\n\t"
                   "5:\n\t"
                   PVL_RM(8, m8) PVL_ADDS(9)
                   "s_cmp_le_u32 %[md], 10\n\t"
                   "s_cbranch_scc1 6f\n\t"
                   PVL_ADDS(10) PVL_ADDS(11)
                   "s_cmp_le_u32 %[md], 12\n\t"
                   "s_cbranch_scc1 6f\n\t"
                   PVL_ADDS(12)
                   "s_cmp_le_u32 %[md], 13\n\t"
                   "s_cbranch_scc1 6f\n\t"
                   PVL_ADDS(13)
                   "s_cmp_le_u32 %[md], 14\n\t"
                   "s_cbranch_scc1 6f\n\t"
                   PVL_ADDS(14) PVL_ADDS(15)
                   "s_branch 6f\n\t"
                   "0:\n\t"
                   "ds_read_b32 v67, %[ro]\n\t"
                   "ds_read2_b32 v[70:71], %[ro] offset0:1 offset1:2\n\t"
                   "v_mov_b32 v95, %[tagn]\n\t"
                   "s_setprio 0\n\t"
                   "s_mov_b64 %[ex], exec\n\t"
                   "s_mov_b32 %[keep], m0\n\t"
                   "s_mov_b32 m0, %[dst]\n\t"
                   "s_mov_b32 %[cnt], 0\n\t"
                   "s_mov_b32 %[outer], 0\n\t"
                   "s_mov_b64 %[pn], %[fm]\n\t"
                   "1:\n\t"
                   "s_mov_b64 exec, %[pn]\n\t"
                   "global_load_lds_dwordx4 %[src], off sc1\n\t"
                   "s_mov_b64 exec, %[ex]\n\t"
                   "ds_read_b32 v64, %[ra] offset:12\n\t"
                   "ds_read_b32 v65, %[fa] offset:12\n\t"
                   "ds_read_b32 v66, %[ra]\n\t"
                   "ds_read2_b32 v[68:69], %[ra] offset0:1 offset1:2\n\t"
                   "s_add_u32 %[cnt], %[cnt], 1\n\t"
                   "s_waitcnt lgkmcnt(0)\n\t"
                   "v_cmp_ne_u32_e32 vcc, %[tag], v65\n\t"
                   "s_and_b64 %[pn], vcc, %[fm]\n\t"
                   "v_cmp_ne_u32_e32 vcc, %[tag], v64\n\t"
                   "s_cmp_lt_u32 %[cnt], 64\n\t"
                   "s_cbranch_vccz 2f\n\t"
                   "s_cbranch_scc1 1b\n\t"
                   "v_mov_b32 v97, 0\n\t"
                   "global_load_dword v97, v97, %[abp] sc1\n\t"
                   "s_waitcnt vmcnt(0)\n\t"
                   "v_readfirstlane_b32 %[ab], v97\n\t"
                   "s_add_u32 %[outer], %[outer], 1\n\t"
                   "s_cmp_lg_u32 %[ab], 0\n\t"
                   "s_cbranch_scc1 7f\n\t"
                   "s_mov_b32 %[cnt], 0\n\t"
                   "s_cmp_le_u32 %[outer], %[omax]\n\t"
                   "s_cbranch_scc1 1b\n\t"
                   "7:\n\t"
                   "s_or_b32 %[pl], vcc_lo, vcc_hi\n\t"
                   "v_mov_b32 %[tv], v64\n\t"
                   "s_branch 8f\n\t"
                   "2:\n\t"
                   "s_setprio 3\n\t"
                   // ---- dual update of this half-edge's private q copy (cc:99-110) ----
                   // (source - target) of the EDGE, whichever end this lane is: sg * own - sg * neighbour in one rounding (sg = +-1: the
                   // product is exact).  own - neighbour times a negated weight is the same value except where it is a zero: x - x is +0.0
                   // for either order, and its negation is not.
                   "v_mul_f32 v76, %[sg], v67\n\t"
                   "v_pk_mul_f32 v[72:73], %[sg2], v[70:71]\n\t"
                   "v_fma_f32 v76, v66, -%[sg], v76\n\t"
                   "v_pk_fma_f32 v[72:73], v[68:69], %[sg2], v[72:73] neg_lo:[0,1,0] neg_hi:[0,1,0]\n\t"
                   "v_cndmask_b32_e64 v75, v71, v69, %[itm]\n\t"
                   "v_cndmask_b32_e64 v74, v70, v68, %[itm]\n\t"
                   "v_mul_f32 v76, %[al], v76\n\t"
                   "v_pk_mul_f32 v[74:75], %[P12], v[74:75]\n\t"
                   "v_pk_mul_f32 v[72:73], %[be2], v[72:73]\n\t"
                   "v_sub_f32 v76, v76, v74\n\t"
                   "v_sub_f32 v76, v76, v75\n\t"
                   "v_mul_f32 v76, %[sq], v76\n\t"
                   "v_add_f32 v96, %[q1], v76\n\t"
                   "v_pk_mul_f32 v[72:73], %[sq2], v[72:73]\n\t"
                   "v_med3_f32 %[q1], v96, -1.0, 1.0\n\t"
                   "v_pk_add_f32 v[98:99], %[q23], v[72:73]\n\t"
                   // ---- this endpoint's share of the primal scatter (cc:126-141) as ordered contributions ----
                   "v_mul_f32 v77, %[sx], %[q1]\n\t"
                   "v_med3_f32 v100, v98, -1.0, 1.0\n\t"
                   "v_med3_f32 v101, v99, -1.0, 1.0\n\t"
                   "v_pk_mul_f32 v[78:79], %[sx2], v[100:101]\n\t"
                   "v_mul_f32 v77, %[ac], v77\n\t"
                   "v_cndmask_b32_e64 v81, v77, v79, %[itm]\n\t"
                   "v_cndmask_b32_e64 v80, v77, v78, %[itm]\n\t"
                   "v_pk_mul_f32 v[80:81], %[C2], v[80:81]\n\t"
                   "v_pk_mul_f32 v[82:83], %[nb2], v[78:79]\n\t"
                   "v_pk_add_f32 v[86:87], %[w12], v[80:81]\n\t"
                   "v_cndmask_b32_e64 v83, v83, %[nz], %[itm]\n\t"
                   "v_cndmask_b32_e64 v82, v82, %[nz], %[itm]\n\t"
                   "v_pk_add_f32 v[86:87], v[82:83], v[86:87]\n\t"
                   "v_add_f32 v84, %[x], v77\n\t"
                   // ---- ordered accumulation across the lanes of the vertex, towards its head ----
                   // (a DPP source must be two instructions old: v82 / v83 are, the s_mov and the adds in front of them count)
                   PVL_RM(1, m1) PVL_RM(2, m2) PVL_RM(3, m3) PVL_RM(4, m4) PVL_RM(5, m5) PVL_RM(6, m6) PVL_RM(7, m7)
                   "s_cmp_gt_u32 %[md], 8\n\t"
                   "s_cbranch_scc1 5b\n\t"
                   "6:\n\t"
                   "s_mov_b64 exec, %[ex]\n\t"
                   // ---- vertex update: proxL1, extragradient (vertex_update of nltgv2_persistent_common.hpp) ----
                   "v_sub_f32 v85, v84, %[dat]\n\t"
                   "v_add_f32 v90, %[thr], v84\n\t"
                   "v_cmp_lt_f32_e64 vcc, v85, -%[thr]\n\t"
                   "v_sub_f32 v91, v84, %[thr]\n\t"
                   "v_pk_add_f32 v[88:89], v[86:87], %[w12] neg_lo:[0,1] neg_hi:[0,1]\n\t"
                   "v_cndmask_b32_e32 v90, %[dat], v90, vcc\n\t"
                   "v_cmp_gt_f32_e32 vcc, v85, %[thr]\n\t"
                   "v_pk_mul_f32 v[88:89], %[th2], v[88:89]\n\t"
                   "v_mov_b64 %[wp], %[w12]\n\t"
                   "v_cndmask_b32_e32 v90, v90, v91, vcc\n\t"
                   "v_cmp_gt_f32_e32 vcc, %[xmn], v90\n\t"
                   "v_add_f32 v93, v86, v88\n\t"
                   "v_add_f32 v94, v87, v89\n\t"
                   "v_cndmask_b32_e32 v90, v90, %[xmnv], vcc\n\t"
                   "v_cmp_lt_f32_e32 vcc, %[xmx], v90\n\t"
                   "v_mov_b64 %[w12], v[86:87]\n\t"
                   "v_mov_b32 %[xp], %[x]\n\t"
                   "v_cndmask_b32_e32 v91, v90, %[xmxv], vcc\n\t"
                   "v_sub_f32 v85, v91, %[x]\n\t"
                   "v_mul_f32 v85, %[th], v85\n\t"
                   "v_add_f32 v85, v91, v85\n\t"
                   "v_cmp_gt_f32_e32 vcc, %[xmn], v85\n\t"
                   "v_mov_b32 %[x], v91\n\t"
                   "v_mov_b64 %[q23], v[100:101]\n\t"
                   "v_cndmask_b32_e32 v85, v85, %[xmnv], vcc\n\t"
                   "v_cmp_lt_f32_e32 vcc, %[xmx], v85\n\t"
                   "v_cmp_le_f32_e64 %[ta], |v96|, %[fmx]\n\t"
                   "v_cmp_le_f32_e64 %[tb], |v98|, %[fmx]\n\t"
                   "v_cndmask_b32_e32 v92, v85, %[xmxv], vcc\n\t"
                   // ---- the record of step s + 1 leaves: the write-through copy, the copy for this XCD ----
                   "s_mov_b64 exec, %[pubm]\n\t"
                   "global_store_dwordx4 %[pr], v[92:95], off sc1\n\t"
                   "global_store_dwordx4 %[pl2], v[92:95], off\n\t"
                   "s_mov_b64 exec, %[recm]\n\t"
                   "s_setprio 0\n\t"
                   "ds_write_b128 %[wo], v[92:95]\n\t"
                   "s_mov_b64 exec, %[ex]\n\t"
                   "v_cndmask_b32_e64 %[ok], 0, %[ok], %[ta]\n\t"
                   "v_cmp_le_f32_e64 %[ta], |v99|, %[fmx]\n\t"
                   "v_cndmask_b32_e64 %[ok], 0, %[ok], %[tb]\n\t"
                   "s_mov_b32 %[pl], 0\n\t"
                   "v_cndmask_b32_e64 %[ok], 0, %[ok], %[ta]\n\t"
                   "8:\n\t"
                   "s_mov_b32 m0, %[keep]"
                   : [keep] "=&s"(keep), [cnt] "=&s"(cnt), [pl] "=&s"(pend_lo), [pn] "=&s"(pnarrow), [ex] "=&s"(exec_saved), [ta] "=&s"(t64a),
                     [tb] "=&s"(t64b), [outer] "=&s"(outer), [ab] "=&s"(ab), [tv] "=&v"(tag_seen), [ok] "+v"(ok_lane), [q1] "+v"(q1), [q23] "+v"(q23), [x] "+v"(x), [w12] "+v"(w12),
                     [xp] "+v"(x_prev), [wp] "+v"(w_prev)
                   : [src] "v"(src), [dst] "s"(dst), [ra] "v"(rd_nbr), [fa] "v"(own_slot), [ro] "v"(rd_own), [wo] "v"(wr_own), [pr] "v"(pub_r),
                     [pl2] "v"(pub_l), [tag] "s"(s), [tagn] "s"(s_next), [fm] "s"(fetch_mask), [itm] "s"(it_mask), [pubm] "s"(pub_mask),
                     [recm] "s"(rec_mask), [al] "v"(alpha), [sg] "v"(sg), [sg2] "v"(sg2), [P12] "v"(P12), [be2] "v"(beta2), [ac] "v"(ac), [C2] "v"(C2), [nb2] "v"(nbeta2),
                     [nz] "v"(neg_zero), [dat] "v"(data), [thr] "v"(thr), [xmnv] "v"(x_min_v), [xmxv] "v"(x_max_v), [sq] "s"(p.step_q),
                     [sq2] "s"(sq2), [sx] "s"(p.step_x), [sx2] "s"(sx2), [th] "s"(p.theta), [th2] "s"(th2), [xmn] "s"(p.x_min), [xmx] "s"(p.x_max),
                     [fmx] "s"(3.402823466e+38f), [abp] "s"(abort_flag), [omax] "s"(max_spins >> 4), [md] "s"(stride), [m1] "s"(rm1), [m2] "s"(rm2), [m3] "s"(rm3), [m4] "s"(rm4), [m5] "s"(rm5),
                     [m6] "s"(rm6), [m7] "s"(rm7), [m8] "s"(rm8)
                   : PVL_CLOBBERS);
      if (__builtin_expect(__builtin_amdgcn_readfirstlane(pend_lo) != 0u, 0)) {  // the wait expired, or the run is being aborted
        timed_out = true;
        if (__builtin_amdgcn_readfirstlane(ab) == 0u) {  // (the first to give up: the others leave through the abort flag)
          const unsigned long long pm = __ballot(tag_seen != s);
          const int fl = __ffsll((long long)pm) - 1;
          const int ni = __shfl(nbr_idx, fl, 64);
          const int ff = ni >= lcap ? __shfl(frid, ni - lcap, 64) : -2 - ni;  // foreign record id, or -2 - (local index)
          const unsigned gs = (unsigned)__shfl((int)tag_seen, fl, 64);
          if (lane == 0) report_expired(err, 3, wg, it, pm, ff, gs, s);
        }
      }
    }
  };

  // Two steps per trip with the parities fixed: area A holds the records of the first step, B those of the next.
  const int areaA = p0 ? rec_stride : 0, areaB = p0 ? 0 : rec_stride;
  const unsigned rdA_nbr = lds_addr0 + 16u * (unsigned)(areaA + nbr_idx), rdB_nbr = lds_addr0 + 16u * (unsigned)(areaB + nbr_idx);
  const unsigned dstA = __builtin_amdgcn_readfirstlane(lds_addr0 + 16u * (unsigned)(areaA + lcap));
  const unsigned dstB = __builtin_amdgcn_readfirstlane(lds_addr0 + 16u * (unsigned)(areaB + lcap));
  const int wrA_rec = (valid ? areaA : 0) + rec_w, wrB_rec = (valid ? areaB : 0) + rec_w;
  const unsigned ownA = lds_addr0 + 16u * (unsigned)wrA_rec, ownB = lds_addr0 + 16u * (unsigned)wrB_rec;
  // the records of step tag0 + even are in memory buffer p0 ("A"), those of the odd steps in the other
  const char* const srcA = p0 ? src1 : src0;
  const char* const srcB = p0 ? src0 : src1;
  char* const pubA = p0 ? pa1 : pa0;
  char* const pubB = p0 ? pa0 : pa1;
  char* const locA = p0 ? la1 : la0;
  char* const locB = p0 ? la0 : la1;
  int it = 0;
  for (; it + 1 < n_iters && !timed_out; it += 2) {
    step(tag0 + (unsigned)it, rdA_nbr, dstA, ownA, ownB, it, srcA, pubB, locB);
    if (timed_out) break;
    step(tag0 + (unsigned)it + 1u, rdB_nbr, dstB, ownB, ownA, it + 1, srcB, pubA, locA);
  }
  if (it < n_iters && !timed_out) step(tag0 + (unsigned)it, rdA_nbr, dstA, ownA, ownB, it, srcA, pubB, locB);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no LDS-DMA in flight when the wave ends

  if (timed_out) {
    if (lane == 0) {
      give_up(abort_flag, err, false);
      unsigned* const pg = tail->progress;  // (trace runs only) the step this patch was in when it left
      if (pg) pg[wg - wg_begin] = 0x80000000u | (unsigned)(it + 1);
    }
    return;
  }

  // the (x_bar, w_bar) of the last step: the record its head left in LDS (area B after an odd number of steps, A after an even one)
  const float4 last = lds[(n_iters & 1) ? wrB_rec : wrA_rec];
  xb = last.x, wb12 = v2f_t{last.y, last.z};
  if (state_lane) write_back_vertex(pv, x, w12, xb, wb12, x_prev, w_prev, data, vstate_out, bar_out, vprev, perm, tail);
  if (active) hq_out[slot] = make_float4(q1, q23.x, q23.y, beta);
  if (ok_lane == 0u && active) atomicOr(err, 1);
}

#undef PVL_RM
#undef PVL_ADDS
#undef PVL_CLOBBERS

// Dynamic LDS of one patch: the general kernel's map (pv_lds_bytes of nltgv2_persistent.hip)
unsigned pv_lean_lds_bytes(int lcap, int slab_slots) { return 16u * (unsigned)(2 * (lcap + 64) + slab_slots + 64); }

}  // namespace

// Waves of k_persistent_pv_lean REALLY resident per SIMD, by the rule of pv_real_waves_per_simd (nltgv2_persistent.hip): min(512 / VGPRs
// rounded up to 8, 800 / (SGPRs rounded up to 16, + 16), 8) from the register counts as built.  No SGPR cap here: the regime this
// kernel runs in has at most kPvPaceAbovePerCu = 13 patches per CU, four waves per SIMD hold them (tests/test_pv_lean.py re-derives the
// figure from the compiler's resource report).
int pv_lean_real_waves_per_simd() {
  // {VGPRs, SGPRs} -> waves: {<= 128, <= 96} -> min(4, 7)  (105 / 95 as built)
  return 4;
}

int pv_lean_patches_per_cu(const FusedArgs& a) {
  if (!a.wg_rowpack) return 0;
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, (const void*)k_persistent_pv_lean, 64, pv_lean_lds_bytes(a.wg_lcap, a.wg_slab_slots)) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n < 4 * pv_lean_real_waves_per_simd() ? n : 4 * pv_lean_real_waves_per_simd();
}

// One launch of k_persistent_pv_lean: the patch-per-wave branch of launch_persistent_run (nltgv2_persistent.hip) for the plain
// instance with the same-XCD copy on; the planner (nltgv2_run.hip, pv_lean_applies) decides where it may run.
int launch_persistent_pv_lean(const FusedArgs& a, const SolverParams& p, int wave_begin, int n_waves, int parity_in, unsigned tag0, int n_iters,
                              unsigned max_spins, int xcds, const RunTail* tail, bool cooperative, hipStream_t stream) {
  if (n_waves <= 0 || n_iters <= 0) return (int)hipSuccess;
  if (!a.wg_rowpack) return (int)hipErrorInvalidConfiguration;
  if (xcds < 1 || xcds > 8) xcds = 8;
  int wgx = (n_waves + xcds - 1) / xcds;
  const dim3 gv((unsigned)(wgx * 8)), bv(64u);
  int lcap = a.wg_lcap, slab_slots = a.wg_slab_slots, poll_gap = a.wg_poll_gap, dual = 1;
  const int32_t *w0 = a.wg_slot, *w1 = a.wg_vid, *w3 = a.wg_nbr, *w4 = a.wg_fetch, *w5 = a.wg_info;
  const uint32_t* w2 = a.wg_meta;
  const int4* hrec = a.hrec;
  const float4* hq = a.hq;
  const float4* vstate = a.vstate;
  float4* hq_out = a.hq_out;
  float4* vstate_out = a.vstate_out;
  const float2* vaux = a.vaux;
  const float4* bin = a.bar[parity_in];
  float4* bout = a.bar[parity_in ^ 1];  // always the other buffer: the input of a failed run stays intact
  float4* vprev = a.vprev;
  void* xbuf = a.xbuf;
  int rec_bytes = persistent_rec_bytes(a);
  SolverParams pp = p;
  int* err = a.err;
  int* abort_flag = a.abort_flag;
  const int32_t* perm = a.perm;
  unsigned* probe = nullptr;
  char* place_pool = (a.rec_off && wave_begin == 0 && xcds == 8) ? a.place_pool : nullptr;
  const int32_t* rec_off = a.rec_off;
  int rec_off_stride = a.rec_off_stride;
  unsigned* rot_word = place_pool ? a.rot_word : nullptr;
  const unsigned ldsv = pv_lean_lds_bytes(lcap, slab_slots);
  void* vargs[] = {&wave_begin, &n_waves, &wgx, &lcap, &slab_slots, &w0, &w1, &w2, &w3, &w4, &w5, &hrec, &hq, &vstate,
                   &hq_out, &vstate_out, &vaux, &bin, &bout, &vprev, &xbuf, &rec_bytes, &dual, &tag0, &n_iters,
                   &max_spins, &poll_gap, &pp, &err, &abort_flag, &perm, &tail, &probe, &place_pool, &rec_off, &rec_off_stride, &rot_word};
  const void* fv = (const void*)k_persistent_pv_lean;
  if (cooperative) return (int)hipLaunchCooperativeKernel(fv, gv, bv, vargs, ldsv, stream);
  return (int)hipExtLaunchKernel(fv, gv, bv, vargs, ldsv, stream, nullptr, a.stop_event, 0);
}

// Loads this translation unit's code object ahead of the first frame (see warm_module_persistent).
void warm_module_persistent_lean() {
  hipFuncAttributes fa;
  if (hipFuncGetAttributes(&fa, (const void*)k_persistent_pv_lean) != hipSuccess) (void)hipGetLastError();
}

}  // namespace flame_hip
