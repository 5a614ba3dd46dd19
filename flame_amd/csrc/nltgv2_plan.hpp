// nltgv2_plan.hpp -- the pure part of planning a persistent run (nltgv2_run.hip: plan_run), no HIP and no context: the wave groups of a graph too
// large for one launch, what the launch of a group is given, and where an open run / the lean patch kernel can apply as far as counts and options
// decide it.  tests/cpp/run_plan_test.cc pins every threshold.
#ifndef FLAME_AMD_NLTGV2_PLAN_HPP_
#define FLAME_AMD_NLTGV2_PLAN_HPP_

#include <cstddef>
#include <cstdint>
#include <vector>

namespace flame_hip {
namespace host {

constexpr int kPv2PaceAbovePerCu = 10, kPv2DensePreSleep = 2, kPv2DenseGap = 2;  // k_persistent_pv2's polls are paced from this many of its waves per CU (x64 cycles before the first poll / between rounds)
constexpr int kPvPaceAbovePerCu = 13;  // k_persistent_pv: above this many patches per CU its polls are paced (kPvDensePreSleep, kPvDenseGap)
constexpr int kPvDensePreSleep = 3, kPvDenseGap = 2;  // x64 cycles before the first poll of a step / between poll rounds (re-swept with the issue priorities in: 8 / 4 before them; profiles/r03_priority.txt)
constexpr int kPvPaceMoreAbovePerCu = 23;  // ... and above this many more slowly (a 1080p frame: 25 per CU)
constexpr int kPvDenserPreSleep = 5, kPvDenserGap = 4;
constexpr int kPvPreSleep = 0;         // k_persistent_pv: x64 cycles between a step's start and its first poll
constexpr int kPvPollGap = 2;          // k_persistent_pv polls: re-loading only the fetch entries still waiting, no pause between
                                       // rounds (with the round-2 first form of the kernel an s_sleep between rounds won by 1-3 %;
                                       // with the shorter hand-off path of its final form no pause wins by 3-4 % at 640x480)
constexpr int kDualMinWavesPerCu = 0;  // auto: exchange through the XCD's L2 when more waves than this share a CU
constexpr int kPreSleepTv = 2;  // x64-cycle sleep between publishing and the first neighbour poll of k_persistent_tv (insensitive, shortest wins)
constexpr unsigned kMaxSpins = 1u << 20;  // bound of every neighbour wait in the persistent run (~1 s of polling bursts)

// A persistent launch covers a contiguous range of waves of one form.
struct WaveGroup {
  int begin, count;
};

// `total` waves of `form` over groups of whole components (cw: first wave of every component), each at most `cap` waves.
inline int plan_groups(int form, int total, int cap, const std::vector<int32_t>& cw, std::vector<WaveGroup>* groups) {
  if (total <= cap) {
    groups->push_back(WaveGroup{0, total});
    return form;
  }
  if (cw.size() < 3) return 0;  // one component that does not fit: stream it
  // Groups of about equal size (the per-step time of a group grows with its waves, and a small last group would run at low occupancy): cut at the
  // component boundaries nearest to k * total / n_groups, never beyond what the chip holds; if the components are too uneven for that, fill greedily.
  for (size_t c = 0; c + 1 < cw.size(); ++c)
    if (cw[c + 1] - cw[c] > cap) return 0;  // a single component larger than the chip
  const int n_groups = (total + cap - 1) / cap;
  bool ok = true;
  {
    size_t c = 0;
    int begin = cw[0];
    for (int gi = 1; gi <= n_groups && ok; ++gi) {
      const long ideal = cw[0] + (long)gi * total / n_groups;
      size_t e = c + 1;  // at least one component per group
      while (e + 1 < cw.size() && cw[e] < ideal) ++e;
      if (gi == n_groups) e = cw.size() - 1;
      while (e > c + 1 && cw[e] - begin > cap) --e;
      if (cw[e] - begin > cap) ok = false;
      groups->push_back(WaveGroup{begin, cw[e] - begin});
      begin = cw[e], c = e;
      if (c + 1 >= cw.size() && gi < n_groups) break;
    }
    if (ok && begin != cw.back()) ok = false;  // balanced cuts did not cover everything within n_groups groups
  }
  if (!ok) {
    groups->clear();
    int begin = cw[0];
    for (size_t c = 0; c + 1 < cw.size(); ++c) {
      if (cw[c + 1] - begin > cap) {
        groups->push_back(WaveGroup{begin, cw[c] - begin});
        begin = cw[c];
      }
    }
    groups->push_back(WaveGroup{begin, cw.back() - begin});
  }
  return form;
}

// The values of the FLAME_NLTGV2_OPT_* test options a plan depends on (0 = default but for `dual`), and finish()'s replay rung.
struct PlanOptions {
  int dual = 1, xcds = 0, poll_gap = 0, presleep = 0, verify = 0, probe = 0, fault = 0, pv_lean = 0, replaying = 0;
};

// same-XCD exchange through L2: with the waves laid out along the Morton curve it wins at every size (per step: 640x480 -16 %, 1280x720 -23 %, 1080p -18 %, 7 frames -20 %, 15 -19 %)
inline bool dual_exchange_on(const PlanOptions& o, int count, int cus) {
  return o.dual == 2 || (o.dual == 1 && count > kDualMinWavesPerCu * cus);
}

// What the launch of one group is given.
struct GroupLaunch {
  int pw, dual, xcds;      // waves per workgroup | bit 0: same-XCD exchange, bits 1, 2: record verification, its test hook | XCDs it spreads over
  int presleep, poll_gap;  // the vertex-per-lane form's pre-sleep | the patch forms' (3, 4) poll gap | pre-sleep << 8
  unsigned spins_arg;      // bound of every wait, or the test hook's fault
  bool place;              // record placement is wanted (set by plan_run: it depends on the groups as a whole)
};

inline GroupLaunch group_launch(int form, int count, int cus, const PlanOptions& o) {
  GroupLaunch g{};
  g.pw = count <= 4 * cus ? 1 : 4;
  g.dual = (dual_exchange_on(o, count, cus) ? 1 : 0) | (o.verify == 2 ? 6 : o.verify == 1 ? 2 : 0);
  // A graph small enough runs on ONE XCD (32 CUs) entirely: every exchange stays in that XCD's L2 -- while its CUs get at most two patches each
  // (measured: 48 patches 0.98 against 1.21 us per step on all eight, 208 patches 1.53 against 1.33)
  const bool one_xcd = form == 3 && count <= 2 * (cus / 8);
  g.xcds = o.xcds > 0 ? o.xcds : one_xcd ? 1 : 8;
  g.presleep = o.presleep > 0 ? o.presleep - 1 : kPreSleepTv;
  // (test hook: a fault of 2^22 + n also hits the persistent replay of the chain, so that the per-step rung below it is exercised)
  g.spins_arg = (o.fault > 0 && (o.replaying == 0 || o.fault >= (1 << 22))) ? (0x80000000u | (unsigned)(o.fault & ((1 << 22) - 1))) : kMaxSpins;
  // pacing of the patch-per-wave form: none where a CU holds few patches (a poll costs nothing there and a pause only delays the hand-off); at high
  // residency the polls of ~20 waves per CU saturate the L2s' request ports and the fabric and it is the hand-off itself that slows down (probe: 0.72 us
  // at 4 patches per CU, 1.03 at 15; 26 per CU unpaced: 50 us per step) -- a pause before the first poll and between rounds then wins (tools/pv_big.py
  // sweeps, profiles/r03_pv_dense.txt).  The two-half-edges form has its own (swept: profiles/r03_pv2.txt).
  const bool dense = count > (form == 4 ? kPv2PaceAbovePerCu : kPvPaceAbovePerCu) * cus;
  const bool denser = form == 3 && count > kPvPaceMoreAbovePerCu * cus;
  const int dense_gap = form == 4 ? kPv2DenseGap : denser ? kPvDenserGap : kPvDenseGap;
  const int dense_pre = form == 4 ? kPv2DensePreSleep : denser ? kPvDenserPreSleep : kPvDensePreSleep;
  const int gap = o.poll_gap > 0 ? o.poll_gap - 1 : dense ? (3 | ((dense_gap - 1) << 4)) : kPvPollGap;
  if (form == 3 || form == 4) g.poll_gap = gap | ((o.presleep > 0 ? o.presleep - 1 : dense ? dense_pre : kPvPreSleep) << 8);
  return g;
}

// An open run: ONE launch of the patch-per-wave form or of the two-half-edges form, of an even number of steps, without probe or record
// verification.  Their OPEN instances keep fewer patches resident than the plain ones (24 instead of 28 per CU; 16 instead of 20:
// tests/test_abi.py): graphs of at most 20 / 14 patches per CU.
inline bool open_run_applies(int form, size_t n_groups, int count, int cus, int n, const PlanOptions& o) {
  if (n_groups != 1 || (n & 1) != 0 || o.probe != 0 || o.verify != 0 || o.replaying != 0) return false;
  return (form == 3 && count <= 20 * cus) || (form == 4 && count <= 14 * cus);
}

// Where the lean patch kernel (k_persistent_pv_lean, nltgv2_persistent_lean.hip) can run instead of k_persistent_pv, as far as counts and options say:
// the patch-per-wave form as ONE launch of what would be the plain instance -- no probe, no verification, not an open run, not a replay, no fault
// injection -- with the default poll gap and pre-sleep, the same-XCD exchange on, below the paced regime.  (plan_run adds the layout's and the
// occupancy's say.  FLAME_NLTGV2_OPT_PV_LEAN: 1 = never, 2 = or the run fails.)  Everything else runs the general kernel.
inline bool pv_lean_may_apply(int form, size_t n_groups, int count, int cus, bool open_run, const PlanOptions& o) {
  if (form != 3 || n_groups != 1 || o.pv_lean == 1) return false;
  if (o.probe != 0 || o.verify != 0 || open_run || o.replaying != 0 || o.fault != 0) return false;
  if (o.poll_gap != 0 || o.presleep != 0) return false;
  return dual_exchange_on(o, count, cus) && count <= kPvPaceAbovePerCu * cus;
}

}  // namespace host
}  // namespace flame_hip

#endif  // FLAME_AMD_NLTGV2_PLAN_HPP_
