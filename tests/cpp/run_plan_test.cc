// tests/cpp/run_plan_test.cc -- host-only check of flame_amd/csrc/nltgv2_plan.hpp, built by `make -C flame_amd/csrc sanitize` under
// ASan + UBSan: the cut of a large graph into wave groups (plan_groups) and what the launch of a group is given (group_launch), on
// both sides of every threshold, plus where an open run and the lean patch kernel can apply.
// The expected launch parameters were written down from the expressions enqueue_run held before they moved into the header (one
// function of the same inputs, compared with group_launch over every count up to 30 waves per CU, both patch forms and every option
// value the tests set: no difference) -- they are not derived from the code under test.
#include <cstdio>
#include <vector>

#include "nltgv2_plan.hpp"

using namespace flame_hip::host;

static int fails = 0;
#define EXPECT(cond, ...)                       \
  do {                                          \
    if (!(cond)) {                              \
      std::printf("FAILED %s: ", #cond);        \
      std::printf(__VA_ARGS__);                 \
      std::printf("\n");                        \
      ++fails;                                  \
    }                                           \
  } while (0)

// component table from component sizes, first wave at `first`
static std::vector<int32_t> table(const std::vector<int>& sizes, int first = 0) {
  std::vector<int32_t> cw{first};
  for (int s : sizes) cw.push_back(cw.back() + s);
  return cw;
}

// groups are contiguous, start and end on component boundaries, cover [cw.front(), cw.back()) exactly, each at most cap
static void check_groups(const char* what, const std::vector<int32_t>& cw, int cap, size_t want_groups) {
  std::vector<WaveGroup> g;
  const int total = cw.back() - cw.front();
  const int form = plan_groups(3, total, cap, cw, &g);
  EXPECT(form == 3, "%s: form %d", what, form);
  EXPECT(g.size() == want_groups, "%s: %zu groups, expected %zu", what, g.size(), want_groups);
  if (g.empty()) return;
  int at = cw.front();
  for (const WaveGroup& gr : g) {
    EXPECT(gr.begin == at, "%s: group begins at %d, the one before ended at %d", what, gr.begin, at);
    EXPECT(gr.count > 0 && gr.count <= cap, "%s: group of %d waves, cap %d", what, gr.count, cap);
    bool b0 = false, b1 = false;
    for (int32_t c : cw) b0 = b0 || c == gr.begin, b1 = b1 || c == gr.begin + gr.count;
    EXPECT(b0 && b1, "%s: group [%d, %d) is not made of whole components", what, gr.begin, gr.begin + gr.count);
    at = gr.begin + gr.count;
  }
  EXPECT(at == cw.back(), "%s: groups end at %d, the components at %d", what, at, cw.back());
}

static void test_plan_groups() {
  const int cap = 100;
  {  // total <= cap: one group from wave 0, whatever the components
    std::vector<WaveGroup> g;
    EXPECT(plan_groups(2, 100, cap, table({40, 60}), &g) == 2 && g.size() == 1 && g[0].begin == 0 && g[0].count == 100, "one group");
    g.clear();
    EXPECT(plan_groups(4, 7, cap, {}, &g) == 4 && g.size() == 1 && g[0].count == 7, "one group without a component table");
  }
  check_groups("even components", table(std::vector<int>(12, 25)), cap, 3);          // 300 waves: ceil(300 / 100) balanced groups of 4
  check_groups("even components, ragged", table(std::vector<int>(7, 30)), cap, 3);   // 210 waves: 3 groups (3 + 2 + 2 components)
  check_groups("even components, offset", table(std::vector<int>(6, 50), 10), cap, 3);
  {  // balanced cuts of {cap, 1, cap, 1, cap} (ceil(302 / 100) = 4 groups) would need a group beyond cap: the greedy fill takes over
    const std::vector<int32_t> cw = table({cap, 1, cap, 1, cap});
    check_groups("uneven components", cw, cap, 5);
    std::vector<WaveGroup> g;
    plan_groups(3, 302, cap, cw, &g);
    const int want[5][2] = {{0, 100}, {100, 1}, {101, 100}, {201, 1}, {202, 100}};
    for (size_t i = 0; i < g.size() && i < 5; ++i) EXPECT(g[i].begin == want[i][0] && g[i].count == want[i][1], "uneven: group %zu = [%d, +%d)", i, g[i].begin, g[i].count);
  }
  check_groups("uneven components, small ones first", table({1, 1, cap, 60, 60, 1}), cap, 4);
  {
    std::vector<WaveGroup> g;
    EXPECT(plan_groups(3, 231, cap, table({50, cap + 1, 80}), &g) == 0, "one component larger than cap: no groups");
    g.clear();
    EXPECT(plan_groups(3, 150, cap, table({150}), &g) == 0, "a single component over cap: no groups");
    g.clear();
    EXPECT(plan_groups(3, 150, cap, {}, &g) == 0, "no component table over cap: no groups");
  }
}

struct LaunchCase {
  int form, count;
  int opt[7];  // dual, xcds, poll_gap, presleep, verify, fault, replaying
  struct { int pw, dual, xcds, presleep, poll_gap; unsigned spins_arg; } want;
};

static void test_group_launch() {
  const int cus = 256;
  static const LaunchCase cases[] = {
    // 4 * cus: one wave per workgroup up to it, four beyond (every form)
    {3, 1024, {1, 0, 0, 0, 0, 0, 0}, {1, 1, 8, 2, 0x2, 0x100000u}},
    {3, 1025, {1, 0, 0, 0, 0, 0, 0}, {4, 1, 8, 2, 0x2, 0x100000u}},
    {4, 1024, {1, 0, 0, 0, 0, 0, 0}, {1, 1, 8, 2, 0x2, 0x100000u}},
    {4, 1025, {1, 0, 0, 0, 0, 0, 0}, {4, 1, 8, 2, 0x2, 0x100000u}},
    {2, 1024, {1, 0, 0, 0, 0, 0, 0}, {1, 1, 8, 2, 0x0, 0x100000u}},
    {2, 1025, {1, 0, 0, 0, 0, 0, 0}, {4, 1, 8, 2, 0x0, 0x100000u}},
    // 2 * cus / 8: the patch-per-wave form on one XCD up to it -- the other forms and OPT_XCDS never mind
    {3, 64, {1, 0, 0, 0, 0, 0, 0}, {1, 1, 1, 2, 0x2, 0x100000u}},
    {3, 65, {1, 0, 0, 0, 0, 0, 0}, {1, 1, 8, 2, 0x2, 0x100000u}},
    {4, 64, {1, 0, 0, 0, 0, 0, 0}, {1, 1, 8, 2, 0x2, 0x100000u}},
    {3, 64, {1, 8, 0, 0, 0, 0, 0}, {1, 1, 8, 2, 0x2, 0x100000u}},
    {3, 65, {1, 1, 0, 0, 0, 0, 0}, {1, 1, 1, 2, 0x2, 0x100000u}},
    // kDualMinWavesPerCu (0): OPT_DUAL_PUBLISH = 1 exchanges through the XCD's L2 above it, 0 never, 2 always; the verification bits
    {3, 0, {1, 0, 0, 0, 0, 0, 0}, {1, 0, 1, 2, 0x2, 0x100000u}},
    {3, 1, {1, 0, 0, 0, 0, 0, 0}, {1, 1, 1, 2, 0x2, 0x100000u}},
    {3, 1, {0, 0, 0, 0, 0, 0, 0}, {1, 0, 1, 2, 0x2, 0x100000u}},
    {3, 0, {2, 0, 0, 0, 0, 0, 0}, {1, 1, 1, 2, 0x2, 0x100000u}},
    {3, 1, {1, 0, 0, 0, 1, 0, 0}, {1, 3, 1, 2, 0x2, 0x100000u}},
    {3, 1, {0, 0, 0, 0, 2, 0, 0}, {1, 6, 1, 2, 0x2, 0x100000u}},
    // kPvPaceAbovePerCu, kPvPaceMoreAbovePerCu: the patch-per-wave form's pacing (the two-half-edges form has one regime beyond its own)
    {3, 3328, {1, 0, 0, 0, 0, 0, 0}, {4, 1, 8, 2, 0x2, 0x100000u}},
    {3, 3329, {1, 0, 0, 0, 0, 0, 0}, {4, 1, 8, 2, 0x313, 0x100000u}},
    {3, 5888, {1, 0, 0, 0, 0, 0, 0}, {4, 1, 8, 2, 0x313, 0x100000u}},
    {3, 5889, {1, 0, 0, 0, 0, 0, 0}, {4, 1, 8, 2, 0x533, 0x100000u}},
    {4, 3329, {1, 0, 0, 0, 0, 0, 0}, {4, 1, 8, 2, 0x213, 0x100000u}},
    {4, 5889, {1, 0, 0, 0, 0, 0, 0}, {4, 1, 8, 2, 0x213, 0x100000u}},
    // kPv2PaceAbovePerCu: the two-half-edges form's (the patch-per-wave form is not paced there yet)
    {4, 2560, {1, 0, 0, 0, 0, 0, 0}, {4, 1, 8, 2, 0x2, 0x100000u}},
    {4, 2561, {1, 0, 0, 0, 0, 0, 0}, {4, 1, 8, 2, 0x213, 0x100000u}},
    {3, 2561, {1, 0, 0, 0, 0, 0, 0}, {4, 1, 8, 2, 0x2, 0x100000u}},
    // OPT_POLL_GAP / OPT_PRESLEEP override the pacing
    {3, 3329, {1, 0, 1, 0, 0, 0, 0}, {4, 1, 8, 2, 0x300, 0x100000u}},
    {3, 3329, {1, 0, 4, 0, 0, 0, 0}, {4, 1, 8, 2, 0x303, 0x100000u}},
    {3, 3329, {1, 0, 0, 1, 0, 0, 0}, {4, 1, 8, 0, 0x13, 0x100000u}},
    {3, 5889, {1, 0, 0, 5, 0, 0, 0}, {4, 1, 8, 4, 0x433, 0x100000u}},
    {4, 2561, {1, 0, 3, 5, 0, 0, 0}, {4, 1, 8, 4, 0x402, 0x100000u}},
    {2, 2561, {1, 0, 0, 5, 0, 0, 0}, {4, 1, 8, 4, 0x0, 0x100000u}},
    // OPT_FAULT_INJECT: not in a replay, unless it is 2^22 + n
    {3, 100, {1, 0, 0, 0, 0, 200, 0}, {1, 1, 8, 2, 0x2, 0x800000c8u}},
    {3, 100, {1, 0, 0, 0, 0, 200, 1}, {1, 1, 8, 2, 0x2, 0x100000u}},
    {3, 100, {1, 0, 0, 0, 0, 4194504, 0}, {1, 1, 8, 2, 0x2, 0x800000c8u}},
    {3, 100, {1, 0, 0, 0, 0, 4194504, 1}, {1, 1, 8, 2, 0x2, 0x800000c8u}},
  };
  for (const LaunchCase& c : cases) {
    PlanOptions o;
    o.dual = c.opt[0], o.xcds = c.opt[1], o.poll_gap = c.opt[2], o.presleep = c.opt[3], o.verify = c.opt[4], o.fault = c.opt[5], o.replaying = c.opt[6];
    const GroupLaunch g = group_launch(c.form, c.count, cus, o);
    EXPECT(g.pw == c.want.pw && g.dual == c.want.dual && g.xcds == c.want.xcds && g.presleep == c.want.presleep && g.poll_gap == c.want.poll_gap &&
               g.spins_arg == c.want.spins_arg && !g.place,
           "form %d, %d waves, options {%d %d %d %d %d %d %d}: pw %d dual %d xcds %d presleep %d poll_gap 0x%x spins 0x%x", c.form, c.count, c.opt[0],
           c.opt[1], c.opt[2], c.opt[3], c.opt[4], c.opt[5], c.opt[6], g.pw, g.dual, g.xcds, g.presleep, (unsigned)g.poll_gap, g.spins_arg);
  }
}

static void test_open_and_lean() {
  const int cus = 256;
  const PlanOptions def;
  // an open run: one group of at most 20 (patch-per-wave) / 14 (two half-edges) waves per CU, an even bound, no probe / verification / replay
  EXPECT(open_run_applies(3, 1, 20 * cus, cus, 8, def) && !open_run_applies(3, 1, 20 * cus + 1, cus, 8, def), "open run, patch-per-wave limit");
  EXPECT(open_run_applies(4, 1, 14 * cus, cus, 8, def) && !open_run_applies(4, 1, 14 * cus + 1, cus, 8, def), "open run, two-half-edges limit");
  EXPECT(!open_run_applies(2, 1, 100, cus, 8, def) && !open_run_applies(0, 0, 0, cus, 8, def), "open run: the other forms never");
  EXPECT(!open_run_applies(3, 1, 100, cus, 7, def) && !open_run_applies(4, 1, 100, cus, 1001, def), "open run: odd n refused");
  EXPECT(!open_run_applies(3, 2, 100, cus, 8, def), "open run: one launch only");
  PlanOptions o = def;
  o.verify = 1;
  EXPECT(!open_run_applies(3, 1, 100, cus, 8, o), "open run: not with record verification");
  o = def, o.probe = 1;
  EXPECT(!open_run_applies(3, 1, 100, cus, 8, o), "open run: not with the probe");
  o = def, o.replaying = 1;
  EXPECT(!open_run_applies(3, 1, 100, cus, 8, o), "open run: not in a replay");
  // the lean patch kernel: below the paced regime, the same-XCD exchange on, nothing but defaults
  EXPECT(pv_lean_may_apply(3, 1, kPvPaceAbovePerCu * cus, cus, false, def) && !pv_lean_may_apply(3, 1, kPvPaceAbovePerCu * cus + 1, cus, false, def), "lean: paced regime");
  EXPECT(!pv_lean_may_apply(4, 1, 100, cus, false, def) && !pv_lean_may_apply(3, 2, 100, cus, false, def) && !pv_lean_may_apply(3, 1, 100, cus, true, def), "lean: form, groups, open run");
  for (int k = 0; k < 8; ++k) {
    o = def;
    (k == 0 ? o.dual : k == 1 ? o.poll_gap : k == 2 ? o.presleep : k == 3 ? o.verify : k == 4 ? o.probe : k == 5 ? o.fault : k == 6 ? o.replaying : o.pv_lean) = k == 0 ? 0 : 1;
    EXPECT(!pv_lean_may_apply(3, 1, 100, cus, false, o), "lean: option %d off its default", k);
  }
  o = def, o.dual = 2, o.pv_lean = 2, o.xcds = 1;
  EXPECT(pv_lean_may_apply(3, 1, 100, cus, false, o), "lean: forced exchange, required kernel, one XCD");
}

int main() {
  test_plan_groups();
  test_group_launch();
  test_open_and_lean();
  std::printf(fails ? "run plan: %d check(s) FAILED\n" : "run plan: all ok\n", fails);
  return fails ? 1 : 0;
}
