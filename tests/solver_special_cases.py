"""Solver inputs at the edges of float32 -- signed zeros, subnormals, non-finite values, the extremes of flame_nltgv2_params -- and, per
case, what the CPU checker's result must still show for the case to be worth running (check_reaches).  The synthetic graphs of the rest
of the suite hold positive data around 1: nothing there tells +0.0 from -0.0, holds a subnormal, or reaches a clamp with infinite bounds.

A case is a function that returns a graph dict ready for upload_graph (state arrays included), wrapped in a Case with its parameters
and the step counts it is run for.  reference(case, n) runs the C checker (oracle/nltgv2_oracle.c) once per (case, n) and keeps the
result: tests/test_solver_special_values_ref.py holds the numpy restatement and check_reaches against it, and
tests/test_gpu_solver_special_values.py every run path of the device.  The floors in check_reaches are conditions on the checker's
output, never on the device's; the counts quoted beside them are what the checker gives for these inputs (x86-64, no FMA)."""
from __future__ import annotations

import numpy as np

from flame_amd import synth
from oracle import capi as oracle
from tests.helpers import float_bits, random_graph

F = np.float32
TINY = np.finfo(F).tiny  # 2**-126, the smallest normal float32
NEG_ZERO, POS_ZERO = 0x80000000, 0x00000000
DATA_KEYS = ("data_term", "x", "x_bar", "x_prev")
W_KEYS = ("w1", "w2", "w1_bar", "w2_bar", "w1_prev", "w2_prev")
Q_KEYS = ("q1", "q2", "q3")
STEPS = (1, 2, 7)  # the per-step path (and the lean kernel's tail, then one trip of its two-step loop); every persistent form, odd


def n_subnormal(a) -> int:
    return int(((a != 0) & (np.abs(a) < TINY)).sum())


def n_bits(a, pattern) -> int:
    return int((float_bits(a) == pattern).sum())


def n_saturated(g) -> int:
    """Duals at exactly +1 or -1: proxNLTGV2Conj clamped them."""
    return sum(int((np.abs(g[k]) == 1).sum()) for k in Q_KEYS)


def n_nan(g) -> int:
    return sum(int(np.isnan(g[k]).sum()) for k in synth.STATE_KEYS)


def degrees(g):
    return np.bincount(np.concatenate([g["src"], g["dst"]]), minlength=g["V"])


_BASE = {}


def base_graph():
    """G: 420 vertices, 1200 edges, largest degree <= 16 (the lean kernel takes it), small enough for one XCD."""
    if "G" not in _BASE:
        g = random_graph(420, 1200, seed=11)
        assert degrees(g).max() <= 16
        _BASE["G"] = g
    return synth.copy_graph(_BASE["G"])


def local_graph():
    """L: G's data and weights on a graph whose edges are LOCAL -- a jittered 21 x 20 grid, 50 apart (edges as long as G's: the same alpha),
    with right, down and diagonal edges (1179 of them), each oriented at random, the list shuffled.  G joins random pairs: a patch of
    k_persistent_pv2 (two half-edges per lane) would have to fetch more than its 64 distinct foreign records, so the library runs G one
    launch per step under FLAME_NLTGV2_OPT_PERSISTENT = 6.  L is the graph on which that kernel meets the cases made from G; every
    other path takes both."""
    if "L" not in _BASE:
        g0 = base_graph()
        rng = np.random.default_rng(12)
        W, H = 21, 20
        ii, jj = np.meshgrid(np.arange(W), np.arange(H))
        pos = (np.stack([ii.ravel(), jj.ravel()], 1) * 50.0 + rng.random((W * H, 2)) * 20.0).astype(F)
        vid = lambda x, y: y * W + x  # noqa: E731
        edges = []
        for y in range(H):
            for x in range(W):
                edges += [(vid(x, y), vid(x + 1, y))] if x + 1 < W else []
                edges += [(vid(x, y), vid(x, y + 1))] if y + 1 < H else []
                edges += [(vid(x, y), vid(x + 1, y + 1))] if x + 1 < W and y + 1 < H else []
        e = np.array(edges, np.int32)
        flip = rng.random(len(e)) < 0.5
        e[flip] = e[flip][:, ::-1]
        e = e[rng.permutation(len(e))]
        g = synth.assemble_graph(pos, g0["data_term"], e, weight=g0["data_weight"])
        g["beta"] = (0.5 + rng.random(len(e))).astype(F)
        assert g["V"] == 420 and g["E"] == 1179 and degrees(g).max() <= 6 and degrees(g).min() >= 2
        _BASE["L"] = g
    return synth.copy_graph(_BASE["L"])


BASES = {"G": base_graph, "L": local_graph}
ISOLATED = 200  # the vertex of with_an_isolated_vertex() that has lost its edges


def with_an_isolated_vertex(g):
    """g without the edges of vertex ISOLATED; the edge list keeps its order."""
    E = g["E"]
    keep = (g["src"] != ISOLATED) & (g["dst"] != ISOLATED)
    for k in ("src", "dst", "alpha", "beta") + Q_KEYS:
        g[k] = np.ascontiguousarray(g[k][keep])
    g["E"] = int(keep.sum())
    assert degrees(g)[ISOLATED] == 0 and 0 < g["E"] < E
    return g


def base_graph_with_an_isolated_vertex():
    return with_an_isolated_vertex(base_graph())


def scaled(g, factor, every=1):
    """The data term and the three copies of x times `factor` (a power of two: exact wherever the result is normal), at every
    `every`-th vertex."""
    for k in DATA_KEYS:
        g[k][::every] = (g[k][::every] * F(factor)).astype(F)
    return g


# ---- the value cases -------------------------------------------------------------------------------------------------------------
def subnormal_all(g=None):
    """Every datum subnormal (0.5 .. 1.5 times 2**-128): the whole state stays below 2**-126, no dual ever saturates."""
    return scaled(g if g is not None else base_graph(), 2.0 ** -128)


def subnormal_band(g=None):
    """Every third vertex scaled by 2**-126, the others left around 1: normal and subnormal operands meet in one sum, duals saturate."""
    return scaled(g if g is not None else base_graph(), 2.0 ** -126, every=3)


def subnormal_band_on_l(g):
    """L's band: every other COLUMN of the grid scaled by 2**-126.  Every third vertex, G's recipe, leaves 8 subnormal w1 after one step on
    L, under the floor of 10; by columns a scaled vertex keeps scaled neighbours above and below: 91 subnormal x, 18 w1, 141 q1, 823 duals
    at +-1 after one step."""
    column = (np.arange(g["V"]) % 21) % 2 == 0
    for k in DATA_KEYS:
        g[k][column] = (g[k][column] * F(2.0 ** -126)).astype(F)
    return g


def negative_zero_data(g=None):
    """-0.0 as datum and x at every fourth vertex, all w -0.0, the duals -0.0 and +0.0 in turn.  proxL1's `new_x = data` branch hands the
    -0.0 through both clamps with x_min = +0.0 (-0.0 < +0.0 is false): a clamp done with a hardware max would make it +0.0."""
    g = g if g is not None else base_graph()
    for k in DATA_KEYS:
        g[k][::4] = F(-0.0)
    for k in W_KEYS:
        g[k][:] = F(-0.0)
    for k in Q_KEYS:
        g[k][0::2] = F(-0.0)
        g[k][1::2] = F(0.0)
    return g


def negative_zero_duals(g=None):
    """A flat datum, all w and ALL duals -0.0: every K is a zero, and its sign decides.  The reference forms K from (source - target):
    x - x is +0.0 whichever zero x is, so every K is +0.0, every dual becomes +0.0 in the first step and every vertex with an edge gets
    w = +0.0 unless all it ever adds is t1 * dx with dx < 0.  A path that forms (target - source) and negates -- exact for every other
    value -- makes K -0.0 and keeps -0.0 duals and slopes where the reference has +0.0, for good: nothing here ever moves off zero."""
    g = g if g is not None else base_graph()
    for k in DATA_KEYS:
        g[k][:] = F(0.75)
    for k in W_KEYS + Q_KEYS:
        g[k][:] = F(-0.0)
    return g


HUB_DEGREES = (3, 8, 9, 12, 16, 17, 40)


def negative_zero_hub(d):
    """A hub that is the SOURCE of all its d edges, every neighbour to its upper right (dx < 0, dy < 0), a flat datum and all w -0.0:
    every contribution to the hub's w1 and w2 is a -0.0 (t1 * dx = +0.0 * negative, then - +0.0), so they stay -0.0 -- unless a lane
    that holds nothing adds a +0.0 for it.  3 and 8 edges: the common ordered sum; 9, 12, 16: the code for 9-16 edges; 17 and 40: the
    row-after-row sum of k_persistent_pv.  The other 60 + d vertices form a chain of alternating orientation, the edge list shuffled."""
    V = 61 + d
    rng = np.random.default_rng(1000 + d)
    pos = (1.0 + 60.0 * rng.random((V, 2))).astype(F)
    pos[0] = 0.0
    edges = [(0, i) for i in range(1, d + 1)] + [(i, i + 1) if i % 2 else (i + 1, i) for i in range(1, V - 1)]
    e = np.array(edges, np.int32)[rng.permutation(len(edges))]
    g = synth.assemble_graph(pos, np.full(V, 0.75, F), e)
    for k in W_KEYS:
        g[k][:] = F(-0.0)
    deg = degrees(g)
    assert deg[0] == d and np.all(g["src"][(g["src"] == 0) | (g["dst"] == 0)] == 0) and deg[1:].max() <= 3
    return g


# ---- the extremes of flame_nltgv2_params (the library validates none of them) -----------------------------------------------------------
INF = float("inf")
PARAM_SETS = {
    "theta=0": dict(theta=0.0),
    "theta=1": dict(theta=1.0),
    "x_min=x_max": dict(x_min=0.9, x_max=0.9),
    "x_min>x_max": dict(x_min=1.2, x_max=0.8),
    "data_factor=0": dict(data_factor=0.0),
    "step_x=0": dict(step_x=0.0),
    "step_q=0": dict(step_q=0.0),
    "unbounded": dict(x_min=-INF, x_max=INF),
    "x_min=-1": dict(x_min=-1.0, x_max=1.0),
}


def signed_graph(g=None):
    """G with its data lowered by 1.0: values of both signs."""
    g = g if g is not None else base_graph()
    for k in DATA_KEYS:
        g[k] = (g[k] - F(1.0)).astype(F)
    return g


# ---- non-finite inputs ----------------------------------------------------------------------------------------------------------------
def poisoned(**at):
    """with_an_isolated_vertex(g) with array[index] = value for every name = [(index, value), ...]."""
    def make(g=None):
        g = with_an_isolated_vertex(g if g is not None else base_graph())
        for name, items in at.items():
            for index, value in items:
                g[name][index] = F(value)
        return g
    return make


NAN = float("nan")
LAST = 419
# name -> (the input, the step count from which the checker reports a NaN: None = never)
NON_FINITE = {
    "overflow to inf, then inf / inf": (poisoned(x_bar=[(17, 3e38), (18, -3e38)]), 1),
    "x_bar[17] = inf": (poisoned(x_bar=[(17, INF)]), 1),
    "x_bar[0] = inf": (poisoned(x_bar=[(0, INF)]), 1),
    "x_bar[V - 1] = -inf": (poisoned(x_bar=[(LAST, -INF)]), 1),
    "x_bar[17] = NaN": (poisoned(x_bar=[(17, NAN)]), 1),
    # proxL1 takes `new_x = data` (every comparison with a NaN is false) and both clamps let it pass: x[17] and x_bar[17] are NaN after the
    # first step, no dual is; the second step's duals read x_bar[17]
    "data_term[17] = NaN": (poisoned(data_term=[(17, NAN)]), 2),
    "data_term[0] = NaN": (poisoned(data_term=[(0, NAN)]), 2),
    # step() overwrites both before anything reads them
    "x_prev[17] = NaN, w1_prev[5] = inf": (poisoned(x_prev=[(17, NAN)], w1_prev=[(5, INF)]), None),
    # a vertex without an edge: no dual reads it
    "x_bar[isolated] = inf": (poisoned(x_bar=[(ISOLATED, INF)]), None),
    "x_bar[isolated] = NaN": (poisoned(x_bar=[(ISOLATED, NAN)]), None),
    "data_term[isolated] = NaN": (poisoned(data_term=[(ISOLATED, NAN)]), None),
}


class Case:
    """name; make() -> a fresh graph dict; params: keyword arguments over the defaults; steps: the run lengths the GPU tests use; kind: which
    check_reaches applies; arg: what that check needs to know (the hub's degree, the parameter set, the first reporting step); local:
    the edges join neighbours (k_persistent_pv2 takes only such graphs, see local_graph)."""

    def __init__(self, name, make, kind, params=None, steps=STEPS, arg=None, local=True):
        self.name, self.make, self.kind, self.params, self.steps, self.arg = name, make, kind, dict(params or {}), tuple(steps), arg
        self.local = local
        self._graph = None

    def graph(self):
        """The case's input (built once; callers do not write to it)."""
        if self._graph is None:
            self._graph = self.make()
        return self._graph

    def max_degree(self):
        return int(degrees(self.graph()).max())

    def __repr__(self):
        return self.name


def _on(base, f):
    return lambda: f(BASES[base]())


def _on_bases(name, f, kind, **kw):
    """The case made from G and the same recipe on L."""
    return [Case(name if base == "G" else f"{name} on L", _on(base, f), kind, local=base == "L", **kw) for base in BASES]


VALUE_CASES = (_on_bases("subnormal_all", subnormal_all, "subnormal_all")
               + [Case("subnormal_band", _on("G", subnormal_band), "subnormal_band", local=False),
                  Case("subnormal_band on L", _on("L", subnormal_band_on_l), "subnormal_band")]
               + _on_bases("negative_zero_data", negative_zero_data, "negative_zero_data")
               + _on_bases("negative_zero_duals", negative_zero_duals, "negative_zero_duals")
               + [Case(f"negative_zero_hub({d})", (lambda d=d: negative_zero_hub(d)), "negative_zero_hub", arg=d) for d in HUB_DEGREES])
PARAM_CASES = [c for name, kw in PARAM_SETS.items() for gname, make in (("data around 1", lambda g: g), ("signed data", signed_graph))
               for c in _on_bases(f"params {name}, {gname}", make, "params_extremes", params=kw, steps=(7,), arg=(name, gname == "signed data"))]
NON_FINITE_CASES = [c for name, (make, first) in NON_FINITE.items() for c in _on_bases(f"non-finite: {name}", make, "non_finite", arg=first)]


def frame_subnormal_all():
    """The 320x240 frame (2120 vertices, 6342 edges, all eight XCDs: the values cross them through the record exchange), every datum
    subnormal.  Its edges are ~6 px where G's are ~50, so alpha is ten times G's and the duals grow ten times as fast: scaled by
    2**-128 as G is, only 30 % of q1 are still subnormal after 7 steps (G: 46 %, the floor 41 %).  2**-132 keeps the floors of G, scaled
    to this size: after 7 steps 2120 subnormal x, 2119 w1, 2120 w2, 6003 q1, 6333 q2, 6333 q3, no dual saturated."""
    return scaled(synth.make_graph("320x240", seed=11), 2.0 ** -132)


def frame_subnormal_band():
    """The same frame, the data scaled by 2**-126 in vertical stripes of 16 px (1066 of its vertices).  Every third vertex, G's recipe, leaves
    no subnormal x after one step here (every scaled vertex has unscaled neighbours, and with this alpha they pull it off its datum);
    inside a stripe the neighbours are scaled too, across its borders normal and subnormal operands meet.  After 1 step: 161 subnormal x,
    471 w1, 1138 q1, 2871 duals at +-1 (the floors of G at this size: 100, 50, 211, 2642)."""
    g = synth.make_graph("320x240", seed=11)
    stripe = (g["pos"][:, 0] // F(16)).astype(np.int64) % 2 == 0
    for k in DATA_KEYS:
        g[k][stripe] = (g[k][stripe] * F(2.0 ** -126)).astype(F)
    return g


FRAME_CASES = [Case("subnormal_all, 320x240", frame_subnormal_all, "subnormal_all", steps=(1, 7)),
               Case("subnormal_band, 320x240", frame_subnormal_band, "subnormal_band", steps=(1, 7))]
ALL_CASES = VALUE_CASES + PARAM_CASES + NON_FINITE_CASES + FRAME_CASES

_REFS = {}


def reference(case, n):
    """(state after n steps of the C checker, its NaN report): computed once per (case, n); callers do not write to it."""
    key = (case.name, n)
    if key not in _REFS:
        ref = synth.copy_graph(case.graph())
        bad = oracle.run(ref, n, oracle.make_params(**case.params))
        _REFS[key] = (ref, int(bad != 0))
    return _REFS[key]


def references(case):
    return {n: reference(case, n) for n in case.steps}


# ---- what each case must reach -------------------------------------------------------------------------------------------------
def _scale(floor, have, of):
    """A floor stated for G (`of` vertices or edges) for a graph that has `have`: the same share, rounded down."""
    return floor * have // of


def _reaches_subnormal_all(case, refs):
    # G after 7 steps: 420 subnormal x, 420 w1, 420 w2, 557 q1, 943 q2, 941 q3; no dual saturates
    ref, bad = refs[7]
    V, E = ref["V"], ref["E"]
    assert bad == 0
    for k in ("x", "w1", "w2"):
        assert n_subnormal(ref[k]) >= _scale(400, V, 420), (case, k, n_subnormal(ref[k]))
    assert n_subnormal(ref["q1"]) >= _scale(500, E, 1200), (case, n_subnormal(ref["q1"]))
    assert n_subnormal(ref["q2"]) >= _scale(900, E, 1200), (case, n_subnormal(ref["q2"]))
    assert n_saturated(ref) == 0, case
    assert n_subnormal(case.graph()["x_bar"]) == V, "the input itself: every x_bar subnormal"


def _reaches_subnormal_band(case, refs):
    # G after 1 step: 28 subnormal x, 13 w1, 60 q1, 749 duals at +-1; after 2 steps 880 at +-1
    ref, bad = refs[1]
    V, E = ref["V"], ref["E"]
    assert bad == 0
    assert n_subnormal(ref["x"]) >= _scale(20, V, 420), (case, n_subnormal(ref["x"]))
    assert n_subnormal(ref["w1"]) >= _scale(10, V, 420), (case, n_subnormal(ref["w1"]))
    assert n_subnormal(ref["q1"]) >= _scale(40, E, 1200), (case, n_subnormal(ref["q1"]))
    assert n_saturated(ref) >= _scale(500, E, 1200), (case, n_saturated(ref))
    assert all(b == 0 for _, b in refs.values())
    x_in = case.graph()["x_bar"]
    assert n_subnormal(x_in) >= V // 8 and int((np.abs(x_in) >= 0.01).sum()) >= V // 3, "normal and subnormal operands in one input"


def _reaches_negative_zero_data(case, refs):
    # G after 1, 2, 7 steps: 55, 54, 52 vertices with x == -0.0
    for n, (ref, bad) in refs.items():
        assert bad == 0
        assert n_bits(ref["x"], NEG_ZERO) >= 40, (case, n, n_bits(ref["x"], NEG_ZERO))
    g = case.graph()
    assert all(n_bits(g[k], NEG_ZERO) == g["V"] for k in W_KEYS)
    assert all(n_bits(g[k], NEG_ZERO) == (g["E"] + 1) // 2 and n_bits(g[k], POS_ZERO) == g["E"] // 2 for k in Q_KEYS)


def _reaches_negative_zero_duals(case, refs):
    g = case.graph()
    only_target = np.setdiff1d(g["dst"], g["src"])  # vertices that are the target of every edge they have: they add t2, t3 and nothing else
    assert only_target.size >= 10, (case, only_target.size)
    for n, (ref, bad) in refs.items():
        assert bad == 0
        assert np.all(ref["x"] == F(0.75))
        for k in Q_KEYS:  # every dual has become +0.0
            assert n_bits(ref[k], POS_ZERO) == g["E"], (case, n, k)
        for axis, k in enumerate(("w1", "w2")):
            # -0.0 is kept exactly where a vertex is the source of all its edges and every one of them points down that axis: all it adds
            # is t1 * d = +0.0 * negative = -0.0 and then - +0.0; one +0.0 from a target's role or a d > 0 makes the sum +0.0
            d = g["pos"][g["src"], axis] - g["pos"][g["dst"], axis]
            stays_negative = np.setdiff1d(np.setdiff1d(g["src"], g["dst"]), g["src"][d >= 0])
            want = np.full(g["V"], POS_ZERO, np.uint32)
            want[stays_negative] = NEG_ZERO
            assert np.array_equal(float_bits(ref[k]), want), (case, n, k)
            assert np.all(want[only_target] == POS_ZERO), (case, k)


def _reaches_negative_zero_hub(case, refs):
    # the other vertices with w == +0.0: 52 to 91 over the seven hubs
    assert degrees(case.graph())[0] == case.arg
    for n, (ref, bad) in refs.items():
        assert bad == 0
        for k in ("w1", "w2"):
            assert int(float_bits(ref[k])[0]) == NEG_ZERO, (case, n, k, hex(int(float_bits(ref[k])[0])))
            assert n_bits(ref[k][1:], POS_ZERO) >= 50, (case, n, k, n_bits(ref[k][1:], POS_ZERO))


def _reaches_params_extremes(case, refs):
    name, signed_data = case.arg
    ref, bad = refs[7]
    assert bad == 0 and n_nan(ref) == 0, case
    p = dict(oracle.DEFAULT_PARAMS, **case.params)
    if p["x_min"] > p["x_max"]:  # the second clamp wins
        assert np.all(ref["x"] == F(p["x_max"])) and np.all(ref["x_bar"] == F(p["x_max"])), case
    elif p["x_min"] == p["x_max"]:
        assert np.all(ref["x"] == F(p["x_min"])), case
    else:
        assert ref["x"].min() >= F(p["x_min"]) and ref["x"].max() <= F(p["x_max"]), case
    if signed_data:
        d = case.graph()["data_term"]
        assert (d < 0).sum() > 100 and (d > 0).sum() > 100
        if p["x_min"] < 0:
            assert (ref["x"] < 0).sum() > 100 and (ref["x"] > 0).sum() > 100, (case, int((ref["x"] < 0).sum()))
    if name == "step_q=0":
        assert all(np.all(ref[k] == 0) for k in Q_KEYS)
    if name == "step_x=0":  # the primal never moves, proxL1 snaps to the datum at once
        assert np.all(ref["w1"] == 0) and n_saturated(ref) > 0


def _reaches_non_finite(case, refs):
    first = case.arg
    for n, (ref, bad) in refs.items():
        assert bad == int(first is not None and n >= first), (case, n, bad)
    g = case.graph()  # the input holds a non-finite value, or one that overflows in the first product
    assert any((~np.isfinite(g[k])).any() for k in synth.STATE_KEYS + ("data_term",)) or np.abs(g["x_bar"]).max() >= F(1e38), case
    if "x_prev" in case.name:  # both overwritten before they are read
        assert n_nan(refs[7][0]) == 0 and all(np.isfinite(refs[7][0][k]).all() for k in synth.STATE_KEYS)
    if case.name.endswith("data_term[17] = NaN"):
        ref = refs[1][0]
        assert np.isnan(ref["x"][17]) and np.isnan(ref["x_bar"][17]) and n_nan(ref) == 2
    if "data_term[isolated]" in case.name:  # the NaN stays where it is: a state with a NaN that is compared in full
        ref = refs[7][0]
        assert np.isnan(ref["x"][ISOLATED]) and np.isnan(ref["x_bar"][ISOLATED]) and np.isnan(ref["x_prev"][ISOLATED]) and n_nan(ref) == 3


_REACHES = dict(subnormal_all=_reaches_subnormal_all, subnormal_band=_reaches_subnormal_band, negative_zero_data=_reaches_negative_zero_data,
                negative_zero_duals=_reaches_negative_zero_duals, negative_zero_hub=_reaches_negative_zero_hub,
                params_extremes=_reaches_params_extremes, non_finite=_reaches_non_finite)


def check_reaches(case, ref_by_steps):
    """Asserts, from the checker's output alone -- ref_by_steps: {steps: (state, NaN report)} for every step count of the case -- that
    the case still reaches what it is there for."""
    _REACHES[case.kind](case, ref_by_steps)
