"""k_update_feature_idepths (flame_amd/csrc/stereo_kernels.hip, update_one_feature) AROUND the epipolar walk: predict, the
rescale gate and the move to the newest pose-frame, search_region with its two clips, the padding and the cut, the valid
rectangle, the reference-patch gradient gate, the measurement model, the fusion with its outlier gate, fail_feature.
(The walk itself: tests/test_stereo_walk_edges.py.  Frame::create: tests/test_frame_planes_edges.py.)

CPU part
  coverage   the checker's stage columns (oracle/stereo_oracle.c, STAGE_*) show that tests/stereo_update_cases.py reaches
             every exit, both fail_feature bits alone and together, the forced variance factor on both paths and each
             SET edge (the `expect` of a case, counted per family: per path, per border) on both sides with
             COVERAGE_FLOOR features or more.  The set edges are those of the double constant 1e-6, the rectangle's
             rounding (own and moved position), idepth_var_max, max_dropouts, both rescale factors, min_baseline and
             min_grad_mag.  The measurement model's three `< 1e-3` gates are reached far from their threshold only
             (a zero disparity, a zero gradient, edn == 0): their exits are covered, their edges are not.
             Three classes cannot be reached through
             the driver and are CPU-only or absent:
               * the measurement model's `mu < 0` exit and `mu_post` clamped to +0: reached by calling stereo_meas_idepth and
                 stereo_fuse directly (test_direct_calls_reach_the_two_exits_the_driver_cannot);
               * "no region: second clip": after the first clip the segment lies in the box, the padding lengthens it
                 on its own line and the cut keeps its start, so the second clip always sees a point of the box.
  decisions  for every feature the stage the checker took equals the stage of the float64 restatement
             (tests/stereo_update_ref64.py), except where a float64 decision value lies within its float32 bound of its
             threshold (left out, at most LEFT_OUT_CAP of a family; every such feature counts, set on an edge or not).
             Features SET ON an edge are compared with the exact expectation written in the case; float64 is told the
             outcome of that one comparison (the case's `decide`) and takes every other decision itself, so that what
             lies behind the edge is compared like anything else.
  values     predict, the search segment, mu_meas / var_meas (do_meas_fusion = 0) and the fused pair (do_meas_fusion = 1)
             against float64, each within the running float32 bound that the R32 arithmetic of
             tests/stereo_update_ref64.py carries beside every value (its rules are in that module's docstring: one EPS
             per operation on the magnitudes involved, the conditioning -- 1 / h2, 1 / pc.z, 1 / ATA, 1 / edn^2, 1 / edg^2,
             the slope of a clipped segment -- through the division rule from the float64 values; nothing is taken from
             the checker or the kernel).  The matched position comes from the float64 walk (tests/stereo_ref64.walk64)
             with the position bound of tests/test_stereo_walk_edges._position_bound (_walk_for below).  Left out, and
             counted against LEFT_OUT_CAP of the family: every feature with a decision in doubt (none of its values is
             compared) and every feature with an infinite bound (float32 overflow, a divisor whose interval holds 0).
             A bound that is merely wide is compared.  THROUGH THE DRIVER the bounds of mu_meas, var_meas and the fused
             pair are wide (up to 4e-2 of the value: the match is known to a thousandth of a pixel): those comparisons
             are sanity checks.  What pins the arithmetic of the measurement model and the fusion is the repetition
             with the match, and then the measurement, GIVEN as exact float32 inputs to both sides.

GPU part (-m gpu): every family through the 16-lane row, one lane per feature and the resident set, and once more with the
matches records switched on (the kRecord instantiation), against the checker: records byte for byte, all seven counters,
status and error_feature of the assert case.

Observed on the CPU, largest over all families: |checker - float64| / bound (allowed: 1), and how large that bound was
relative to the value at the worst feature.
  through the driver       predict x 0.30 (6e-7), y 0.28 (2e-6), mu_pred 0.54 (2e-7), var_pred 0.46 (2e-6); segment 0.31 (5e-7);
                           moved x 0.22, y 0.21, mu 0.48, var 0.34 (all below 2e-6); variance after fail_feature 0.85 (6e-8);
                           (sanity only:) mu_meas 0.017 (1.5e-4), var_meas 0.008 (4e-2); fused mu 0.035 (5e-5), var 0.011 (3e-2)
  given exact inputs       mu_meas 0.12 (3e-6), var_meas 0.23 (4e-4); fused mu 0.67 (2e-7), fused var 0.85 (2e-7)
Left out of either check: 27 of 280 features at most, mostly features whose best step is not clear of its neighbour
or whose gradient is nearly perpendicular to the epipolar line (1 / edn^2); the 12 features of each mu-edge family whose
mu is subnormal have no bound for the predicted position (float32 overflows there).
Features per stage, per fail_feature bit and per set edge: printed by test_families_reach_every_exit_and_every_edge.
"""
import functools

import numpy as np
import pytest

from oracle import stereo_capi as so
from tests import stereo_ref64 as r64
from tests import stereo_update_cases as uc
from tests import stereo_update_ref64 as u64
from tests import stereo_walk_cases as wc
from tests.test_stereo_walk_edges import EPS, STAT_NAMES, _assert_gpu_equals_checker, _position_bound

gpu = pytest.mark.gpu
T = {n: i for i, n in enumerate(so.TRACE_COLS)}
S = so.STAGE
COVERAGE_FLOOR = 4          # the floor of tests/test_stereo_walk_edges.py
LEFT_OUT_CAP = 0.10
ALLOWED = 1.0               # times the running bound
UNREACHABLE = ("no region: second clip",)
CPU_ONLY = ("meas: mu < 0",)


def test_trace_columns_are_tied_together():
    assert so.lib().stereo_trace_cols() == len(so.TRACE_COLS) == 11
    assert so.TRACE_COLS[:8] == ("steps", "c_best", "c_second", "n_ties", "tie16", "second_eq_best", "subpixel", "match_rc")
    assert so.TRACE_COLS[8:] == ("stage", "fail_bits", "forced_one")
    assert len(so.STAGES) == 21 and S["updated, prior <= 0"] == 20


@functools.lru_cache(maxsize=None)
def _checked(k):
    case = uc.all_cases()[k]
    return wc.run_checker(case)


def _walk_for(case, img12):
    """The float64 walk as stage64's callback: the matched position with its bound.
    Position: the float32 walk starts at the float32 segment start (off by at most the start's bound es) and adds a step
    of length sample_dist whose direction is off by at most 2 (es + ee) / length (both ends move); c steps of it stay
    below the length, so a position is off by at most  pe = es + 2 (es + ee) + _position_bound(c)  per coordinate.
    Cost: each of a step's five residuals r_k is off by at most  dv = 2 lip pe + 8 EPS 255 + (the patch's bound):
    the image changes by `lip` per pixel at most in x and in y around the segment.  sum (r_k + d_k)^2 - sum r_k^2 <= 2 dv sum |r_k| +
    5 dv^2 <= 2 dv sqrt(5 cost) + 5 dv^2 (Cauchy-Schwarz), and five float32 additions add 25 EPS 255^2.
    The best step is taken where its cost plus its bound stays below every other cost minus that one's bound.  The
    loop's test compares a position with the segment's end in each coordinate: a step within 2 pe of the end in a
    coordinate that moves may or may not run in float32 (a padded or cut segment is a whole number of steps long, so
    its last step always is such a one); it is costed too, and the best step must be another one and clear of it.
    Elsewhere any step may be the best: the match is the middle of the segment, uncertain by half its extent."""
    pad, sd = case["pad"], float(case["pkw"].get("sample_dist", 1.0))
    coord_max = float(max(img12.shape))
    f12 = img12.astype(np.float64)

    def walk(patch, seg):
        es, ee = max(seg[0].e, seg[1].e), max(seg[2].e, seg[3].e)
        s = np.array([v.v for v in seg]) + pad
        ref = r64.walk64(np.array([p.v for p in patch], np.float32), img12, s[:2], s[2:], sd)
        if ref is None:
            return None
        costs, c = ref["costs"], ref["c_best"]
        n = costs.size
        pe = es + 2 * (es + ee) + _position_bound(n + 3, coord_max, sd)
        x0, x1 = sorted((s[0], s[2]))
        y0, y1 = sorted((s[1], s[3]))
        box = f12[max(int(y0) - 3, 0):int(y1) + 5, max(int(x0) - 3, 0):int(x1) + 5]     # the walk's samples: two steps beyond
        lip = max(np.abs(np.diff(box, axis=0)).max(), np.abs(np.diff(box, axis=1)).max())
        dv = 2 * lip * pe + 255 * 8 * EPS + max(p.e for p in patch) + 255 * EPS
        inc = ref["inc"]
        moving = [k for k in range(2) if abs(inc[k]) * n > 2 * pe]
        fickle = any(inc[k] != 0.0 and k not in moving for k in range(2))    # a coordinate whose test rounding decides

        def near_end(t):
            return any(abs(s[k] + t * inc[k] - s[2 + k]) <= 2 * pe for k in moving)

        t_d = None                                 # the step that may or may not run
        if near_end(n - 1):
            t_d = n - 1
        elif near_end(n):
            ext = r64.walk64(np.array([p.v for p in patch], np.float32), img12, s[:2], s[:2] + (n + 0.5) * inc, sd)
            if ext is None or ext["costs"].size != n + 1:
                fickle = True
            else:
                t_d, costs = n, ext["costs"]
                c = int(np.argmin(costs))
        b = 2 * dv * np.sqrt(5 * costs) + 5 * dv * dv + 25 * EPS * 255.0 ** 2
        others = np.delete(costs - b, c)
        if not fickle and c != t_d and not (others.size and others.min() <= costs[c] + b[c]):
            e = es + 2 * (es + ee) + _position_bound(c, coord_max, sd)
            return u64.R32(s[0] + c * inc[0] - pad, e), u64.R32(s[1] + c * inc[1] - pad, e)
        half = 0.5 * np.abs(s[2:] - s[:2]) + sd + pe
        mid = 0.5 * (s[:2] + s[2:]) - pad
        return u64.R32(mid[0], half[0]), u64.R32(mid[1], half[1])

    return walk


@functools.lru_cache(maxsize=None)
def _float64(k):
    """stage64 of every feature of family k."""
    case = uc.all_cases()[k]
    sc, pad = case["sc"], case["pad"]
    P = so.Params(**case["pkw"])
    geos = {p["id"]: (u64.Geo64(so.load_geometry(sc.K32, sc.Kinv32, p["q_to_new"], p["t_to_new"])),
                      u64.Geo64(so.load_geometry(sc.K32, sc.Kinv32, p["q_to_pf"], p["t_to_pf"]))) for p in case["poses"]}
    ref_pads = {a: so.make_frame(case["imgs"][a], pad)[0] for a in (10, 11)}
    img12, gx12, gy12 = so.make_frame(case["imgs"][12], pad)
    walk = _walk_for(case, img12) if case["walk"] else None
    out = []
    for i, f in enumerate(case["feats"]):
        a = int(f["frame_id"])
        out.append(u64.stage64(P, S, geos[a][0], geos[a][1], sc.width, sc.height, pad, ref_pads[a], gx12, gy12, f, walk,
                               decide=case["decide"].get(i)))
    return out


def _edge_features(case):
    return set().union(*[set(v) for v in case["expect"].values()]) if case["expect"] else set()


N_CASES = len(uc.all_cases())


# ---- coverage --------------------------------------------------------------------------------------------------------------

def test_families_reach_every_exit_and_every_edge():
    stage_count = np.zeros(len(so.STAGES), np.int64)
    fail_count, forced_count = np.zeros(4, np.int64), np.zeros(4, np.int64)
    edge_count = {}
    outlier_prior = {"prior > 0": 0, "prior = 0": 0}
    region = {k: 0 for k in ("left", "right", "top", "bottom", "padded", "padded and clipped again", "cut")}
    for k, case in enumerate(uc.all_cases()):
        if "assert_at" in case:
            continue
        rc, _, _, tr = _checked(k)
        assert rc == 0, (case["name"], rc)
        st = tr[:, T["stage"]]
        assert (st >= 0).all(), case["name"]
        stage_count += np.bincount(st, minlength=len(so.STAGES))
        fail_count += np.bincount(tr[:, T["fail_bits"]], minlength=4)
        forced_count += np.bincount(tr[:, T["forced_one"]], minlength=4)
        is_out = st == S["outlier"]
        outlier_prior["prior > 0"] += int((is_out & (case["feats"]["idepth_mu"] > 0)).sum())
        outlier_prior["prior = 0"] += int((is_out & (case["feats"]["idepth_mu"] == 0)).sum())
        for kind, d in case["expect"].items():
            for i, v in d.items():
                key = (case["name"], kind, v)
                edge_count[key] = edge_count.get(key, 0) + 1
        if case["name"].startswith("clipped segments"):
            for r in _float64(k):
                sr = r.get("region")
                if sr and sr["exit"] is None and not r["doubt"]:
                    for side in sr["sides"]:
                        region[side] += 1
                    region["padded"] += sr["padded"]
                    region["padded and clipped again"] += bool(sr["padded"] and sr["sides2"])
                    region["cut"] += sr["cut"]
    print("\nfeatures per stage (checker's trace):")
    for name, n in zip(so.STAGES, stage_count):
        print("  %-42s %d" % (name, n))
    print("fail_feature bits 0..3:", fail_count.tolist(), " forced_one 0..3:", forced_count.tolist())
    print("search regions of the clip families (float64):", region, " outliers:", outlier_prior)
    print("edge features per (family, kind, expectation):")
    for key, n in sorted(edge_count.items(), key=str):
        print("  %-60s %d" % (key, n))
    short = {n: int(c) for n, c in zip(so.STAGES, stage_count) if c < COVERAGE_FLOOR and n not in UNREACHABLE + CPU_ONLY}
    assert not short, short
    assert all(stage_count[S[n]] == 0 for n in UNREACHABLE + CPU_ONLY)
    assert (fail_count[1:] >= COVERAGE_FLOOR).all(), fail_count           # variance alone, dropouts alone, both
    # forced by predict alone (the new-frame path), on the move path too (3), and left alone on either path (0)
    assert min(forced_count[0], forced_count[1], forced_count[3]) >= COVERAGE_FLOOR, forced_count
    assert min(outlier_prior.values()) >= COVERAGE_FLOOR, outlier_prior
    assert min(region.values()) >= COVERAGE_FLOOR, region
    assert min(edge_count.values()) >= COVERAGE_FLOOR, edge_count


def test_direct_calls_reach_the_two_exits_the_driver_cannot():
    """`mu < 0` of the measurement model needs a match beyond the epipole, which no search segment reaches; `mu_post`
    clamped to 0 needs a measurement <= 0, which that exit has already removed."""
    sc = uc._scene((0.1, 0.0, 0.5))
    g = so.load_geometry(sc.K32, sc.Kinv32, *sc.relative(10, 12))
    g64 = u64.Geo64(g)
    _, gx, gy = so.make_frame(sc.render(12), uc.PAD)
    P = so.Params()
    ex = float(g.epx)
    assert 100.0 < ex < 110.0
    for x in (100.0, 96.5, 90.25, 85.0):
        for beyond in (3.0, 12.0):
            rc, mu, var = so.meas_idepth(P, g, gx, gy, x, 60.0, ex + beyond, 60.0)
            assert rc == 0 and mu.tobytes() == np.float32(0.0).tobytes() and var == np.float32(1e10)
            D = u64.Doubt()
            assert u64.meas64(P, g64, gx, gy, x, 60.0, ex + beyond, 60.0, D)["exit"] == u64.MEAS_EXITS.index("mu < 0") and not D
        rc, mu, _ = so.meas_idepth(P, g, gx, gy, x, 60.0, x + 2.0, 60.0)       # before the epipole: a measurement
        assert rc == 1 and mu > 0
    zero = np.float32(0.0).tobytes()
    for mu_pred, var_pred, mu_meas, var_meas in ((0.0, 0.02, -0.0, 0.01), (0.1, 1.0, -0.5, 0.01), (0.0, 1.0, -0.25, 0.01),
                                                 (0.05, 0.5, -0.1, 1e-3)):
        ok, mu, var = so.fuse(mu_pred, var_pred, np.float32(mu_meas), var_meas, 3.0)
        assert ok and mu.tobytes() == zero, (mu_pred, mu_meas, mu)
        D = u64.Doubt()
        fu = u64.fuse64(mu_pred, var_pred, u64.R32(mu_meas), u64.R32(var_meas), 3.0, D)
        assert not fu["outlier"] and (fu["mu"].v == 0.0 or D)
    ok, mu, _ = so.fuse(np.float32("nan"), 1.0, np.float32(-0.0), 0.01, 3.0)   # a NaN prior: dist is NaN, no outlier
    assert ok and mu.tobytes() == zero


# ---- decisions ---------------------------------------------------------------------------------------------------------------

def _stage_name(code):
    return "assert" if code < 0 else so.STAGES[code]


def _check_expectations(case, tr):
    st, fail, forced = tr[:, T["stage"]], tr[:, T["fail_bits"]], tr[:, T["forced_one"]]
    name = case["name"]
    for kind, d in case["expect"].items():
        for i, want in d.items():
            got = _stage_name(st[i])
            what = (name, kind, i, want, got, case["feats"][i])
            if kind == "forced":
                assert forced[i] == want, what + (forced[i],)
            elif kind == "fail":
                assert fail[i] == want, what + (fail[i],)
            elif kind == "stage":
                assert got == want, what
            elif kind == "outside":
                assert (st[i] == S["outside the valid rectangle"]) == want and st[i] >= S["outside the valid rectangle"], what
            elif kind == "moved":
                assert (st[i] in (S["moved"], S["move failed: predict"], S["move failed: rectangle"])) == want, what
                assert want or st[i] >= S["no region: empty idepth window"], what
            elif kind == "skipped":
                assert (st[i] == S["baseline skip"]) == want, what
            elif kind == "no_grad":
                assert (st[i] == S["search status 1"]) == want and st[i] >= S["search status 1"], what
            else:
                raise KeyError(kind)


@pytest.mark.parametrize("k", range(N_CASES), ids=lambda k: uc.all_cases()[k]["name"])
def test_decisions_match_float64(k):
    case = uc.all_cases()[k]
    rc, stats, out, tr = _checked(k)
    feats = case["feats"]
    n = feats.shape[0]
    if "assert_at" in case:
        assert rc == -(1 + case["assert_at"])
        refs = _float64(k)
        # (float64 sees pc.z = 0 +- one roundoff of 1 / mu, which float32 computes exactly: the case states the expectation)
        assert refs[case["assert_at"]]["stage"] == -1 or "pc.z against 0" in refs[case["assert_at"]]["doubt"]
        assert all(r["stage"] >= 0 or r["doubt"] for r in refs[:case["assert_at"]])
        return
    assert rc == 0
    _check_expectations(case, tr)
    assert set(case["decide"]) <= _edge_features(case)          # float64 is told a decision only where the case expects one
    left_out, compared = 0, 0
    for i, r in enumerate(_float64(k)):
        if r["doubt"]:
            left_out += 1
            continue
        got, want = int(tr[i, T["stage"]]), r["stage"]
        what = (case["name"], i, _stage_name(got), want if want == u64.REACHED_THE_WALK else _stage_name(want), feats[i])
        if want == u64.REACHED_THE_WALK:
            assert got >= S["search status 2"], what         # the walk's own outcome: tests/test_stereo_walk_edges.py
        else:
            assert got == want, what
            assert int(tr[i, T["fail_bits"]]) == r["fail"], what + (tr[i, T["fail_bits"]], r["fail"])
        assert int(tr[i, T["forced_one"]]) == r["forced"], what + (tr[i, T["forced_one"]], r["forced"])
        compared += 1
    print("\n%s: %d features, %d compared with float64, %d left out, %d on set edges"
          % (case["name"], n, compared, left_out, len(_edge_features(case))))
    assert left_out <= LEFT_OUT_CAP * n, (case["name"], left_out, n)
    # what the stage says must be what the record shows
    st = tr[:, T["stage"]]
    upd = (st == S["updated, prior > 0"]) | (st == S["updated, prior <= 0"])
    assert stats[0] == upd.sum() and np.array_equal(out["num_updates"] - feats["num_updates"], upd.astype(np.uint32))
    assert stats[1] == (tr[:, T["fail_bits"]] & 1).sum() and stats[2] == (tr[:, T["fail_bits"]] >> 1).sum()
    skipped = st == S["baseline skip"]
    assert out[skipped].tobytes() == feats[skipped].tobytes()
    for code, name in ((1, "search status 1"), (2, "search status 2"), (3, "search status 3")):
        assert (out["search_status"][st == S[name]] == code).all()


# ---- values ---------------------------------------------------------------------------------------------------------------------

def _ratio(got, ref):
    """|float32 result - float64 value| / running bound; None when there is no finite bound (left out).  A feature whose
    bound passes 1e-3 of the value is NOT left out: a wide bound makes the comparison weaker, not wrong.  Through the
    driver the bounds of the measurement are wide (the match is known to 1e-3 pixel only); the direct calls repeat the
    comparison with the match as an exact input, where they are narrow."""
    got = float(got)
    if not np.isfinite(ref.e) or not np.isfinite(ref.v):
        return None
    d = abs(got - ref.v)
    return 0.0 if d == 0.0 else d / ref.e if ref.e > 0.0 else np.inf


@pytest.mark.parametrize("k", [k for k in range(N_CASES) if "assert_at" not in uc.all_cases()[k]],
                         ids=lambda k: uc.all_cases()[k]["name"])
def test_values_match_float64(k):
    case = uc.all_cases()[k]
    rc, _, out, tr = _checked(k)
    sc, feats = case["sc"], case["feats"]
    P = so.Params(**case["pkw"])
    geos = {p["id"]: so.load_geometry(sc.K32, sc.Kinv32, p["q_to_new"], p["t_to_new"]) for p in case["poses"]}
    n = feats.shape[0]
    worst, left_out, checked = {}, {}, {}

    g64s = {a: u64.Geo64(g) for a, g in geos.items()}
    _, gx12, gy12 = so.make_frame(case["imgs"][12], case["pad"])

    def cmp(what, i, got, ref):
        r = _ratio(got, ref)
        if r is None:
            left_out.setdefault(what, set()).add(i)
            return
        checked[what] = checked.get(what, 0) + 1
        if r > worst.get(what, (0.0,))[0]:
            worst[what] = (r, i, float(got), ref)

    in_doubt = set()
    for i, r in enumerate(_float64(k)):
        f = feats[i]
        if r["doubt"]:
            in_doubt.add(i)         # counted against the cap below
            continue
        if r["stage"] in (-1, S["baseline skip"]):
            continue                # nothing was computed for the feature
        g = geos[int(f["frame_id"])]
        pr = r["predict"]
        prc, x, y, mu_pred, var_pred = so.predict(g, P.process_var_factor, f["x"], f["y"], f["idepth_mu"], f["idepth_var"])
        assert prc == (1 if pr["decision"] == "no" else 0)
        for key, got in (("x", x), ("y", y), ("mu_pred", mu_pred), ("var_pred", var_pred)):
            cmp("predict " + key, i, got, pr[key])
        sr = r.get("region")
        if sr and sr["exit"] is None:
            got = so.search_region(P, g, sc.width, sc.height, f["x"], f["y"], f["idepth_mu"], f["idepth_var"])
            assert got[0] == 1
            for j in range(4):
                cmp("segment", i, got[1 + j], sr["seg"][j])
        if r.get("meas") and r["meas"]["exit"] is None and r["match"][0].e < 1.0:
            # the two routines alone, on exact inputs: the float64 match rounded to float32, the float64 measurement rounded
            cx, cy = np.float32(r["match"][0].v), np.float32(r["match"][1].v)
            D = u64.Doubt()
            ms = u64.meas64(P, g64s[int(f["frame_id"])], gx12, gy12, float(f["x"]), float(f["y"]), u64.R32(cx), u64.R32(cy), D)
            mrc, mu32, var32 = so.meas_idepth(P, g, gx12, gy12, f["x"], f["y"], cx, cy)
            if not D and ms["exit"] is None:
                assert mrc == 1, (case["name"], i, mrc)
                cmp("meas mu, given the match", i, mu32, ms["mu"])
                cmp("meas var, given the match", i, var32, ms["var"])
                D = u64.Doubt()
                fu = u64.fuse64(f["idepth_mu"], f["idepth_var"], u64.R32(mu32), u64.R32(var32), float(P.outlier_sigma_thresh), D)
                ok, mu_post, var_post = so.fuse(f["idepth_mu"], f["idepth_var"], mu32, var32, P.outlier_sigma_thresh)
                if not D:
                    assert ok == (not fu["outlier"]), (case["name"], i, ok, fu)
                    if ok:
                        cmp("fusion, given the measurement", i, mu_post, fu["mu"])
                        cmp("fusion var, given the measurement", i, var_post, fu["var"])
        if r["stage"] in (S["updated, prior > 0"], S["updated, prior <= 0"]):
            ref = r["fuse"] if P.do_meas_fusion else r["meas"]
            tag = "fused" if P.do_meas_fusion else "meas"
            cmp(tag + " mu", i, out["idepth_mu"][i], ref["mu"])
            cmp(tag + " var", i, out["idepth_var"][i], ref["var"])
        elif r["stage"] != u64.REACHED_THE_WALK and r["stage"] != S["moved"]:
            cmp("failed var", i, out["idepth_var"][i], r["fail_var"])
        elif r["stage"] == S["moved"]:
            cmp("moved x", i, out["x"][i], r["move"]["x"])
            cmp("moved y", i, out["y"][i], r["move"]["y"])
            cmp("moved mu", i, out["idepth_mu"][i], r["move"]["mu_pred"])
            cmp("moved var", i, out["idepth_var"][i], r["fail_var"])
    print("\n%s: deviation / running bound (allowed %.1f)" % (case["name"], ALLOWED))
    for what in sorted(set(worst) | set(checked)):
        w = worst.get(what, (0.0, -1, 0.0, None))
        print("  %-34s %5d checked, %3d left out, worst %.3f (feature %d: %r against %r)"
              % (what, checked.get(what, 0), len(left_out.get(what, ())), w[0], w[1], w[2], w[3]))
    for what, w in worst.items():
        assert w[0] <= ALLOWED, (case["name"], what, w)
    all_left = in_doubt.union(*left_out.values())
    print("  left out: %d in doubt, %d in all, of %d" % (len(in_doubt), len(all_left), n))
    assert len(all_left) <= LEFT_OUT_CAP * n, (case["name"], len(in_doubt), {k2: len(v) for k2, v in left_out.items()}, n)


# ---- GPU: every family through every way in, with and without the matches records ---------------------------------------------

@gpu
@pytest.mark.parametrize("k", range(N_CASES), ids=lambda k: uc.all_cases()[k]["name"])
def test_gpu_family_matches_checker(built, k):
    case = uc.all_cases()[k]
    rc = _assert_gpu_equals_checker(case, expect_assert=case.get("assert_at"))
    assert (rc < 0) == ("assert_at" in case)


@gpu
@pytest.mark.parametrize("k", range(N_CASES), ids=lambda k: uc.all_cases()[k]["name"])
def test_gpu_family_matches_checker_with_match_records(built, k):
    """The same through the kRecord instantiation of the kernel: the records it writes for the matches picture change
    nothing in the features, the counters or the error report."""
    from flame_amd.stereo import FEATURE_DTYPE, FeatureTracker, StereoParams

    case = uc.all_cases()[k]
    sc, feats = case["sc"], case["feats"]
    rc_o, st_o, out_o, _ = _checked(k)
    with FeatureTracker(sc.K32, sc.Kinv32, sc.width, sc.height, border=case["pad"]) as tr:
        for fid, img in case["imgs"].items():
            tr.add_frame(fid, img)
        tr.set_record_matches(True)
        for lanes in (16, 1):
            tr.set_lanes_per_feature(lanes)
            out = feats.copy().view(FEATURE_DTYPE)
            rc, st = tr.update_feature_idepths(StereoParams(**case["pkw"]), 12, 11, case["poses"], out, raise_on_error=False)
            what = (case["name"], lanes, rc, st)
            if rc_o < 0:
                assert rc == -8 and st["error_feature"] == -rc_o - 1 == case["assert_at"], what
                continue
            assert rc == 0 and st["error_feature"] == -1, what
            assert [st[n] for n in STAT_NAMES] == [int(v) for v in st_o], what + (st_o,)
            assert out.tobytes() == out_o.tobytes(), what
        if rc_o == 0:
            tr.set_lanes_per_feature(16)
            tr.set_features(feats.copy().view(FEATURE_DTYPE))
            rc, st = tr.update_resident(StereoParams(**case["pkw"]), 12, 11, case["poses"], raise_on_error=False)
            assert rc == 0 and [st[n] for n in STAT_NAMES] == [int(v) for v in st_o], (case["name"], "resident", rc, st, st_o)
            assert tr.get_features().tobytes() == out_o.tobytes(), (case["name"], "resident")
