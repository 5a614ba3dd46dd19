"""The epipolar walk of k_update_feature_idepths at the places where its 16-lane form (line_match_row,
flame_amd/csrc/stereo_kernels.hip) can disagree with the sequential loop: cost ties, best steps at the ends of a walk
and at round joins, walks of one to seven rounds, rows of one wave that leave the loop rounds apart, clipped segments,
small images, partly filled waves, reference asserts raised from inside the walk.

CPU part: (1) the claim the kernel's comment makes about the best / second-best bookkeeping, on two Python models;
(2) the checker's walk trace shows that tests/stereo_walk_cases.py reaches every class; (3) the checker's walk against an
independent float64 restatement (tests/stereo_ref64.py).
GPU part (-m gpu): the HIP path -- 16-lane row, one lane per feature, resident set -- against the checker, bit for bit.
"""
import functools
import itertools

import numpy as np
import pytest

from oracle import stereo_capi as so
from tests import stereo_ref64 as r64
from tests import stereo_walk_cases as wc
from tests.test_stereo import _gpu_update, _scene_case

gpu = pytest.mark.gpu
T = {n: i for i, n in enumerate(so.TRACE_COLS)}

# ---- (1) best / second-best bookkeeping: sequential update == per-lane pairs + two lexicographic reductions ----------------

FMAX, IMAX = 3.402823466e+38, 0x7fffffff


def _model_sequential(costs):
    """line_stereo.h's update, as oracle/stereo_oracle.c restates it: (best, c_best, second, c_second)."""
    best = second = FMAX
    c_best = c_second = -1
    for t, ee in enumerate(costs):
        if ee < best:
            second, c_second = best, c_best
            best, c_best = ee, t
        elif ee < second:
            second, c_second = ee, t
    return best, c_best, second, c_second


def _row_min_pair(v, i):
    """row_min_pair of the kernel: four row_ror butterfly steps, every lane ends with the (value, index) minimum."""
    v, i = list(v), list(i)
    for n in (8, 4, 2, 1):
        ov = [v[(k - n) % 16] for k in range(16)]   # row_ror:n -- lane k reads lane k - n
        oi = [i[(k - n) % 16] for k in range(16)]
        for k in range(16):
            if ov[k] < v[k] or (ov[k] == v[k] and oi[k] < i[k]):
                v[k], i[k] = ov[k], oi[k]
    assert len(set(zip(v, i))) == 1, "the butterfly must leave the same pair in every lane"
    return v[0], i[0]


def _model_lanes(costs):
    """line_match_row: lane t mod 16 keeps the two smallest (cost, step) pairs of its own steps, then two reductions."""
    lb, ls = [FMAX] * 16, [FMAX] * 16
    lb_i, ls_i = [IMAX] * 16, [IMAX] * 16
    for t, ee in enumerate(costs):
        k = t % 16
        if ee < lb[k]:
            ls[k], ls_i[k] = lb[k], lb_i[k]
            lb[k], lb_i[k] = ee, t
        elif ee < ls[k]:
            ls[k], ls_i[k] = ee, t
    best, c_best = _row_min_pair(lb, lb_i)
    win = [lb_i[k] == c_best for k in range(16)]
    second, c_second = _row_min_pair([ls[k] if win[k] else lb[k] for k in range(16)],
                                     [ls_i[k] if win[k] else lb_i[k] for k in range(16)])
    return best, c_best, second, (-1 if c_second == IMAX else c_second)


def test_bookkeeping_models_agree_exhaustive_short():
    n = 0
    for length in range(1, 11):
        for seq in itertools.product((1.0, 2.0, 3.0), repeat=length):
            assert _model_lanes(seq) == _model_sequential(seq), seq
            n += 1
    assert n == sum(3 ** k for k in range(1, 11))


def test_bookkeeping_models_agree_random_long():
    rng = np.random.default_rng(16)
    seen_same_lane_tie = 0
    for trial in range(6000):
        length = 1 + trial % 70
        alphabet = (3, 4)[trial & 1]
        seq = [float(c) for c in rng.integers(0, alphabet, length)]
        if trial % 7 == 0:                                  # mostly-high sequences: few, far-apart minima
            seq = [c + 5.0 * (rng.random() < 0.9) for c in seq]
        a, b = _model_lanes(seq), _model_sequential(seq)
        assert a == b, (seq, a, b)
        m = [t for t, c in enumerate(seq) if c == b[0]]
        seen_same_lane_tie += any((t - m[0]) % 16 == 0 for t in m[1:])
    assert seen_same_lane_tie > 100   # ties that meet inside one lane were among them


# ---- (2) coverage: what the checker's trace counts over the case families ----------------------------------------------

COVERAGE_FLOOR = 4


def _classify(tr, out, feats):
    """Per-class feature counts of one case from the checker's trace (rows of -1: match not reached)."""
    reached = tr[:, T["steps"]] >= 0
    r = tr[reached]
    s, cb, cs, nt, t16, se, sp, rc = (r[:, k] for k in range(8))
    walked = s > 0     # (steps == 0: the first four samples already left the image -- a reference assert)
    d = {"walk <= 2 steps": (walked & (s <= 2)).sum()}
    for k in (15, 16, 17, 31, 32, 33):
        d["walk of %d steps" % k] = (s == k).sum()
    d["walk >= 49 steps"] = (s >= 49).sum()
    d["best at step 0"] = (walked & (cb == 0)).sum()
    d["best at last step"] = (walked & (cb == s - 1)).sum()
    d["best at step 15"] = (cb == 15).sum()
    d["best at step 16"] = (cb == 16).sum()
    d["best at step 31 or 32"] = ((cb == 31) | (cb == 32)).sum()
    # a tie makes second_err == best_err, and c_second is then the FIRST tied step behind the best
    d["tie at distance 1"] = ((se == 1) & (cs - cb == 1)).sum()
    d["tie at distance > 1"] = ((nt > 0) & ((cs - cb > 1) | (nt > 1))).sum()
    d["tie at a multiple of 16"] = (t16 == 1).sum()
    d["second == best"] = (se == 1).sum()
    for k, name in enumerate(("none", "pre", "post")):
        d["sub-pixel %s" % name] = ((rc == 0) & (sp == k)).sum()
    moved = out["search_status"] != feats["search_status"]
    for k in range(4):
        d["search status %d" % k] = ((out["search_status"] == k) & (reached if k != 1 else moved)).sum()
    g = np.where(reached, tr[:, T["steps"]], -1)
    g = g[:g.size // 4 * 4].reshape(-1, 4)
    lo = np.where(g >= 0, g, 1 << 30).min(axis=1)
    d["4-group with walks >= 32 steps apart"] = ((g.max(axis=1) - lo >= 32) & (lo < (1 << 30))).sum()
    return {k: int(v) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _coverage():
    total = {}
    n_cases = 0
    cases = itertools.chain(*(wc.grid_cases(sd) for sd in wc.SAMPLE_DISTS), [wc.short_walk_case()])
    for case in cases:
        rc, _, out, tr = wc.run_checker(case)
        assert rc == 0, (case["name"], rc)
        for k, v in _classify(tr, out, case["feats"]).items():
            total[k] = total.get(k, 0) + v
        n_cases += 1
    return n_cases, total


def test_case_families_reach_every_class():
    n_cases, total = _coverage()
    print("\n%d cases; features per class (checker's trace):" % n_cases)
    for k, v in total.items():
        print("  %-40s %d" % (k, v))
    short = {k: v for k, v in total.items() if v < COVERAGE_FLOOR}
    assert not short, short


def test_single_case_reaches_the_tie_classes():
    """The case the feature-count sweep is cut from has ties of every kind among its first 257 features."""
    case = wc.tied_case()
    rc, _, out, tr = wc.run_checker(case)
    assert rc == 0
    d = _classify(tr[:256], out[:256], case["feats"][:256])
    print("\nfirst 256 features of the tied case:", d)
    for k in ("tie at distance > 1", "tie at a multiple of 16", "second == best", "best at step 0", "best at last step",
              "walk >= 49 steps", "4-group with walks >= 32 steps apart"):
        assert d[k] >= COVERAGE_FLOOR, (k, d[k])


def test_trace_leaves_the_outputs_alone():
    case = wc.make_case("checker8", "+x-y", **wc.walk_params(0.5))
    rc_a, st_a, out_a, _ = wc.run_checker(case, trace=True)
    rc_b, st_b, out_b, _ = wc.run_checker(case, trace=False)
    assert rc_a == rc_b and np.array_equal(st_a, st_b) and out_a.tobytes() == out_b.tobytes()


# ---- (3) the checker's walk against float64 ---------------------------------------------------------------------------

EPS = 2.0 ** -24     # float32 unit roundoff


def _position_bound(t, coord_max, sample_dist):
    """How far the checker's float32 position after t additions, cp_t = fl(cp_{t-1} + inc), may lie from the exact
    start + t * inc, per coordinate.
      * every addition rounds to nearest: at most half an ulp of the result, and every coordinate stays below
        coord_max, so at most ulp(coord_max) / 2 = coord_max' * EPS with coord_max' the power of two above coord_max;
      * inc itself is rounded: d = fl(e - s) [EPS], d*d [EPS each], their sum [EPS], sqrt [halves the 4 EPS so far, adds
        EPS: 3 EPS], sample_dist / epl [4 EPS], d * that [EPS + 4 EPS + EPS = 6 EPS]; 7 EPS covers the second-order
        terms.  |inc| <= sample_dist per coordinate, so each of the t additions carries at most 7 EPS * sample_dist
        of that.
    Nothing here is measured on the code under test."""
    pow2 = 2.0 ** np.ceil(np.log2(coord_max))
    return t * (pow2 * EPS + 7 * EPS * sample_dist)


def _cost_bound(n_steps, coord_max, sample_dist, lipschitz):
    """How far a float32 cost may lie from its float64 value: the five sample positions of step t are off by at most
    _position_bound(t + 3) per coordinate (t additions, the lead's `+ 2 * inc`, one for the four start samples'
    own `- 2 * inc`); bilinear interpolation moves by at most `lipschitz` (the largest difference of neighbouring
    pixels) per pixel in x and in y; its own float32 arithmetic (8 operations on values <= 255) adds 255 * 8 EPS.
    A residual e <= 255 off by dv changes e^2 by at most 2 * 255 * dv + dv^2; five of them, and five float32
    additions of a sum <= 5 * 255^2 add 5 EPS * 5 * 255^2."""
    dv = 2 * lipschitz * _position_bound(n_steps + 3, coord_max, sample_dist) + 255 * 8 * EPS
    return 5 * (2 * 255 * dv + dv * dv) + 25 * EPS * 255.0 ** 2


def test_checker_walk_matches_float64():
    """On the random-texture scene, for every feature whose float64 best cost is clear of ALL other costs by twice the
    float32 cost bound (clear of the non-adjacent ones would do for the position; the adjacent ones are included because
    c_best can only be required equal where they are clear too) and is not the walk's last step (whether the last
    step runs is itself a rounded comparison): c_best equal, matched position within _position_bound(c_best)."""
    sc, imgs, feats, poses = _scene_case()
    pad, sd = 5, 1.0
    pkw = dict(do_subpixel=0, second_best_factor=1.0, max_cost=1e9, sample_dist=sd)   # every walk returns its best step
    P = so.Params(**pkw)
    case = dict(sc=sc, imgs=imgs, feats=feats, poses=poses, pkw=pkw, pad=pad)
    rc, _, _, tr = wc.run_checker(case)
    assert rc == 0
    _, seg = wc.search_segments(case)
    img12 = so.make_frame(imgs[12], pad)[0]
    ref_pads = {a: so.make_frame(imgs[a], pad)[0] for a in (10, 11)}
    geos = {p["id"]: so.load_geometry(sc.K32, sc.Kinv32, p["q_to_new"], p["t_to_new"]) for p in poses}
    f12 = img12.astype(np.float64)
    lipschitz = max(np.abs(np.diff(f12, axis=0)).max(), np.abs(np.diff(f12, axis=1)).max())
    coord_max = float(max(img12.shape))
    n_checked, worst, worst_bound, worst_ratio = 0, 0.0, 0.0, 0.0
    for i in np.nonzero(tr[:, T["steps"]] > 0)[0]:
        f = feats[i]
        ux, uy = np.float32(f["x"] + np.float32(pad)), np.float32(f["y"] + np.float32(pad))
        ex, ey = so.reference_epiline(geos[int(f["frame_id"])], ux, uy)
        js = np.arange(-2, 3)
        patch = r64.bilinear64(ref_pads[int(f["frame_id"])], float(ux) + js * float(ex), float(uy) + js * float(ey)).astype(np.float32)
        s = seg[i] + np.float32(pad)
        ref = r64.walk64(patch, img12, s[:2], s[2:], sd)
        if ref is None:
            continue
        c = ref["c_best"]
        n = ref["costs"].size
        margin = 2 * _cost_bound(n, coord_max, sd, lipschitz)
        others = np.delete(ref["costs"], c)
        if c >= n - 1 or (others.size and others.min() < ref["costs"][c] + margin):
            continue
        mrc, mx, my, _ = so.line_match(P, 1.0, patch, img12, s[0], s[1], s[2], s[3])
        assert mrc == 0, (i, mrc)
        # which step the checker matched: its position is within a fraction of |inc| of exactly one start + t * inc
        inc = ref["inc"]
        t32 = int(np.rint(((float(mx) - float(s[0])) * inc[0] + (float(my) - float(s[1])) * inc[1]) / (inc @ inc)))
        assert t32 == c, "feature %d: checker matched step %d, float64 step %d" % (i, t32, c)
        dev = max(abs(float(mx) - ref["x"]), abs(float(my) - ref["y"]))
        bound = _position_bound(c, coord_max, sd)
        if dev > worst:
            worst, worst_bound = dev, bound
        worst_ratio = max(worst_ratio, dev / bound if bound else (0.0 if dev == 0 else np.inf))
        n_checked += 1
    print("\nfloat64 cross-check: %d features, largest position deviation %.3e (bound there %.3e), largest deviation / bound %.3f"
          % (n_checked, worst, worst_bound, worst_ratio))
    assert n_checked >= 100, n_checked
    assert worst_ratio <= 1.0, "largest deviation %.3e against bound %.3e (ratio %.3f)" % (worst, worst_bound, worst_ratio)


# ---- GPU: every way in against the checker, bit for bit ----------------------------------------------------------------

STAT_NAMES = ("num_idepth_updates", "num_fail_max_var", "num_fail_max_dropouts", "num_fail_ref_patch_grad",
              "num_fail_ambiguous_match", "num_fail_max_cost", "success")


def _assert_gpu_equals_checker(case, feats=None, expect_assert=None):
    """Records and all counters when the checker runs through; the index of the first asserting feature when not.
    _gpu_update itself asserts that the 16-lane row, one lane per feature and the resident set agree."""
    feats = case["feats"] if feats is None else feats
    rc_o, st_o, out_o, _ = wc.run_checker(case, feats, trace=False)
    rc_g, st_g, out_g = _gpu_update(case["sc"], case["imgs"], feats, case["poses"], case["pkw"], pad=case["pad"],
                                    raise_on_error=False)
    what = "%s, %d features" % (case["name"], feats.shape[0])
    if expect_assert is not None:
        assert rc_o == -(1 + expect_assert), (what, rc_o, expect_assert)
    if rc_o < 0:
        assert rc_g == -8 and st_g["error_feature"] == -rc_o - 1, (what, rc_o, rc_g, st_g)
        return rc_o
    assert rc_o == 0 and rc_g == 0, (what, rc_o, rc_g, st_g)
    assert st_g["error_feature"] == -1, (what, st_g)
    assert [st_g[n] for n in STAT_NAMES] == [int(v) for v in st_o], (what, st_g, st_o)
    if out_g.tobytes() != out_o.tobytes():
        for name in out_o.dtype.names:
            a, b = out_g[name], out_o[name]
            bad = np.nonzero((a != b) & ~((a != a) & (b != b)) if a.ndim == 1 else np.any(a != b, axis=1))[0]
            if bad.size:
                i = int(bad[0])
                raise AssertionError("%s: %s differs on %d features, first %d: gpu %r checker %r (input %r)"
                                     % (what, name, bad.size, i, a[i], b[i], feats[i]))
        raise AssertionError("%s: records differ in their padding bytes" % what)
    return 0


@gpu
@pytest.mark.parametrize("sample_dist", wc.SAMPLE_DISTS)
@pytest.mark.parametrize("pattern", list(wc.PATTERNS))
def test_gpu_pattern_motion_grid(built, pattern, sample_dist):
    for motion in wc.MOTIONS:
        assert _assert_gpu_equals_checker(wc.make_case(pattern, motion, **wc.walk_params(sample_dist))) == 0


@gpu
def test_gpu_short_walks(built):
    assert _assert_gpu_equals_checker(wc.short_walk_case()) == 0


@functools.lru_cache(maxsize=None)
def _tied():
    return wc.tied_case()


@gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 63, 64, 65, 255, 256, 257, 4097])
def test_gpu_feature_counts(built, n):
    """Partly filled last wave in both forms; blockIdx % kStatSlots wraps at 256 features (row) and 4096 (one lane)."""
    case = _tied()
    assert case["feats"].shape[0] >= 4097
    assert _assert_gpu_equals_checker(case, case["feats"][:n].copy()) == 0


def _geometry_case(w, h, border, pattern, motion, sample_dist):
    return wc.make_case(pattern, motion, w=w, h=h, pad=border, nx=max(6, w // 8), ny=max(5, h // 8), border=5,
                        **wc.walk_params(sample_dist))


@gpu
@pytest.mark.parametrize("border", [2, 3, 5, 8])
@pytest.mark.parametrize("size", [(37, 29), (48, 40), (64, 48), (161, 121)])
def test_gpu_image_geometry(built, size, border):
    """Small and odd images, every border: (37, 2), (48, 3), (64, 5) and (161, 8) among them have a padded width that
    is no multiple of 16.  Where the leading sample leaves a thin border both sides must name the same feature."""
    for pattern, motion, sd in (("saw_v12", "+x", 0.5), ("saw_h12", "-y", 1.0), ("stripes_v6", "-x+y", 1.5),
                                ("saw_d12", "forward", 0.5)):
        _assert_gpu_equals_checker(_geometry_case(size[0], size[1], border, pattern, motion, sd))


@gpu
def test_gpu_segment_clipping(built):
    """Features whose search segment the [1, w-1] x [1, h-1] box clips, at least 4 on each of its four sides."""
    sides = {"left": 0, "right": 0, "top": 0, "bottom": 0}
    for motion in ("+x", "-x", "+y", "-y", "+x-y", "-x+y"):
        case = wc.make_case("saw_d12", motion, border=5, **wc.walk_params(1.0))
        rc, seg = wc.search_segments(case)
        _, _, _, tr = wc.run_checker(case)
        walked = (rc == 1) & (tr[:, T["steps"]] > 0)
        w, h = case["sc"].width, case["sc"].height
        on = {"left": (seg[:, [0, 2]] == 1.0).any(axis=1), "right": (seg[:, [0, 2]] == np.float32(w - 1)).any(axis=1),
              "top": (seg[:, [1, 3]] == 1.0).any(axis=1), "bottom": (seg[:, [1, 3]] == np.float32(h - 1)).any(axis=1)}
        pick = np.zeros(rc.size, bool)
        for k, m in on.items():
            sides[k] += int((m & walked).sum())
            pick |= m & walked
        assert pick.sum() >= 4, (motion, pick.sum())
        assert _assert_gpu_equals_checker(case, case["feats"][pick].copy()) == 0
    assert min(sides.values()) >= 4, sides


def _asserting_features(case):
    """Indices of all features the checker asserts on, one run per hit (it stops at the first)."""
    hits, base = [], 0
    feats = case["feats"]
    while base < feats.shape[0]:
        rc = wc.run_checker(case, feats[base:].copy(), trace=False)[0]
        if rc >= 0:
            break
        hits.append(base - rc - 1)
        base = hits[-1] + 1
    return np.array(hits, np.int64)


@gpu
@pytest.mark.parametrize("border", [0, 1])
def test_gpu_reference_asserts_from_the_walk(built, border):
    """With a border of 0 or 1 pixel the walk's leading sample leaves the padded image for segments that end at the
    box: the reference asserts, the checker returns -(1 + index) and the kernel reports the lowest such index."""
    # (border 1 needs whole-pixel steps: the leading sample is two steps ahead of a position that stops at w - 1)
    case = wc.make_case("saw_d12", "+x", pad=border, **wc.walk_params((0.5, 1.0)[border]))
    feats = case["feats"]
    bad = _asserting_features(case)
    is_bad = np.zeros(feats.shape[0], bool)
    is_bad[bad] = True
    _, _, _, tr = wc.run_checker(case, feats[~is_bad].copy())
    clean = np.nonzero(~is_bad)[0]
    long_walk = clean[tr[:, T["steps"]] >= 33]   # three rounds or more; a short one is done in its first
    short = clean[(tr[:, T["steps"]] > 0) & (tr[:, T["steps"]] <= 8)]
    assert bad.size >= 12 and long_walk.size >= 8 and short.size >= 8, (bad.size, long_walk.size, short.size)
    # the whole set: asserting features in many waves
    assert len(set(bad // 4)) >= 3
    _assert_gpu_equals_checker(case, feats, expect_assert=int(bad[0]))
    # three waves with one asserting feature each, the one of the lowest index in the last row of the middle wave
    idx = np.concatenate([short[:4], [short[4], short[5], short[6], bad[1]], short[:3], [bad[0]], [bad[2]], short[:3]])
    _assert_gpu_equals_checker(case, feats[idx].copy(), expect_assert=7)
    # several in one wave, behind two clean waves
    idx = np.concatenate([short[:8], [short[0], bad[3], bad[4], bad[5]]])
    _assert_gpu_equals_checker(case, feats[idx].copy(), expect_assert=9)
    # one asserting row between rows that go on walking for rounds
    idx = np.concatenate([short[:4], [long_walk[0], bad[6], long_walk[1], long_walk[2]]])
    _assert_gpu_equals_checker(case, feats[idx].copy(), expect_assert=5)
    # ... and a whole wave of long walks in front of it
    idx = np.concatenate([long_walk[:4], [long_walk[4], long_walk[5], bad[7], long_walk[6]]])
    _assert_gpu_equals_checker(case, feats[idx].copy(), expect_assert=6)
