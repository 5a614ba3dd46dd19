"""Inputs that drive k_update_feature_idepths through the stages AROUND the epipolar walk -- predict, the rescale gate and
the move to the newest pose-frame, the search region, the valid rectangle, the gradient gate, the measurement model, the
fusion, fail_feature -- at their exits and at the edges of their threshold comparisons.  Plain numpy, shared by the CPU and
the GPU tests of tests/test_stereo_update_edges.py; built like tests/stereo_walk_cases.make_case.

A case is the dict of stereo_walk_cases (sc, imgs, feats, poses, pkw, pad, name) plus
    walk     True: the walk returns its best step whatever it costs (no sub-pixel step, no ambiguity test, no cost limit),
             so that the float64 walk of tests/stereo_ref64.py gives the matched position
    expect   {kind: {feature index: expected}} for the features whose inputs are SET ON an edge; the expectation is
             worked out here from the inputs in exact or float32 arithmetic, never from the checker:
               "forced"   value of the trace's forced_one column
               "stage"    the stage name
               "outside"  True: stage "outside the valid rectangle"; False: the feature passed that test
               "moved"    True: the feature took the move path (moved or move failed); False: it went on to the region
               "skipped"  True: baseline skip; False: not
               "no_grad"  True: search status 1; False: the feature passed the gradient gate
               "fail"     value of the trace's fail_bits column
    decide   {feature index: {decision name of tests/stereo_update_ref64.py: outcome}} for the same features: the
             outcome of the comparison their inputs were set on, as the expectation above implies it.  The float64
             restatement cannot take such a decision (the value sits on its threshold); it follows this one and goes
             on, so that everything behind the decision is compared with float64 as for any other feature
    assert_at   index of the feature the reference asserts on (the checker returns -(1 + index)), or absent
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import stereo_capi as so
from tests import stereo_walk_cases as wc

W, H, PAD = 160, 120, 5
F = np.float32
WALK = dict(do_subpixel=0, second_best_factor=1.0, max_cost=1e9)


def up(x):
    return np.nextafter(F(x), F(np.inf))


def down(x):
    return np.nextafter(F(x), F(-np.inf))


def _scene(t_new, t_pf=None, seed=1, distance=2.0, sigma=2.4):
    """sigma: the blur of the plane's texture in pixels.  PlaneScene's own 1.6 is rough for these tests: a smoother image
    has a smoother gradient, so the measurement model is better conditioned in the match's position, which float64 knows
    to a thousandth of a pixel only; fewer features are then left out for a gradient that may point anywhere."""
    from flame_amd import synth_stereo as ss

    sc = ss.PlaneScene(W, H, seed=seed, normal=(0.0, 0.0, 1.0), distance=distance)
    sc.tex = ss.texture(W, H, seed, sigma=sigma, margin=sc.margin)
    t_new = np.asarray(t_new, np.float64)
    sc.add_camera(10, np.eye(3), [0, 0, 0])
    sc.add_camera(11, np.eye(3), 0.5 * t_new if t_pf is None else np.asarray(t_pf, np.float64))
    sc.add_camera(12, np.eye(3), t_new)
    return sc


def _grid(sc, nx=14, ny=10, border=12, seed=0, mu_noise=0.1, var=0.02):
    """Features on a jittered nx x ny grid in each of the anchors 10 and 11, priors around the truth."""
    rng = np.random.default_rng(4321 + seed)
    n1 = nx * ny
    feats = np.zeros(2 * n1, so.FEATURE_DTYPE)
    gx = border + (np.arange(nx) + 0.5) * ((W - 2 * border) / nx)
    gy = border + (np.arange(ny) + 0.5) * ((H - 2 * border) / ny)
    for a_i, anchor in enumerate((10, 11)):
        s = slice(a_i * n1, (a_i + 1) * n1)
        xy = np.stack([np.tile(gx, ny) + rng.uniform(-1.5, 1.5, n1), np.repeat(gy, nx) + rng.uniform(-1.5, 1.5, n1)], 1).astype(F)
        feats["frame_id"][s] = anchor
        feats["x"][s], feats["y"][s] = xy[:, 0], xy[:, 1]
        feats["idepth_mu"][s] = (sc.true_idepth(anchor, xy) * (1.0 + mu_noise * rng.uniform(-1.0, 1.0, n1))).astype(F)
    feats["id"] = np.arange(2 * n1)
    feats["idepth_var"] = F(var)
    feats["valid"] = 1
    return feats


def _case(name, sc, feats, pkw, imgs=None, walk=True, expect=None, assert_at=None, decide=None):
    from flame_amd import synth_stereo as ss

    if imgs is None:
        imgs = {c: sc.render(c) for c in (10, 11, 12)}
    pkw = dict(WALK, **pkw) if walk else dict(pkw)
    c = dict(sc=sc, imgs=imgs, feats=feats, poses=ss.poses_for(sc, [10, 11], 12, 11), pkw=pkw, pad=PAD, name=name, walk=walk,
             expect=expect or {}, decide=decide or {})
    if assert_at is not None:
        c["assert_at"] = assert_at
    return c


# ---- plain scenes: every t.z branch of the epiline, fusion on and off, the walk's own failures ------------------------------

def scene_cases():
    for name, t, fusion in (("scene tz=0 fused", (0.2, 0.05, 0.0), 1), ("scene tz<0 measured", (0.18, 0.04, -0.1), 0),
                            ("scene tz>0 fused", (-0.15, 0.06, 0.12), 1), ("scene tz=0 measured", (-0.04, 0.2, 0.0), 0)):
        sc = _scene(t)
        yield _case(name, sc, _grid(sc, seed=len(name)), dict(do_meas_fusion=fusion))
    sc = _scene((0.2, 0.05, -0.05))
    yield _case("scene, the walk's own parameters", sc, _grid(sc, mu_noise=0.35, var=0.04, seed=7), {}, walk=False)


# ---- idepth_mu at the double constant 1e-6 ---------------------------------------------------------------------------------

DENORMAL = F(1e-38)                   # 1 / DENORMAL is finite in float32; K * pc then overflows to infinity
MU_EDGES = (F(0.0), F(1e-6), down(1e-6), up(1e-6), F(1e-7), F(0.0), F(1e-6), down(1e-6), up(1e-6), F(1e-7), F(1e-6), DENORMAL,
            F(0.0), F(1e-6), down(1e-6), up(1e-6), F(1e-7), F(0.0), F(1e-6), down(1e-6), up(1e-6), F(1e-7), F(1e-6), up(1e-6))


def mu_edge_case():
    """float32(1e-6) is below the double 1e-6: (double)mu < 1e-6 forces the variance factor for it, mu < 1e-6f would not."""
    sc = _scene((0.2, 0.03, 0.0))
    feats = _grid(sc, var=0.1, seed=2)
    feats["idepth_mu"] = np.resize(np.array(MU_EDGES, F), feats.shape[0])
    assert float(F(1e-6)) < 1e-6 < float(up(1e-6))
    forced = {i: int(float(m) < 1e-6) for i, m in enumerate(feats["idepth_mu"])}
    return _case("mu edges", sc, feats, {}, expect=dict(forced=forced))


def mu_edge_move_case():
    """rescale_factor_max = 1: far points take the move path (idepth_cmp / mu >= 1 with the new camera ahead), and
    idepth_pf = 1 / (1 / mu + 0) decides (double)idepth_pf < 1e-6.  Pose-frame 11 is displaced sideways only, the
    rotation is the identity: pc.z = 1 / mu exactly, in float32 arithmetic here."""
    sc = _scene((0.02, 0.01, -0.3), t_pf=(0.05, 0.0, 0.0))
    feats = _grid(sc, var=0.1, seed=3)
    mus = np.resize(np.array(MU_EDGES, F), feats.shape[0])
    feats["idepth_mu"] = mus
    forced, stage, decide = {}, {}, {}
    for i, m in enumerate(mus):
        # idepth_cmp / mu >= 1 = rescale_factor_max: `rescale < max` is false for every feature here
        if m == DENORMAL:
            stage[i] = "move failed: rectangle"       # u_pf overflows
            forced[i] = 1
            decide[i] = {"rescale_factor_max": False, "moved point in the rectangle": False}
            continue
        with np.errstate(divide="ignore"):
            idepth_pf = F(0.0) if m == 0 else F(1.0) / (F(1.0) / m)
        stage[i] = "moved"
        forced[i] = int(float(m) < 1e-6) | (2 if float(idepth_pf) < 1e-6 else 0)
        decide[i] = {"rescale_factor_max": False, "idepth_pf < 1e-6": float(idepth_pf) < 1e-6}
    return _case("mu edges, move path", sc, feats, dict(rescale_factor_max=1.0), expect=dict(forced=forced, stage=stage),
                 decide=decide)


# ---- the valid rectangle: ties round to even --------------------------------------------------------------------------------

def rect_edge_cases():
    from tests import stereo_update_ref64 as u64

    for name, pkw in (("border 4", {}), ("border 5", dict(rescale_factor_max=1.6)), ("letterbox", dict(do_letterbox=1)),
                      ("letterbox, border 5", dict(do_letterbox=1, rescale_factor_max=1.6))):
        sc = _scene((0.2, 0.04, 0.0))
        feats = _grid(sc, seed=5, border=3)
        vx, vy, vw, vh = u64.valid_rect(so.Params(**pkw), W, H)
        outside = {}
        k = 0
        for rep in range(6):
            for j in range(4):     # the position across the edge: v - 0.5, v + 0.5, v + size - 0.5, v + size - 1.5
                for axis in (0, 1):
                    i = 3 + 2 * k          # spread through both anchors
                    k += 1
                    v, size = (vx, vw) if axis == 0 else (vy, vh)
                    across = F(v + (-0.5, 0.5, size - 0.5, size - 1.5)[j])
                    along = F((vy, vx)[axis] + 3.25 + rep * ((vh, vw)[axis] - 7) / 6.0)
                    x, y = (across, along) if axis == 0 else (along, across)
                    feats["x"][i], feats["y"][i] = x, y
                    # a far, narrow prior: its segment is a pixel long and stays inside the image box at every edge
                    feats["idepth_mu"][i], feats["idepth_var"][i] = F(0.05), F(1e-4)
                    ix, iy = round(float(x)), round(float(y))          # Python rounds ties to even
                    outside[i] = not (vx <= ix < vx + vw and vy <= iy < vy + vh)
        yield _case("rectangle edges, " + name, sc, feats, pkw, expect=dict(outside=outside))


def moved_rect_edge_case():
    """Rounding ties of the MOVED position.  Pose-frame 11 shares the rotation of 10 and features with mu = 0 move by
    the homography K R K^-1 alone, which float32 makes the identity here (asserted below from the Geometry's fields):
    u_pf = u exactly.  rescale_factor_min = 1 sends exactly them to the move path (their rescale factor is 1 by
    definition, every other feature's exceeds 1 with the new camera ahead); rescale_factor_max = 1.6 makes the border
    5, where half-up rounding would differ from ties-to-even at both edges."""
    from tests import stereo_update_ref64 as u64

    pkw = dict(rescale_factor_min=1.0, rescale_factor_max=1.6)
    sc = _scene((0.02, 0.01, -0.3), t_pf=(0.05, 0.0, 0.0))
    feats = _grid(sc, seed=19)
    from flame_amd import synth_stereo as ss
    vx, vy, vw, vh = u64.valid_rect(so.Params(**pkw), W, H)
    stage, decide = {}, {}
    k = 0
    for rep in range(6):
        for j in range(4):
            for axis in (0, 1):
                i = 2 + 2 * k
                k += 1
                v, size = (vx, vw) if axis == 0 else (vy, vh)
                across = F(v + (-0.5, 0.5, size - 0.5, size - 1.5)[j])
                along = F((vy, vx)[axis] + 3.25 + rep * ((vh, vw)[axis] - 7) / 6.0)
                x, y = (across, along) if axis == 0 else (along, across)
                feats["x"][i], feats["y"][i], feats["idepth_mu"][i] = x, y, F(0.0)
                p = [q for q in ss.poses_for(sc, [10, 11], 12, 11) if q["id"] == int(feats["frame_id"][i])][0]
                M = np.array(so.load_geometry(sc.K32, sc.Kinv32, p["q_to_pf"], p["t_to_pf"]).KRKinv, F)
                h = [(M[3 * r] * x + M[3 * r + 1] * y) + M[3 * r + 2] for r in range(3)]
                inv = F(1.0) / h[2]
                assert (h[0] * inv, h[1] * inv) == (x, y), (x, y, h)
                inside = vx <= round(float(x)) < vx + vw and vy <= round(float(y)) < vy + vh      # Python rounds ties to even
                stage[i] = "moved" if inside else "move failed: rectangle"
                decide[i] = {"moved point in the rectangle": inside}
    return _case("moved position on the rectangle's edges", sc, feats, pkw, expect=dict(stage=stage), decide=decide)


# ---- fail_feature -----------------------------------------------------------------------------------------------------------

def fail_edge_cases():
    """Every feature fails (its window lies above idepth_max).  idepth_var_max is the float32 product var * factor itself
    (`>` keeps the feature) or the float32 number below it; num_dropouts is max_dropouts - 1, max_dropouts, 0xffffffff."""
    sc = _scene((0.2, 0.0, 0.0))
    base = _grid(sc, nx=8, ny=6, seed=6)
    base["idepth_mu"] = F(5.0)
    base["idepth_var"] = F(0.01)
    drops = np.resize(np.array([4, 5, 0xffffffff], np.uint32), base.shape[0])
    base["num_dropouts"] = drops
    prod = F(0.01) * F(1.1)
    for name, vmax, vbit in (("at the product", prod, 0), ("below the product", down(prod), 1)):
        fail = {i: vbit | (2 if int(d) == 5 else 0) for i, d in enumerate(drops)}
        yield _case("fail edges, idepth_var_max " + name, sc, base.copy(), dict(idepth_var_max=float(vmax)), expect=dict(fail=fail),
                    decide={i: {"idepth_var_max": bool(vbit)} for i in fail})         # idepth_var_max < var * factor


# ---- the rescale gate --------------------------------------------------------------------------------------------------------

def rescale_edge_cases():
    """A third of the anchor-10 features carry mu = 0.5: with identity rotations pc.z = 2 + t.z for all of them, one
    float32 rescale factor r.  `>= max` and `<= min` move them at r; the neighbour of r that leaves it inside does not."""
    # (with the new camera behind, a sideways part keeps the epipole, where disparities vanish, at the image's edge)
    for side, t in (("max", (0.02, 0.01, -0.45)), ("min", (0.25, 0.08, 0.5))):
        sc = _scene(t)
        feats = _grid(sc, seed=8)
        n1 = feats.shape[0] // 2
        pick = np.arange(0, n1, 3)
        feats["idepth_mu"][pick] = F(0.5)
        from flame_amd import synth_stereo as ss
        p10 = ss.poses_for(sc, [10, 11], 12, 11)[0]
        g = so.load_geometry(sc.K32, sc.Kinv32, p10["q_to_new"], p10["t_to_new"])
        rs = {float(so.project_idepth(g, feats["x"][i], feats["y"][i], F(0.5))[2] / F(0.5)) for i in pick}
        assert len(rs) == 1, rs
        r = F(rs.pop())
        inside = up(r) if side == "max" else down(r)
        for name, value, moved in (("at the factor", r, True), ("beside it", inside, False)):
            yield _case("rescale_factor_%s %s" % (side, name), sc, feats.copy(), {"rescale_factor_" + side: float(value)},
                        expect=dict(moved={int(i): moved for i in pick}),
                        # "rescale_factor_max": rescale < max; "rescale_factor_min": min < rescale
                        decide={int(i): {"rescale_factor_" + side: not moved} for i in pick})


# ---- min_baseline -------------------------------------------------------------------------------------------------------------

def baseline_edge_cases():
    """min_baseline at the float32 baseline of pose-frame 11 (`<` keeps it) and just above (its features are untouched and
    uncounted while those of pose-frame 10, twice as far away, update)."""
    sc = _scene((0.2, 0.05, 0.03))
    feats = _grid(sc, seed=9)
    from flame_amd import synth_stereo as ss
    t = np.asarray(ss.poses_for(sc, [10, 11], 12, 11)[1]["t_to_new"], F)
    b = np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2])
    assert b.dtype == F
    is11 = feats["frame_id"] == 11
    for name, value, skipped in (("at the baseline", b, False), ("above it", up(b), True)):
        yield _case("min_baseline " + name, sc, feats.copy(), dict(min_baseline=float(value)),
                    expect=dict(skipped={int(i): bool(skipped and is11[i]) for i in range(feats.shape[0])}),
                    decide={int(i): {"baseline": skipped} for i in np.nonzero(is11)[0]})      # baseline < min_baseline


# ---- min_grad_mag --------------------------------------------------------------------------------------------------------------

def grad_edge_cases():
    """An integer-valued sawtooth across x (16 grey levels per pixel), K t = (32, 0, 0) exactly, mu = 0.5: the reference
    epiline is (1, 0) and the rescale factor 1 in float32, so the patch is the five pixels x - 2 .. x + 2 and gmax = 16
    exactly wherever they hold no wrap of the sawtooth."""
    from flame_amd import synth_stereo as ss

    fx = float(ss.intrinsics(W, H)[0][0, 0])
    tx = F(32.0 / fx)
    for cand in (tx, up(tx), down(tx)):
        if F(fx) * cand == F(32.0):
            tx = cand
            break
    assert F(fx) * tx == F(32.0)
    sc = _scene((float(tx), 0.0, 0.0))
    img = wc.PATTERNS["saw_v12"](W, H)                                  # rows 0..59: 16 per pixel
    img[60:] = (20 + (np.arange(W) % 8) * 24).astype(np.uint8)[None, :]   # rows 60..: 24 per pixel, for the other features
    feats = _grid(sc, seed=10)
    n1 = feats.shape[0] // 2
    pick = np.arange(0, n1, 2)
    is_pick = np.zeros(feats.shape[0], bool)
    is_pick[pick] = True
    feats["y"] = np.where(is_pick, np.rint(12 + (feats["y"] - 12) * 0.45), 64 + (feats["y"] - 12) * 0.45).astype(F)
    feats["x"][pick] = np.rint(feats["x"][pick])
    feats["idepth_mu"][pick] = F(0.5)
    flat = {}
    for i in pick:
        x, y = int(feats["x"][i]), int(feats["y"][i])
        row = img[y, x - 2:x + 3].astype(np.int64)
        if np.abs(np.diff(row)).max() == 16:
            flat[int(i)] = True
    assert len(flat) >= 8
    for name, value, no_grad in (("at gmax", F(16.0), False), ("above gmax", up(16.0), True)):
        yield _case("min_grad_mag " + name, sc, feats.copy(), dict(min_grad_mag=float(value)), imgs={10: img, 11: img, 12: img},
                    walk=False, expect=dict(no_grad={i: no_grad for i in flat}),
                    decide={i: {"min_grad_mag": no_grad} for i in flat})                      # gmax < min_grad_mag


# ---- the silent exits -------------------------------------------------------------------------------------------------------------

def behind_case(with_assert=False):
    """t_to_new.z = -0.5 for pose-frame 10: mu = 4 puts the point behind the new camera (predict says no); mu = 1.6 is in
    front of it, too close for the rescale gate, and behind pose-frame 11 at z = -0.7 (the move fails in predict);
    mu = 2 is pc.z == 0 exactly: the reference asserts."""
    sc = _scene((0.02, 0.01, -0.5), t_pf=(0.01, 0.0, -0.7))
    feats = _grid(sc, seed=11)
    n1 = feats.shape[0] // 2
    stage = {}
    for i in range(0, n1, 4):
        feats["idepth_mu"][i] = F(4.0)
        stage[i] = "predict no"
    for i in range(1, n1, 4):
        feats["idepth_mu"][i] = F(1.6)
        stage[i] = "move failed: predict"
    if with_assert:
        feats["idepth_mu"][[37, 90]] = F(2.0)
        return _case("pc.z == 0", sc, feats, {}, assert_at=37)
    return _case("behind the camera", sc, feats, {}, expect=dict(stage=stage))


def window_case():
    """idepth windows with no region: above idepth_max, below idepth_min, of zero width (var = 0), projected wholly
    outside the image box, and touching the box in one point (K t = (32, 0, 0), idepth_min = 0.5: the far end of the
    window projects to x + 16 = 159 exactly, the rest lies to the right of the box)."""
    from flame_amd import synth_stereo as ss

    fx = float(ss.intrinsics(W, H)[0][0, 0])
    tx = F(32.0 / fx)
    for cand in (tx, up(tx), down(tx)):
        if F(fx) * cand == F(32.0):
            tx = cand
            break
    sc = _scene((float(tx), 0.0, 0.0))
    feats = _grid(sc, seed=12)
    n1 = feats.shape[0] // 2
    stage, decide = {}, {}
    for k, i in enumerate(range(0, n1, 2)):
        kind = k % 5
        if kind == 0:
            feats["idepth_mu"][i], feats["idepth_var"][i] = F(5.0), F(0.01)
            stage[i] = "no region: empty idepth window"
        elif kind == 1:
            feats["idepth_mu"][i], feats["idepth_var"][i] = F(0.3), F(1e-10)
            stage[i] = "no region: empty idepth window"           # wholly below idepth_min = 0.5
        elif kind == 2:
            feats["idepth_mu"][i], feats["idepth_var"][i] = F(0.52), F(0.0)
            stage[i] = "no region: zero length"
        elif kind == 3:
            feats["x"][i], feats["idepth_mu"][i], feats["idepth_var"][i] = F(150.0 + (k % 7)), F(0.54), F(1e-8)
            stage[i] = "no region: first clip"                    # 150 + 32 * 0.54 > 159
        else:
            feats["x"][i], feats["y"][i] = F(143.0), np.rint(feats["y"][i])
            feats["idepth_mu"][i], feats["idepth_var"][i] = F(0.51), F(0.01)
            stage[i] = "no region: zero length after the clip"
            decide[i] = {"first clip: visible": False, "clipped length > 0": False}   # not t1 < t0, not 0 < length
    return _case("idepth windows without a region", sc, feats, dict(idepth_min=0.5, idepth_max=0.55), expect=dict(stage=stage),
                 decide=decide)


def clip_cases():
    """Segments that the image box clips on each side, that are padded to epilength_min (and clipped again where the
    padding leaves the box) and that are cut to epilength_max."""
    for name, t in (("+x", (0.2, 0.05, 0.0)), ("-x", (-0.2, 0.04, 0.0)), ("+y", (0.05, 0.2, 0.0)), ("-y", (-0.04, -0.2, 0.0))):
        sc = _scene(t)
        feats = _grid(sc, seed=13, border=6, mu_noise=0.0005)
        feats["idepth_var"] = np.resize(np.array([0.02, 0.02, 0.02, 0.02, 0.02, 0.24, 0.02, 0.02, 0.02, 0.02, 0.02, 0.02, 0.02, 0.02, 0.02], F),
                                        feats.shape[0])
        n1 = feats.shape[0] // 2
        shift = float(sc.K[0, 0]) * 0.2 * 0.5       # disparity of the prior mu = 0.5 seen from anchor 10
        for k in range(10):                        # tiny segments that end within the padding's reach of the box
            i = 4 * k
            main = 0 if abs(t[0]) > abs(t[1]) else 1
            edge = (W - 1.0, H - 1.0)[main] if t[main] > 0 else 1.0
            pos = edge - np.sign(t[main]) * (shift + 0.3 + 0.1 * k)
            if main == 0:
                feats["x"][i] = F(pos)
            else:
                feats["y"][i] = F(pos)
            feats["idepth_mu"][i], feats["idepth_var"][i] = F(0.5), F(1e-6)
        yield _case("clipped segments, motion " + name, sc, feats, {})


def zero_disparity_case():
    """idepth_min = 0 and the same image in every frame: the best match is the window's far end, the point at infinity."""
    sc = _scene((0.2, 0.0, 0.0))
    img = sc.render(10)
    feats = _grid(sc, seed=14, var=0.01)
    feats["idepth_mu"] = F(0.05)
    return _case("zero disparity", sc, feats, dict(idepth_min=0.0), imgs={10: img, 11: img, 12: img})


def constant_new_image_case():
    sc = _scene((0.2, 0.0, 0.0))
    imgs = {10: sc.render(10), 11: sc.render(11), 12: np.full((H, W), 117, np.uint8)}
    return _case("constant new image", sc, _grid(sc, seed=15, var=0.005), {}, imgs=imgs)


def parallel_stripes_case():
    """The new image changes across the epipolar line only (its gradient is (0, 2)), the epiline is (1, 0) exactly:
    edn == 0 and geo_var is infinite before the |edn| test."""
    sc = _scene((0.2, 0.0, 0.0))
    ref = wc.PATTERNS["saw_v12"](W, H)
    ramp = np.repeat((10 + 2 * np.arange(H))[:, None], W, axis=1).astype(np.uint8)      # 2 grey levels per row, no wrap
    imgs = {10: ref, 11: ref, 12: ramp}
    return _case("new image striped along the epipolar line", sc, _grid(sc, seed=16, var=0.005), {}, imgs=imgs)


def outlier_case():
    """A search window of six sigma against an outlier gate of three: priors four to five sigma off the truth, half of them
    mu = 0 (the measurement would replace the prior)."""
    sc = _scene((0.2, 0.03, 0.0))
    feats = _grid(sc, seed=17)
    n = feats.shape[0]
    truth = feats["idepth_mu"].copy()
    k = np.arange(n) % 4
    feats["idepth_mu"] = np.where(k == 0, F(0.0), np.where(k == 1, (truth * 0.45).astype(F), truth)).astype(F)
    feats["idepth_var"] = np.where(k == 0, F(0.011), np.where(k == 1, F(0.004), F(0.02))).astype(F)
    return _case("outliers", sc, feats, dict(search_sigma=6.0, epilength_max=48.0))


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = list(scene_cases()) + [mu_edge_case(), mu_edge_move_case()] + list(rect_edge_cases()) + [moved_rect_edge_case()] + list(fail_edge_cases()) \
        + list(rescale_edge_cases()) + list(baseline_edge_cases()) + list(grad_edge_cases()) \
        + [behind_case(), behind_case(with_assert=True), window_case()] + list(clip_cases()) \
        + [zero_disparity_case(), constant_new_image_case(), parallel_stripes_case(), outlier_case()]
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return tuple(cases)
