"""The matches picture (getDebugImageMatches; include/flame_stereo.h, flame_stereo_draw_matches) on the CPU: the drawing primitives of
the checker tests/matches_ref.py against known answers, the checker's own control flow against the oracle's update, and the cases
the GPU tests (tests/test_gpu_matches*.py) compare byte for byte.

The cases live here.  Each is a dict: width, height, pad, K, Kinv, imgs {frame id: grey image}, poses, feats (oracle
FEATURE_DTYPE), pkw (parameters that differ from the defaults), curr_pf, new.  case(name) builds one, reference(name) is the
checker's result for it, computed once and shared."""
import functools

import numpy as np
import pytest

from oracle import stereo_capi as so
from tests import matches_ref as mr

F = np.float32


# ---- the cases ---------------------------------------------------------------------------------------------------------------

def _scene(width, height, n_per_anchor, seed, **feat_kw):
    from flame_amd import synth_stereo as ss

    sc = ss.standard_scene(width, height, seed=seed)
    imgs = {c: sc.render(c) for c in (10, 11, 12)}
    feats = ss.make_features(sc, so.FEATURE_DTYPE, [10, 11], n_per_anchor, seed, **feat_kw)
    return dict(width=width, height=height, pad=5, K=sc.K32, Kinv=sc.Kinv32, imgs=imgs, poses=ss.poses_for(sc, [10, 11], 12, 11),
                feats=feats, pkw={}, curr_pf=11, new=12)


def _edge_features(f):
    """The inputs of test_gpu_edge_case_features (tests/test_stereo.py), plus records that were updated before."""
    f["idepth_mu"][0:20] = 0.0
    f["idepth_var"][20:40] = 0.24                   # any failure pushes the variance past idepth_var_max: green
    f["num_dropouts"][40:60] = 5                    # = max_dropouts on input, one more dropout: blue
    f["x"][60:70] = 2.0                             # outside the valid region: nothing but the rings
    f["y"][70:80] = f["y"].max() + 6.0
    f["idepth_mu"][80:100] *= 3.0
    f["idepth_var"][100:120] = 1e-6
    f["idepth_var"][120:140] = 0.0                  # empty search segment: black
    f["search_status"][140:160] = 2
    f["idepth_mu"][160:170] = 1e-7
    f["idepth_mu"][170:180] = 5.0                   # beyond idepth_max: black
    f["idepth_var"][180:200] = 0.25                 # fresh features: idepth_var_init = idepth_var_max
    f["num_dropouts"][190:200] = 5                  # both rings
    return f


def _case_scene(width=320, height=240):
    c = _scene(width, height, 300, 8)
    _edge_features(c["feats"])
    return c


def _case_variants():
    """Parameter variants of test_gpu_parameter_variants that change which branch a feature takes."""
    c = _scene(320, 240, 250, 5)
    c["pkw"] = dict(max_cost=300.0, second_best_factor=3.0, search_sigma=3.0, min_grad_mag=12.0)
    c["feats"]["num_updates"][::3] = 2
    return c


def _case_move(width=320, height=240, n_per_anchor=400):
    """The input of test_gpu_feature_move_to_newest_poseframe: brown and magenta."""
    from flame_amd import synth_stereo as ss

    sc = ss.PlaneScene(width, height, 4, normal=(0.0, 0.0, 1.0), distance=1.0)
    sc.add_camera(10, np.eye(3), [0, 0, 0])
    sc.add_camera(11, np.eye(3), [0.0, 0.0, -0.33])
    sc.add_camera(12, np.eye(3), [0.01, 0.0, -0.35])
    imgs = {c: sc.render(c) for c in (10, 11, 12)}
    feats = ss.make_features(sc, so.FEATURE_DTYPE, [10, 11], n_per_anchor, 4)
    feats["idepth_var"][::7] = 0.24
    return dict(width=width, height=height, pad=5, K=sc.K32, Kinv=sc.Kinv32, imgs=imgs, poses=ss.poses_for(sc, [10, 11], 12, 11),
                feats=feats, pkw={}, curr_pf=11, new=12)


def _case_textureless(width=320, height=240, n_per_anchor=200):
    """A reference patch without gradient: white for fresh features, cyan for those updated before; every one with its segment."""
    c = _scene(width, height, n_per_anchor, 6)
    for fid in (10, 11):
        c["imgs"][fid] = np.full((height, width), 117, np.uint8)
    f = c["feats"]
    f["num_updates"][1::2] = 3
    f["idepth_var"][::5] = 0.25
    f["num_dropouts"][::9] = 5
    return c


def _case_stripes():
    """The same periodic stripes in every frame, across a horizontal epipolar direction: equal minima a period apart, red."""
    from flame_amd import synth_stereo as ss

    sc = ss.PlaneScene(320, 240, 9)
    sc.add_camera(10, np.eye(3), [0, 0, 0])
    sc.add_camera(11, np.eye(3), [-0.03, 0.0, 0.0])
    sc.add_camera(12, np.eye(3), [-0.1, 0.0, 0.0])
    x = np.arange(320, dtype=np.float64)
    row = np.rint(128.0 + 100.0 * np.sin(2.0 * np.pi * x / 8.0)).astype(np.uint8)
    img = np.repeat(row[None, :], 240, axis=0)
    feats = ss.make_features(sc, so.FEATURE_DTYPE, [10, 11], 150, 9, var=0.05)
    feats["idepth_var"][::4] = 0.25
    return dict(width=320, height=240, pad=5, K=sc.K32, Kinv=sc.Kinv32, imgs={10: img, 11: img, 12: img},
                poses=ss.poses_for(sc, [10, 11], 12, 11), feats=feats, pkw={}, curr_pf=11, new=12)


def _case_altered():
    """The new image replaced by noise: no step of the walk comes near the reference patch, yellow."""
    from flame_amd.synth import uniform01

    c = _scene(320, 240, 150, 12)
    c["imgs"][12] = (uniform01(12, 320 * 240, stream=3) * 255.0).astype(np.uint8).reshape(240, 320)
    c["feats"]["idepth_var"][::6] = 0.25
    return c


def _case_order():
    """Features a few pixels apart in front of a textureless reference, white and cyan alternating, some with rings: segments run
    over later rectangles, rectangles lie under later segments, and segments of two colours share pixels."""
    from flame_amd import synth_stereo as ss

    c = _scene(320, 240, 4, 6)
    sc = ss.standard_scene(320, 240, seed=6)
    for fid in (10, 11):
        c["imgs"][fid] = np.full((240, 320), 90, np.uint8)
    gx, gy = np.meshgrid(150.0 + 5.0 * np.arange(7), 110.0 + 2.0 * np.arange(6))
    xy = np.stack([gx.ravel(), gy.ravel()], axis=1).astype(F)
    f = np.zeros(xy.shape[0], so.FEATURE_DTYPE)
    f["id"] = np.arange(f.shape[0])
    f["frame_id"] = 10
    f["x"], f["y"] = xy[:, 0], xy[:, 1]
    f["idepth_mu"] = sc.true_idepth(10, xy).astype(F)
    f["idepth_var"] = 0.02
    f["idepth_var"][::4] = 0.25
    f["valid"] = 1
    f["num_updates"][1::2] = 3
    c["feats"] = f
    return c


def _case_clip():
    """A camera that moves forward pushes the features near the border outwards: predicted points within r2 of every edge and
    corner, and outside the image.  Textureless reference, fresh features: rectangle, segment and green ring each."""
    from flame_amd import synth_stereo as ss

    w, h = 320, 240
    sc = ss.PlaneScene(w, h, 3, normal=(0.0, 0.0, 1.0), distance=2.0)
    sc.add_camera(10, np.eye(3), [0, 0, 0])
    sc.add_camera(11, np.eye(3), [0.0, 0.0, -0.01])
    sc.add_camera(12, np.eye(3), [0.0, 0.0, -0.09])
    pts = []
    for d in (4.25, 5.5, 7.0, 9.5):
        for x in np.arange(d, w - d + 0.1, 13.0):
            pts += [(x, d), (x, h - 1 - d)]
        for y in np.arange(d, h - d + 0.1, 11.0):
            pts += [(d, y), (w - 1 - d, y)]
        pts += [(w - 1 - d, h - 1 - d), (w - 1 - d, d), (d, h - 1 - d)]
    xy = np.array(pts, F)
    f = np.zeros(xy.shape[0], so.FEATURE_DTYPE)
    f["id"] = np.arange(f.shape[0])
    f["frame_id"] = 10
    f["x"], f["y"] = xy[:, 0], xy[:, 1]
    f["idepth_mu"] = sc.true_idepth(10, xy).astype(F)
    f["idepth_var"] = 0.25
    f["valid"] = 1
    f["num_dropouts"][::3] = 5
    blank = np.full((h, w), 60, np.uint8)
    return dict(width=w, height=h, pad=5, K=sc.K32, Kinv=sc.Kinv32, imgs={10: blank, 11: blank, 12: sc.render(12)},
                poses=ss.poses_for(sc, [10, 11], 12, 11), feats=f, pkw={}, curr_pf=11, new=12)


def _case_overflow():
    """About 5 k fresh features on a textureless reference at 320x240: more entries than the first entry buffer holds."""
    c = _case_textureless(320, 240, 2600)
    c["feats"]["idepth_var"] = 0.25
    c["feats"]["num_updates"] = 0
    return c


def _case_success():
    """A frame where every feature succeeds: the features of the plain scene that the checker updates."""
    c = _scene(320, 240, 150, 3)
    out = run_checker(c, draw=False)
    keep = (out["feats"]["num_updates"] == 1) & (c["feats"]["frame_id"] == out["feats"]["frame_id"])
    c["feats"] = np.ascontiguousarray(c["feats"][keep])
    return c


def _case_empty():
    c = _scene(320, 240, 4, 3)
    c["feats"] = c["feats"][:0].copy()
    return c


CASES = {
    "scene": _case_scene, "variants": _case_variants, "move": _case_move, "textureless": _case_textureless, "stripes": _case_stripes,
    "altered": _case_altered, "order": _case_order, "clip": _case_clip,
    "scene640": lambda: _case_scene(640, 480), "textureless640": lambda: _case_textureless(640, 480, 150),
    "move640": lambda: _case_move(640, 480, 150),
    "small": lambda: _case_textureless(160, 120, 60), "wide": lambda: _case_textureless(1280, 120, 100),
    "overflow": _case_overflow, "success": _case_success, "empty": _case_empty,
}
KIND_CASES = ("scene", "variants", "move", "textureless", "stripes", "altered")  # every kind of draw, at 320x240
KIND_CASES_640 = ("scene640", "textureless640", "move640")                       # ... and once at 640x480 (r1 = 2, r2 = 8)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def _frames(c):
    frames = [dict(p, img_pad=so.make_frame(c["imgs"][p["id"]], c["pad"])[0]) for p in c["poses"]]
    return frames, so.make_frame(c["imgs"][c["new"]], c["pad"])


def run_checker(c, feats=None, flip=False, draw=True, trace=None):
    """tests/matches_ref.py on a case (or on another feature array for it); the result carries the updated records as `feats`."""
    frames, newf = _frames(c)
    out = (c["feats"] if feats is None else feats).copy()
    res = mr.update_and_draw(so.Params(**c["pkw"]), c["K"], c["Kinv"], c["width"], c["height"], c["pad"], frames, newf,
                             c["imgs"][c["new"]], c["curr_pf"], out, flip=flip, draw=draw, trace=trace)
    res["feats"] = out
    return res


@functools.lru_cache(maxsize=None)
def reference(name, reverse=False):
    """The checker's picture, counters and records of a case, computed once; the arrays are read-only."""
    c = case(name)
    res = run_checker(c, feats=c["feats"][::-1].copy() if reverse else None)
    res["img"].setflags(write=False)
    res["feats"].setflags(write=False)
    return res


# ---- the primitives ------------------------------------------------------------------------------------------------------------

RING_OCTANTS = {0: [(0, 0)], 1: [(1, 0)], 2: [(2, 0), (1, 1)], 4: [(4, 0), (3, 1), (3, 2)],
                8: [(8, 0), (7, 1), (7, 2), (7, 3), (6, 4), (6, 5)]}
RING_TOTALS = {0: 1, 1: 4, 2: 8, 4: 20, 8: 44, 24: 132}


def _from_octant(pts):
    out = set()
    for dx, dy in pts:
        for a, b in ((dx, dy), (dy, dx)):
            out |= {(a, b), (-a, b), (a, -b), (-a, -b)}
    return out


@pytest.mark.parametrize("r", sorted(RING_TOTALS))
def test_ring_known_answers(r):
    pts = mr.ring_points(100, 50, r)
    assert len(pts) == len(set(pts)) == RING_TOTALS[r], "each pixel once"
    if r in RING_OCTANTS:
        assert set(pts) == {(100 + a, 50 + b) for a, b in _from_octant(RING_OCTANTS[r])}
    assert {(2 * 100 - x, y) for x, y in pts} == set(pts) and {(x, 2 * 50 - y) for x, y in pts} == set(pts)
    assert {(100 + (y - 50), 50 + (x - 100)) for x, y in pts} == set(pts)


def _literal_ring(cx, cy, r):
    """The rule as include/flame_stereo.h words it: all eight points of every step, coinciding ones included."""
    out = []
    err, dx, dy, plus, minus = 0, r, 0, 1, 2 * r - 1
    while dx >= dy:
        out += [(cx + dx, cy + dy), (cx - dx, cy + dy), (cx + dx, cy - dy), (cx - dx, cy - dy),
                (cx + dy, cy + dx), (cx - dy, cy + dx), (cx + dy, cy - dx), (cx - dy, cy - dx)]
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return out


@pytest.mark.parametrize("r", range(0, 65))
def test_ring_is_the_eight_point_rule_with_coinciding_points_once(r):
    """Every radius up to 64 (a 5120-column image): plotting each pixel once, as the checker and the kernels do, gives the pixel set
    of the literal eight-point rule, so `entries` is the number of distinct pixels a ring touches."""
    pts, lit = mr.ring_points(7, -3, r), _literal_ring(7, -3, r)
    assert len(pts) == len(set(pts)) and set(pts) == set(lit)
    for x, y in pts:  # an outline of radius r: within one pixel of the circle
        assert abs(np.hypot(x - 7, y + 3) - r) < 1.0


# centres on each corner, on each edge and one pixel outside, in a 40 x 30 image
CLIP_CENTRES = [(0, 0), (39, 0), (0, 29), (39, 29), (20, 0), (20, 29), (0, 15), (39, 15), (-1, -1), (40, -1), (-1, 30), (40, 30),
                (20, -1), (20, 30), (-1, 15), (40, 15), (-5, 15), (20, 34), (-9, -9), (10 ** 9, 3), (3, -2 ** 31)]


@pytest.mark.parametrize("centre", CLIP_CENTRES)
def test_ring_and_rectangle_clipping(centre):
    cx, cy = centre
    img = np.zeros((30, 40, 3), np.int32)
    n = mr.draw_ring(img, cx, cy, 4, (1, 2, 3))
    want = {(x, y) for x, y in ((cx + a, cy + b) for a, b in _from_octant(RING_OCTANTS[4])) if 0 <= x < 40 and 0 <= y < 30}
    got = {(int(x), int(y)) for y, x in zip(*np.nonzero(img[:, :, 0]))}
    assert got == want and n == len(want)
    for r in (0, 1, 2):
        img = np.zeros((30, 40, 3), np.int32)
        n = mr.fill_rect(img, cx, cy, r, (1, 2, 3))
        want = {(x, y) for x in range(cx - r, cx + r + 1) for y in range(cy - r, cy + r + 1) if 0 <= x < 40 and 0 <= y < 30} \
            if abs(cx) < 1000 and abs(cy) < 1000 else set()
        got = {(int(x), int(y)) for y, x in zip(*np.nonzero(img[:, :, 0]))}
        assert got == want and n == len(want)


def test_blend_is_the_shifted_sum_for_every_byte_pair():
    """colour * 0.5f + pixel * (1.0f - 0.5f), stored into a uchar (visualization.h:255-257): both products and the sum are exact in
    float, so the truncation equals (colour + pixel) >> 1."""
    c, v = np.meshgrid(np.arange(256), np.arange(256))
    as_float = (c.astype(F) * F(0.5) + v.astype(F) * (F(1.0) - F(0.5))).astype(np.uint8)
    assert np.array_equal(as_float, ((c + v) >> 1).astype(np.uint8))
    assert np.array_equal(mr.blend(v, c), (c + v) >> 1)


def test_center_truncates_and_saturates():
    assert mr.center(F(3.49), F(3.5)) == (3, 4)
    assert mr.center(F(-0.4), F(-0.6)) == (0, 0) and mr.center(F(-1.6), F(-2.5)) == (-1, -2)  # C truncation, not floor
    assert mr.center(F(1e20), F(-1e20)) == (2 ** 31 - 1, -2 ** 31)
    assert mr.center(F("nan"), F("inf")) == (0, 2 ** 31 - 1)


# ---- the checker against the oracle, and what the cases cover ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_checker_control_flow_matches_the_oracle(name):
    """The records the sequential walk ends with are those of the oracle's stereo_update_feature_idepths, record for record."""
    c = case(name)
    frames, newf = _frames(c)
    want = c["feats"].copy()
    rc, stats = so.update_feature_idepths(so.Params(**c["pkw"]), c["K"], c["Kinv"], c["width"], c["height"], c["pad"], frames, newf,
                                          c["curr_pf"], want)
    res = reference(name)
    assert rc == 0 and res["rc"] == 0
    assert [int(v) for v in res["stats"]] == [int(v) for v in stats]
    assert res["feats"].tobytes() == want.tobytes()
    # the invariants the GPU tests repeat on the library's counters
    assert res["kind_count"][mr.GREEN] + res["green_skipped"] == stats[1]
    assert res["kind_count"][mr.BLUE] + res["blue_skipped"] == stats[2]
    assert res["rings_skipped"] == res["green_skipped"] + res["blue_skipped"]


def test_cases_cover_every_kind_of_draw():
    """What keeps the GPU tests from passing on empty pictures: over the cases taken together every kind is drawn at least three times
    and at least ten segments are blended; every kind occurs at 320x240 and once at 640x480."""
    for names in (sorted(CASES), KIND_CASES, KIND_CASES_640):
        total = np.sum([reference(n)["kind_count"] for n in names], axis=0)
        lines = sum(reference(n)["lines_drawn"] for n in names)
        assert total.min() >= 3 and lines >= 10, (names, total, lines)
    for n in CASES:
        assert case(n)["width"] // 320 == (2 if n in KIND_CASES_640 else 0 if n == "small" else 4 if n == "wide" else 1)
    assert reference("success")["kind_count"] == [0] * 9 and reference("success")["stats"][0] == case("success")["feats"].shape[0] > 50
    assert np.array_equal(reference("success")["img"][:, :, 0], case("success")["imgs"][12]) and reference("success")["entries"] == 0
    assert reference("overflow")["entries"] > 2 * 320 * 240 and 4500 < case("overflow")["feats"].shape[0] < 5500


def _pixels(entry, r1, r2):
    _, _, what, g = entry
    if what == "rect":
        return {(x, y) for x in range(g[0] - r1, g[0] + r1 + 1) for y in range(g[1] - r1, g[1] + r1 + 1)}
    if what == "line":
        return set(mr.walk(*g))
    return set(mr.ring_points(g[0], g[1], r2))


def test_order_case_depends_on_the_order():
    """The order case holds a segment that crosses a LATER rectangle, a rectangle under a LATER segment and two segments of different
    colours that share a pixel; its picture with the feature array reversed differs from the forward one."""
    trace = []
    run_checker(case("order"), trace=trace)
    rects = [(e, _pixels(e, 1, 4)) for e in trace if e[2] == "rect"]
    lines = [(e, _pixels(e, 1, 4)) for e in trace if e[2] == "line"]
    assert any(le[0] < re[0] and le[0] // 4 != re[0] // 4 and lp & rp for le, lp in lines for re, rp in rects)
    assert any(re[0] < le[0] and le[0] // 4 != re[0] // 4 and lp & rp for le, lp in lines for re, rp in rects)
    assert any(a[1] != b[1] and pa & pb for a, pa in lines for b, pb in lines if a[0] < b[0])
    fwd, rev = reference("order"), reference("order", True)
    assert fwd["kind_count"] == rev["kind_count"] and fwd["entries"] == rev["entries"]
    assert not np.array_equal(fwd["img"], rev["img"])


def test_clip_case_reaches_every_edge_and_corner():
    """Ring centres (radius 4) within r2 of every edge and corner of the image, and outside it."""
    trace = []
    run_checker(case("clip"), trace=trace)
    w, h, r2 = 320, 240, 4
    cen = [e[3] for e in trace if e[2] == "ring"]
    near = dict(left=lambda x, y: 0 <= x < r2, right=lambda x, y: w - r2 <= x < w, top=lambda x, y: 0 <= y < r2,
                bottom=lambda x, y: h - r2 <= y < h)
    for name, fn in near.items():
        assert sum(fn(x, y) and 0 <= x < w and 0 <= y < h for x, y in cen) >= 3, name
    for a, b in (("left", "top"), ("right", "top"), ("left", "bottom"), ("right", "bottom")):
        assert any(near[a](x, y) and near[b](x, y) for x, y in cen), (a, b)
    assert sum(not (0 <= x < w and 0 <= y < h) for x, y in cen) >= 3
    rc = [e[3] for e in trace if e[2] == "rect"]
    assert sum(not (0 <= x < w and 0 <= y < h) for x, y in rc) >= 1 and sum(x in (0, w - 1) or y in (0, h - 1) for x, y in rc) >= 1


def test_flip_reverses_the_pixel_order():
    c = case("order")
    a, b = reference("order")["img"], run_checker(c, flip=True)["img"]
    assert np.array_equal(b.reshape(-1, 3), a.reshape(-1, 3)[::-1])
