"""Flame::projectGraph and the rescale_data block on the device state (k_project_graph, k_block_sum + k_rescale_apply:
flame_nltgv2_project_graph, flame_nltgv2_rescale_data) at their edges.

CPU: the checker (oracle/photometric_oracle.c: graph_project, graph_rescale) against float64 statements of the two operations
  written from their definitions (tests/maint_ref64.py), within bounds derived from the operations' roundings: a camera with
  fx != fy and an off-centre principal point, rotation about two axes, forward, backward, lateral and behind-the-camera
  motion and a roll about z; sums of V = 1 ... 3000 terms, random, of mixed sign, equal, zero, one huge among small ones.
GPU: bit for bit with the checker (NaN as NaN), at V = 0, 1, 255, 256, 257 and 1500 for the projection and V = 1, 2, 1023, 1024,
  1025, 2049, 3000 for the rescale.  The 1500-vertex graph carries an edge grid: vertices whose projection falls exactly on
  each of the four lines of the region and one float32 ulp either side (the region is made from projected coordinates, its
  rows offset as the letterbox call site's are), and x = 0, -0, the smallest denormal, a value whose product with the scale
  underflows to 0, negative, NaN, very large, and the depth that puts the vertex at z = 0 in the other camera.  Paths: a
  settled context with and without pos_out, two projections without a sync between them, and the call behind run_async
  chains in every form of option 5 -- each followed by solver steps in that form, which must equal the checker's steps on the
  projected graph."""
import ctypes as C
import math

import numpy as np
import pytest

from flame_amd import synth
from oracle import capi as oracle
from tests import maint_ref64 as m64
from tests.helpers import random_graph
from tests.test_graph_maintenance import quat_wxyz_from_rot
from tests.test_photometric_edges import MOTIONS as PHOTO_MOTIONS
from tests.test_photometric_edges import camera, scene

F = np.float32
EPS32 = float(np.finfo(np.float32).eps)
FORMS = [0, 1, 3, 4, 6]
ALL_STATE = ("x", "w1", "w2", "x_bar", "w1_bar", "w2_bar", "x_prev", "w1_prev", "w2_prev", "q1", "q2", "q3")


def _rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


MOTIONS = dict(PHOTO_MOTIONS)
MOTIONS["roll"] = (_rot_z(0.05), np.array([0.01, -0.02, 0.015]))


def geometry(K, R, t):
    """What the call takes, each the float32 rounding of its float64 value."""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    Kinv = np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]])
    return dict(K=K.astype(F), Kinv=Kinv.astype(F), KRKinv=(K @ R @ Kinv).astype(F), q=quat_wxyz_from_rot(R), t=np.asarray(t, F))


def checker_project(pos, x, gs, geo, region):
    """-> (keep, new pos, new x) of oracle.graph_project on copies."""
    pos, x = np.array(pos, F, copy=True), np.array(x, F, copy=True)
    keep = oracle.graph_project(pos, x, float(gs), geo["K"], geo["Kinv"], geo["q"], geo["t"], geo["KRKinv"], region)
    return keep, pos, x


def same_bits(got, want, what):
    """Bit for bit, NaN as NaN (the payload of a NaN is not compared: the default NaN's sign differs between x86 and the device)."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    bad = (gn != wn) | (~wn & ~gn & (got.view(np.uint32) != want.view(np.uint32)))
    assert not bad.any(), (what, np.flatnonzero(bad)[:8], got.ravel()[np.flatnonzero(bad)[:8]], want.ravel()[np.flatnonzero(bad)[:8]])


def same_state(got, want, what, keys=ALL_STATE):
    for k in keys:
        same_bits(got[k], want[k], (what, k))


# ---- CPU: the float64 statements on their own ------------------------------------------------------------------------------------
def test_float64_statements_known_answers():
    """Answers that a swapped axis, a transposed rotation, a mirrored quaternion or an off-by-one region gets wrong."""
    K = np.array([[128.0, 0, 32.0], [0, 256.0, 48.0], [0, 0, 1]])  # (powers of two: K and its inverse are exact in float32)
    ident = geometry(K, np.eye(3), np.zeros(3))
    region = (10.0, 20.0, 40.0, 30.0)  # [10, 50) x [20, 50)
    pos = np.array([[40.0, 30.0], [10.0, 20.0], [50.0, 30.0], [30.0, 50.0], [49.5, 49.5], [9.5, 30.0]], F)
    x = np.full(len(pos), 0.5, F)
    r = m64.project64(pos, x, 2.0, region=region, **ident)  # idepth 1
    assert np.allclose(r["pos"], pos, atol=1e-12) and np.allclose(r["x"], 0.5) and np.allclose(r["z"], 1.0)
    assert r["keep"].tolist() == [True, True, False, False, True, False]  # the lower lines belong to the region, the upper do not
    # a step to the right in the other camera moves x only, by fx t_x idepth; a step down y only, by fy t_y idepth
    r = m64.project64(pos[:1], [0.5], 1.0, region=region, **geometry(K, np.eye(3), np.array([0.2, 0.0, 0.0])))
    assert np.allclose(r["pos"], [[40.0 + 128 * 0.2 * 0.5, 30.0]], atol=1e-5)
    r = m64.project64(pos[:1], [0.5], 1.0, region=region, **geometry(K, np.eye(3), np.array([0.0, 0.1, 0.0])))
    assert np.allclose(r["pos"], [[40.0, 30.0 + 256 * 0.1 * 0.5]], atol=1e-5)
    # backing off by 2 from a point at depth 2: idepth 1/4, the pixel pulled halfway to the principal point
    r = m64.project64(pos[:1], [0.5], 1.0, region=region, **geometry(K, np.eye(3), np.array([0.0, 0.0, 2.0])))
    assert np.allclose(r["pos"], [[36.0, 39.0]], atol=1e-5) and np.allclose(r["idepth"], 0.25) and r["keep"][0]
    r = m64.project64(pos[:1], [0.5], 1.0, region=region, **geometry(K, np.eye(3), np.array([0.0, 0.0, -3.0])))
    assert r["z"][0] == pytest.approx(-1.0) and r["idepth"][0] < 0 and not r["keep"][0]  # behind: never kept
    # a quarter roll about z takes the ray (a, 0, 1) to (0, a, 1): q = (w, x, y, z), counter-clockwise for x -> y
    quarter = geometry(K, _rot_z(np.pi / 2), np.zeros(3))
    assert np.allclose(quarter["q"], [math.sqrt(0.5), 0, 0, math.sqrt(0.5)], atol=1e-6)
    assert np.allclose(m64.rotation_from_quaternion(quarter["q"]), _rot_z(np.pi / 2), atol=1e-6)
    for xv in (0.5, 0.0):  # finite depth and at infinity (the homography)
        r = m64.project64(np.array([[32.0 + 128 * 0.3, 48.0]], F), [xv], 1.0, region=region, **quarter)
        assert np.allclose(r["pos"], [[32.0, 48.0 + 256 * 0.3]], atol=1e-4), xv
    assert r["at_inf"][0] and r["x"][0] == 0.0
    # -0.0 is at infinity too
    assert m64.project64(pos[:1], [-0.0], 1.0, region=region, **ident)["at_inf"][0]
    # rescale: the mean of data * scale; the four arrays times scale / mean; data_factor times mean / scale
    s = m64.rescale64([1, 1, 1], [2, 2, 2], [4, 4, 4], [1, 2, 3], 2.0, 0.1)
    assert s["new_scale"] == 4.0 and s["mean_abs"] == 4.0 and s["data_factor"] == pytest.approx(0.1 * 2.0, rel=1e-7)
    assert s["x"].tolist() == [0.5] * 3 and s["x_bar"].tolist() == [1.0] * 3 and s["x_prev"].tolist() == [2.0] * 3
    assert s["data_term"].tolist() == [0.5, 1.0, 1.5]
    assert m64.rescale64([1], [1], [1], [3, -3, 1, -1], 1.0, 0.1)["mean_abs"] == 2.0


@pytest.mark.parametrize("motion", sorted(MOTIONS))
def test_checker_projection_against_float64_statement(motion):
    """oracle.graph_project within m64.project_bound (derived there, doubled) of m64.project64 in position and new x, on about
    3000 vertices; its keep mask equal to the float64 one for every vertex further than the bound from all four region lines
    and with |z| further than its bound from 0.  So that the bound cannot hide a failure: the vertices that are not live
    (a bound that is not finite, or above 0.25 px) stay under 20 % of the scene."""
    rows, cols, gs = 479, 641, F(1.25)
    R, t = MOTIONS[motion]
    geo = geometry(camera(rows, cols), R, t)
    pos, x = scene(rows, cols, 5)
    x = (x / gs).astype(F)
    region = (3.0, 40.0, cols - 6.0, rows - 80.0)  # (every sum of the region is exact in float32)
    keep32, pos32, x32 = checker_project(pos, x, gs, geo, region)
    r = m64.project64(pos, x, gs, region=region, **geo)
    b_pos, b_x, b_z = m64.project_bound(pos, x, gs, **geo)
    live = np.isfinite(b_pos).all(1) & (b_pos < 0.25).all(1)
    assert (~live).sum() < 0.2 * len(x), (~live).sum()
    dev, dev_x = np.abs(pos32 - r["pos"]), np.abs(x32 - r["x"])
    ratio = float((dev[live] / b_pos[live]).max())
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio_x = float(np.nanmax(np.where(b_x[live] > 0, dev_x[live] / b_x[live], 0.0)))
    print(f"projection checker vs float64: {motion}: max deviation / bound = {ratio:.3f} (position), {ratio_x:.3f} (x); "
          f"not live {int((~live).sum())} of {len(x)}")
    assert (dev[live] <= b_pos[live]).all(), (motion, ratio)
    assert (dev_x[live] <= b_x[live]).all(), (motion, ratio_x)
    assert (x32[r["at_inf"]] == 0).all() and r["at_inf"].sum() > 50
    lines = np.array([[region[0], region[1]], [region[0] + region[2], region[1] + region[3]]])
    with np.errstate(invalid="ignore"):
        near = ((np.abs(r["pos"] - lines[0]) <= b_pos) | (np.abs(r["pos"] - lines[1]) <= b_pos)).any(1) | (np.abs(r["z"]) <= b_z)
    assert (~near).sum() > 0.8 * len(x)
    differ = keep32.astype(bool) != r["keep"]
    assert not (differ & ~near).any(), np.flatnonzero(differ & ~near)[:10]
    assert np.array_equal(keep32.astype(bool)[~near], r["keep"][~near])
    if motion == "behind":
        assert ((r["z"] < 0) & (x > 0)).sum() > 100 and not r["keep"][(r["z"] < 0) & (x > 0) & ~near].any()
    else:
        assert r["keep"].sum() > 0.5 * len(x)


RESCALE_V = [1, 2, 1023, 1024, 1025, 2049, 3000]
RESCALE_SCALES = [1e-30, 1.0, 1e30]
RESCALE_KINDS = ["random", "mixed", "equal", "zero", "huge"]


def rescale_data_term(kind, V, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.uniform(0.2, 3.0, V).astype(F)
    if kind == "mixed":
        return (rng.uniform(0.2, 3.0, V) * rng.choice([-1.0, 1.0], V)).astype(F)
    if kind == "equal":
        return np.full(V, 0.7, F)
    if kind == "zero":
        return np.zeros(V, F)
    d = rng.uniform(1e-3, 3e-3, V).astype(F)  # "huge": one huge value among small ones
    d[(V * 2) // 3] = 1e6
    return d


def rescale_graph(V, kind, seed):
    """A random graph whose state arrays are all different and non-trivial, so that an array scaled by mistake shows."""
    g = random_graph(V, min(3 * V, V * (V - 1) // 2), seed)
    rng = np.random.default_rng(seed + 1)
    g["data_term"] = rescale_data_term(kind, V, seed + 2)
    for k in ("x", "x_bar", "x_prev", "w1", "w2", "w1_bar", "w2_bar", "w1_prev", "w2_prev"):
        g[k] = rng.uniform(-1.0, 2.0, V).astype(F)
    for k in ("q1", "q2", "q3"):
        g[k] = rng.uniform(-1.0, 1.0, g["E"]).astype(F)
    return g


@pytest.mark.parametrize("V", RESCALE_V)
def test_checker_rescale_against_float64_statement(V):
    """oracle.graph_rescale: new_scale within (ceil(V / 1024) + 12) eps32 mean|data_term * graph_scale| of the correctly
    rounded mean (the strided sum's depth: V / 1024 sequential additions and 10 pairwise levels, the product and the division);
    x, x_bar, x_prev, data_term within 3 eps32 |value| of their float64 value for the new_scale the checker itself returned
    (two roundings each; how far that new_scale is from the mean is the first check); data_factor likewise; w1, w2, q1, q2,
    q3 and the other arrays untouched."""
    worst = 0.0
    for kind in RESCALE_KINDS:
        for gs in RESCALE_SCALES:
            g = rescale_graph(V, kind, 100 + V)
            before = synth.copy_graph(g)
            with np.errstate(all="ignore"):
                ns, df = oracle.graph_rescale(g, gs, 0.1)
            s = m64.rescale64(before["x"], before["x_bar"], before["x_prev"], before["data_term"], gs, 0.1)
            bound = (math.ceil(V / 1024) + 12) * EPS32 * s["mean_abs"]
            assert abs(ns - s["new_scale"]) <= bound, (kind, gs, ns, s["new_scale"], bound)
            if bound > 0:
                worst = max(worst, abs(ns - s["new_scale"]) / bound)
            for k in before:
                if isinstance(before[k], np.ndarray) and k not in ("x", "x_bar", "x_prev", "data_term"):
                    assert np.array_equal(g[k].view(np.uint32), before[k].view(np.uint32)), k
            if kind == "zero":
                assert ns == 0.0 and df == 0.0
                continue
            s = m64.rescale64(before["x"], before["x_bar"], before["x_prev"], before["data_term"], gs, 0.1, new_scale=ns)
            for k in ("x", "x_bar", "x_prev", "data_term"):
                assert (np.abs(g[k] - s[k]) <= 3 * EPS32 * np.abs(s[k])).all(), (kind, gs, k)
            assert abs(df - s["data_factor"]) <= 3 * EPS32 * abs(s["data_factor"])
    print(f"rescale checker vs float64: V = {V}: max |new_scale - mean| / bound = {worst:.3f}")


# ---- GPU: the projection ----------------------------------------------------------------------------------------------------------
ROWS, COLS = 120, 160
DENORM = np.float32(1e-45)  # the smallest denormal
NOMINAL = ((12.0, COLS - 12.0), (20.0, ROWS - 22.0))  # about where the region's lines go: x, then y (rows offset: a letterbox)


def _ulps(v, k):
    v = F(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F(np.inf if k > 0 else -np.inf))
    return v


def _move_onto(pos, x, b, axis, target, gs, geo):
    """Moves vertex b along `axis` (and its x by a few ulps) until the checker projects it onto `target` exactly; False if
    no such place is found near it (the caller takes another vertex)."""
    anywhere = (0.0, 0.0, 1.0, 1.0)
    p, xb = pos[b:b + 1].copy(), x[b:b + 1].copy()
    for _ in range(8):  # Newton steps, the slope from a second point half a pixel on
        two = np.repeat(p, 2, 0)
        two[1, axis] += F(0.5)
        cb = checker_project(two, np.repeat(xb, 2), gs, geo, anywhere)[1][:, axis].astype(np.float64)
        p[0, axis] = F(p[0, axis] + (float(target) - cb[0]) / ((cb[1] - cb[0]) / 0.5))
    # ... then in steps of a quarter of the target's ulp in the coordinate (or the coordinate's own ulp, if coarser), ulp by ulp in x
    kp, kx = np.arange(-64, 65), np.arange(-24, 25)
    steps = np.unique((p[0, axis] + kp * float(np.spacing(target)) / 4).astype(F))
    cand_p = np.repeat(p, len(steps) * len(kx), 0)
    cand_p[:, axis] = np.repeat(steps, len(kx))
    cand_x = np.tile(np.array([_ulps(xb[0], k) for k in kx], F), len(steps))
    hit = np.flatnonzero(checker_project(cand_p, cand_x, gs, geo, anywhere)[1][:, axis] == target)
    if len(hit):
        pos[b], x[b] = cand_p[hit[0]], cand_x[hit[0]]
    return bool(len(hit))


def place_on_lines(pos, x, gs, geo):
    """Moves vertices so that, projected by the checker, one lies exactly on each of the four region lines and one a float32
    ulp either side of it.  The lower lines are projected coordinates of vertices of the scene, the upper ones the float32
    sum of the lower line and the extent: -> (pos, x, region, {(axis, side): [line, vertex on it, vertex one ulp below,
    vertex one ulp above]}, the vertices used)."""
    pos, x = pos.copy(), x.copy()
    _, c, xn = checker_project(pos, x, gs, geo, (0.0, 0.0, 1.0, 1.0))
    free = np.isfinite(c).all(1) & (x * gs > 0.2) & (xn * gs > 0.05) & (xn * gs < 10)  # (in front of both cameras, not too near)
    placed, used = {}, []
    for axis in (0, 1):
        other_ok = (c[:, 1 - axis] > NOMINAL[1 - axis][0] + 8) & (c[:, 1 - axis] < NOMINAL[1 - axis][1] - 8)
        for side, nominal in enumerate(NOMINAL[axis]):
            order = [v for v in np.argsort(np.abs(c[:, axis] - nominal)) if free[v] and other_ok[v]][:30]
            if side == 0:  # the lower line is where a vertex of the scene projects to ...
                line, group = c[order[0], axis], [order.pop(0)]
            else:  # ... the upper one is lower line + extent in float32, and all three vertices are moved
                line, group = F(placed[(axis, 0)][0] + F(NOMINAL[axis][1] - NOMINAL[axis][0])), []
            targets = ([] if side == 0 else [line]) + [np.nextafter(line, F(-np.inf)), np.nextafter(line, F(np.inf))]
            for target in targets:
                while order and not _move_onto(pos, x, order[0], axis, target, gs, geo):
                    order.pop(0)
                assert order, ("no vertex found that projects onto", axis, side, target)
                group.append(order.pop(0))
            placed[(axis, side)] = [line] + group
            free[group] = False
            used += group
    region = (float(placed[(0, 0)][0]), float(placed[(1, 0)][0]), NOMINAL[0][1] - NOMINAL[0][0], NOMINAL[1][1] - NOMINAL[1][0])
    return pos, x, region, placed, np.array(used)


def special_x(gs):
    """The x of the edge grid and whether the projection of each stays finite whatever the motion (x = 0.5 / scale is the
    depth 2 that t_z = -2 takes to z = 0)."""
    return np.array([0.0, -0.0, DENORM, 3 * DENORM, -0.3, -2.0, np.nan, 2.0e4, 1e30, 3e38, 0.5 / float(gs)], F)


def projection_scene(V, seed, gs, geo, grid=True, finite_only=False):
    """-> (graph, region, placed, slots of the special x).  V vertices over the image and a margin, depths 0.4 ... 3.3; with
    grid: the line vertices and the special x (finite_only: specials whose projection is not finite, or that the solver cannot
    hold, are put back to 0.7)."""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-4, COLS + 4, V), rng.uniform(-4, ROWS + 4, V)], 1).astype(F)
    x = (1.0 / rng.uniform(0.4, 3.3, V) / float(gs)).astype(F)
    region, placed, slots = (NOMINAL[0][0], NOMINAL[1][0], NOMINAL[0][1] - NOMINAL[0][0], NOMINAL[1][1] - NOMINAL[1][0]), {}, np.zeros(0, int)
    if grid:
        pos, x, region, placed, used = place_on_lines(pos, x, gs, geo)
        rest = np.setdiff1d(np.arange(V), used)
        sp = special_x(gs)
        slots = rest[np.arange(3 * len(sp)) * 7 % len(rest)]
        assert len(np.unique(slots)) == len(slots)
        x[slots] = np.tile(sp, 3)
        if finite_only:
            _, c, xn = checker_project(pos, x, gs, geo, region)
            bad = ~(np.isfinite(c).all(1) & np.isfinite(xn)) | (np.abs(x) > 1e6)  # (data_weight * 1e30 is beyond float32: the solver's own limit)
            assert not bad[used].any() and bad.sum() <= 3 * 7
            x[bad] = 0.7
    elif V:
        x[0] = 0.0
    if V >= 1000:
        edges = synth.delaunay_edges_native(pos)
    else:
        r = random_graph(V, min(3 * V, V * (V - 1) // 2), seed, width=float(COLS))
        edges = np.stack([r["src"], r["dst"]], 1).astype(np.int32).reshape(-1, 2)
        edges = edges[(pos[edges[:, 0]] != pos[edges[:, 1]]).any(1)] if len(edges) else edges
    # data_weight 1e30: every primal step lands x on data_term exactly, so that the special x (and the line vertices' x, ulp for
    # ulp) are what the projection meets after any number of solver steps
    g = synth.assemble_graph(pos, x, edges, weight=np.full(V, 1e30, F))
    return g, region, placed, slots


def assert_grid_hit_the_lines(g, gs, geo, region, placed):
    """The construction did what it says: on, one ulp below and one ulp above each line, kept as the rule [lo, hi) has it."""
    keep, c, _ = checker_project(g["pos"], g["x"], gs, geo, region)
    lines = {(0, 0): F(region[0]), (1, 0): F(region[1]), (0, 1): F(F(region[0]) + F(region[2])), (1, 1): F(F(region[1]) + F(region[3]))}
    for (axis, side), (line, on, below, above) in placed.items():
        assert lines[(axis, side)] == line
        assert c[on, axis] == line and c[below, axis] == np.nextafter(line, F(-np.inf)) and c[above, axis] == np.nextafter(line, F(np.inf))
        assert [int(keep[on]), int(keep[below]), int(keep[above])] == ([1, 0, 1] if side == 0 else [0, 1, 0]), (axis, side)
    assert region[1] > 4.0  # (a row offset)


def call_project(reg, geo, region, gs, want_pos=True, null_projection=False):
    """flame_nltgv2_project_graph as it is (Regularizer.project_graph always asks for the positions) -> (status, keep, pos)."""
    from flame_amd.regularizer import _FP, _Projection

    pr = _Projection()
    for name, key, n in (("K", "K", 9), ("Kinv", "Kinv", 9), ("KRKinv", "KRKinv", 9), ("q_ref_to_cmp", "q", 4), ("t_ref_to_cmp", "t", 3)):
        setattr(pr, name, (C.c_float * n)(*np.asarray(geo[key], F).reshape(n).tolist()))
    pr.region_x, pr.region_y, pr.region_w, pr.region_h = [float(r) for r in region]
    keep = np.full(reg.V, 7, np.uint8)
    pos = np.full((reg.V, 2), -777.0, F)
    rc = reg._L.flame_nltgv2_project_graph(reg._ctx, None if null_projection else C.byref(pr), C.c_float(float(gs)),
                                           keep.ctypes.data_as(C.POINTER(C.c_uint8)), pos.ctypes.data_as(_FP) if want_pos else None)
    return rc, keep, (pos if want_pos else None)


def ref_project(ref, gs, geo, region):
    return oracle.graph_project(ref["pos"], ref["x"], float(gs), geo["K"], geo["Kinv"], geo["q"], geo["t"], geo["KRKinv"], region)


GPU_MOTIONS = sorted(MOTIONS)
Z_ZERO = (np.eye(3), np.array([0.01, 0.0, -2.0]))  # identity rotation: the vertex at depth 2 lands on z = 0 exactly


def gpu_geometry(motion):
    R, t = Z_ZERO if motion == "z_zero" else MOTIONS[motion]
    return geometry(camera(ROWS, COLS), R, t)


def wide_params(flame_amd):
    return flame_amd.Params(x_min=-1e6, x_max=1e6), oracle.make_params(x_min=-1e6, x_max=1e6)


@pytest.mark.gpu
@pytest.mark.parametrize("motion", GPU_MOTIONS + ["z_zero"])
def test_gpu_projection_edge_grid_settled(built, motion):
    """The full edge grid (non-finite results included) on a settled context: with pos_out; without it, followed at once --
    no sync in between -- by a second projection whose pos_out shows both (the first call keeps the old positions as the
    layout's, the second in the undo buffer); keep, positions and the downloaded state bit for bit with the checker."""
    import torch  # noqa: F401

    import flame_amd

    gs = F(1.25) if motion == "z_zero" else (F(1.25), F(0.4))[GPU_MOTIONS.index(motion) % 2]
    geo = gpu_geometry(motion)
    g, region, placed, slots = projection_scene(1500, 11, gs, geo)
    assert_grid_hit_the_lines(g, gs, geo, region, placed)
    sp = special_x(gs)
    idepth = g["x"][slots[:len(sp)]] * gs
    assert idepth[10] == 0.5 and np.isnan(idepth[6]) and idepth[9] > 1e38 and np.signbit(idepth[1]) and idepth[1] == 0
    if gs < 1:
        assert idepth[2] == 0 and g["x"][slots[2]] != 0 and idepth[3] != 0  # the product underflows to 0 / stays a denormal
    else:
        assert 0 < idepth[2] < 1e-44
    other = gpu_geometry(GPU_MOTIONS[(GPU_MOTIONS.index(motion) + 1) % len(GPU_MOTIONS)] if motion != "z_zero" else "roll")
    with flame_amd.Regularizer(0) as reg:
        reg.upload_graph(g)
        ref = synth.copy_graph(g)
        rc, keep, pos = call_project(reg, geo, region, gs)
        rkeep = ref_project(ref, gs, geo, region)
        assert rc == 0 and np.array_equal(keep, rkeep) and 0 < keep.sum() < g["V"]
        same_bits(pos, ref["pos"], "positions, with pos_out")
        same_state(reg.download_state(), ref, "state, with pos_out")
        if motion == "z_zero":
            v = slots[10]
            assert not np.isfinite(ref["pos"][v]).all() and not keep[v]  # z = 0: the projection is not a number, the vertex goes
        # again from the start, without pos_out, and a second projection right behind it
        reg.upload_graph(g)
        ref = synth.copy_graph(g)
        rc, keep, pos = call_project(reg, geo, region, gs, want_pos=False)
        assert rc == 0 and pos is None and np.array_equal(keep, ref_project(ref, gs, geo, region))
        rc, keep, pos = call_project(reg, other, region, gs)
        assert rc == 0 and np.array_equal(keep, ref_project(ref, gs, other, region))
        same_bits(pos, ref["pos"], "positions after two projections")
        same_state(reg.download_state(), ref, "state after two projections")


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_gpu_projection_paths_then_solver_steps(built, form):
    """The edge grid restricted to finite results, every motion, in one form of option 5: the projection on a settled context
    (with and without pos_out), two projections without a sync between them, and the projection behind a chain of two
    run_async -- each bit for bit with the checker and followed by 12 solver steps in that form, which must equal the
    checker's steps on the projected graph: the packed records picked the moved positions up."""
    import torch  # noqa: F401

    import flame_amd

    p, rp = wide_params(flame_amd)
    with flame_amd.Regularizer(0) as reg:
        reg.set_option(5, form)
        for m, motion in enumerate(GPU_MOTIONS):
            gs = (F(1.25), F(0.4))[m % 2]
            geo, other = gpu_geometry(motion), gpu_geometry(GPU_MOTIONS[(m + 2) % len(GPU_MOTIONS)])
            g, region, placed, slots = projection_scene(1500, 20 + m, gs, geo, finite_only=True)
            assert_grid_hit_the_lines(g, gs, geo, region, placed)
            for path in ("settled", "settled, no pos_out", "two in a row", "behind a chain", "behind a chain, no pos_out"):
                what = (form, motion, path)
                reg.upload_graph(g)
                ref = synth.copy_graph(g)
                if path.startswith("behind"):
                    reg.run_async(p, 17)
                    reg.run_async(p, 9)
                    assert oracle.run(ref, 26, rp) == 0
                    assert np.array_equal(ref["x"].view(np.uint32), g["x"].view(np.uint32))  # (x sits on data_term: the grid stands)
                rc, keep, pos = call_project(reg, geo, region, gs, want_pos=path in ("settled", "behind a chain"))
                assert rc == 0 and np.array_equal(keep, ref_project(ref, gs, geo, region)), what
                for (axis, side), (line, on, below, above) in placed.items():
                    assert keep[[on, below, above]].tolist() == ([1, 0, 1] if side == 0 else [0, 1, 0]), what
                if path == "two in a row":
                    rc, keep, pos = call_project(reg, other, region, gs)
                    assert rc == 0 and np.array_equal(keep, ref_project(ref, gs, other, region)), what
                if pos is not None:
                    same_bits(pos, ref["pos"], what)
                assert np.isfinite(ref["pos"]).all() and np.isfinite(ref["x"]).all()
                same_state(reg.download_state(), ref, (what, "after the projection"))
                reg.run(p, 12)
                assert oracle.run(ref, 12, rp) == 0
                same_state(reg.download_state(), ref, (what, "12 steps after the projection"))
                assert np.abs(ref["w1"]).max() > 0 and np.abs(ref["q1"]).max() > 0  # (the steps did something that depends on pos)


@pytest.mark.gpu
@pytest.mark.parametrize("V", [0, 1, 255, 256, 257])
def test_gpu_projection_small_graphs(built, V):
    """Vertex counts around one workgroup of k_project_graph (256 lanes): none, one, one short of a block, a full block, one
    more; settled and behind a chain, every motion, then solver steps."""
    import torch  # noqa: F401

    import flame_amd

    p, rp = wide_params(flame_amd)
    gs = F(1.1)
    with flame_amd.Regularizer(0) as reg:
        for m, motion in enumerate(GPU_MOTIONS):
            geo = gpu_geometry(motion)
            g, region, _, _ = projection_scene(V, 40 + m, gs, geo, grid=False)
            for chain in (False, True):
                reg.upload_graph(g)
                ref = synth.copy_graph(g)
                if chain:
                    reg.run_async(p, 7)
                    reg.run_async(p, 5)
                    assert oracle.run(ref, 12, rp) == 0
                rc, keep, pos = call_project(reg, geo, region, gs, want_pos=(m % 2 == 0))
                rkeep = ref_project(ref, gs, geo, region)
                assert rc == 0 and keep.shape == (V,) and np.array_equal(keep, rkeep), (V, motion, chain)
                if pos is not None:
                    same_bits(pos, ref["pos"], (V, motion, chain))
                same_state(reg.download_state(), ref, (V, motion, chain))
                reg.run(p, 12)
                assert oracle.run(ref, 12, rp) == 0
                same_state(reg.download_state(), ref, (V, motion, chain, "steps after"))


@pytest.mark.gpu
def test_gpu_projection_errors_change_nothing(built):
    """graph_scale 0, negative or NaN and a NULL projection: the invalid-argument status, keep_out and pos_out not written,
    the state and the positions as they were (a valid projection afterwards starts from them) -- settled and with runs in
    flight."""
    import torch  # noqa: F401

    import flame_amd

    p, rp = wide_params(flame_amd)
    gs = F(1.25)
    geo = gpu_geometry("roll")
    g, region, _, _ = projection_scene(1500, 50, gs, geo, finite_only=True)
    with flame_amd.Regularizer(0) as reg:
        for chain in (False, True):
            reg.upload_graph(g)
            ref = synth.copy_graph(g)
            if chain:
                reg.run_async(p, 9)
                reg.run_async(p, 4)
                assert oracle.run(ref, 13, rp) == 0
            for bad_scale, null in ((0.0, False), (-0.0, False), (-1.25, False), (float("nan"), False), (1.25, True)):
                rc, keep, pos = call_project(reg, geo, region, bad_scale, null_projection=null)
                assert rc == -1 and reg.last_error() == -1, (bad_scale, null, rc)  # FLAME_NLTGV2_ERR_INVALID_ARG
                assert (keep == 7).all() and (pos == -777.0).all()
                same_state(reg.download_state(), ref, ("state after a refused call", bad_scale, null, chain))
            rc, keep, pos = call_project(reg, geo, region, gs)
            assert rc == 0 and np.array_equal(keep, ref_project(ref, gs, geo, region))
            same_bits(pos, ref["pos"], "positions after refused calls")
            same_state(reg.download_state(), ref, "state after refused calls and a valid one")


# ---- GPU: the rescale -------------------------------------------------------------------------------------------------------------
def check_rescale(reg, params, ref, gs, data_factor, what):
    """One rescale on the device and in the checker: new_scale, data_factor and the state equal; what the operation leaves
    alone is what it was.  -> the checker's data_factor.  (data_term and data_weight cannot be read back: the solver steps that
    follow in the chain test equal the checker's only if the first was scaled and the second left alone.)"""
    before = {k: ref[k].copy() for k in ALL_STATE}
    ns = reg.rescale_data(float(gs), params)
    with np.errstate(all="ignore"):
        rs, rdf = oracle.graph_rescale(ref, float(gs), data_factor)
    same_bits(F(ns), F(rs), (what, "new_scale"))
    same_bits(F(params.data_factor), F(rdf), (what, "data_factor"))
    st = reg.download_state()
    same_state(st, ref, what)
    for k in ALL_STATE:
        if k not in ("x", "x_bar", "x_prev"):
            same_bits(st[k], before[k], (what, k, "left alone"))
    return rdf


@pytest.mark.gpu
@pytest.mark.parametrize("V", RESCALE_V)
def test_gpu_rescale_settled(built, V):
    """k_block_sum's strided sum at V below, at and above multiples of its 1024 lanes, on every kind of data_term and three
    scales: new_scale, data_factor and all state arrays bit for bit with the checker (a new_scale of 0 leaves inf and NaN: the
    same ones), w1, w2, q and the _bar / _prev copies of w untouched; a second rescale on top of the first (the scaled
    data_term is what it sums)."""
    import torch  # noqa: F401

    import flame_amd

    with flame_amd.Regularizer(0) as reg:
        for kind in RESCALE_KINDS:
            for gs in RESCALE_SCALES:
                g = rescale_graph(V, kind, 100 + V)
                ref = synth.copy_graph(g)
                reg.upload_graph(g)
                params = flame_amd.Params()
                df = check_rescale(reg, params, ref, gs, 0.1, (V, kind, gs))
                if kind != "zero":
                    check_rescale(reg, params, ref, 0.8, df, (V, kind, gs, "second"))


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_gpu_rescale_behind_chains_then_solver_steps(built, form):
    """The rescale behind a chain of two run_async in one form of option 5: the same assertions, and 15 further steps with the
    returned data_factor equal the checker's (the scaled data_term and x reached the packed state)."""
    import torch  # noqa: F401

    import flame_amd

    with flame_amd.Regularizer(0) as reg:
        reg.set_option(5, form)
        for V in (1025, 3000):
            for kind in ("random", "huge", "equal"):
                for gs in RESCALE_SCALES:
                    g = random_graph(V, 3 * V, 300 + V)
                    g["data_term"] = rescale_data_term(kind, V, 7)
                    for k in ("x", "x_bar", "x_prev"):
                        g[k] = g["data_term"].copy()
                    ref = synth.copy_graph(g)
                    reg.upload_graph(g)
                    params = flame_amd.Params()
                    reg.run_async(params, 17)
                    reg.run_async(params, 9)
                    assert oracle.run(ref, 26) == 0
                    rdf = check_rescale(reg, params, ref, gs, 0.1, (form, V, kind, gs))
                    reg.run(params, 15)
                    assert oracle.run(ref, 15, oracle.make_params(data_factor=rdf)) == 0
                    same_state(reg.download_state(), ref, (form, V, kind, gs, "15 steps after the rescale"))


@pytest.mark.gpu
def test_gpu_rescale_errors_change_nothing(built):
    """An invalid graph_scale (0, negative, NaN) is an error: nothing changes, neither the state nor data_factor."""
    import torch  # noqa: F401

    import flame_amd

    g = rescale_graph(1025, "random", 9)
    with flame_amd.Regularizer(0) as reg:
        reg.upload_graph(g)
        params = flame_amd.Params()
        for bad in (0.0, -0.0, -1.0, float("nan")):
            with pytest.raises(flame_amd.NLTGV2Error) as e:
                reg.rescale_data(bad, params)
            assert e.value.status == -1 and F(params.data_factor) == F(0.1)
            same_state(reg.download_state(), g, ("state after a refused rescale", bad))
        ref = synth.copy_graph(g)
        check_rescale(reg, params, ref, 1.3, 0.1, "a valid rescale after the refused ones")
