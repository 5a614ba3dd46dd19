"""Every stage that takes a camera matrix or a pose, with matrices none of whose entries is 0 (tests/general_cameras.py): the cases the
device is compared on in tests/test_gpu_general_cameras.py, and three things about the float32 checkers alone, without a GPU --

  a. the probe (blind_entries) is empty with the general matrices: swapping any two entries a stage reads, or zeroing one, changes the
     checker's output in some bit, so a kernel, host copy or binding that drops an entry or reads it from another index cannot equal it;
  b. the probe is NOT empty with the matrices the older tests use (pinhole cameras, rotations about one axis): what those could not see;
  c. the float32 checker agrees with a float64 statement of the same rule written as matrix products (`@`, np.linalg.inv), within a
     forward bound propagated from the operation count (the rules of tests/volume_ref64.py).  A discrete result whose float64 value lies
     within its bound of the threshold is doubtful and left out; at most 2 % of a case may be.  The share and the worst error / bound
     ratio are printed per stage.
"""
import functools

import numpy as np
import pytest

from flame_amd import synth
from tests import general_cameras as gc
from tests import input_ref as ir
from tests import mesh_ref as mr
from tests import metric_ref as xr
from tests import raw_frame_cases as rc
from tests import test_render_view_ref as cases
from tests import view_ref as vr
from tests.general_cameras import EPS, affine, product, quotient
from tests.metric_helpers import INF, POSE, kinv_for

F = np.float32
f8 = np.float64
DOUBT_CAP = 0.02
ALL9, ALL12 = range(9), range(12)


def report(stage, doubtful, n, ratio):
    print("%s: doubtful %d of %d (%.2f %%), worst error / bound %.3f" % (stage, doubtful, n, 100.0 * doubtful / max(n, 1), ratio))
    assert doubtful <= DOUBT_CAP * n, stage
    assert ratio <= 1.0, stage


def worst(err, bound, keep):
    keep = np.broadcast_to(keep, err.shape)
    with np.errstate(all="ignore"):
        r = np.where(keep, err / np.maximum(bound, 1e-300), 0.0)
    assert np.isfinite(r).all()
    return float(r.max()) if r.size else 0.0


def add(x, ex, y, ey):
    return x + y, ex + ey + EPS * (np.abs(x) + np.abs(y))


# ---- metric outputs: the points ---------------------------------------------------------------------------------------------------------
METRIC_SHAPE = (37, 29)
METRIC_WINDOWS = ((0.0, INF), (0.5, 3.0))
METRIC_K64 = gc.general_K64(20, 19, 16, 12)
METRIC_KINV = gc.general_kinv(METRIC_K64)
METRIC_POSE = gc.pose(17.0, (0.25, -1.5, 3.0))  # T_world_cam: no two of the twelve entries equal, the rows of t differ


@functools.lru_cache(maxsize=None)
def metric_map():
    """The `half` pattern of tests/test_gpu_metric_outputs.py on its 37 x 29 map: inverse depths in (0.2, 4), half of them NaN."""
    rng = np.random.default_rng(100 * METRIC_SHAPE[0] + METRIC_SHAPE[1])
    v = rng.uniform(0.2, 4.0, METRIC_SHAPE).astype(F)
    v[rng.random(METRIC_SHAPE) < 0.5] = np.nan
    v.setflags(write=False)
    return v


def metric_probe(Kinv, pose):
    v = metric_map()
    blind = gc.blind_entries(lambda M: xr.metric_points(v, M, pose, 0.5, 3.0), Kinv, ALL9)
    return blind + [("pose",) + b for b in gc.blind_entries(lambda M: xr.metric_points(v, Kinv, M, 0.5, 3.0), pose, ALL12)]


def test_metric_points_depend_on_every_entry_of_kinv_and_the_pose():
    assert metric_probe(METRIC_KINV, METRIC_POSE) == []
    for lo, hi in METRIC_WINDOWS:
        n = xr.metric_points(metric_map(), METRIC_KINV, METRIC_POSE, lo, hi)["n_points"]
        assert 0 < n < np.isfinite(metric_map()).sum() or (lo, hi) == (0.0, INF) and n == np.isfinite(metric_map()).sum()
    assert 0 < xr.metric_points(metric_map(), METRIC_KINV, METRIC_POSE, 0.5, 3.0)["n_points"] < np.isfinite(metric_map()).sum()


def test_the_older_metric_matrices_leave_mutations_unseen():
    blind = metric_probe(kinv_for(METRIC_SHAPE[1], METRIC_SHAPE[0]), POSE)
    print("metric points, pinhole Kinv and rot_z: %d blind mutations %s" % (len(blind), blind))
    assert len([b for b in blind if b[0] == "swap"]) >= 6 and len([b for b in blind if b[0] == "pose"]) >= 7


def metric_points64(v, Kinv, pose, lo, hi):
    """The header's rule as matrix products -> dict(P_w (3, rows, cols), e (3, ...), z, ez, valid, doubt)."""
    rows, cols = v.shape
    Ki, T = np.asarray(Kinv, F).astype(f8).reshape(3, 3), np.asarray(pose, F).astype(f8).reshape(3, 4)
    row, col = np.mgrid[0:rows, 0:cols].astype(f8)
    pix = np.stack([col, row, np.ones_like(col)])
    vd = np.asarray(v, F).astype(f8)
    with np.errstate(all="ignore"):
        q = np.einsum("ij,jrc->irc", Ki, pix)
        P = q / vd
        Pw = np.einsum("ij,jrc->irc", T[:, :3], P) + T[:, 3][:, None, None]
        _, eq = gc.homogeneous(Ki, col, row)
        eP = [quotient(q[i], eq[i], vd, 0.0)[1] for i in range(3)]
        _, ePw = affine(T[:, :3], T[:, 3], list(P), eP)
        z, ez = P[2], eP[2]
        positive = vd > 0
        valid = positive & (z > f8(F(lo))) & (z < f8(F(hi)))
        doubt = positive & ((np.abs(z - f8(F(lo))) <= ez) | (np.abs(z - f8(F(hi))) <= ez))
        zm, ezm = product(z, ez, 1000.0, 0.0)
        mm = np.where(valid & (np.rint(zm) >= 1) & (np.rint(zm) <= 65535), np.rint(zm), 0.0)
        doubt |= valid & (np.abs(np.abs(zm - np.floor(zm)) - 0.5) <= ezm)
    return dict(P_w=Pw, e=np.stack(ePw), z=z, ez=ez, valid=valid, doubt=doubt, depth_mm=mm)


@pytest.mark.parametrize("window", METRIC_WINDOWS)
def test_metric_points_checker_agrees_with_the_float64_products(window):
    v = metric_map()
    got = xr.metric_points(v, METRIC_KINV, METRIC_POSE, *window)
    want = metric_points64(v, METRIC_KINV, METRIC_POSE, *window)
    sure = ~want["doubt"]
    valid32 = ~np.isnan(got["depth"])
    assert np.array_equal(valid32[sure], want["valid"][sure])
    keep = sure & want["valid"]
    assert keep.sum() > 100
    err = np.abs(np.moveaxis(got["organized"].astype(f8), 2, 0) - want["P_w"])
    ratio = max(worst(err, want["e"], keep), worst(np.abs(got["depth"].astype(f8) - want["z"]), want["ez"], keep))
    assert np.array_equal(got["depth_mm"][sure].astype(f8), want["depth_mm"][sure])
    norm = np.sqrt((want["P_w"] ** 2).sum(0))
    print("metric points, window %s: worst point error %.2f x 2^-24 of the point's norm" % (window, (err.max(0) / norm)[keep].max() / EPS))
    report("metric points, window %s" % (window,), int(want["doubt"].sum()), int((np.asarray(v) > 0).sum()), ratio)


# ---- metric outputs: the mesh; the mesh outputs ------------------------------------------------------------------------------------------
MESH_K64 = gc.general_K64(0.82 * 320, 0.81 * 320, 0.5 * 320 + 10.5, 0.5 * 240 - 9.75)
MESH_KINV = gc.general_kinv(MESH_K64)
MESH_POSE = gc.pose(17.0, (0.25, -1.5, 3.0))
MESH_SCALE = 1.25
PROBE_TRIS = 300  # the probe runs the checker's plain loop over the triangles 54 times: the first triangles of the list serve it


@functools.lru_cache(maxsize=None)
def mesh_scene():
    """The `small` scene of tests/test_gpu_metric_outputs.py and tests/test_mesh_outputs.py."""
    g = synth.make_graph("320x240", seed=9)
    return g, synth.delaunay_triangles_scipy(g["pos"])


def mesh_outputs_probe(Kinv):
    g, tris = mesh_scene()
    part = tris[:PROBE_TRIS]

    def fn(M):
        out = mr.mesh_outputs(g["pos"], g["x"], part, M, 240, 320, graph_scale=MESH_SCALE)
        return out["tri_valid"], out["normals"]

    return gc.blind_entries(fn, Kinv, ALL9)


def metric_mesh_probe(Kinv, pose):
    g, tris = mesh_scene()
    normals = mr.vertex_normals(g["pos"], mr.vertex_idepths(g["x"], MESH_SCALE), tris[:PROBE_TRIS], Kinv)
    valid = np.ones(len(tris), np.uint8)

    def fn(Ki, T):
        out = xr.metric_mesh(g["pos"], g["x"], MESH_SCALE, Ki, normals, tris, valid, T)
        return out["mesh_vertices"], out["mesh_normals"]

    return gc.blind_entries(lambda M: fn(M, pose), Kinv, ALL9) + [("pose",) + b for b in gc.blind_entries(lambda M: fn(Kinv, M), pose, ALL12)]


def test_mesh_outputs_and_the_metric_mesh_depend_on_every_entry():
    assert mesh_outputs_probe(MESH_KINV) == []
    assert metric_mesh_probe(MESH_KINV, MESH_POSE) == []
    g, tris = mesh_scene()
    out = mr.mesh_outputs(g["pos"], g["x"], tris, MESH_KINV, 240, 320, graph_scale=MESH_SCALE)
    t = mr.filter_tests(g["pos"], out["vtx_idepth"], tris, MESH_KINV, 320)
    assert 0 < out["n_valid"] < len(tris) and t["angle"].any() and not t["angle"].all()  # (the oblique filter sees the general Kinv)


def test_the_older_mesh_matrices_leave_mutations_unseen():
    a, b = mesh_outputs_probe(kinv_for(320, 240)), metric_mesh_probe(kinv_for(320, 240), POSE)
    print("mesh outputs, pinhole Kinv: %d blind mutations %s" % (len(a), a))
    print("metric mesh, pinhole Kinv and rot_z: %d blind mutations %s" % (len(b), b))
    assert a and b


def test_mesh_vertices_and_posed_normals_agree_with_the_float64_products():
    g, tris = mesh_scene()
    out = mr.mesh_outputs(g["pos"], g["x"], tris, MESH_KINV, 240, 320, graph_scale=MESH_SCALE)
    got = xr.metric_mesh(g["pos"], g["x"], MESH_SCALE, MESH_KINV, out["normals"], tris, out["tri_valid"], MESH_POSE)
    Ki, T = MESH_KINV.astype(f8), MESH_POSE.astype(f8)
    pos, x = g["pos"].astype(f8), g["x"].astype(f8)
    idepth, eid = product(x, 0.0, f8(F(MESH_SCALE)), 0.0)
    q = Ki @ np.stack([pos[:, 0], pos[:, 1], np.ones(len(pos))])
    _, eq = gc.homogeneous(Ki, pos[:, 0], pos[:, 1])
    P = q / idepth
    eP = [quotient(q[i], eq[i], idepth, eid)[1] for i in range(3)]
    Pw = T[:, :3] @ P + T[:, 3:]
    _, ePw = affine(T[:, :3], T[:, 3], list(P), eP)
    every = np.ones(len(pos), bool)
    ratio_v = worst(np.abs(got["mesh_vertices"].astype(f8).T - Pw), np.stack(ePw), every)
    # the unposed vertices against the existing float64 form, the same bound
    P32 = np.stack(mr.backproject(g["pos"], out["vtx_idepth"], MESH_KINV))
    ratio_b = worst(np.abs(P32.astype(f8) - P), np.stack(eP), every)
    assert np.abs(np.stack(mr.backproject(g["pos"], idepth, MESH_KINV, f8)) - P).max() <= 1e-12 * np.abs(P).max()
    # R n: the normals are float32 data, rotated and NOT translated
    n = out["normals"].astype(f8).T
    Rn = T[:, :3] @ n
    _, eRn = affine(T[:, :3], None, list(n), [0.0, 0.0, 0.0])
    ratio_n = worst(np.abs(got["mesh_normals"].astype(f8).T - Rn), np.stack(eRn), every)
    assert np.abs(np.linalg.norm(Rn, axis=0) - np.linalg.norm(n, axis=0)).max() < 1e-6  # (a rotation, in float32 entries)
    report("metric mesh vertices / back-projection / posed normals", 0, len(pos), max(ratio_v, ratio_b, ratio_n))


# ---- the view renderer --------------------------------------------------------------------------------------------------------------------
VIEW_SRC = (48, 64)
VIEW_K_SRC64 = np.array([[60, .9, 32], [.4, 58, 24], [4e-4, -7e-4, 1]], f8)
VIEW_K_DST64 = np.array([[55, -1.1, 30], [.6, 57, 26], [-5e-4, 3e-4, 1]], f8)
VIEW_T = np.array([0.08, -0.05, 0.04], F)


def general_view(seed=5, step=6, deg=6.0, t=VIEW_T, K_src64=VIEW_K_SRC64):
    """A jittered grid over the 48 x 64 source (tests/test_gpu_render_view.py: mesh_case) seen through general cameras and a rotation
    about (1, 2, 3)."""
    pos, tris = cases.grid_mesh(*VIEW_SRC, step, seed=seed)
    idepth = np.random.default_rng(seed).uniform(0.3, 1.5, len(pos)).astype(F)
    return dict(tris=tris, pos=pos, idepth=idepth, Kinv_src=gc.general_kinv(K_src64), K_dst=VIEW_K_DST64.astype(F), R=gc.rotation(deg).astype(F),
                t=np.asarray(t, F), rows=VIEW_SRC[0], cols=VIEW_SRC[1])


def pinhole_view(seed=5):
    K, Kinv = cases.camera(60.0, 32.0, 24.0)
    return dict(general_view(seed), Kinv_src=Kinv, K_dst=K, R=cases.rotation_y(4.0))


VIEW_MATRICES = (("Kinv_src", ALL9), ("K_dst", ALL9), ("R", ALL9), ("t", range(3)))


def view_probe(c):
    blind = []
    for name, read in VIEW_MATRICES:
        blind += [(name,) + b for b in gc.blind_entries(lambda M: cases.render(c, **{name: M}), c[name], read)]
    return blind


def test_the_view_renderer_depends_on_every_entry_of_its_four_matrices():
    c = general_view()
    r = cases.render(c)
    print("general view: %s" % (cases.counts(r),))
    assert r["tris_drawn"] > 0 and r["tris_culled_facing"] > 0 and r["coverage"] > 1000
    assert view_probe(c) == []


def test_the_older_view_matrices_leave_mutations_unseen():
    blind = view_probe(pinhole_view())
    print("view renderer, pinhole cameras and rotation_y: %d blind mutations %s" % (len(blind), blind))
    assert all(sum(1 for b in blind if b[0] == name) >= 7 for name in ("Kinv_src", "K_dst", "R"))


def transform64(c):
    """Rule 1 as matrix products for every vertex -> dict of float64 arrays with their bounds."""
    Ki, K, R, t = (np.asarray(c[k], F).astype(f8) for k in ("Kinv_src", "K_dst", "R", "t"))
    pos, idv = c["pos"].astype(f8), c["idepth"].astype(f8)
    q = Ki @ np.stack([pos[:, 0], pos[:, 1], np.ones(len(pos))])
    _, eq = gc.homogeneous(Ki, pos[:, 0], pos[:, 1])
    P = q / idv
    eP = [quotient(q[i], eq[i], idv, 0.0)[1] for i in range(3)]
    Pd = R @ P + t[:, None]
    _, ePd = affine(R, t, list(P), eP)
    h = K @ Pd
    _, eh = affine(K, None, list(Pd), ePd)
    out = dict(z=Pd[2], ez=ePd[2])
    for name, i in (("sx", 0), ("sy", 1)):
        u, eu = quotient(h[i], eh[i], h[2], eh[2])
        out[name], out["e" + name] = 16.0 * u, 16.0 * eu  # (a power of two: no rounding)
    out["id"], out["eid"] = quotient(1.0, 0.0, Pd[2], ePd[2])
    return out


def test_transform_vertex_agrees_with_the_float64_products():
    c = general_view()
    near = 0.0
    want = transform64(c)
    got = [vr.transform_vertex(c["pos"][v], c["idepth"][v], c["Kinv_src"], c["K_dst"], c["R"], c["t"], near) for v in range(len(c["pos"]))]
    usable64 = (c["idepth"] > 0) & (want["z"] > near) & (np.abs(want["sx"]) <= 2.0 ** 20) & (np.abs(want["sy"]) <= 2.0 ** 20)
    doubt = (np.abs(want["z"] - near) <= want["ez"]) | (np.abs(np.abs(want["sx"]) - 2.0 ** 20) <= want["esx"]) | \
        (np.abs(np.abs(want["sy"]) - 2.0 ** 20) <= want["esy"])
    sure = ~doubt
    assert np.array_equal(np.array([g[0] for g in got])[sure], usable64[sure]) and usable64.sum() > 80
    keep = sure & usable64
    X, Y, Xs, Ys, idd = (np.array([g[i] for g in got], f8) for i in range(1, 6))
    # X = rint(sx): within half a sixteenth of the float32 sx, which is within its bound of the float64 one
    ratio = max(worst(np.abs(X - want["sx"]), 0.5 + want["esx"], keep), worst(np.abs(Y - want["sy"]), 0.5 + want["esy"], keep),
                worst(np.abs(idd - want["id"]), want["eid"], keep))
    assert np.array_equal(Xs[keep], np.rint(16.0 * c["pos"][:, 0].astype(f8))[keep]) and np.array_equal(Ys[keep], np.rint(16.0 * c["pos"][:, 1].astype(f8))[keep])
    print("view renderer: largest bound on a target coordinate %.2e sixteenths" % max(want["esx"][keep].max(), want["esy"][keep].max()))
    report("view renderer, rule 1", int(doubt.sum()), len(doubt), ratio)


# ---- the fusion of views ---------------------------------------------------------------------------------------------------------------------
FUSE_K_DST = VIEW_K_DST64.astype(F)
FUSE_PLANE_N, FUSE_PLANE_D = np.array([0.1, -0.05, 1.0]), 2.0  # the plane of tests/test_fuse_views_ref.py: n . P = 2 in the target's frame
FUSE_CAMERAS = [  # K_src (float64), degrees about (1, 2, 3), t: four different ones
    (VIEW_K_SRC64, 6.0, (0.08, -0.05, 0.04)),
    (gc.general_K64(60, 60, 32, 24), -5.0, (-0.15, 0.02, 0.03)),
    (gc.general_K64(62, 59, 31, 25, skew=-0.8, shear=0.5, bottom=(-3e-4, 6e-4)), 4.0, (0.2, 0.03, -0.02)),
    (gc.general_K64(58, 61, 33, 23, skew=0.5, shear=-0.7, bottom=(5e-4, 4e-4)), -3.0, (-0.05, -0.25, 0.1)),
]
FUSE_WEIGHTS = (1.0, 0.3, 1.7, 0.9)
FUSE_REL_TOL = 0.02


@functools.lru_cache(maxsize=None)
def fuse_scene():
    """Four views of one plane, as tests/test_fuse_views_ref.py: scene, each through its own general camera and pose."""
    out = []
    for s, (K64, deg, t) in enumerate(FUSE_CAMERAS):
        pos, tris = cases.grid_mesh(*VIEW_SRC, 6, seed=30 + s)
        Kinv, R, t = gc.general_kinv(K64), gc.rotation(deg).astype(F), np.asarray(t, F)
        q = Kinv.astype(f8) @ np.stack([pos[:, 0], pos[:, 1], np.ones(len(pos))])
        idepth = (FUSE_PLANE_N @ (R.astype(f8) @ q)) / (FUSE_PLANE_D - FUSE_PLANE_N @ t.astype(f8))
        out.append(dict(tris=tris, pos=pos, idepth=idepth.astype(F), Kinv_src=Kinv, R=R, t=t, weight=FUSE_WEIGHTS[s]))
    return tuple(out)


def test_every_source_of_the_general_fusion_draws_and_they_agree_on_the_plane():
    from tests import fuse_ref as fr

    want = fr.fuse_sources(fuse_scene(), FUSE_K_DST, *VIEW_SRC, FUSE_REL_TOL, 2)
    assert all(r["tris_drawn"] > 0 and r["coverage"] > 500 for r in want["renders"])
    assert want["coverage"] > 1500 and want["support_hist"][4] > 500  # (four general views of one plane: they agree where all see it)
    for s, src in enumerate(fuse_scene()):  # each source's matrices through the probe of the renderer
        c = dict(src, K_dst=FUSE_K_DST, rows=VIEW_SRC[0], cols=VIEW_SRC[1])
        assert view_probe(c) == [], s


# ---- the raw-frame input stage -----------------------------------------------------------------------------------------------------------------
INPUT_OUT, INPUT_RAW = (61, 37), (67, 41)
INPUT_K64 = np.array([[48, .6, 30.2], [-.4, 47, 18.1], [0, 0, 1]], f8)  # the working camera: rows 0 and 1 of its inverse have no zero
INPUT_K_RAW = np.array([[50, 0.8, 33.5], [0, 49, 20.25], [0, 0, 1]], F)   # K_raw[1], the skew, is 0.8
INPUT_DIST = (0.3, 0.05, 2e-3, -1e-3)
INPUT_FORMATS = ((ir.BGR8, 5), (ir.GREY8, 0))  # (format, bytes of padding behind each row)


def input_case():
    """(w, h, K, Kinv, params) in the form of tests/raw_frame_cases.py: setup."""
    d = np.zeros(8, F)
    d[:len(INPUT_DIST)] = INPUT_DIST
    return INPUT_OUT[0], INPUT_OUT[1], INPUT_K64.astype(F), gc.general_kinv(INPUT_K64), dict(
        remap=1, raw_width=INPUT_RAW[0], raw_height=INPUT_RAW[1], K_raw=INPUT_K_RAW, dist=d)


@functools.lru_cache(maxsize=None)
def input_expected(fmt, pad):
    w, h, K, Kinv, p = input_case()
    raw = rc.raw_bytes(p["raw_width"], p["raw_height"], fmt, pad)
    raw.setflags(write=False)
    return raw, ir.rectify(raw, fmt, p, K, Kinv, w, h)


INPUT_KINV_READ, INPUT_KRAW_READ = range(6), (0, 1, 2, 4, 5)


def input_probe(Kinv, K_raw):
    w, h, K, _, p = input_case()
    raw = input_expected(ir.GREY8, 0)[0]
    blind = gc.blind_entries(lambda M: ir.rectify(raw, ir.GREY8, dict(p, K_raw=K_raw), K, M, w, h), Kinv, INPUT_KINV_READ)
    return blind + [("K_raw",) + b for b in gc.blind_entries(lambda M: ir.rectify(raw, ir.GREY8, dict(p, K_raw=M), K, Kinv, w, h), K_raw,
                                                             INPUT_KRAW_READ)]


def test_the_input_stage_depends_on_every_entry_it_reads():
    w, h, K, Kinv, p = input_case()
    assert input_probe(Kinv, p["K_raw"]) == []
    for fmt, pad in INPUT_FORMATS:
        n_outside = input_expected(fmt, pad)[1][1]
        assert 0 < n_outside < w * h == 2257


def test_the_older_input_matrices_leave_mutations_unseen():
    _, Kinv = ir.cam(*rc.CAM_A)
    blind = input_probe(Kinv, ir.cam(50, 49, 33.5, 20.25)[0])
    print("input stage, pinhole working camera and raw camera: %d blind mutations %s" % (len(blind), blind))
    assert ("swap", 1, 3) in blind and ("K_raw", "zero", 1) in blind


def source_map64(K_raw, dist, Kinv, w, h, raw_w, raw_h):
    """The header's map with its two linear steps as matrix products -> xs, ys with bounds, inside, doubt."""
    Ki = np.asarray(Kinv, F).astype(f8).reshape(3, 3)
    Kr = np.asarray(K_raw, F).astype(f8).reshape(3, 3)
    k1, k2, p1, p2, k3, k4, k5, k6 = np.asarray(dist, F).astype(f8)
    v, u = np.mgrid[0:h, 0:w].astype(f8)
    xy = np.einsum("ij,jrc->irc", Ki[:2], np.stack([u, v, np.ones_like(u)]))
    (x, y), (ex, ey) = xy, gc.homogeneous(Ki, u, v)[1][:2]
    xx, yy = product(x, ex, x, ex), product(y, ey, y, ey)
    r2 = add(*xx, *yy)
    r4 = product(*r2, *r2)
    r6 = product(*r4, *r2)

    def poly(a, b, c):  # ((1 + a r2) + b r4) + c r6
        s = add(1.0, 0.0, *product(a, 0.0, *r2))
        s = add(*s, *product(b, 0.0, *r4))
        return add(*s, *product(c, 0.0, *r6))

    rad = quotient(*poly(k1, k2, k3), *poly(k4, k5, k6))
    tx, ty = (2.0 * x, 2.0 * ex), (2.0 * y, 2.0 * ey)
    a1 = product(*tx, y, ey)
    a2 = add(*r2, *product(*tx, x, ex))
    a3 = add(*r2, *product(*ty, y, ey))
    xd = add(*add(*product(x, ex, *rad), *product(p1, 0.0, *a1)), *product(p2, 0.0, *a2))
    yd = add(*add(*product(y, ey, *rad), *product(p1, 0.0, *a3)), *product(p2, 0.0, *a1))
    # xs = K_raw row 0 . (xd, yd, 1); ys = (0, K_raw[4], K_raw[5]) . (xd, yd, 1): K_raw[3] is not read
    M = np.array([Kr[0], [0.0, Kr[1, 1], Kr[1, 2]], [0.0, 0.0, 1.0]])
    s = np.einsum("ij,jrc->irc", M, np.stack([xd[0], yd[0], np.ones_like(u)]))
    _, es = affine(M, None, [xd[0], yd[0], np.ones_like(u)], [xd[1], yd[1], np.zeros_like(u)])
    xs, ys, exs, eys = s[0], s[1], es[0], es[1]
    inside = (xs >= 0) & (ys >= 0) & (xs < raw_w - 1) & (ys < raw_h - 1)
    doubt = (np.abs(xs) <= exs) | (np.abs(ys) <= eys) | (np.abs(xs - (raw_w - 1)) <= exs) | (np.abs(ys - (raw_h - 1)) <= eys)
    return dict(xs=xs, ys=ys, exs=exs, eys=eys, inside=inside, doubt=doubt)


def test_the_source_map_agrees_with_the_float64_products():
    w, h, K, Kinv, p = input_case()
    args = (p["K_raw"], p["dist"], Kinv, w, h, p["raw_width"], p["raw_height"])
    xs, ys, inside = ir.source_map(*args)
    want = source_map64(*args)
    sure = ~want["doubt"]
    assert np.array_equal(inside[sure], want["inside"][sure]) and 0 < want["inside"].sum() < w * h
    # the existing float64 form, in the header's association, is the same map
    xs8, ys8, _ = ir.source_map(*args, dtype=f8)
    assert max(np.abs(xs8 - want["xs"]).max(), np.abs(ys8 - want["ys"]).max()) < 1e-9
    every = np.ones((h, w), bool)  # the coordinates of every pixel, inside or not
    ratio = max(worst(np.abs(xs.astype(f8) - want["xs"]), want["exs"], every), worst(np.abs(ys.astype(f8) - want["ys"]), want["eys"], every))
    report("input stage, the source map", int(want["doubt"].sum()), w * h, ratio)


# ---- the selection of the graph's vertices: the height rule ----------------------------------------------------------------------------------
SELECT_N = 257  # of tests/select_cases.py: SIZES, the smallest with a second workgroup
SELECT_POSE_DEG = (8.0, -11.0, 14.0, -17.0, 20.0)  # one turn about (1, 2, 3) per pose-frame, composed with the scene's own pose
SELECT_POSE_SHIFT = np.array([0.05, 0.13, -0.08])


@functools.lru_cache(maxsize=None)
def select_case():
    """The records of select_cases.make(257) seen through a general Kinv, each pose-frame's camera turned about (1, 2, 3): every entry of
    Kinv and all four components of every quaternion take part in the height.  -> dict(sc, feats, proj, Kinv, world, poses64)."""
    from flame_amd import synth_stereo as ss
    from tests import prune_cases as pc
    from tests import select_cases as sc_

    case = sc_.make(SELECT_N)
    sc = case["sc"]
    K = np.asarray(sc.K, f8).reshape(3, 3)
    K64 = gc.general_K64(K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    world, poses64 = [], {}
    for k, deg in zip(pc.PF_IDS, SELECT_POSE_DEG):
        R, t = sc_.world_pose64(sc, k)
        R, t = R @ gc.rotation(deg), t + SELECT_POSE_SHIFT  # (the first pose-frame sits at the origin: its t.y would be 0)
        q = ss.quat_from_rot(R).astype(F)
        world.append(dict(id=k, q=q, t=np.asarray(t, F)))
        poses64[k] = (q, np.asarray(t, F))
    return dict(sc=sc, feats=case["feats"], proj=case["proj"], K64=K64, Kinv=gc.general_kinv(K64), world=world, poses64=poses64)


def select_probe(Kinv, world, feats, proj):
    from tests import select_ref as sr

    def classes(Ki, w):
        rc, _, cls = sr.classify(feats, Ki, w)
        assert rc == 0
        return cls, sr.heights32(feats, Ki, w)[0]

    blind = gc.blind_entries(lambda M: classes(M, world), np.asarray(Kinv, F), ALL9)
    for i, p in enumerate(world):
        def with_pose(M, i=i, p=p):
            return classes(Kinv, world[:i] + [dict(p, q=M[:4], t=[0, M[4], 0])] + world[i + 1:])

        row = np.concatenate([np.asarray(p["q"], F), [F(p["t"][1])]])  # what the rule reads of a pose: q and t.y
        blind += [("pose", p["id"]) + b for b in gc.blind_entries(with_pose, row, range(5))]
    return blind


def test_the_height_rule_depends_on_every_entry_of_kinv_and_of_each_pose():
    from tests import select_ref as sr

    c = select_case()
    assert select_probe(c["Kinv"], c["world"], c["feats"], c["proj"]) == []
    rc, res = sr.select(c["feats"], c["proj"], c["Kinv"], c["world"], 1.0)
    print("general selection: V %d, counters %s" % (res["V"], {k: res[k] for k in sr.COUNTERS}))
    assert rc == 0 and res["V"] > 0 and res["num_fail_height"] > 0  # (both a taken record and one that fails the height)


def test_the_older_selection_matrices_leave_mutations_unseen():
    from tests import select_cases as sc_

    case = sc_.make(SELECT_N)
    blind = select_probe(case["sc"].Kinv32, case["world"], case["feats"], case["proj"])
    print("selection, pinhole Kinv and the scene's poses: %d blind mutations %s" % (len(blind), blind))
    assert [b for b in blind if b[0] == "swap"]


def test_the_height_checker_agrees_with_the_float64_products():
    """world = R Kinv (x, y, 1) / mu + t in float64 from the float32 Kinv and quaternion the device is given; the band of every record
    whose float64 height is farther from both thresholds than its bound is the checker's."""
    from tests import select_ref as sr

    c = select_case()
    feats = c["feats"]
    h32, _ = sr.heights32(feats, c["Kinv"], c["world"])
    Ki = c["Kinv"].astype(f8)
    lo, hi = f8(F(sr.DEFAULT_GP["min_height"])), f8(F(sr.DEFAULT_GP["max_height"]))
    doubtful, ratio, n = 0, 0.0, 0
    for k, (q, t) in c["poses64"].items():
        sel = (feats["frame_id"] == k) & (feats["idepth_mu"] > 0)
        f = feats[sel]
        w, x, y, z = q.astype(f8)
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        mu = f["idepth_mu"].astype(f8)
        with np.errstate(all="ignore"):
            pix = np.stack([f["x"].astype(f8) / mu, f["y"].astype(f8) / mu, 1.0 / mu])
            epix = [EPS * np.abs(p) for p in pix]
            xyz = Ki @ pix
            _, exyz = affine(Ki, None, list(pix), epix)
            world = R @ xyz + t.astype(f8)[:, None]
            # an entry of row 1 of R takes four roundings on magnitudes of at most 3: 16 EPS absolute (tests/test_select_graph_features.py)
            _, ew = affine(R, t.astype(f8), list(xyz), exyz)
            e = ew[1] + 16.0 * EPS * np.abs(xyz).sum(0)
        h64 = -world[1]
        finite = np.isfinite(h64) & np.isfinite(e)
        near = finite & ((np.abs(h64 - lo) <= e) | (np.abs(h64 - hi) <= e))
        with np.errstate(all="ignore"):
            band32, band64 = (h32[sel] >= F(lo)) & (h32[sel] <= F(hi)), (h64 >= lo) & (h64 <= hi)
        assert np.array_equal(band32[~near], band64[~near]), k
        ratio = max(ratio, worst(np.abs(h32[sel].astype(f8) - h64), e, finite))
        doubtful, n = doubtful + int(near.sum()), n + int(sel.sum())
    report("selection, the height", doubtful, n, ratio)


# ---- the photometric residual ------------------------------------------------------------------------------------------------------------------
def test_the_photometric_cases_already_have_a_full_krkinv():
    """KRKinv of tests/test_photometric_edges.py: camera_geometry comes from a pinhole K and a rotation about two axes, and has no zero:
    the probe is empty as it is, so photo_residual, photo_fuse and the PHOTO source of map_error get no new case."""
    from oracle import capi as oracle
    from tests import test_photometric_edges as pe

    rows, cols, border = 61, 97, 2
    g, _ = pe.edge_graph(rows, cols, border, "320x240", pe.SHIFT, seed=31 + border)
    ref, cmp = pe.image_pair(rows, cols, 0, seed=border * 10)
    M, Kt = pe.camera_geometry(rows, cols)
    x = np.abs(g["x"]).astype(F)
    assert np.isfinite(oracle.photo_residual(g["pos"], x, 1.0, M, Kt, ref, cmp, border)).sum() > 1000
    assert gc.blind_entries(lambda A: oracle.photo_residual(g["pos"], x, 1.0, A, Kt, ref, cmp, border), M, ALL9) == []
    assert gc.blind_entries(lambda A: oracle.photo_residual(g["pos"], x, 1.0, M, A, ref, cmp, border), Kt, range(3)) == []


# ---- the alignment -----------------------------------------------------------------------------------------------------------------------------
def test_the_alignment_cases_already_have_a_general_rotation():
    """flame_stereo_align_frame refuses a K that is no pinhole's (tested in tests/test_gpu_align_edges.py), and small_pose of
    tests/align_cases.py turns about (0.01, -0.012, 0.008): no entry of R or t is blind as it is, so the alignment gets no new case."""
    from tests import align_cases as ac
    from tests import align_ref as ar

    ref, new, d, _, _ = ac.driver_scene()
    rp, npyr = ar.build_pyramid(ref, 3), ar.build_pyramid(new, 3)
    q, t = ac.small_pose()
    R, t = np.asarray(ar.quat_to_rot(q), F).reshape(-1), np.asarray(t, F)

    def terms(R, t):
        return ar.pixel_terms(rp[0][0], npyr[0], d, 0, ac.DRIVER_K, 2, 10.0, R, t)

    assert gc.blind_entries(lambda M: terms(M, t), R, ALL9) == [] and gc.blind_entries(lambda M: terms(R, M), t, range(3)) == []
