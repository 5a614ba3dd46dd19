"""Mesh outputs of Flame::update() on the device (flame_nltgv2_mesh_outputs: vtx_idepths, vertex normals, triangle validity,
filtered dense map; flame.cc:372-407) against the numpy restatement tests/mesh_ref.py.

CPU part: known answers for the checker itself, the definition of the angle test's bound D*, the order dependence of the
normals, the mirror's defaults.  GPU part: every output bit for bit -- no tolerance: nothing transcendental runs on the device."""
import ctypes as C

import numpy as np
import pytest

from flame_amd import synth
from oracle import capi as oracle
from tests import mesh_ref as mr

F = np.float32
INF = float("inf")


def pinhole_kinv(fx=525.0, fy=520.0, cx=330.5, cy=230.25):
    """Kinv of a pinhole camera with an off-centre principal point, rounded to float32 as Flame holds it."""
    return np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]], np.float64).astype(F)


def bits(a):
    """The float32 bit patterns, every NaN mapped to one pattern.  A finding of the first GPU run, not a tolerance: IEEE 754 leaves
    the sign and payload of a NaN an operation GENERATES (inf - inf, 0 * inf, 0 / 0) to the implementation -- x86 SSE makes
    0xFFC00000, gfx950 0x7FC00000 -- and the reference never reads them.  Where a NaN stands, and every bit of every other value
    (signed zeros and infinities included), is compared."""
    u = np.ascontiguousarray(a, F).view(np.uint32).copy()
    u[np.isnan(np.ascontiguousarray(a, F))] = 0x7FC00000
    return u


def only(**kw):
    """Filter parameters with every test out of the way except what kw sets."""
    p = mr.params(oblique_normal_thresh=4.0, oblique_idepth_diff_factor=INF, oblique_idepth_diff_abs=INF,
                  edge_length_thresh=INF, min_triangle_idepth=-INF)
    p.update(kw)
    return p


# ---- CPU: known answers for the checker ------------------------------------------------------------------------------------------
def grid_mesh(nx=9, ny=7, step=20.0, x0=100.0, y0=80.0):
    xs, ys = np.meshgrid(np.arange(nx), np.arange(ny))
    pos = np.stack([x0 + step * xs.ravel(), y0 + step * ys.ravel()], axis=1).astype(F)
    tris = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i, (j + 1) * nx + i + 1
            tris += [[a, b, c], [b, d, c]]  # positive signed area in (x, y): the triangulator's winding
    return pos, np.array(tris, np.int32)


def test_checker_fronto_parallel_plane():
    """Constant idepth: every back-projected point has the same z, every triangle faces the camera.  Every triangle is valid under
    the defaults, every vertex normal is exactly (0, 0, -1) -- OUTWARD: towards the camera, against the viewing ray -- and
    d = ray . inward normal is 1 up to rounding at the image centre and cos(angle of the viewing ray) elsewhere."""
    pos, tris = grid_mesh()
    Kinv = pinhole_kinv()
    idepth = np.full(len(pos), 0.5, F)
    out = mr.mesh_outputs(pos, idepth, tris, Kinv, 480, 640, graph_scale=1.0)
    assert out["tri_valid"].all() and out["n_valid"] == len(tris)
    n = out["normals"]
    assert np.array_equal(n[:, 2], np.full(len(pos), -1, F)) and not n[:, :2].any()
    d, outward, _ = mr.triangle_geometry(pos, idepth, tris, Kinv)
    d64, _, _ = mr.triangle_geometry(pos, idepth, tris, Kinv, np.float64)
    assert np.abs(d - d64).max() < 4 * np.finfo(F).eps and d.min() > 0.88 and d.max() <= 1.0  # (cos of the corner ray: 0.886)
    # a triangle whose centroid lies on the optical axis: d == 1 up to rounding
    c = np.array([330.5, 230.25])
    p3 = np.array([c + [-6, -3], c + [6, -3], c + [0, 6]], F)
    d1, _, _ = mr.triangle_geometry(p3, np.full(3, 0.5, F), [[0, 1, 2]], Kinv)
    assert abs(float(d1[0]) - 1.0) <= 2 * np.finfo(F).eps


def tilted_triangle(phi, depth=2.0, r=0.02):
    """A small triangle around the optical axis on a plane tilted by phi about the y axis: pixel positions and idepths (float32)."""
    K = np.linalg.inv(pinhole_kinv().astype(np.float64))
    X = np.array([[-r, -r / 2], [r, -r / 2], [0.0, r]])
    X3 = np.stack([X[:, 0], X[:, 1], depth + np.tan(phi) * X[:, 0]], axis=1)
    uv = (K @ (X3 / X3[:, 2:3]).T).T[:, :2]
    return uv.astype(F), (1.0 / X3[:, 2]).astype(F)


@pytest.mark.parametrize("side", [-1, 1])
def test_checker_tilted_plane_either_side_of_the_angle_threshold(side):
    thresh = mr.DEFAULTS["oblique_normal_thresh"]
    for phi in (thresh - 0.03, thresh + 0.03):
        pos, idepth = tilted_triangle(side * phi)
        p = only(oblique_normal_thresh=thresh)
        valid = mr.triangle_validity(pos, idepth, [[0, 1, 2]], pinhole_kinv(), 640, p)
        d, _, _ = mr.triangle_geometry(pos, idepth, [[0, 1, 2]], pinhole_kinv(), np.float64)
        assert abs(np.arccos(d[0]) - phi) < 0.01, (phi, np.arccos(d[0]))  # (the centroid's ray is the optical axis, nearly)
        assert bool(valid[0]) == (phi < thresh)


def test_checker_each_comparison_at_its_threshold_and_one_ulp_either_side():
    """One triangle per test whose compared quantity is exactly representable (or, for the angle, whose own angle is taken as the
    threshold): at the threshold nothing is cleared (all five comparisons are strict), one ulp beyond it is."""
    Kinv = pinhole_kinv()
    tri = [[0, 1, 2]]
    pos = np.array([[0, 0], [3, 4], [0, 1]], F)  # dist01 = 25 exactly
    up, down = (lambda v: float(mr.next_float(v, 1))), (lambda v: float(mr.next_float(v, -1)))

    def valid(idepth, cols=10, **kw):
        return bool(mr.triangle_validity(pos, np.asarray(idepth, F), tri, Kinv, cols, only(**kw))[0])

    ids = [0.5, 0.75, 1.0]  # max - min = 0.5, (max - min) / max = 0.5
    assert valid(ids, oblique_idepth_diff_abs=0.5) and not valid(ids, oblique_idepth_diff_abs=down(0.5)) and valid(ids, oblique_idepth_diff_abs=up(0.5))
    assert valid(ids, oblique_idepth_diff_factor=0.5) and not valid(ids, oblique_idepth_diff_factor=down(0.5)) and valid(ids, oblique_idepth_diff_factor=up(0.5))
    # edge length: thresh2 = (0.5 * 10)^2 = 25 == the longest squared edge
    assert valid(ids, edge_length_thresh=0.5) and not valid(ids, edge_length_thresh=down(0.5)) and valid(ids, edge_length_thresh=up(0.5))
    assert not valid(ids, cols=9, edge_length_thresh=0.5)  # (the WIDTH scales it)
    ids = [0.25, 0.5, 0.75]  # mean = 0.5
    assert valid(ids, min_triangle_idepth=0.5) and not valid(ids, min_triangle_idepth=up(0.5)) and valid(ids, min_triangle_idepth=down(0.5))
    # the angle: the triangle's own angle as the threshold
    tp, tid = tilted_triangle(1.2)
    d, _, _ = mr.triangle_geometry(tp, tid, tri, Kinv)
    own = F(np.arccos(np.float64(d[0])))

    def valid_angle(t):
        return bool(mr.triangle_validity(tp, tid, tri, Kinv, 640, only(oblique_normal_thresh=t))[0])

    assert valid_angle(own) and not valid_angle(down(own)) and valid_angle(up(own))
    # and a switched-off filter clears nothing
    assert bool(mr.triangle_validity(tp, tid, tri, Kinv, 640, only(oblique_normal_thresh=0.1, do_oblique_triangle_filter=False))[0])


@pytest.mark.parametrize("thresh", [0.5, 1.39626, 3.0])
def test_angle_bound_agrees_with_the_literal_test(built, thresh):
    """D* (mesh_ref.oblique_cos_bound == flame_nltgv2_oblique_cos_bound): `d in [-1, 1] and d < D*` is the literal
    `float32(arccos(float64(d))) > thresh` on every float within 64 ulps of D* and on the special values."""
    import flame_amd

    lib = flame_amd.load_library()
    D = mr.oblique_cos_bound(thresh)
    assert bits(lib.flame_nltgv2_oblique_cos_bound(thresh))[0] == bits(D)[0]
    ds = [mr.next_float(D, k) for k in range(-64, 65)]
    ds += [F(-1), F(1), F(0.0), F(-0.0), mr.next_float(1.0, 1), mr.next_float(-1.0, -1), F(np.nan), F(np.inf), F(-np.inf)]
    ds = np.array(ds, F)
    lit, dev = mr.angle_rejects(ds, thresh), mr.bound_rejects(ds, D)
    assert np.array_equal(lit, dev)
    assert lit[:64].all() and not lit[64:129].any()  # (below D*: rejected; D* and above: kept)
    assert not lit[-5:].any()  # just outside [-1, 1], NaN, +-inf: the reference's angle is a NaN


def test_angle_bound_special_thresholds(built):
    import flame_amd

    lib = flame_amd.load_library()
    assert bits(mr.oblique_cos_bound(1.39626))[0] == bits(F(0.17365146))[0]
    for t, want in ((3.1415927, -1.0), (4.0, -1.0), (INF, -1.0), (-1e-30, INF), (-1.0, INF), (float("nan"), -1.0), (0.0, 1.0)):
        assert float(mr.oblique_cos_bound(t)) == want and float(lib.flame_nltgv2_oblique_cos_bound(t)) == want, t
    d = np.array([-1, -0.5, 0, 0.5, 1], F)
    assert not mr.angle_rejects(d, 3.1415927).any() and not mr.angle_rejects(d, float("nan")).any() and mr.angle_rejects(d, -1.0).all()


def test_normals_depend_on_the_triangle_order_and_on_nothing_else():
    g = synth.make_graph("320x240", seed=3)
    tris = synth.delaunay_triangles_scipy(g["pos"])
    Kinv = pinhole_kinv(fx=260, fy=255, cx=165.5, cy=118.25)
    idepth = mr.vertex_idepths(g["x"], 1.0)
    n0 = mr.vertex_normals(g["pos"], idepth, tris, Kinv)
    rng = np.random.default_rng(1)
    n1 = mr.vertex_normals(g["pos"], idepth, tris[rng.permutation(len(tris))], Kinv)
    changed = (bits(n0) != bits(n1)).any(axis=1)
    assert changed.any(), "the running mean is order dependent: some vertex must change"
    # (not in the last bits only: re-normalising after every triangle weights the triangles by their place in the list)
    # relabelling the vertices (same triangles, same order) only moves the normals along
    perm = rng.permutation(len(idepth))  # old id -> new id
    pos2, id2 = np.empty_like(g["pos"]), np.empty_like(idepth)
    pos2[perm], id2[perm] = g["pos"], idepth
    n2 = mr.vertex_normals(pos2, id2, perm[tris].astype(np.int32), Kinv)
    assert np.array_equal(bits(n2[perm]), bits(n0))
    v2 = mr.triangle_validity(pos2, id2, perm[tris], Kinv, 320)
    assert np.array_equal(v2, mr.triangle_validity(g["pos"], idepth, tris, Kinv, 320))


def test_mirror_exposes_mesh_outputs_with_the_reference_defaults(built):
    import flame_amd
    from flame_amd.regularizer import ABI_SYMBOLS

    for name in ("mesh_outputs", "mesh_outputs_begin", "mesh_outputs_end"):
        assert callable(getattr(flame_amd.Regularizer, name))
        assert "flame_nltgv2_" + name in ABI_SYMBOLS
    want = [1, F(1.39626), F(0.35), F(0.1), 1, F(0.333), 1, F(0.01)]  # params.h:69-85
    p = flame_amd.MeshFilterParams()
    c = flame_amd.MeshFilterParams(0, 0, 0, 0, 0, 0, 0, 0)
    flame_amd.load_library().flame_nltgv2_default_mesh_filter_params(C.byref(c))
    for q in (p, c):
        got = [getattr(q, n) for n, _ in flame_amd.MeshFilterParams._fields_]
        assert got == want, got
    assert [n for n, _ in flame_amd.MeshFilterParams._fields_] == list(mr.DEFAULTS)
    assert all(F(mr.DEFAULTS[n]) == F(getattr(p, n)) for n in mr.DEFAULTS)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu(built):
    import torch  # noqa: F401

    import flame_amd

    return flame_amd


def check_outputs(flame_amd, reg, pos, tris, Kinv, rows, cols, scale, p=None, x=None, want_map=True, triangles_arg="given", what=""):
    """reg.mesh_outputs against the checker on state x (default: the downloaded one), every output bit for bit."""
    if x is None:
        x = reg.download_state(("x",))["x"]
    p = mr.params() if p is None else p
    arg = tris if triangles_arg == "given" else None
    got = reg.mesh_outputs(arg, Kinv, rows, cols, graph_scale=scale, filter=flame_amd.MeshFilterParams(**p), want_filtered_map=want_map)
    ref = mr.mesh_outputs(pos, x, tris, Kinv, rows, cols, graph_scale=scale, p=p)
    assert np.array_equal(bits(got["vtx_idepth"]), bits(ref["vtx_idepth"])), what + ": vtx_idepth"
    diff = np.flatnonzero(got["tri_valid"] != ref["tri_valid"])
    assert diff.size == 0, f"{what}: tri_valid differs at {diff[:8]} ({diff.size} of {len(tris)})"
    assert got["n_valid"] == ref["n_valid"], what
    bad = np.flatnonzero((bits(got["normals"]) != bits(ref["normals"])).any(axis=1))
    assert bad.size == 0, f"{what}: normals differ at vertices {bad[:8]} ({bad.size}): {got['normals'][bad[:2]]} vs {ref['normals'][bad[:2]]}"
    if want_map:
        fmap = oracle.raster_interpolate_mesh(tris, pos, ref["vtx_idepth"], rows, cols, tri_valid=ref["tri_valid"])
        assert np.array_equal(bits(got["filtered_map"])[~np.isnan(fmap)], bits(fmap)[~np.isnan(fmap)]), what + ": filtered map"
        assert np.array_equal(np.isnan(got["filtered_map"]), np.isnan(fmap)), what + ": filtered map coverage pattern"
        assert got["filtered_coverage"] == oracle.raster_coverage(np.ascontiguousarray(fmap)), what
    else:
        assert "filtered_map" not in got
    return got, ref


def kinv_for(cols, rows):
    return pinhole_kinv(fx=0.82 * cols, fy=0.81 * cols, cx=0.5 * cols + 10.5, cy=0.5 * rows - 9.75)


@pytest.mark.gpu
def test_gpu_mesh_outputs_synthetic_graphs_and_every_test_mixed(gpu):
    """320x240 and 640x480, initial state and after 300 iterations, graph_scale 1 and 0.37, the reference's defaults; plus
    min_triangle_idepth 0.8 and edge_length_thresh 0.02.  Over all cases each of the five comparisons clears and keeps a triangle."""
    cleared, kept = set(), set()
    for config in ("320x240", "640x480"):
        w, h, _ = synth.CONFIGS[config]
        g = synth.make_graph(config, seed=31)
        tris = synth.delaunay_triangles_scipy(g["pos"])
        Kinv = kinv_for(w, h)
        with gpu.Regularizer(0) as reg:
            reg.upload_graph(g)
            for iters in (0, 300):
                if iters:
                    reg.run(gpu.Params(), iters)
                x = reg.download_state(("x",))["x"]
                cases = [(1.0, mr.params()), (0.37, mr.params())]
                if iters == 0:
                    cases += [(1.0, mr.params(min_triangle_idepth=0.8)), (1.0, mr.params(edge_length_thresh=0.02))]
                for scale, p in cases:
                    what = f"{config} after {iters} iterations, scale {scale}, {p}"
                    _, ref = check_outputs(gpu, reg, g["pos"], tris, Kinv, h, w, scale, p, x=x, what=what)
                    t = mr.filter_tests(g["pos"], ref["vtx_idepth"], tris, Kinv, w, p)
                    for k, v in t.items():
                        print(what, k, int(v.sum()), "of", len(v))
                        if v.any():
                            cleared.add(k)
                        if not v.all():
                            kept.add(k)
    assert cleared == kept == {"angle", "rel", "abs", "edge", "mean"}, (cleared, kept)


@pytest.fixture(scope="module")
def small(gpu):
    g = synth.make_graph("320x240", seed=9)
    return g, synth.delaunay_triangles_scipy(g["pos"]), kinv_for(320, 240)


@pytest.mark.gpu
def test_gpu_filters_switched_off_one_by_one_all_off_and_rejecting_all(gpu, small):
    g, tris, Kinv = small
    with gpu.Regularizer(0) as reg:
        reg.upload_graph(g)
        for off in ("do_oblique_triangle_filter", "do_edge_length_filter", "do_idepth_triangle_filter"):
            check_outputs(gpu, reg, g["pos"], tris, Kinv, 240, 320, 1.0, mr.params(**{off: False}), what=off + " off")
        all_off = mr.params(do_oblique_triangle_filter=False, do_edge_length_filter=False, do_idepth_triangle_filter=False)
        got, _ = check_outputs(gpu, reg, g["pos"], tris, Kinv, 240, 320, 1.0, all_off, what="all off")
        assert got["n_valid"] == len(tris) and got["tri_valid"].all()
        plain, cov = reg.interpolate_mesh(tris, 240, 320)
        assert np.array_equal(got["filtered_map"], plain, equal_nan=True) and got["filtered_coverage"] == cov
        for p in (only(oblique_normal_thresh=-1.0), only(oblique_idepth_diff_abs=-1.0), only(edge_length_thresh=0.0),
                  only(min_triangle_idepth=INF)):
            got, _ = check_outputs(gpu, reg, g["pos"], tris, Kinv, 240, 320, 1.0, p, what=f"rejecting all: {p}")
            assert got["n_valid"] == 0 and got["filtered_coverage"] == 0 and np.isnan(got["filtered_map"]).all()
        got, _ = check_outputs(gpu, reg, g["pos"], tris, Kinv, 240, 320, 1.0, only(oblique_normal_thresh=float("nan")), what="NaN threshold")
        assert got["n_valid"] == len(tris)


@pytest.mark.gpu
def test_gpu_windings_degenerate_and_repeated_vertices(gpu, small):
    g, tris, Kinv = small
    pos = g["pos"]
    with gpu.Regularizer(0) as reg:
        reg.upload_graph(g)
        rev = np.ascontiguousarray(tris[:, ::-1])
        _, a = check_outputs(gpu, reg, pos, tris, Kinv, 240, 320, 1.0, what="winding as triangulated")
        _, b = check_outputs(gpu, reg, pos, rev, Kinv, 240, 320, 1.0, what="winding reversed")
        assert a["n_valid"] > 0 and b["n_valid"] < a["n_valid"]  # (d changes sign: the angle test now clears what faced the camera)
        # degenerate: three collinear back-projections (equal idepth on a pixel line) -> zero cross product, zero normal;
        # repeated vertices: (v, v, u), (v, v, v)
        x = reg.download_state(("x",))["x"]
        line = np.array([20, 21, 22])
        pos2 = pos.copy()
        pos2[21] = pos[20] + F([3, 0])  # three vertices on one pixel row with one idepth: delta y and delta z are exactly 0
        pos2[22] = pos[20] + F([7, 0])
        x2 = x.copy()
        x2[line] = F(0.75)
        # and a plane perpendicular to its viewing ray on which the rounding leaves d = 1.0000001: just outside [-1, 1], where the
        # reference's acos gives a NaN angle that rejects nothing (found with the checker; asserted below)
        pos2[[30, 31, 32]] = F([[264.8751525878906, 113.89742279052734], [249.28048706054688, 113.39288330078125], [257.4194030761719, 100.96844482421875]])
        x2[[30, 31, 32]] = F([0.6578121781349182, 0.646276593208313, 0.6523892283439636])
        odd = np.array([line, [5, 5, 9], [7, 7, 7], [9, 5, 5], [30, 31, 32]], np.int32)
        d_odd, _, _ = mr.triangle_geometry(pos2, x2, odd, Kinv)
        assert d_odd[4] > 1 and not d_odd[:4].any()
        tr = np.concatenate([tris[:50], odd, tris[50:90]]).astype(np.int32)
        g2 = synth.copy_graph(g)
        g2["pos"] = pos2
        reg.upload_graph(g2)
        reg.upload_state({"x": x2})
        check_outputs(gpu, reg, pos2, tr, Kinv, 240, 320, 1.0, only(oblique_normal_thresh=1.39626), x=x2, what="degenerate and repeated")
        check_outputs(gpu, reg, pos2, odd, Kinv, 240, 320, 1.0, x=x2, what="only the odd triangles")
        got, _ = check_outputs(gpu, reg, pos2, odd, Kinv, 240, 320, 1.0, only(oblique_normal_thresh=-1.0), x=x2, what="d outside [-1, 1]")
        assert got["tri_valid"].tolist() == [0, 0, 0, 0, 1]  # (a threshold that rejects every d of [-1, 1] keeps the one outside)


@pytest.mark.gpu
def test_gpu_each_comparison_at_its_threshold(gpu, small):
    """The known-answer triangles of the CPU part on the device: the compared quantity exactly AT the threshold clears nothing
    (all five comparisons are strict), one ulp beyond it does."""
    g, _, Kinv = small
    pos, x = g["pos"].copy(), g["x"].copy()
    pos[[40, 41, 42]] = F([[0, 0], [3, 4], [0, 1]])  # longest squared edge 25 = (0.015625 * 320)^2
    x[[40, 41, 42]] = F([0.5, 0.75, 1.0])            # max - min = 0.5, (max - min) / max = 0.5, mean = 0.75
    tp, tid = tilted_triangle(1.2)
    pos[[50, 51, 52]], x[[50, 51, 52]] = tp, tid
    tr = np.array([[40, 41, 42], [50, 51, 52]], np.int32)
    d, _, _ = mr.triangle_geometry(pos, x, tr, Kinv)
    own = float(F(np.arccos(np.float64(d[1]))))
    up, down = (lambda v: float(mr.next_float(v, 1))), (lambda v: float(mr.next_float(v, -1)))
    g2 = synth.copy_graph(g)
    g2["pos"] = pos
    with gpu.Regularizer(0) as reg:
        reg.upload_graph(g2)
        reg.upload_state({"x": x})
        for name, at, beyond, t in (("oblique_idepth_diff_abs", 0.5, down(0.5), 0), ("oblique_idepth_diff_factor", 0.5, down(0.5), 0),
                                    ("edge_length_thresh", 0.015625, down(0.015625), 0), ("min_triangle_idepth", 0.75, up(0.75), 0),
                                    ("oblique_normal_thresh", own, down(own), 1)):
            got, _ = check_outputs(gpu, reg, pos, tr, Kinv, 240, 320, 1.0, only(**{name: at}), x=x, what=name + " at the threshold")
            assert got["tri_valid"][t] == 1, name
            got, _ = check_outputs(gpu, reg, pos, tr, Kinv, 240, 320, 1.0, only(**{name: beyond}), x=x, what=name + " one ulp beyond")
            assert got["tri_valid"][t] == 0, name


@pytest.mark.gpu
def test_gpu_special_idepths(gpu, small):
    """0, -0, negative, subnormal, +inf and NaN at chosen vertices (via upload_state) and everywhere (graph_scale 0 and inf): the
    skip rule of the normals (idepth <= 0 skips, NaN does not), NaN never clearing validity."""
    g, tris, Kinv = small
    with gpu.Regularizer(0) as reg:
        reg.upload_graph(g)
        x = g["x"].copy()
        special = [0.0, -0.0, -0.5, 1e-42, INF, float("nan")]
        for i, s in enumerate(special):
            x[10 + 7 * i] = F(s)
        reg.upload_state({"x": x})
        got, ref = check_outputs(gpu, reg, g["pos"], tris, Kinv, 240, 320, 1.0, x=x, what="special idepths")
        touched = np.isin(tris, [10 + 7 * i for i in range(len(special))]).any(axis=1)
        assert touched.sum() > 12 and np.isnan(got["normals"]).any()
        # a NaN in a compared quantity never clears validity: with every idepth NaN (graph_scale NaN) all of angle, relative and
        # absolute difference and mean are NaN, whatever the thresholds
        p = only(oblique_normal_thresh=0.0, oblique_idepth_diff_factor=-1.0, oblique_idepth_diff_abs=-1.0, min_triangle_idepth=INF)
        got, _ = check_outputs(gpu, reg, g["pos"], tris, Kinv, 240, 320, float("nan"), p, x=g["x"], what="NaN never clears validity")
        assert got["n_valid"] == len(tris) and np.isnan(got["normals"][np.unique(tris)]).all()
        got, _ = check_outputs(gpu, reg, g["pos"], tris, Kinv, 240, 320, 1.0, p, x=x, what="the same thresholds on finite idepths")
        assert not got["tri_valid"][~touched].any()
        for scale in (0.0, INF, -1.0):
            got, _ = check_outputs(gpu, reg, g["pos"], tris, Kinv, 240, 320, scale, x=x, what=f"graph_scale {scale}")
        reg.upload_state({"x": g["x"]})
        got, _ = check_outputs(gpu, reg, g["pos"], tris, Kinv, 240, 320, 0.0, what="graph_scale 0")
        assert not got["normals"].any()  # every triangle skipped: (0, 0, 0)


@pytest.mark.gpu
def test_gpu_hub_of_300_triangles_in_either_order(gpu, small):
    g, tris, Kinv = small
    fan = np.array([[0, i, i + 1] for i in range(1, 301)], np.int32)
    rng = np.random.default_rng(4)
    shuffled = fan[rng.permutation(300)]
    with gpu.Regularizer(0) as reg:
        reg.upload_graph(g)
        a, _ = check_outputs(gpu, reg, g["pos"], fan, Kinv, 240, 320, 1.0, what="fan")
        b, _ = check_outputs(gpu, reg, g["pos"], shuffled, Kinv, 240, 320, 1.0, what="fan, shuffled")
        assert not np.array_equal(bits(a["normals"][0]), bits(b["normals"][0]))  # (each equals the checker for its own order)
        both = np.concatenate([tris, shuffled, tris[::-1]]).astype(np.int32)
        check_outputs(gpu, reg, g["pos"], both, Kinv, 240, 320, 1.0, what="mesh + fan + mesh again")


@pytest.mark.gpu
def test_gpu_empty_lists_resident_triangles_and_errors(gpu, small):
    g, tris, Kinv = small
    with gpu.Regularizer(0) as reg:
        with pytest.raises(gpu.NLTGV2Error) as ei:
            reg.mesh_outputs(tris, Kinv, 240, 320)
        assert ei.value.status == -4  # no graph
        reg.upload_graph(g)
        got, _ = check_outputs(gpu, reg, g["pos"], np.zeros((0, 3), np.int32), Kinv, 240, 320, 1.0, what="T = 0")
        assert got["n_valid"] == 0 and not got["normals"].any() and np.isnan(got["filtered_map"]).all()
        part = tris[: len(tris) // 3]  # leaves vertices in no triangle
        got, _ = check_outputs(gpu, reg, g["pos"], part, Kinv, 240, 320, 1.0, what="a third of the mesh")
        lonely = np.setdiff1d(np.arange(g["V"]), part.ravel())
        assert lonely.size and not got["normals"][lonely].any()
        # triangles = NULL: what interpolate_mesh_begin left on the device
        with gpu.Regularizer(0) as fresh:
            fresh.upload_graph(g)
            with pytest.raises(gpu.NLTGV2Error) as ei:
                fresh.mesh_outputs(len(tris), Kinv, 240, 320)  # nothing resident yet
            assert ei.value.status == -1
        reg.interpolate_mesh_begin(tris, 240, 320, graph_scale=1.25)
        same, _ = check_outputs(gpu, reg, g["pos"], tris, Kinv, 240, 320, 1.25, triangles_arg="resident", what="resident triangles")
        again, _ = check_outputs(gpu, reg, g["pos"], tris, Kinv, 240, 320, 1.25, what="the same triangles passed again")
        for k in ("tri_valid", "normals", "vtx_idepth", "filtered_map"):
            assert np.array_equal(same[k], again[k], equal_nan=True), k
        reg.interpolate_mesh_end()
        # errors: reported before anything is enqueued, the earlier outputs stay
        reg.mesh_outputs_begin(tris, Kinv, 240, 320, graph_scale=1.25, want_filtered_map=True)
        bad = tris.copy()
        bad[17, 1] = g["V"]
        neg = tris.copy()
        neg[3, 0] = -1
        for call in (lambda: reg.mesh_outputs_begin(len(tris) - 1, Kinv, 240, 320),       # another T than the resident one
                     lambda: reg.mesh_outputs_begin(bad, Kinv, 240, 320),
                     lambda: reg.mesh_outputs_begin(neg, Kinv, 240, 320),
                     lambda: reg.mesh_outputs_begin(tris, Kinv, 0, 320),
                     lambda: reg.mesh_outputs_begin(tris, Kinv, 240, -1)):
            with pytest.raises(gpu.NLTGV2Error) as ei:
                call()
            assert ei.value.status == -1
        lib = gpu.load_library()
        tp = np.ascontiguousarray(tris, np.int32)
        IP, FP = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        f = gpu.MeshFilterParams()
        assert lib.flame_nltgv2_mesh_outputs_begin(reg._ctx, tp.ctypes.data_as(IP), len(tp), None, C.byref(f), 240, 320, C.c_float(1), 0) == -1
        assert lib.flame_nltgv2_mesh_outputs_begin(reg._ctx, tp.ctypes.data_as(IP), len(tp), Kinv.ctypes.data_as(FP), None, 240, 320, C.c_float(1), 0) == -1
        kept = reg.mesh_outputs_end()
        for k in ("tri_valid", "normals", "vtx_idepth", "filtered_map"):
            assert np.array_equal(kept[k], again[k], equal_nan=True), k
        assert kept["n_valid"] == again["n_valid"] and kept["filtered_coverage"] == again["filtered_coverage"]
        # a new topology: the resident triangles belong to the old one
        g2 = synth.make_graph("320x240", seed=10)
        reg.upload_graph(g2)
        with pytest.raises(gpu.NLTGV2Error):
            reg.mesh_outputs_begin(len(tris), Kinv, 240, 320)


@pytest.mark.gpu
def test_gpu_resident_map_survives_the_filtered_map(gpu, small):
    """interpolate_mesh_begin / _end, then mesh_outputs with the filtered map: a sync_graph with init_from_map starts its new
    vertices exactly where it does without the mesh_outputs call, and interpolate_mesh_end's pinned map is unchanged."""
    g, tris, Kinv = small
    rng = np.random.default_rng(8)
    V = g["V"]
    keep = np.sort(rng.permutation(V)[: V - 40])
    new_pos = (rng.random((60, 2)) * [300, 220] + 10).astype(F)
    feat_id = np.concatenate([keep, np.arange(V, V + 60)]).astype(np.int32)
    pos = np.concatenate([g["pos"][keep], new_pos]).astype(F)
    data = np.concatenate([g["data_term"][keep], np.full(60, 0.6, F)]).astype(F)
    weight = np.ones(len(feat_id), F)
    edges = synth.delaunay_edges_scipy(pos)
    states, maps = [], []
    for with_outputs in (False, True):
        with gpu.Regularizer(0) as reg:
            reg.upload_graph(g)
            reg.run(gpu.Params(), 40)
            reg.interpolate_mesh_begin(tris, 240, 320, graph_scale=1.25)
            dense_view, cov = reg.interpolate_mesh_end(copy=False)
            dense = dense_view.copy()
            if with_outputs:
                got, _ = check_outputs(gpu, reg, g["pos"], tris, Kinv, 240, 320, 1.25, triangles_arg="resident", what="beside the resident map")
                assert got["filtered_coverage"] < cov  # (the filtered map differs: had it gone into the resident buffer, the sync would show it)
                assert np.array_equal(dense_view, dense, equal_nan=True), "interpolate_mesh_end's pinned map changed"
            reg.sync_graph(feat_id, pos, data, weight, edges, init_graph_scale=1.25, init_from_map=True)
            states.append(reg.download_state())
            maps.append(dense)
    assert np.array_equal(maps[0], maps[1], equal_nan=True)
    for k in states[0]:
        assert np.array_equal(bits(states[0][k]), bits(states[1][k])), k
    assert not np.array_equal(states[0]["x"][-60:], data[-60:])  # (the new vertices did start at the map's prediction)


@pytest.mark.gpu
def test_gpu_state_of_the_last_settle_and_the_stage_only_reads(gpu, small):
    """FLAME_NLTGV2_OPT_MESH_STATE = 1: settle, download, interpolate_mesh_begin, run_async(2000), mesh_outputs_begin -- the outputs
    are those of the downloaded state; afterwards the solver's state equals that of a context that never made the calls."""
    from flame_amd.regularizer import OPT_MESH_STATE

    g, tris, Kinv = small
    params = gpu.Params()
    with gpu.Regularizer(0) as reg, gpu.Regularizer(0) as plain:
        reg.upload_graph(g), plain.upload_graph(g)
        reg.run(params, 40), plain.run(params, 40)
        reg.set_option(OPT_MESH_STATE, 1)
        at40 = reg.download_state()
        plain.download_state()
        reg.interpolate_mesh_begin(tris, 240, 320, graph_scale=0.9)
        reg.run_async(params, 2000)
        reg.mesh_outputs_begin(None, Kinv, 240, 320, graph_scale=0.9, want_filtered_map=True)
        dense, cov = reg.interpolate_mesh_end()
        got = reg.mesh_outputs_end()
        ref = mr.mesh_outputs(g["pos"], at40["x"], tris, Kinv, 240, 320, graph_scale=0.9)
        assert np.array_equal(bits(got["vtx_idepth"]), bits(ref["vtx_idepth"])) and np.array_equal(got["tri_valid"], ref["tri_valid"])
        assert np.array_equal(bits(got["normals"]), bits(ref["normals"])) and got["n_valid"] == ref["n_valid"]
        fmap = oracle.raster_interpolate_mesh(tris, g["pos"], ref["vtx_idepth"], 240, 320, tri_valid=ref["tri_valid"])
        assert np.array_equal(got["filtered_map"], fmap, equal_nan=True)
        assert np.array_equal(dense, oracle.raster_interpolate_mesh(tris, g["pos"], ref["vtx_idepth"], 240, 320), equal_nan=True)
        plain.run(params, 2000)
        a, b = reg.download_state(), plain.download_state()
        for k in a:
            assert np.array_equal(bits(a[k]), bits(b[k])), k
        assert not np.array_equal(a["x"], at40["x"])
        # default option: the runs are settled, the outputs are of what they leave
        reg.set_option(OPT_MESH_STATE, 0)
        reg.run_async(params, 30)
        got = reg.mesh_outputs(tris, Kinv, 240, 320, graph_scale=0.9)
        x = reg.download_state(("x",))["x"]
        assert not np.array_equal(x, a["x"])
        assert np.array_equal(bits(got["vtx_idepth"]), bits(mr.vertex_idepths(x, 0.9)))


@pytest.mark.gpu
def test_gpu_run_twice_and_under_every_persistent_form(gpu):
    from flame_amd.regularizer import OPT_PERSISTENT

    g = synth.make_graph("640x480", seed=5)
    tris = synth.delaunay_triangles_scipy(g["pos"])
    Kinv = kinv_for(640, 480)
    paths, first = set(), None
    for form in (1, 0, 3, 4, 6):
        with gpu.Regularizer(0) as reg:
            reg.set_option(OPT_PERSISTENT, form)
            reg.upload_graph(g)
            reg.run(gpu.Params(), 120)
            paths.add(reg.info()["last_run_path"])
            a = reg.mesh_outputs(tris, Kinv, 480, 640, graph_scale=1.1, want_filtered_map=True)  # straight from the packed state
            b = reg.mesh_outputs(tris, Kinv, 480, 640, graph_scale=1.1, want_filtered_map=True)
            for k in ("tri_valid", "normals", "vtx_idepth", "filtered_map"):
                assert a[k].tobytes() == b[k].tobytes(), (form, k)  # (the same device twice: NaN patterns included)
            assert a["n_valid"] == b["n_valid"] and a["filtered_coverage"] == b["filtered_coverage"]
            if first is None:
                first, _ = check_outputs(gpu, reg, g["pos"], tris, Kinv, 480, 640, 1.1, what=f"form {form}")
            for k in ("tri_valid", "normals", "vtx_idepth", "filtered_map"):
                assert np.array_equal(a[k], first[k], equal_nan=True), (form, k)
    assert len(paths) >= 3, paths
