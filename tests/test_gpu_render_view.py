"""flame_nltgv2_render_view_begin / _end / _arrays through the C-ABI against the checker tests/view_ref.py, bit for bit: the map as
uint32, the owner indices and the four counters equal.  The one-triangle cases of tests/test_render_view_ref.py through both forms,
targets of other sizes and cameras than the source, a triangle that covers the whole target, a mesh past 256 workgroups, no triangles
at all, repeats, a smaller mesh behind a larger one, the three sources of validity, every error before anything is enqueued, runs in
flight, and what the _arrays form leaves alone."""
import numpy as np
import pytest

from flame_amd import synth
from tests import test_render_view_ref as cases
from tests import view_ref as vr
from tests.metric_helpers import fetch

F = np.float32
EYE = np.eye(3, dtype=F)
SRC = (48, 64)  # rows, cols of the source view
K, KINV = cases.camera(60.0, 32.0, 24.0)


@pytest.fixture(scope="module")
def gpu(built):
    import torch  # noqa: F401

    import flame_amd

    assert hasattr(flame_amd.load_library(), "flame_nltgv2_render_view_begin")
    return flame_amd


@pytest.fixture(scope="module")
def reg(gpu):
    with gpu.Regularizer(0) as r:
        yield r


def graph_of(pos, idepth, tris):
    """A graph whose vertices are the mesh's, x its inverse depths and edges the triangles' sides."""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    e = np.unique(np.sort(e, axis=1), axis=0).astype(np.int32)
    return synth.assemble_graph(np.asarray(pos, F), np.asarray(idepth, F), e)


def make_resident(reg, pos, idepth, tris):
    reg.upload_graph(graph_of(pos, idepth, tris))
    reg.interpolate_mesh(tris, *SRC)


def view_params(gpu, c, **kw):
    return gpu.ViewParams(Kinv_src=c.get("Kinv_src"), K_dst=c.get("K_dst"), R=c.get("R"), t=c.get("t"), near_depth=c.get("near_depth", 0.0), **kw)


def both_forms(gpu, reg, c, what):
    """The case through begin / end on the resident mesh and through the _arrays form; both against the checker."""
    rows, cols = c.get("rows", 8), c.get("cols", 8)
    want = cases.render(c)
    tv = c.get("tri_valid")
    validity = 0 if tv is None else 1
    make_resident(reg, c["pos"], c["idepth"], c["tris"])
    got = reg.render_view(view_params(gpu, c, validity=validity), rows, cols, tri_valid=tv)
    vr.assert_same(got, want, what + " (resident)")
    assert "map" in got and "tri_index" in got and got["T"] == len(c["tris"]) and (got["rows"], got["cols"]) == (rows, cols)
    arr = reg.render_view_arrays(view_params(gpu, c, validity=validity), c["tris"], c["pos"], c["idepth"], rows, cols, tri_valid=tv)
    vr.assert_same(arr, want, what + " (arrays)")
    return got, want


def mesh_case(seed, step=6, **cam):
    pos, tris = cases.grid_mesh(*SRC, step, seed=seed)
    idepth = np.random.default_rng(seed).uniform(0.3, 1.5, len(pos)).astype(F)
    return dict(dict(tris=tris, pos=pos, idepth=idepth, Kinv_src=KINV, K_dst=K, rows=SRC[0], cols=SRC[1]), **cam)


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases.one_triangle_cases(), ids=lambda c: c["name"])
def test_gpu_one_triangle_per_rule(gpu, reg, case):
    got, _ = both_forms(gpu, reg, case, case["name"])
    if case["expect"] is not None:
        assert cases.counts(got) == case["expect"]


TARGETS = {
    "1x1": dict(rows=1, cols=1, K_dst=cases.camera(60.0, 2.0, 2.0)[0]),
    "5x3_downscaled": dict(rows=3, cols=5, K_dst=cases.camera(6.0, 2.5, 1.5)[0], t=np.array([0.1, 0, 0], F)),
    "64x48_translated": dict(rows=48, cols=64, t=np.array([0.5, -0.1, 0.05], F)),
    "75x100_other_camera_turned_20_degrees": dict(rows=75, cols=100, K_dst=cases.camera(90.0, 50.0, 37.5)[0], R=cases.rotation_y(20.0),
                                                  t=np.array([-0.6, 0.05, 0.1], F)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TARGETS))
def test_gpu_targets_of_other_sizes_and_cameras(gpu, reg, name):
    """(75 x 100 and 5 x 3 pixels are no multiple of the resolve's tile of 2048.)"""
    got, want = both_forms(gpu, reg, mesh_case(11, **TARGETS[name]), name)
    assert want["coverage"] > 0 and want["tris_drawn"] > 0
    if name.startswith("75x100"):
        assert want["coverage"] > 2048


@pytest.mark.gpu
def test_gpu_one_triangle_over_the_whole_target(gpu, reg):
    c = dict(tris=np.array([[0, 1, 2]], np.int32), pos=np.array([[-100, -100], [300, -100], [-100, 300]], F), idepth=np.array([0.4, 1.1, 2.3], F),
             Kinv_src=KINV, K_dst=K, t=np.array([0.05, 0, 0], F), rows=48, cols=64)
    got, want = both_forms(gpu, reg, c, "whole target")
    assert got["coverage"] == 48 * 64
    # a box of 2048 pixels is the last one a wavefront walks alone; from 2049 on it is shared
    for rows in (32, 33):
        got, _ = both_forms(gpu, reg, dict(c, rows=rows), "whole target of %d rows" % rows)
        assert got["coverage"] == rows * 64


@pytest.mark.gpu
def test_gpu_more_large_triangles_than_are_in_work_at_a_time(gpu, reg):
    """150 triangles that each cover the whole 64x48 target (more than the 128 list rows of the kernel for large boxes), at inverse
    depths that cross each other inside the image."""
    rng = np.random.default_rng(19)
    n = 150
    corners = np.array([[-10, -10], [150, -10], [-10, 130]], F)
    pos = (corners[None] + rng.uniform(-8, 8, (n, 3, 2))).reshape(-1, 2).astype(F)
    c = dict(tris=np.arange(3 * n, dtype=np.int32).reshape(n, 3), pos=pos, idepth=rng.uniform(0.3, 2.0, 3 * n).astype(F), Kinv_src=KINV, K_dst=K,
             t=np.array([0.05, 0, 0], F), rows=48, cols=64)
    got, want = both_forms(gpu, reg, c, "150 large triangles")
    assert got["coverage"] == 48 * 64 and got["tris_drawn"] == n and len(np.unique(got["tri_index"])) > 3


@pytest.mark.gpu
def test_gpu_a_mesh_past_256_workgroups_and_the_box_scene(gpu, reg):
    c = mesh_case(12, step=3, t=np.array([0.3, 0.1, 0], F), R=cases.rotation_y(-5.0))
    assert len(c["tris"]) >= 600
    both_forms(gpu, reg, c, "630 triangles")
    box, near = cases.box_scene()
    got, want = both_forms(gpu, reg, box, "box")
    assert got["tris_culled_facing"] > 0
    n_near = near[box["tris"]].sum(1)
    both_forms(gpu, reg, dict(box, tri_valid=(n_near == 3).astype(np.uint8)), "box, near layer")


@pytest.mark.gpu
def test_gpu_no_triangles(gpu, reg):
    c = mesh_case(13)
    c["tris"] = np.zeros((0, 3), np.int32)
    got, want = both_forms(gpu, reg, c, "T = 0")
    assert cases.counts(got) == (0, 0, 0, 0) and (vr.bits(got["map"]) == vr.HOLE).all() and (got["tri_index"] == -1).all()


@pytest.mark.gpu
def test_gpu_two_calls_give_the_same_bytes_and_a_smaller_mesh_sees_no_stale_keys(gpu, reg):
    big = mesh_case(14, step=3, t=np.array([0.4, 0, 0], F))
    make_resident(reg, big["pos"], big["idepth"], big["tris"])
    p = view_params(gpu, big)
    a, b = reg.render_view(p, *SRC), reg.render_view(p, *SRC)
    assert a["map"].tobytes() == b["map"].tobytes() and a["tri_index"].tobytes() == b["tri_index"].tobytes() and cases.counts(a) == cases.counts(b)
    vr.assert_same(a, cases.render(big), "the larger mesh")
    # a third of the triangles on a smaller target, in the buffers the larger call left behind
    small = dict(big, tris=big["tris"][::3], rows=30, cols=40)
    got, want = both_forms(gpu, reg, small, "the smaller mesh")
    assert 0 < got["coverage"] < 30 * 40
    # the outputs one by one, and on the device alone
    make_resident(reg, big["pos"], big["idepth"], big["tris"])
    only_map = reg.render_view(view_params(gpu, big, want_tri_index=False), *SRC)
    only_idx = reg.render_view(view_params(gpu, big, want_map=False), *SRC)
    assert "tri_index" not in only_map and "map" not in only_idx and list(only_map["device"]) == ["map"] and list(only_idx["device"]) == ["tri_index"]
    vr.assert_same(only_map, cases.render(big), "map alone")
    vr.assert_same(only_idx, cases.render(big), "tri_index alone")
    dev = reg.render_view(view_params(gpu, big, copy_out=False), *SRC)
    assert "map" not in dev and "tri_index" not in dev and cases.counts(dev) == cases.counts(a)
    assert fetch(dev["device"]["map"], SRC, F).tobytes() == a["map"].tobytes()
    assert fetch(dev["device"]["tri_index"], SRC, np.int32).tobytes() == a["tri_index"].tobytes()


@pytest.mark.gpu
def test_gpu_validity_from_nowhere_the_host_and_the_filters(gpu, reg):
    c = mesh_case(15, t=np.array([0.3, 0, 0], F))
    tris = c["tris"]
    make_resident(reg, c["pos"], c["idepth"], tris)
    mo = reg.mesh_outputs(None, KINV, *SRC, filter=gpu.MeshFilterParams(do_oblique_triangle_filter=False, do_edge_length_filter=False, min_triangle_idepth=0.6))
    filt = np.asarray(mo["tri_valid"], np.uint8)
    assert 0 < filt.sum() < len(tris)
    got = reg.render_view(view_params(gpu, c, validity=2), *SRC)
    vr.assert_same(got, cases.render(c, tri_valid=filt), "validity 2")
    assert got["tris_drawn"] + got["tris_culled_vertex"] + got["tris_culled_facing"] == filt.sum()
    mask = (np.arange(len(tris)) % 3 != 0).astype(np.uint8)
    vr.assert_same(reg.render_view(view_params(gpu, c, validity=1), *SRC, tri_valid=mask), cases.render(c, tri_valid=mask), "validity 1")
    vr.assert_same(reg.render_view(view_params(gpu, c, validity=0), *SRC), cases.render(c), "validity 0")
    # another upload of triangles makes the filters' validity stale
    reg.interpolate_mesh(tris[::-1].copy(), *SRC)
    with pytest.raises(gpu.NLTGV2Error):
        reg.render_view_begin(view_params(gpu, c, validity=2), *SRC)
    for validity, tv in ((0, mask), (1, None), (2, mask), (3, None), (-1, None)):
        with pytest.raises(gpu.NLTGV2Error):
            reg.render_view_begin(view_params(gpu, c, validity=validity), *SRC, tri_valid=tv)


@pytest.mark.gpu
def test_gpu_every_error_comes_before_anything_is_enqueued_and_leaves_the_previous_outputs(gpu):
    c = mesh_case(16, t=np.array([0.2, 0, 0], F))
    p = view_params(gpu, c)
    with gpu.Regularizer(0) as reg:
        with pytest.raises(gpu.NLTGV2Error):  # no graph
            reg.render_view_begin(p, *SRC)
        reg.upload_graph(graph_of(c["pos"], c["idepth"], c["tris"]))
        with pytest.raises(gpu.NLTGV2Error):  # no resident triangles
            reg.render_view_begin(p, *SRC)
        with pytest.raises(gpu.NLTGV2Error):  # nothing begun
            reg.render_view_end()
        reg.interpolate_mesh(c["tris"], *SRC)
        reg.render_view_begin(p, *SRC)
        for rows, cols in ((0, 64), (48, 0), (-1, 64), (32768, 64), (48, 32768)):
            with pytest.raises(gpu.NLTGV2Error):
                reg.render_view_begin(p, rows, cols)
        with pytest.raises(gpu.NLTGV2Error):
            reg.render_view_begin(view_params(gpu, c, validity=2), *SRC)  # no mesh_outputs_begin yet
        with pytest.raises(gpu.NLTGV2Error):
            reg.render_view_begin(view_params(gpu, c, validity=1), *SRC)  # no array
        for bad in (dict(triangles=np.array([[0, 1, len(c["pos"])]], np.int32)), dict(triangles=np.array([[0, -1, 2]], np.int32)), dict(rows=0),
                    dict(validity=2), dict(validity=1)):
            a = dict(dict(triangles=c["tris"], rows=48, validity=0), **bad)
            with pytest.raises(gpu.NLTGV2Error):
                reg.render_view_arrays(view_params(gpu, c, validity=a["validity"]), a["triangles"], c["pos"], c["idepth"], a["rows"], 64)
        # the begin before all those errors still has its _end, with its outputs
        got = reg.render_view_end()
        vr.assert_same(got, cases.render(c), "the view begun before the errors")
        assert got["device_ms"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("mesh_state", [0, 1])
def test_gpu_runs_in_flight(gpu, mesh_state):
    """Behind run_async the stage describes the state interpolate_mesh_begin would: with FLAME_NLTGV2_OPT_MESH_STATE = 0 the state the
    runs leave, with 1 the state the last settle left -- and the solver's result is the same as without the stage."""
    from flame_amd.regularizer import OPT_MESH_STATE

    g = synth.make_graph("320x240", seed=5)
    tris = synth.delaunay_triangles_scipy(g["pos"])
    Kqinv = cases.camera(250.0, 160.0, 120.0)[1]
    cam = dict(Kinv_src=Kqinv, K_dst=cases.camera(125.0, 80.0, 60.0)[0], t=np.array([0.05, 0, 0], F))  # a target of half the size
    params = gpu.Params()
    with gpu.Regularizer(0) as reg, gpu.Regularizer(0) as plain:
        for r in (reg, plain):
            r.set_option(OPT_MESH_STATE, mesh_state)
            r.upload_graph(g)
            r.run(params, 20)
        before = reg.download_state(("x",))["x"]
        reg.interpolate_mesh_begin(tris, 240, 320)
        plain.interpolate_mesh_begin(tris, 240, 320)
        reg.run_async(params, 150)
        plain.run_async(params, 150)
        reg.render_view_begin(view_params(gpu, cam), 120, 160)
        got = reg.render_view_end()
        dense, _ = reg.interpolate_mesh_end()
        plain.interpolate_mesh_end()
        after = reg.download_state(("x",))["x"]
        assert not np.array_equal(before, after)
        assert np.array_equal(after, plain.download_state(("x",))["x"])  # the stage only read
        x = after if mesh_state == 0 else before
        vr.assert_same(got, vr.render_view(tris, g["pos"], x, Kqinv, cam["K_dst"], EYE, cam["t"], 120, 160), "mesh_state %d" % mesh_state)
        assert got["coverage"] > 10000


@pytest.mark.gpu
def test_gpu_arrays_form_leaves_the_resident_map_and_triangles_usable(gpu, reg):
    c = mesh_case(17, t=np.array([0.3, 0, 0], F))
    make_resident(reg, c["pos"], c["idepth"], c["tris"])
    dense, cov = reg.interpolate_mesh(c["tris"], *SRC)
    first = reg.render_view(view_params(gpu, c), *SRC)
    other = mesh_case(18, step=4, t=np.array([-0.2, 0, 0], F), rows=20, cols=90)
    arr = reg.render_view_arrays(view_params(gpu, other), other["tris"], other["pos"], other["idepth"], 20, 90)
    vr.assert_same(arr, cases.render(other), "the caller's mesh")
    # the resident triangles still serve this stage, the mesh outputs and the wireframe's bookkeeping; the resident map the metric stage
    again = reg.render_view(view_params(gpu, c), *SRC)
    assert again["map"].tobytes() == first["map"].tobytes() and again["tri_index"].tobytes() == first["tri_index"].tobytes()
    mo = reg.mesh_outputs(None, KINV, *SRC)
    assert len(mo["tri_valid"]) == len(c["tris"])
    depth = reg.metric_outputs(KINV, *SRC, params=gpu.MetricParams(want_depth_mm=False, want_organized=False, want_cloud=False))["depth"]
    ok = ~np.isnan(dense)
    assert ok.sum() == cov and depth.shape == SRC and (depth[ok] > 0).all()  # (the resident map is still the graph's, SRC in size)
