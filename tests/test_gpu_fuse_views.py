"""flame_nltgv2_keep_mesh* / flame_nltgv2_fuse_views_begin / _end through the C-ABI against the checker tests/fuse_ref.py, bit for bit:
fused and spread as uint32, both masks, the layers and all 32 counter words.  The scene of tests/test_fuse_views_ref.py at three
min_support; the store (a snapshot equals an upload, x * graph_scale, survival across topologies, drop and reuse, kept validity); one,
eight, live and doubled sources; the edges of the batched kernels (tiny and odd targets, empty sources, source boundaries inside a
workgroup, large boxes in one source and in three); repeats; outputs that stay on the device; every error before anything is enqueued."""
import numpy as np
import pytest

from flame_amd import synth
from tests import fuse_ref as fr
from tests import test_fuse_views_ref as ref
from tests import test_gpu_render_view as tg
from tests import view_ref as vr
from tests.metric_helpers import fetch, on_device

F = np.float32
SRC, K, KINV = ref.SRC, ref.K, ref.KINV


@pytest.fixture(scope="module")
def gpu(built):
    import torch  # noqa: F401

    import flame_amd

    assert hasattr(flame_amd.load_library(), "flame_nltgv2_fuse_views_begin")
    return flame_amd


@pytest.fixture(scope="module")
def reg(gpu):
    with gpu.Regularizer(0) as r:
        yield r


def fuse_source(gpu, slot, s, **kw):
    return gpu.FuseSource(slot=slot, Kinv_src=s.get("Kinv_src"), R=s.get("R"), t=s.get("t"), weight=s.get("weight", 1.0), **kw)


def keep_all(reg, sources):
    for i, s in enumerate(sources):
        reg.keep_mesh_arrays(i, s["tris"], s["pos"], s["idepth"], s.get("tri_valid"))


def fuse_kept(gpu, reg, sources, rows, cols, min_support=1, rel_tol=ref.REL_TOL, K_dst=K, what="", **kw):
    """The sources into slots 0 .. N - 1 and fused, with every output; against the checker."""
    keep_all(reg, sources)
    p = gpu.FuseParams(sources=[fuse_source(gpu, i, s) for i, s in enumerate(sources)], K_dst=K_dst, rel_tol=rel_tol, min_support=min_support,
                       want_layers=True, **kw)
    got = reg.fuse_views(p, rows, cols)
    want = fr.fuse_sources(sources, K_dst, rows, cols, rel_tol, min_support, kw.get("near_depth", 0.0))
    fr.assert_same(got, want, what)
    assert all(k in got for k in ("fused", "spread", "layers", "present_mask", "inlier_mask")) and got["n_sources"] == len(sources)
    return got, want


# ---- the scene -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("min_support", [1, 2, 3])
def test_gpu_the_scene(gpu, reg, min_support):
    ref.test_the_scene_has_every_support_outliers_ties_and_a_coverage_that_falls()  # the checker alone first: nothing passes by being empty
    want = ref.scene_fused(min_support)
    keep_all(reg, ref.scene())
    p = gpu.FuseParams(sources=[fuse_source(gpu, i, s) for i, s in enumerate(ref.scene())], K_dst=K, rel_tol=ref.REL_TOL, min_support=min_support,
                       want_layers=True)
    got = reg.fuse_views(p, *SRC)
    print("min_support %d: counters %s, device_ms %.3f" % (min_support, got["counts"].tolist(), got["device_ms"]))
    fr.assert_same(got, want, "the scene at min_support %d" % min_support)
    for s, r in enumerate(want["renders"]):  # each layer is the view renderer's picture of its source
        assert (vr.bits(got["layers"][s]) == vr.bits(r["map"])).all() and got["present"][s] == r["coverage"] > 0
    assert got["coverage"] == want["coverage"] > 0 and got["device_ms"] > 0


# ---- the store -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_a_snapshot_equals_an_upload_and_scales_x(gpu, reg):
    s = ref.plane_source(2)
    tg.make_resident(reg, s["pos"], s["idepth"], s["tris"])
    reg.keep_mesh(0)
    reg.keep_mesh_arrays(1, s["tris"], s["pos"], s["idepth"])
    a, b = reg.get_kept_mesh(0), reg.get_kept_mesh(1)
    for k in ("vertices", "idepths", "triangles"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["tri_valid"] is None and b["tri_valid"] is None and reg.kept_mesh_info(0) == (len(s["pos"]), len(s["tris"]), False)
    assert a["idepths"].tobytes() == s["idepth"].tobytes() and (a["triangles"] == s["tris"]).all()
    outs = [reg.fuse_views(gpu.FuseParams(sources=[fuse_source(gpu, slot, s)], K_dst=K, want_layers=True), *SRC) for slot in (0, 1)]
    want = fr.fuse_sources([s], K, *SRC, 0.05, 1)
    for o in outs:
        fr.assert_same(o, want, "a snapshot and an upload")
    # ... and both are what render_view gives on the live mesh at this moment
    live = reg.render_view(gpu.ViewParams(Kinv_src=KINV, K_dst=K, R=s["R"], t=s["t"]), *SRC)
    assert vr.bits(live["map"]).tobytes() == vr.bits(outs[0]["layers"][0]).tobytes()
    # id = x * graph_scale in float32, for a scale that is no power of two
    reg.keep_mesh(2, graph_scale=1.7)
    scaled = (s["idepth"] * F(1.7)).astype(F)
    assert reg.get_kept_mesh(2)["idepths"].tobytes() == scaled.tobytes() and not np.array_equal(scaled, s["idepth"])
    got = reg.fuse_views(gpu.FuseParams(sources=[fuse_source(gpu, 2, s)], K_dst=K, want_layers=True), *SRC)
    fr.assert_same(got, fr.fuse_sources([dict(s, idepth=scaled)], K, *SRC, 0.05, 1), "x * 1.7")
    live = reg.render_view(gpu.ViewParams(Kinv_src=KINV, K_dst=K, R=s["R"], t=s["t"]), *SRC, graph_scale=1.7)
    assert vr.bits(live["map"]).tobytes() == vr.bits(got["layers"][0]).tobytes()


@pytest.mark.gpu
def test_gpu_a_slot_survives_other_topologies_and_is_dropped_and_reused(gpu):
    s = ref.plane_source(0)
    want = fr.fuse_sources([s], K, *SRC, 0.05, 1)
    p = gpu.FuseParams(sources=[fuse_source(gpu, 5, s)], K_dst=K, want_layers=True)
    with gpu.Regularizer(0) as reg:
        assert reg.kept_mesh_info(5) == (-1, -1, False)
        reg.drop_mesh(5)  # (dropping an empty slot is fine)
        g = tg.graph_of(s["pos"], s["idepth"], s["tris"])
        reg.upload_graph(g)
        reg.interpolate_mesh(s["tris"], *SRC)
        reg.keep_mesh(5)
        fr.assert_same(reg.fuse_views(p, *SRC), want, "fresh")
        # another graph altogether
        other = synth.make_graph("320x240", seed=3)
        reg.upload_graph(other)
        reg.run(gpu.Params(), 4)
        fr.assert_same(reg.fuse_views(p, *SRC), want, "after upload_graph of another graph")
        # a sync_graph that changes V
        V = int(other["V"]) - 40
        edges = np.stack([other["src"], other["dst"]], 1)
        edges = edges[(edges < V).all(1)]
        reg.set_feature_ids(np.arange(other["V"], dtype=np.int32))
        reg.sync_graph(np.arange(V, dtype=np.int32), other["pos"].reshape(-1, 2)[:V], other["data_term"][:V], other["data_weight"][:V], edges)
        assert reg.V == V
        fr.assert_same(reg.fuse_views(p, *SRC), want, "after a sync_graph that changed V")
        kept = reg.get_kept_mesh(5)
        assert kept["idepths"].tobytes() == s["idepth"].tobytes() and (kept["triangles"] == s["tris"]).all()
        # dropped: naming it is an error; reused with a larger mesh
        reg.drop_mesh(5)
        assert reg.kept_mesh_info(5) == (-1, -1, False)
        with pytest.raises(gpu.NLTGV2Error):
            reg.fuse_views_begin(p, *SRC)
        with pytest.raises(gpu.NLTGV2Error):
            reg.get_kept_mesh(5)
        big = ref.plane_source(0, step=2, seed=41)
        assert len(big["pos"]) > 4 * len(s["pos"])
        reg.keep_mesh_arrays(5, big["tris"], big["pos"], big["idepth"])
        assert reg.kept_mesh_info(5) == (len(big["pos"]), len(big["tris"]), False)
        fr.assert_same(reg.fuse_views(p, *SRC), fr.fuse_sources([big], K, *SRC, 0.05, 1), "the larger mesh in the reused slot")


@pytest.mark.gpu
def test_gpu_the_filters_validity_is_kept_and_honoured(gpu, reg):
    s = ref.plane_source(1)
    tg.make_resident(reg, s["pos"], s["idepth"], s["tris"])
    with pytest.raises(gpu.NLTGV2Error):
        reg.keep_mesh(3, validity=2)  # no mesh_outputs_begin yet
    mo = reg.mesh_outputs(None, KINV, *SRC, filter=gpu.MeshFilterParams(do_oblique_triangle_filter=False, do_edge_length_filter=False, min_triangle_idepth=0.5))
    filt = np.asarray(mo["tri_valid"], np.uint8)
    assert 0 < filt.sum() < len(s["tris"])
    reg.keep_mesh(3, validity=2)
    assert reg.kept_mesh_info(3) == (len(s["pos"]), len(s["tris"]), True)
    assert reg.get_kept_mesh(3)["tri_valid"].tobytes() == filt.tobytes()
    got = reg.fuse_views(gpu.FuseParams(sources=[fuse_source(gpu, 3, s)], K_dst=K, want_layers=True), *SRC)
    want = fr.fuse_sources([dict(s, tri_valid=filt)], K, *SRC, 0.05, 1)
    fr.assert_same(got, want, "kept validity")
    assert 0 < want["tris_drawn"] <= filt.sum() and want["coverage"] < fr.fuse_sources([s], K, *SRC, 0.05, 1)["coverage"]
    # an upload with a validity array keeps it too
    mask = (np.arange(len(s["tris"])) % 3 != 0).astype(np.uint8)
    fuse_kept(gpu, reg, [dict(s, tri_valid=mask), ref.plane_source(0)], *SRC, min_support=1, what="uploaded validity")


# ---- sources ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_one_source_fuses_to_its_layer(gpu, reg):
    s = dict(ref.plane_source(3), weight=1.0)
    got, want = fuse_kept(gpu, reg, [s], *SRC, what="one source")
    assert vr.bits(got["fused"]).tobytes() == vr.bits(got["layers"][0]).tobytes() and got["coverage"] == got["present"][0] > 1000
    assert got["support_hist"][1] == got["coverage"] and set(np.unique(got["present_mask"])) == {0, 1}


@pytest.mark.gpu
def test_gpu_eight_sources_use_every_mask_bit(gpu, reg):
    sources = [ref.plane_source(s, outliers=s in (1, 3, 6)) for s in range(8)]
    for k in (1, 5):
        got, want = fuse_kept(gpu, reg, sources, *SRC, min_support=k, what="eight sources, min_support %d" % k)
    assert all(want["present"][s] > 0 and want["inlier"][s] > 0 for s in range(8)) and want["support_hist"][8] > 0
    assert np.bitwise_or.reduce(got["present_mask"].ravel()) == 255 and np.bitwise_or.reduce(got["inlier_mask"].ravel()) == 255


@pytest.mark.gpu
@pytest.mark.parametrize("mesh_state", [0, 1])
def test_gpu_a_live_source_between_kept_ones_with_runs_in_flight(gpu, mesh_state):
    from flame_amd.regularizer import OPT_MESH_STATE

    live, kept_a, kept_b = ref.plane_source(1, outliers=False), ref.plane_source(0), ref.plane_source(2)
    # (noise on the plane: the solver has something to smooth, so the state changes under the runs in flight)
    noisy = (live["idepth"] * np.random.default_rng(9).uniform(0.97, 1.03, len(live["idepth"]))).astype(F)
    g = tg.graph_of(live["pos"], noisy, live["tris"])
    params = gpu.Params()
    with gpu.Regularizer(0) as reg, gpu.Regularizer(0) as plain:
        for r in (reg, plain):
            r.set_option(OPT_MESH_STATE, mesh_state)
            r.upload_graph(g)
            r.run(params, 20)
        reg.keep_mesh_arrays(7, kept_a["tris"], kept_a["pos"], kept_a["idepth"])
        reg.keep_mesh_arrays(9, kept_b["tris"], kept_b["pos"], kept_b["idepth"])
        before = reg.download_state(("x",))["x"]
        reg.interpolate_mesh_begin(live["tris"], *SRC)
        plain.interpolate_mesh_begin(live["tris"], *SRC)
        reg.run_async(params, 150)
        plain.run_async(params, 150)
        p = gpu.FuseParams(sources=[fuse_source(gpu, 7, kept_a), fuse_source(gpu, -1, live, graph_scale=1.25), fuse_source(gpu, 9, kept_b)], K_dst=K,
                           rel_tol=0.1, min_support=2, want_layers=True)
        reg.fuse_views_begin(p, *SRC)
        got = reg.fuse_views_end()
        reg.interpolate_mesh_end()
        plain.interpolate_mesh_end()
        after = reg.download_state(("x",))["x"]
        assert not np.array_equal(before, after)
        assert np.array_equal(after, plain.download_state(("x",))["x"])  # the stage only read
        x = after if mesh_state == 0 else before
        want = fr.fuse_sources([kept_a, dict(live, idepth=(x * F(1.25)).astype(F)), kept_b], K, *SRC, 0.1, 2)
        fr.assert_same(got, want, "live source, mesh_state %d" % mesh_state)
        assert want["present"][1] > 1000 and want["coverage"] > 1000
        with pytest.raises(gpu.NLTGV2Error):  # two live sources
            reg.fuse_views_begin(gpu.FuseParams(sources=[fuse_source(gpu, -1, live), fuse_source(gpu, -1, live)], K_dst=K), *SRC)
        assert reg.fuse_views_end()["counts"].tolist() == got["counts"].tolist()


@pytest.mark.gpu
def test_gpu_the_same_slot_twice_ties_at_every_present_pixel(gpu, reg):
    s = ref.plane_source(2)
    reg.keep_mesh_arrays(4, s["tris"], s["pos"], s["idepth"])
    twice = [dict(s, weight=0.3), dict(s, weight=1.7)]
    for rel_tol in (0.02, 0.0):
        p = gpu.FuseParams(sources=[fuse_source(gpu, 4, t) for t in twice], K_dst=K, rel_tol=rel_tol, min_support=2, want_layers=True)
        got = reg.fuse_views(p, *SRC)
        fr.assert_same(got, fr.fuse_sources(twice, K, *SRC, rel_tol, 2), "one slot twice, rel_tol %g" % rel_tol)
        present = got["present_mask"] != 0
        assert present.sum() > 1000 and (got["present_mask"][present] == 3).all() and (got["inlier_mask"][present] == 3).all()
        assert got["support_hist"][2] == present.sum() == got["coverage"] and got["support_hist"][1] == 0
        assert (vr.bits(got["spread"])[present] == 0).all()


# ---- the edges of the batched kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1x1", "5x3_downscaled", "75x100_other_camera_turned_20_degrees"])
def test_gpu_targets_of_other_sizes(gpu, reg, name):
    """(75 x 100 and 5 x 3 pixels are no multiple of the vote's tile of 2048.)"""
    t = tg.TARGETS[name]
    got, want = fuse_kept(gpu, reg, list(ref.scene()), t["rows"], t["cols"], min_support=2, K_dst=t["K_dst"], what=name)
    assert got["fused"].shape == (t["rows"], t["cols"]) and sum(want["present"]) > 0
    if name.startswith("75x100"):
        assert want["coverage"] > 2048 and want["support_hist"][0] > 0


@pytest.mark.gpu
def test_gpu_empty_sources_between_ordinary_ones(gpu, reg):
    a, b = ref.plane_source(0), ref.plane_source(2)
    no_tris = dict(ref.plane_source(1), tris=np.zeros((0, 3), np.int32))
    no_vertices = dict(ref.plane_source(3), tris=np.zeros((0, 3), np.int32), pos=np.zeros((0, 2), F), idepth=np.zeros(0, F))
    got, want = fuse_kept(gpu, reg, [a, no_tris, no_vertices, b], *SRC, min_support=1, what="T = 0 and V = 0 in the middle")
    assert reg.kept_mesh_info(1) == (len(no_tris["pos"]), 0, False) and reg.kept_mesh_info(2) == (0, 0, False)
    assert want["present"][:4] == [want["renders"][0]["coverage"], 0, 0, want["renders"][3]["coverage"]] and want["present"][3] > 1000
    assert want["tris_drawn"] == 280
    got, want = fuse_kept(gpu, reg, [no_vertices, no_tris], 5, 7, what="nothing at all")
    assert want["counts"].tolist() == [0, 35] + [0] * 30 and (vr.bits(got["fused"]) == fr.HOLE).all() and (vr.bits(got["spread"]) == fr.HOLE).all()


@pytest.mark.gpu
def test_gpu_source_boundaries_inside_workgroups(gpu, reg):
    fine = ref.plane_source(1, step=1, seed=44)
    assert len(fine["pos"]) == 48 * 64 and len(fine["tris"]) > 20 * 256
    sources = [ref.plane_source(0), fine, ref.plane_source(2), ref.plane_source(3)]
    starts = np.cumsum([len(s["pos"]) for s in sources]), np.cumsum([len(s["tris"]) for s in sources])
    assert all(v % 256 != 0 for v in starts[0]) and all(t % 256 != 0 for t in starts[1])
    got, want = fuse_kept(gpu, reg, sources, *SRC, min_support=2, what="a fine mesh between coarse ones")
    # (a jitter of 1.5 pixels on a 1-pixel grid folds some triangles over: those are culled, on both sides alike)
    assert 5000 < want["tris_drawn"] < sum(len(s["tris"]) for s in sources) and all(want["present"][s] > 1000 for s in range(4))


def whole_target_triangles(n, seed, weight=1.0):
    """n triangles that each cover the whole 64x48 target, at inverse depths that cross each other inside the image."""
    rng = np.random.default_rng(seed)
    corners = np.array([[-10, -10], [150, -10], [-10, 130]], F)
    pos = (corners[None] + rng.uniform(-8, 8, (n, 3, 2))).reshape(-1, 2).astype(F)
    return dict(tris=np.arange(3 * n, dtype=np.int32).reshape(n, 3), pos=pos, idepth=rng.uniform(0.3, 0.6, 3 * n).astype(F), Kinv_src=KINV, R=ref.EYE,
                t=np.array([0.05, 0, 0], F), weight=weight)


@pytest.mark.gpu
def test_gpu_a_large_box_in_one_source_only(gpu, reg):
    """A box of more than 2048 pixels goes through the list of (source, triangle) pairs: the pair's source must be honoured."""
    whole = whole_target_triangles(1, seed=5, weight=1.7)
    sources = [ref.plane_source(0), ref.plane_source(1), whole, ref.plane_source(3)]
    got, want = fuse_kept(gpu, reg, sources, *SRC, rel_tol=0.2, what="the whole target in source 2")
    assert want["present"][2] == 48 * 64 and want["present"][0] < 48 * 64 and want["support_hist"][0] == 0


@pytest.mark.gpu
def test_gpu_more_large_boxes_than_list_rows_over_three_sources(gpu, reg):
    sources = [whole_target_triangles(50, seed=6), ref.plane_source(1), whole_target_triangles(60, seed=7, weight=0.3), whole_target_triangles(40, seed=8, weight=1.7)]
    got, want = fuse_kept(gpu, reg, sources, *SRC, rel_tol=0.2, min_support=2, what="150 large triangles in three sources")
    assert want["tris_drawn"] == 150 + 140 and [want["present"][s] for s in (0, 2, 3)] == [48 * 64] * 3
    assert len(np.unique(vr.bits(got["layers"][0]))) > 1000 and 0 < want["coverage"]


# ---- the two stages are one projection -----------------------------------------------------------------------------------------------------
def one_projection_cases():
    grid = tg.mesh_case(14, step=3, rows=30, cols=40, R=tg.cases.rotation_y(-5.0), t=np.array([0.3, 0.1, 0], F))
    large = dict(tris=np.array([[0, 1, 2]], np.int32), pos=np.array([[-100, -100], [300, -100], [-100, 300]], F), idepth=np.array([0.4, 1.1, 2.3], F),
                 Kinv_src=KINV, K_dst=K, t=np.array([0.05, 0, 0], F), rows=60, cols=80)
    return {"630_triangles_30x40": grid, "one_large_box_60x80": large, "no_triangles": dict(grid, tris=np.zeros((0, 3), np.int32))}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(one_projection_cases()))
def test_gpu_render_view_is_the_fusion_of_one_live_source(gpu, reg, name):
    """render_view and fuse_views with one live source run the same projection (view_project.hpp): one camera, validity 0 and 2 --
    the map is layer 0 bit for bit, and coverage and tris_drawn are the same numbers."""
    c = one_projection_cases()[name]
    rows, cols, T = c["rows"], c["cols"], len(c["tris"])
    tg.make_resident(reg, c["pos"], c["idepth"], c["tris"])
    mo = reg.mesh_outputs(None, KINV, *SRC, filter=gpu.MeshFilterParams(do_oblique_triangle_filter=False, do_edge_length_filter=False, min_triangle_idepth=0.6))
    n_valid = int(np.asarray(mo["tri_valid"], np.uint8).sum())
    drawn = {}
    for validity in (0, 2):
        view = reg.render_view(tg.view_params(gpu, c, validity=validity), rows, cols)
        p = gpu.FuseParams(sources=[fuse_source(gpu, -1, c, validity=validity)], K_dst=c["K_dst"], near_depth=c.get("near_depth", 0.0), want_layers=True)
        fused = reg.fuse_views(p, rows, cols)
        print("%s, validity %d: coverage %d / %d, tris_drawn %d / %d" % (name, validity, view["coverage"], fused["coverage"], view["tris_drawn"], fused["tris_drawn"]))
        assert view["map"].shape == fused["layers"][0].shape == (rows, cols)
        assert vr.bits(view["map"]).tobytes() == vr.bits(fused["layers"][0]).tobytes(), validity
        assert np.uint32(view["coverage"]) == np.uint32(fused["coverage"]) and np.uint32(view["tris_drawn"]) == np.uint32(fused["tris_drawn"]), validity
        drawn[validity] = view["tris_drawn"]
    # nothing passes by being empty, and each mesh takes the path it is here for
    if name == "630_triangles_30x40":
        assert T >= 600 and 0 < n_valid < T and 0 < drawn[2] < drawn[0] and view["coverage"] > 0
    elif name == "one_large_box_60x80":
        assert rows * cols > 2048 and view["coverage"] == rows * cols and drawn == {0: 1, 2: 1}  # (the one box is the whole target: listed)
    else:
        assert T == 0 and drawn == {0: 0, 2: 0} and (vr.bits(view["map"]) == vr.HOLE).all()


# ---- repeats, transfers, errors ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_two_calls_give_the_same_bytes_and_outputs_may_stay_on_the_device(gpu, reg):
    sources = list(ref.scene())
    keep_all(reg, sources)
    srcs = [fuse_source(gpu, i, s) for i, s in enumerate(sources)]
    p = gpu.FuseParams(sources=srcs, K_dst=K, rel_tol=ref.REL_TOL, min_support=2, want_layers=True)
    a, b = reg.fuse_views(p, *SRC), reg.fuse_views(p, *SRC)
    for k in ("fused", "spread", "layers", "present_mask", "inlier_mask", "counts"):
        assert a[k].tobytes() == b[k].tobytes(), k
    want = ref.scene_fused(2)
    fr.assert_same(a, want, "the scene")
    # a smaller target in the buffers the larger call left behind sees no stale keys
    small = reg.fuse_views(p, 30, 40)
    fr.assert_same(small, fr.fuse_sources(sources, K, 30, 40, ref.REL_TOL, 2), "a smaller target")
    # only what was asked for
    only = reg.fuse_views(gpu.FuseParams(sources=srcs, K_dst=K, rel_tol=ref.REL_TOL, min_support=2, want_masks=False, want_spread=False), *SRC)
    assert sorted(only["device"]) == ["fused"] and "spread" not in only and "present_mask" not in only and "layers" not in only
    fr.assert_same(only, want, "fused alone")
    # copy_out = 0: only the counters travel
    dev = reg.fuse_views(gpu.FuseParams(sources=srcs, K_dst=K, rel_tol=ref.REL_TOL, min_support=2, want_layers=True, copy_out=False), *SRC)
    assert not any(k in dev for k in ("fused", "spread", "layers", "present_mask", "inlier_mask")) and dev["counts"].tolist() == want["counts"].tolist()
    assert sorted(dev["device"]) == ["fused", "inlier_mask", "layers", "present_mask", "spread"]
    for k, shape, dt in (("fused", SRC, F), ("spread", SRC, F), ("layers", (4,) + SRC, F), ("present_mask", SRC, np.uint8), ("inlier_mask", SRC, np.uint8)):
        assert fetch(dev["device"][k], shape, dt).tobytes() == a[k].tobytes(), k
    # fused_device serves the metric stage and the map error as the host copy does
    s0 = sources[0]
    tg.make_resident(reg, s0["pos"], s0["idepth"], s0["tris"])
    host_copy = on_device(a["fused"])
    ptr = dev["device"]["fused"]

    def same(x, y, what):
        for k in x:
            if k in ("device_ms", "device"):
                continue
            if isinstance(x[k], np.ndarray):
                assert x[k].tobytes() == y[k].tobytes(), (what, k)
            else:
                assert x[k] == y[k] or (x[k] != x[k] and y[k] != y[k]), (what, k)

    m = [reg.metric_outputs(KINV, *SRC, params=gpu.MetricParams(map_device=q)) for q in (ptr, host_copy.data_ptr())]
    same(m[0], m[1], "metric_outputs")
    assert m[0]["n_points"] == want["coverage"]  # (every fused value is positive and finite: a point each)
    truth = np.where(np.isnan(a["layers"][0]), F(0.5), a["layers"][0]).astype(F)
    e = [reg.map_error(gpu.MapErrorParams(source=gpu.MAP_ERROR_TRUTH, map_device=q, truth=truth, win_size=1), *SRC) for q in (ptr, host_copy.data_ptr())]
    same(e[0], e[1], "map_error, map_device")
    layer0 = on_device(a["layers"][0])
    e = [reg.map_error(gpu.MapErrorParams(source=gpu.MAP_ERROR_TRUTH, map_device=layer0.data_ptr(), truth_device=q, win_size=1), *SRC)
         for q in (ptr, host_copy.data_ptr())]
    same(e[0], e[1], "map_error, truth_device")
    assert e[0]["n_valid"] > 1000


@pytest.mark.gpu
def test_gpu_every_error_comes_before_anything_is_enqueued_and_leaves_the_previous_outputs(gpu):
    s = ref.plane_source(0)
    good = lambda **kw: gpu.FuseParams(**dict(dict(sources=[fuse_source(gpu, 0, s), fuse_source(gpu, 1, s)], K_dst=K, want_layers=True), **kw))  # noqa: E731
    with gpu.Regularizer(0) as reg:
        bad_slots = (-1, 16, 99)
        for slot in bad_slots:  # the store: slot out of range (keep_mesh: -1 too)
            for call in (lambda: reg.keep_mesh(slot), lambda: reg.drop_mesh(slot), lambda: reg.kept_mesh_info(slot), lambda: reg.get_kept_mesh(slot),
                         lambda: reg.keep_mesh_arrays(slot, s["tris"], s["pos"], s["idepth"])):
                with pytest.raises(gpu.NLTGV2Error):
                    call()
        with pytest.raises(gpu.NLTGV2Error):  # no graph
            reg.keep_mesh(0)
        with pytest.raises(gpu.NLTGV2Error):  # nothing begun
            reg.fuse_views_end()
        with pytest.raises(gpu.NLTGV2Error):  # a live source without a graph
            reg.fuse_views_begin(gpu.FuseParams(sources=[fuse_source(gpu, -1, s)], K_dst=K), *SRC)
        reg.keep_mesh_arrays(0, s["tris"], s["pos"], s["idepth"])
        reg.keep_mesh_arrays(1, s["tris"], s["pos"], s["idepth"])
        for bad in (dict(triangles=np.array([[0, 1, len(s["pos"])]], np.int32)), dict(triangles=np.array([[0, -1, 2]], np.int32))):
            with pytest.raises(gpu.NLTGV2Error):  # an index out of range: the slot stays as it was
                reg.keep_mesh_arrays(1, bad["triangles"], s["pos"], s["idepth"])
        assert reg.kept_mesh_info(1) == (len(s["pos"]), len(s["tris"]), False)
        reg.upload_graph(tg.graph_of(s["pos"], s["idepth"], s["tris"]))
        with pytest.raises(gpu.NLTGV2Error):  # no resident triangles
            reg.keep_mesh(1)
        with pytest.raises(gpu.NLTGV2Error):
            reg.fuse_views_begin(gpu.FuseParams(sources=[fuse_source(gpu, -1, s)], K_dst=K), *SRC)
        reg.interpolate_mesh(s["tris"], *SRC)
        for validity in (1, 2, 3, -1):  # bad validity; 2 without mesh_outputs_begin
            with pytest.raises(gpu.NLTGV2Error):
                reg.keep_mesh(1, validity=validity)
            with pytest.raises(gpu.NLTGV2Error):
                reg.fuse_views_begin(gpu.FuseParams(sources=[fuse_source(gpu, -1, s, validity=validity)], K_dst=K), *SRC)
        assert reg.kept_mesh_info(1) == (len(s["pos"]), len(s["tris"]), False)
        # a view and a fusion begun; then every error of the fusion; then both ends still have their own outputs
        view_p = gpu.ViewParams(Kinv_src=KINV, K_dst=K, t=np.array([0.2, 0, 0], F))
        reg.render_view_begin(view_p, *SRC)
        reg.fuse_views_begin(good(), *SRC)
        with pytest.raises(gpu.NLTGV2Error):
            reg.fuse_views_begin(None, *SRC)
        for rows, cols in ((0, 64), (48, 0), (-1, 64), (32768, 64), (48, 32768)):
            with pytest.raises(gpu.NLTGV2Error):
                reg.fuse_views_begin(good(), rows, cols)
        srcs = [fuse_source(gpu, 0, s)] * 9
        for bad in (dict(n_sources=0), dict(n_sources=-1), dict(sources=srcs[:8], n_sources=9),
                    dict(sources=[fuse_source(gpu, 0, s), fuse_source(gpu, 2, s)]),   # an empty slot
                    dict(sources=[fuse_source(gpu, 0, s), fuse_source(gpu, 16, s)]),  # slots out of range
                    dict(sources=[fuse_source(gpu, 0, s), fuse_source(gpu, -2, s)]),
                    dict(sources=[fuse_source(gpu, -1, s), fuse_source(gpu, 0, s), fuse_source(gpu, -1, s)]),  # two live sources
                    dict(sources=[fuse_source(gpu, 0, dict(s, weight=0.0))]), dict(sources=[fuse_source(gpu, 0, dict(s, weight=-1.0))]),
                    dict(sources=[fuse_source(gpu, 0, dict(s, weight=float("inf")))]), dict(sources=[fuse_source(gpu, 0, dict(s, weight=float("nan")))]),
                    dict(rel_tol=-0.01), dict(rel_tol=float("inf")), dict(rel_tol=float("nan")),
                    dict(min_support=0), dict(min_support=3), dict(min_support=-1)):
            with pytest.raises(gpu.NLTGV2Error):
                reg.fuse_views_begin(good(**bad), *SRC)
        got = reg.fuse_views_end()
        fr.assert_same(got, fr.fuse_sources([s, s], K, *SRC, 0.05, 1), "the fusion begun before the errors")
        assert got["device_ms"] > 0
        view = reg.render_view_end()  # begun before the fusion: still the view's own result
        vr.assert_same(view, vr.render_view(s["tris"], s["pos"], s["idepth"], KINV, K, ref.EYE, np.array([0.2, 0, 0], F), *SRC), "the view begun before")
        # ... and the other way round
        reg.fuse_views_begin(good(min_support=2), *SRC)
        reg.render_view(view_p, *SRC)
        fr.assert_same(reg.fuse_views_end(), fr.fuse_sources([s, s], K, *SRC, 0.05, 2), "a fusion with a view in between")
