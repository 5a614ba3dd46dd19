"""flame_nltgv2_volume_* through the C-ABI against the checker tests/volume_ref.py, bit for bit: both arrays of the volume as uint32, the
raycast's map as uint32 and every counter.  The scene of tests/volume_ref.py call by call; volumes smaller than a wave, with x rows that
end inside a wave and span more than two, with an axis of one voxel; voxels placed on the borders of the rules; nothing written where
nothing is seen; two poses in both orders; saturation; the three map sources; repeats; the raycast on uploaded volumes; a map that stays
on the device and feeds the metric outputs and the map error; the store's life cycle; every error before anything is enqueued."""
import ctypes as C

import numpy as np
import pytest

from flame_amd import synth
from tests import map_error_ref as er
from tests import metric_ref as mr
from tests import test_fuse_views_ref as fref
from tests import test_gpu_render_view as tg
from tests import test_volume_ref as cpu
from tests import volume_ref as vr
from tests.metric_helpers import fetch, on_device

F = np.float32
EYE3 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], F)
# nx, ny, nz, voxel_size, origin: each in front of the scene's camera, around its optical axis
VOLUMES = {
    "5x3x7": dict(nx=5, ny=3, nz=7, voxel_size=0.1, origin=(-0.2, -0.1, 0.7), trunc=0.3, max_weight=2.0),
    "16x12x10": dict(vr.SCENE),
    "70x9x5": dict(nx=70, ny=9, nz=5, voxel_size=0.02, origin=(-0.7, -0.08, 0.93), trunc=0.1, max_weight=2.0),
    "130x3x2": dict(nx=130, ny=3, nz=2, voxel_size=0.01, origin=(-0.65, -0.01, 0.99), trunc=0.05, max_weight=2.0),
    "1x1x1": dict(nx=1, ny=1, nz=1, voxel_size=0.1, origin=(0.0, 0.0, 1.0), trunc=0.3, max_weight=2.0),
    "4x1x4": dict(nx=4, ny=1, nz=4, voxel_size=0.1, origin=(-0.15, 0.0, 0.8), trunc=0.3, max_weight=2.0),
}
TARGETS = [(1, 1), (7, 5), (24, 32), (65, 3)]  # rows, cols


def target_kinv(rows, cols):
    """The scene's field of view on a rows x cols target."""
    f = 20.0 * max(cols, rows) / 32.0
    return np.array([1 / f, 0, -(cols // 2) / f, 0, 1 / f, -(rows // 2) / f, 0, 0, 1], np.float64).astype(F)


def turned_pose(deg=5.0, t=(0.05, -0.02, 0.03)):
    """12 floats, row-major [R | t]: a rotation about the vertical axis and a translation."""
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([c, 0, s, t[0], 0, 1, 0, t[1], -s, 0, c, t[2]], np.float64).astype(F)


@pytest.fixture(scope="module")
def gpu(built):
    import torch  # noqa: F401

    import flame_amd

    assert hasattr(flame_amd.load_library(), "flame_nltgv2_volume_create")
    return flame_amd


@pytest.fixture(scope="module")
def reg(gpu):
    with gpu.Regularizer(0) as r:
        yield r


def create(gpu, reg, **params):
    reg.volume_create(gpu.VolumeParams(**params))
    return vr.Volume(**params)


def integrate(gpu, reg, ref, m, K, T, what, **kw):
    """One call on a device copy of the map and in the checker: the counters, then both arrays."""
    m = np.ascontiguousarray(m, F)
    keep = on_device(m)
    got = reg.volume_integrate(K, T, *m.shape, gpu.IntegrateParams(map_device=keep.data_ptr(), **kw))
    with np.errstate(all="ignore"):
        want = ref.integrate(m, K, T, **kw)
    print(what, got["counts"].tolist(), "device_ms %.3f" % got["device_ms"])
    vr.assert_same_counts(got, want, vr.INTEGRATE_COUNTERS, what)
    assert got["counts"][6:].tolist() == [0, 0] and (got["rows"], got["cols"]) == m.shape
    vr.assert_same_volume(reg.volume_download(), ref, what)
    return got, want


def raycast(gpu, reg, ref, Kinv, T, rows, cols, what, **kw):
    got = reg.volume_raycast(Kinv, T, rows, cols, gpu.RaycastParams(**kw))
    want = ref.raycast(Kinv, T, rows, cols, kw["z_near"], kw["dz"], kw["n_steps"])
    print(what, got["counts"].tolist(), "device_ms %.3f" % got["device_ms"])
    vr.assert_same_counts(got, want, vr.RAYCAST_COUNTERS, what)
    vr.assert_same_map(got["map"], want["map"], what)
    assert got["counts"][3] == 0 and (got["rows"], got["cols"]) == (rows, cols)
    return got, want


# ---- the scene -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_the_scene_call_by_call(gpu, reg):
    cpu.test_the_scene_has_every_counter_of_both_stages_above_zero()  # the checker alone first: nothing passes by being empty
    ref = create(gpu, reg, **vr.SCENE)
    vr.assert_same_volume(reg.volume_download(), ref, "fresh")
    m = vr.scene_map()
    for call in range(3):
        got, _ = integrate(gpu, reg, ref, m, vr.SCENE_K, vr.IDENTITY, "the scene, call %d" % call)
        assert got["updated"] > 0 and (got["saturated"] > 0) == (call == 2)
    for T in (vr.IDENTITY, vr.shifted_pose(0.15)):
        got, _ = raycast(gpu, reg, ref, vr.SCENE_KINV, T, vr.SCENE_ROWS, vr.SCENE_COLS, "the scene's raycast", **vr.SCENE_RAYCAST)
        assert got["hits"] > 0 and got["back"] > 0 and got["empty"] > 0 and got["device_ms"] > 0
    info = reg.volume_info()
    assert (info["nx"], info["ny"], info["nz"], info["device_bytes"]) == (16, 12, 10, 8 * 1920) and info["origin"].tobytes() == ref.origin.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VOLUMES))
def test_gpu_volumes_around_a_wave_and_targets_of_other_sizes(gpu, reg, name):
    ref = create(gpu, reg, **VOLUMES[name])
    m = vr.scene_map()
    a, _ = integrate(gpu, reg, ref, m, vr.SCENE_K, vr.IDENTITY, name + " from the front")
    b, _ = integrate(gpu, reg, ref, (m * F(0.97)).astype(F), vr.SCENE_K, turned_pose(), name + " turned", weight=0.5)
    assert a["updated"] > 0 and b["updated"] > 0
    one_voxel_axis = min(ref.nx, ref.ny, ref.nz) == 1
    for rows, cols in TARGETS:
        for T in (vr.IDENTITY, turned_pose(-4.0, (0.03, 0.01, -0.05))):
            got, _ = raycast(gpu, reg, ref, target_kinv(rows, cols), T, rows, cols, "%s into %dx%d" % (name, rows, cols), z_near=0.3, dz=0.04, n_steps=40)
            if one_voxel_axis:  # every ray is a hole and counted empty
                assert (got["hits"], got["back"], got["empty"]) == (0, 0, rows * cols) and np.all(vr.bits(got["map"]) == 0x7FC00000)


# ---- the borders of the integration's rules --------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_voxels_on_the_borders(gpu, reg):
    cpu.test_the_borders_of_the_integration_fall_where_the_header_puts_them()  # each border in the checker first
    K = np.array([1, 0, 0.5, 0, 1, 0, 0, 0, 1], F)
    row = dict(nx=4, ny=1, nz=1, voxel_size=1.0, origin=(-1.0, 0.0, 1.0), trunc=0.5, max_weight=8.0)
    ones = np.full((1, 2), 1.0, F)
    # u == -0.5 (in) and u == cols - 0.5 (out)
    ref = create(gpu, reg, **row)
    got, _ = integrate(gpu, reg, ref, ones, K, vr.IDENTITY, "u on the image's borders")
    assert (got["front"], got["in_image"], got["updated"]) == (4, 2, 2)
    # P.z == near_depth is skipped
    ref = create(gpu, reg, **row)
    got, _ = integrate(gpu, reg, ref, ones, K, vr.IDENTITY, "P.z == near_depth", near_depth=1.0)
    assert got["front"] == 0 and reg.volume_download()["weight"].max() == 0
    # sdf == -trunc is updated, one ulp below is left alone
    for trunc, updated in ((F(0.5), 1), (np.nextafter(F(0.5), F(0)), 0)):
        ref = create(gpu, reg, nx=1, ny=1, nz=1, voxel_size=1.0, origin=(0.0, 0.0, 1.0), trunc=trunc, max_weight=8.0)
        got, _ = integrate(gpu, reg, ref, np.full((1, 1), 2.0, F), EYE3, vr.IDENTITY, "sdf against -trunc %r" % trunc)
        assert (got["valid"], got["behind"], got["updated"]) == (1, 1 - updated, updated)
    # +inf, denormals, NaN, zero, negative values; min_depth and max_depth that cut
    for d, kw, valid in ((np.inf, {}, 0), (1e-40, {}, 0), (1e-45, {}, 0), (6e-39, {}, 1), (6e-39, dict(max_depth=1e38), 0), (np.nan, {}, 0), (0.0, {}, 0),
                         (-0.0, {}, 0), (-1.0, {}, 0), (-np.inf, {}, 0), (1.0, {}, 1), (1.0, dict(min_depth=1.0), 0), (1.0, dict(max_depth=1.0), 0),
                         (1.0, dict(min_depth=0.5, max_depth=1.5), 1)):
        ref = create(gpu, reg, nx=1, ny=1, nz=1, voxel_size=1.0, origin=(0.0, 0.0, 1.0), trunc=0.5, max_weight=8.0)
        got, _ = integrate(gpu, reg, ref, np.full((1, 1), d, F), EYE3, vr.IDENTITY, "d = %r %r" % (d, kw), **kw)
        assert (got["in_image"], got["valid"]) == (1, valid), (d, kw)
    # the whole special map of the metric outputs over a column of voxels per pixel
    from tests.metric_helpers import special_map

    sm = special_map()
    ref = create(gpu, reg, nx=12, ny=3, nz=3, voxel_size=1.0, origin=(0.0, 0.0, 0.5), trunc=2.0, max_weight=8.0)
    Kz = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], F)
    # (x = i, z = 0.5 + k: u = i / z lands on other pixels in every layer)
    integrate(gpu, reg, ref, sm, Kz, vr.IDENTITY, "the special map")


@pytest.mark.gpu
def test_gpu_nothing_seen_nothing_written(gpu, reg):
    ref = create(gpu, reg, **vr.SCENE)
    integrate(gpu, reg, ref, vr.scene_map(), vr.SCENE_K, vr.IDENTITY, "something to keep")
    before = reg.volume_download()
    # the camera turned round: every voxel is behind it
    back = np.array([-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0], F)
    got, _ = integrate(gpu, reg, ref, vr.scene_map(), vr.SCENE_K, back, "behind the camera")
    assert (got["front"], got["updated"]) == (0, 0)
    # moved far to the side: in front of the camera, wholly outside the frustum
    aside = vr.IDENTITY.copy()
    aside[3] = F(50.0)
    got, _ = integrate(gpu, reg, ref, vr.scene_map(), vr.SCENE_K, aside, "outside the frustum")
    assert got["front"] == 1920 and (got["in_image"], got["updated"]) == (0, 0)
    # a map of holes
    got, _ = integrate(gpu, reg, ref, np.full((24, 32), np.nan, F), vr.SCENE_K, vr.IDENTITY, "a map of holes")
    assert got["in_image"] > 0 and (got["valid"], got["updated"]) == (0, 0)
    after = reg.volume_download()
    assert after["tsdf"].tobytes() == before["tsdf"].tobytes() and after["weight"].tobytes() == before["weight"].tobytes()


@pytest.mark.gpu
def test_gpu_two_poses_in_both_orders_weights_and_saturation(gpu, reg):
    a, b = vr.scene_map(), (vr.scene_map() * F(0.9)).astype(F)
    calls = [(a, vr.IDENTITY, 0.5), (b, vr.shifted_pose(-0.05), 3.0)]
    out = []
    for order in (calls, calls[::-1]):
        ref = create(gpu, reg, **vr.SCENE)
        sat = [integrate(gpu, reg, ref, m, vr.SCENE_K, T, "weight %r" % w, weight=w)[0]["saturated"] for m, T, w in order]
        out.append((reg.volume_download(), sat))
    assert out[0][1][0] == 0 and out[0][1][1] > 0 and out[1][1][0] > 0  # (0.5 + 3 and 3 alone both pass max_weight = 2)
    assert np.count_nonzero(vr.bits(out[0][0]["tsdf"]) != vr.bits(out[1][0]["tsdf"])) > 0
    assert out[0][0]["weight"].max() == F(2.0) == out[1][0]["weight"].max()
    # the same sequence twice gives the same bytes
    ref = create(gpu, reg, **vr.SCENE)
    for m, T, w in calls:
        integrate(gpu, reg, ref, m, vr.SCENE_K, T, "again", weight=w)
    again = reg.volume_download()
    assert again["tsdf"].tobytes() == out[0][0]["tsdf"].tobytes() and again["weight"].tobytes() == out[0][0]["weight"].tobytes()
    r = [reg.volume_raycast(vr.SCENE_KINV, vr.IDENTITY, 24, 32, gpu.RaycastParams(**vr.SCENE_RAYCAST)) for _ in range(2)]
    assert r[0]["map"].tobytes() == r[1]["map"].tobytes() and r[0]["counts"].tolist() == r[1]["counts"].tolist()


# ---- the three map sources -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_the_resident_the_filtered_and_a_callers_map(gpu):
    s = fref.plane_source(1)  # (outliers: the filters drop triangles, so the filtered map differs)
    rows, cols = tg.SRC
    vol = dict(nx=24, ny=20, nz=24, voxel_size=0.1, origin=(-1.2, -1.0, 1.0), trunc=0.4, max_weight=50.0)
    K = fref.K
    with gpu.Regularizer(0) as reg:
        ref = create(gpu, reg, **vol)
        with pytest.raises(gpu.NLTGV2Error) as ei:
            reg.volume_integrate_begin(K, vr.IDENTITY, rows, cols)  # a resident map needs a graph
        assert ei.value.status == -4
        reg.upload_graph(tg.graph_of(s["pos"], s["idepth"], s["tris"]))
        dense = reg.interpolate_mesh(s["tris"], rows, cols)[0]
        filtered = reg.mesh_outputs(s["tris"], fref.KINV, rows, cols, want_filtered_map=True)["filtered_map"]
        print("pixels where the filtered map differs from the resident one:", int(np.count_nonzero(vr.bits(dense) != vr.bits(filtered))))
        for m, kw, what in ((dense, {}, "the resident map"), (filtered, dict(use_filtered_map=True), "the filtered map")):
            got = reg.volume_integrate(K, vr.IDENTITY, rows, cols, gpu.IntegrateParams(**kw))
            want = ref.integrate(m, K, vr.IDENTITY)
            vr.assert_same_counts(got, want, vr.INTEGRATE_COUNTERS, what)
            vr.assert_same_volume(reg.volume_download(), ref, what)
            assert got["updated"] > 1000
        # the fused_device of a fuse_views with copy_out = 0
        reg.keep_mesh(0)
        fp = gpu.FuseParams(sources=[gpu.FuseSource(slot=0, Kinv_src=fref.KINV)], K_dst=K, copy_out=False)
        fused = reg.fuse_views(fp, rows, cols)
        assert "fused" not in fused
        m = fetch(fused["device"]["fused"], (rows, cols), F)
        got = reg.volume_integrate(K, turned_pose(), rows, cols, gpu.IntegrateParams(map_device=fused["device"]["fused"], weight=2.0))
        want = ref.integrate(m, K, turned_pose(), weight=2.0)
        vr.assert_same_counts(got, want, vr.INTEGRATE_COUNTERS, "fused_device")
        vr.assert_same_volume(reg.volume_download(), ref, "fused_device")
        # a render_view map
        view = reg.render_view(gpu.ViewParams(Kinv_src=fref.KINV, K_dst=K, t=(0.1, 0.0, 0.0), copy_out=False, want_tri_index=False), rows, cols)
        m = fetch(view["device"]["map"], (rows, cols), F)
        got = reg.volume_integrate(K, vr.shifted_pose(0.1), rows, cols, gpu.IntegrateParams(map_device=view["device"]["map"]))
        want = ref.integrate(m, K, vr.shifted_pose(0.1))
        vr.assert_same_counts(got, want, vr.INTEGRATE_COUNTERS, "a render_view map")
        vr.assert_same_volume(reg.volume_download(), ref, "a render_view map")
        assert got["updated"] > 1000


# ---- the raycast on uploaded volumes ---------------------------------------------------------------------------------------------------
def column(gpu, reg, tsdf_of_k, weight=None, nz=8):
    ref = create(gpu, reg, nx=2, ny=2, nz=nz, voxel_size=1.0, origin=(-0.5, -0.5, 0.0), trunc=1.0, max_weight=8.0)
    ref.tsdf = np.broadcast_to(np.asarray(tsdf_of_k, F)[:, None, None], (nz, 2, 2)).copy()
    ref.weight = np.ones((nz, 2, 2), F) if weight is None else np.asarray(weight, F)
    reg.volume_upload(ref.tsdf, ref.weight)
    vr.assert_same_volume(reg.volume_download(), ref, "an uploaded volume")
    return ref


@pytest.mark.gpu
def test_gpu_raycast_on_uploaded_volumes(gpu, reg):
    cpu.test_the_raycast_on_hand_made_volumes()  # each case in the checker first
    ramp = [3, 2, 1, 0, -1, -2, -3, -4]
    base = dict(z_near=0.0, dz=0.5, n_steps=15)
    w0 = np.ones((8, 2, 2), F)
    w0[3, 1, 1] = 0
    cases = [("a crossing with f_cur == 0", ramp, None, {}, (1, 0, 0)),
             ("between two samples", ramp, None, dict(dz=0.4, n_steps=19), (1, 0, 0)),
             ("starts inside", ramp, None, dict(z_near=4.0), (0, 1, 0)),
             ("starts on the surface", ramp, None, dict(z_near=3.0), (0, 1, 0)),
             ("met from behind", [-1, -1, 0, 1, 2, 3, 4, 5], None, {}, (0, 1, 0)),
             ("enters late", ramp, None, dict(z_near=-2.0), (1, 0, 0)),
             ("never enters", ramp, None, dict(z_near=8.0), (0, 0, 1)),
             ("never ends", [5, 4, 3, 2, 1, 0.5, 0.25, 0.125], None, {}, (0, 0, 0)),
             ("a weight-0 voxel among the eight", ramp, w0, {}, (0, 1, 0)),
             ("g == n_axis - 1 exactly", [7, 6, 5, 4, 3, 2, 1, -1], None, dict(dz=1.0, n_steps=8), (1, 0, 0)),
             ("one step", ramp, None, dict(n_steps=1), (0, 0, 0)),
             ("4096 steps", ramp, None, dict(dz=0.001, n_steps=4096), (1, 0, 0))]
    for what, tsdf, weight, kw, counts in cases:
        ref = column(gpu, reg, tsdf, weight)
        got, _ = raycast(gpu, reg, ref, EYE3, vr.IDENTITY, 1, 1, what, **{**base, **kw})
        assert (got["hits"], got["back"], got["empty"]) == counts, what
    # a random volume with holes in its weights, values an integration would never produce, from two cameras into every target
    rng = np.random.default_rng(5)
    ref = create(gpu, reg, nx=9, ny=7, nz=11, voxel_size=0.1, origin=(-0.4, -0.3, 0.6), trunc=0.3, max_weight=8.0)
    ref.tsdf = (rng.random((11, 7, 9)) * 6 - 3).astype(F)
    ref.weight = np.where(rng.random((11, 7, 9)) < 0.1, 0, rng.random((11, 7, 9)) * 5).astype(F)
    reg.volume_upload(ref.tsdf, ref.weight)
    for rows, cols in TARGETS:
        for T in (vr.IDENTITY, turned_pose(-4.0, (0.03, 0.01, -0.05))):
            raycast(gpu, reg, ref, target_kinv(rows, cols), T, rows, cols, "random into %dx%d" % (rows, cols), z_near=0.3, dz=0.03, n_steps=50)
    # upload checks weight >= 0 and nothing else
    bad = ref.weight.copy()
    bad[2, 3, 4] = -1.0
    with pytest.raises(gpu.NLTGV2Error):
        reg.volume_upload(ref.tsdf, bad)
    bad[2, 3, 4] = np.nan
    with pytest.raises(gpu.NLTGV2Error):
        reg.volume_upload(ref.tsdf, bad)
    vr.assert_same_volume(reg.volume_download(), ref, "after a refused upload")


# ---- a map that stays on the device ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_a_raycast_that_stays_on_the_device_feeds_the_metric_outputs_and_the_map_error(gpu):
    with gpu.Regularizer(0) as reg:
        reg.upload_graph(synth.make_graph("320x240", seed=9))  # (the two consumers need a graph)
        ref = create(gpu, reg, **vr.SCENE)
        m = vr.scene_map()
        for _ in range(2):
            integrate(gpu, reg, ref, m, vr.SCENE_K, vr.IDENTITY, "the scene")
        rows, cols = vr.SCENE_ROWS, vr.SCENE_COLS
        want = ref.raycast(vr.SCENE_KINV, vr.IDENTITY, rows, cols, **vr.SCENE_RAYCAST)
        reg.volume_raycast_begin(vr.SCENE_KINV, vr.IDENTITY, rows, cols, gpu.RaycastParams(copy_out=False, **vr.SCENE_RAYCAST))
        got = reg.volume_raycast_end()
        assert "map" not in got and got["hits"] == want["hits"] > 0
        dev = got["device"]["map"]
        vr.assert_same_map(fetch(dev, (rows, cols), F), want["map"], "the device map")
        metric = reg.metric_outputs(vr.SCENE_KINV, rows, cols, params=gpu.MetricParams(map_device=dev))
        mr.assert_same(metric, mr.metric_points(want["map"], vr.SCENE_KINV), mr.POINT_KEYS, "the raycast as map_device")
        assert metric["n_points"] == want["hits"]
        keep = on_device(m)
        err = reg.map_error(gpu.MapErrorParams(source=gpu.MAP_ERROR_TRUTH, map_device=keep.data_ptr(), truth_device=dev, win_size=5), rows, cols)
        er.assert_same(err, er.map_error(m, er.TRUTH, truth=want["map"], win_size=5), "the raycast as truth_device")
        assert err["n_valid"] > 0
        # ... and the raycast's view is still there behind the two consumers
        still = reg.volume_raycast_end()
        assert still["device"]["map"] == dev and still["counts"].tolist() == got["counts"].tolist()


# ---- the store's life cycle ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_the_volume_survives_topologies_and_runs_and_is_reset_replaced_and_destroyed(gpu):
    with gpu.Regularizer(0) as reg:
        with pytest.raises(gpu.NLTGV2Error):
            reg.volume_info()  # no volume yet
        ref = create(gpu, reg, **vr.SCENE)
        integrate(gpu, reg, ref, vr.scene_map(), vr.SCENE_K, vr.IDENTITY, "before any graph")
        reg.upload_graph(synth.make_graph("320x240", seed=3))
        reg.run(gpu.Params(), 4)
        vr.assert_same_volume(reg.volume_download(), ref, "after upload_graph and run")
        reg.upload_graph(synth.make_graph("320x240", seed=4))
        reg.run(gpu.Params(), 2)
        integrate(gpu, reg, ref, vr.scene_map(), vr.SCENE_K, turned_pose(), "after another graph")
        reg.volume_reset()
        ref.reset()
        vr.assert_same_volume(reg.volume_download(), ref, "after reset")
        assert np.all(ref.tsdf == 1) and np.all(ref.weight == 0)
        # create with other dimensions replaces it
        ref = create(gpu, reg, **VOLUMES["70x9x5"])
        assert reg.volume_info()["nx"] == 70 and reg.volume_download()["tsdf"].shape == (5, 9, 70)
        integrate(gpu, reg, ref, vr.scene_map(), vr.SCENE_K, vr.IDENTITY, "the replacement")
        reg.volume_destroy()
        for call in (lambda: reg.volume_integrate_begin(vr.SCENE_K, vr.IDENTITY, 24, 32, gpu.IntegrateParams(map_device=1)),
                     lambda: reg.volume_raycast_begin(vr.SCENE_KINV, vr.IDENTITY, 24, 32), reg.volume_reset, reg.volume_destroy,
                     reg.volume_download, reg.volume_info):
            with pytest.raises(gpu.NLTGV2Error) as ei:
                call()
            assert ei.value.status == -1
        ref = create(gpu, reg, **vr.SCENE)  # ... and a new one after that
        integrate(gpu, reg, ref, vr.scene_map(), vr.SCENE_K, vr.IDENTITY, "created again")


@pytest.mark.gpu
def test_gpu_every_error_comes_before_anything_is_enqueued(gpu):
    lib = gpu.load_library()
    fp = lambda a: np.ascontiguousarray(a, F).ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    with gpu.Regularizer(0) as reg:
        V, I, R = gpu.VolumeParams, gpu.IntegrateParams, gpu.RaycastParams
        for bad in (V(nx=0), V(ny=1025), V(nz=-1), V(nx=1024, ny=1024, nz=257), V(voxel_size=0.0), V(voxel_size=float("nan")), V(trunc=-1.0),
                    V(trunc=float("inf")), V(max_weight=0.0), V(origin=(0.0, float("inf"), 0.0))):
            with pytest.raises(gpu.NLTGV2Error) as ei:
                reg.volume_create(bad)
            assert ei.value.status == -1
        assert lib.flame_nltgv2_volume_create(reg._ctx, None) == -1
        ref = create(gpu, reg, **vr.SCENE)
        m = vr.scene_map()
        keep = on_device(m)
        dev = dict(map_device=keep.data_ptr())
        integrate(gpu, reg, ref, m, vr.SCENE_K, vr.IDENTITY, "the good call")
        rows, cols = m.shape
        view = reg.volume_raycast(vr.SCENE_KINV, vr.IDENTITY, rows, cols, R(**vr.SCENE_RAYCAST))
        with pytest.raises(gpu.NLTGV2Error):
            reg.volume_create(V(nx=0))  # a refused create leaves the volume
        # a begin of each stage is pending while the errors come
        reg.volume_integrate_begin(vr.SCENE_K, vr.IDENTITY, rows, cols, I(**dev))
        pending = ref.integrate(m, vr.SCENE_K, vr.IDENTITY)
        reg.volume_raycast_begin(vr.SCENE_KINV, vr.shifted_pose(0.15), rows, cols, R(**vr.SCENE_RAYCAST))
        want_view = ref.raycast(vr.SCENE_KINV, vr.shifted_pose(0.15), rows, cols, **vr.SCENE_RAYCAST)
        for name, p in dict(weight_0=I(weight=0.0, **dev), weight_negative=I(weight=-1.0, **dev), weight_nan=I(weight=float("nan"), **dev),
                            weight_inf=I(weight=float("inf"), **dev), no_resident_map=I(), no_filtered_map=I(use_filtered_map=True)).items():
            with pytest.raises(gpu.NLTGV2Error) as ei:
                reg.volume_integrate_begin(vr.SCENE_K, vr.IDENTITY, rows, cols, p)
            assert ei.value.status == (-4 if name.startswith("no_") else -1), name
        for r, c in ((0, cols), (rows, -1), (65536, 65536)):
            with pytest.raises(gpu.NLTGV2Error):
                reg.volume_integrate_begin(vr.SCENE_K, vr.IDENTITY, r, c, I(**dev))
        good_i = I(**dev)
        assert lib.flame_nltgv2_volume_integrate_begin(reg._ctx, None, fp(vr.IDENTITY), C.byref(good_i), rows, cols) == -1
        assert lib.flame_nltgv2_volume_integrate_begin(reg._ctx, fp(vr.SCENE_K), None, C.byref(good_i), rows, cols) == -1
        assert lib.flame_nltgv2_volume_integrate_begin(reg._ctx, fp(vr.SCENE_K), fp(vr.IDENTITY), None, rows, cols) == -1
        assert lib.flame_nltgv2_volume_integrate_end(reg._ctx, None) == -1
        base = dict(vr.SCENE_RAYCAST)
        for name, p in dict(dz_0=R(**{**base, "dz": 0.0}), dz_negative=R(**{**base, "dz": -0.05}), dz_nan=R(**{**base, "dz": float("nan")}),
                            dz_inf=R(**{**base, "dz": float("inf")}), z_near_nan=R(**{**base, "z_near": float("nan")}),
                            z_near_inf=R(**{**base, "z_near": float("inf")}), steps_0=R(**{**base, "n_steps": 0}),
                            steps_4097=R(**{**base, "n_steps": 4097})).items():
            with pytest.raises(gpu.NLTGV2Error) as ei:
                reg.volume_raycast_begin(vr.SCENE_KINV, vr.IDENTITY, rows, cols, p)
            assert ei.value.status == -1, name
        for r, c in ((0, cols), (rows, 0), (32768, 1), (1, 32768)):
            with pytest.raises(gpu.NLTGV2Error):
                reg.volume_raycast_begin(vr.SCENE_KINV, vr.IDENTITY, r, c, R(**base))
        good_r = R(**base)
        assert lib.flame_nltgv2_volume_raycast_begin(reg._ctx, None, fp(vr.IDENTITY), C.byref(good_r), rows, cols) == -1
        assert lib.flame_nltgv2_volume_raycast_begin(reg._ctx, fp(vr.SCENE_KINV), None, C.byref(good_r), rows, cols) == -1
        assert lib.flame_nltgv2_volume_raycast_begin(reg._ctx, fp(vr.SCENE_KINV), fp(vr.IDENTITY), None, rows, cols) == -1
        assert lib.flame_nltgv2_volume_raycast_end(reg._ctx, None) == -1
        assert lib.flame_nltgv2_volume_upload(reg._ctx, fp(ref.tsdf), None) == -1 and lib.flame_nltgv2_volume_upload(reg._ctx, None, fp(ref.weight)) == -1
        # the pending _ends, the volume's bytes and the earlier view are as they were
        got = reg.volume_integrate_end()
        vr.assert_same_counts(got, pending, vr.INTEGRATE_COUNTERS, "the pending integration")
        vr.assert_same_volume(reg.volume_download(), ref, "after the errors")
        got = reg.volume_raycast_end()
        vr.assert_same_counts(got, want_view, vr.RAYCAST_COUNTERS, "the pending raycast")
        vr.assert_same_map(got["map"], want_view["map"], "the pending raycast")
        assert view["hits"] > 0
    with gpu.Regularizer(0) as reg:  # no begin has succeeded
        reg.volume_create(V(**vr.SCENE))
        for end in (reg.volume_integrate_end, reg.volume_raycast_end):
            with pytest.raises(gpu.NLTGV2Error):
                end()
