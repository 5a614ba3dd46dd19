"""flame_nltgv2_metric_outputs_begin / _end through the C-ABI against the checker tests/metric_ref.py, bit for bit, on the shapes and
validity patterns where an ordered compaction can go wrong; the mesh outputs on the scene of tests/test_mesh_outputs.py."""
import ctypes as C

import numpy as np
import pytest

from flame_amd import synth
from tests import mesh_ref as mr
from tests import metric_ref as xr
from tests.metric_helpers import INF, POSE, F, fetch, kinv_for, on_device, pinhole_kinv, special_map


@pytest.fixture(scope="module")
def gpu(built):
    import torch  # noqa: F401

    import flame_amd

    return flame_amd


@pytest.fixture(scope="module")
def small(gpu):
    """The scene of tests/test_mesh_outputs.py."""
    g = synth.make_graph("320x240", seed=9)
    return g, synth.delaunay_triangles_scipy(g["pos"]), kinv_for(320, 240)


@pytest.fixture(scope="module")
def reg(gpu, small):
    with gpu.Regularizer(0) as r:
        r.upload_graph(small[0])
        yield r


def check_points(gpu, reg, v, Kinv, pose=None, min_depth=0.0, max_depth=INF, what="", **flags):
    rows, cols = v.shape
    d = on_device(v)
    p = gpu.MetricParams(min_depth=min_depth, max_depth=max_depth, map_device=d.data_ptr(), **flags)
    got = reg.metric_outputs(Kinv, rows, cols, pose=pose, params=p)
    ref = xr.metric_points(v, Kinv, pose, min_depth, max_depth)
    xr.assert_same(got, ref, xr.POINT_KEYS, what)
    return got, ref


def validity_patterns(shape, rng):
    n = shape[0] * shape[1]
    base = rng.uniform(0.2, 4.0, n).astype(F)  # z in (0.25, 5)
    none, first, last = (np.full(n, np.nan, F) for _ in range(3))
    first[0], last[-1] = base[0], base[-1]
    half = base.copy()
    half[rng.random(n) < 0.5] = np.nan
    return {k: a.reshape(shape) for k, a in dict(none=none, first=first, last=last, all=base, half=half).items()}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1), (1, 63), (1, 64), (1, 65), (3, 70), (37, 29)])
def test_gpu_small_maps_every_validity_pattern_posed_and_clipped(gpu, reg, shape):
    rng = np.random.default_rng(100 * shape[0] + shape[1])
    Kinv = kinv_for(shape[1], shape[0])
    for name, v in validity_patterns(shape, rng).items():
        for pose in (None, POSE):
            for lo, hi in ((0.0, INF), (0.5, 3.0)):
                what = f"{shape} {name} pose={pose is not None} clip=({lo}, {hi})"
                got, ref = check_points(gpu, reg, v, Kinv, pose, lo, hi, what)
                if (lo, hi) == (0.0, INF):
                    assert got["n_points"] == dict(none=0, first=1, last=1, all=v.size).get(name, ref["n_points"]), what
                if name == "first" and got["n_points"]:
                    assert got["cloud_pixel"].tolist() == [0]
                if name == "last" and got["n_points"]:
                    assert got["cloud_pixel"].tolist() == [v.size - 1]
    if shape == (37, 29):
        clipped = xr.metric_points(validity_patterns(shape, np.random.default_rng(1))["all"], Kinv, None, 0.5, 3.0)
        assert 0 < clipped["n_points"] < 37 * 29  # (the window does cut)


@pytest.mark.gpu
def test_gpu_special_values_side_by_side(gpu, reg):
    v = special_map()
    for pose in (None, POSE):
        got, ref = check_points(gpu, reg, v, pinhole_kinv(), pose, what=f"special values, pose={pose is not None}")
        assert got["n_points"] == ref["n_points"] == 3 * 5  # 6e-39, 1e-30, 0.5, 2, 1 in each row
        assert np.isfinite(got["cloud"]).all()
        # both bounds are exclusive ON THE DEVICE: z = 1 / v is exactly 2, 0.5 and 1 for v = 0.5, 2 and 1, so the window (0.5, 2)
        # makes holes of the two pixels that lie on its edges and leaves v = 1; one ulp of room on either side lets them in
        got, _ = check_points(gpu, reg, v, pinhole_kinv(), pose, 0.5, 2.0, f"special values on the window's edges, pose={pose is not None}")
        assert got["n_points"] == 3 and got["cloud_pixel"].tolist() == [11, 12, 28]
        assert (got["depth"].reshape(-1)[[11, 12, 28]] == 1.0).all() and (got["depth_mm"].reshape(-1)[[11, 12, 28]] == 1000).all()
        below, above = np.nextafter(F(0.5), F(0)), np.nextafter(F(2), F(3))
        got, _ = check_points(gpu, reg, v, pinhole_kinv(), pose, below, above, f"one ulp of room, pose={pose is not None}")
        assert got["n_points"] == 9
        for lo, hi, n in ((0.5, above, 6), (below, 2.0, 6), (1.0, 2.0, 0), (0.5, 1.0, 0)):  # each edge alone; z = 1 on an edge
            got, _ = check_points(gpu, reg, v, pinhole_kinv(), pose, lo, hi, f"window ({lo}, {hi}), pose={pose is not None}")
            assert got["n_points"] == n, (lo, hi, got["n_points"])


@pytest.mark.gpu
def test_gpu_1080p_crosses_every_level_of_the_scan(gpu, reg):
    rng = np.random.default_rng(1080)
    v = rng.uniform(0.2, 4.0, (1080, 1920)).astype(F)
    v[rng.random(v.shape) < 0.5] = np.nan
    v[400:500] = np.nan      # whole workgroups without a point ...
    v[700:720] = 0.75        # ... and whole workgroups full of them
    Kinv = kinv_for(1920, 1080)
    plain = int((v > 0).sum())
    for pose in (None, POSE):
        for lo, hi in ((0.0, INF), (0.3, 4.5)):
            got, ref = check_points(gpu, reg, v, Kinv, pose, lo, hi, f"1080p pose={pose is not None} clip=({lo}, {hi})")
            print("1080p: pose", pose is not None, "clip", (lo, hi), "device_ms", got["device_ms"], "n_points", got["n_points"])
            if hi == INF:
                assert got["n_points"] == plain > 900_000
            else:
                assert 500_000 < got["n_points"] < plain  # (about 0.8 of the half that is not NaN lies in the window)


@pytest.mark.gpu
def test_gpu_outputs_one_by_one_and_on_the_device_only(gpu, reg):
    rng = np.random.default_rng(4)
    v = validity_patterns((37, 29), rng)["half"]
    Kinv = kinv_for(29, 37)
    ref = xr.metric_points(v, Kinv, POSE)
    d = on_device(v)
    names = dict(want_depth="depth", want_depth_mm="depth_mm", want_organized="organized", want_cloud="cloud")
    off = {k: False for k in names}
    for flag, key in names.items():
        got = reg.metric_outputs(Kinv, 37, 29, pose=POSE, params=gpu.MetricParams(map_device=d.data_ptr(), **{**off, flag: True}))
        keys = ("cloud", "cloud_pixel") if key == "cloud" else (key,)
        xr.assert_same(got, ref, keys, flag)
        assert set(got) & set(xr.POINT_KEYS) == set(keys) and set(got["device"]) == set(keys), flag
        assert got["n_points"] == (ref["n_points"] if key == "cloud" else 0)
    with pytest.raises(gpu.NLTGV2Error) as ei:
        reg.metric_outputs(Kinv, 37, 29, params=gpu.MetricParams(map_device=d.data_ptr(), **off))  # nothing wanted
    assert ei.value.status == -1
    # copy_out = 0: the counters travel, the arrays are fetched through the device pointers
    got = reg.metric_outputs(Kinv, 37, 29, pose=POSE, params=gpu.MetricParams(map_device=d.data_ptr(), copy_out=False))
    assert not set(got) & set(xr.POINT_KEYS) and got["n_points"] == ref["n_points"]
    n = got["n_points"]
    dev = got["device"]
    fetched = dict(depth=fetch(dev["depth"], (37, 29), F), depth_mm=fetch(dev["depth_mm"], (37, 29), np.uint16),
                   organized=fetch(dev["organized"], (37, 29, 3), F), cloud=fetch(dev["cloud"], (n, 3), F),
                   cloud_pixel=fetch(dev["cloud_pixel"], (n,), np.uint32), n_points=n)
    xr.assert_same(fetched, ref, xr.POINT_KEYS, "through the device pointers")
    # the synchronous entry point: the arrays that are not NULL
    lib = gpu.load_library()
    FP = C.POINTER(C.c_float)
    depth, cloud, pix, npts = np.empty((37, 29), F), np.empty((37 * 29, 3), F), np.empty(37 * 29, np.uint32), C.c_int32(-1)
    p = gpu.MetricParams(map_device=d.data_ptr(), copy_out=False, want_depth=False)
    pose = np.ascontiguousarray(POSE.reshape(-1))
    rc = lib.flame_nltgv2_metric_outputs(reg._ctx, Kinv.ctypes.data_as(FP), pose.ctypes.data_as(FP), C.byref(p), 37, 29, depth.ctypes.data_as(FP),
                                         None, None, cloud.ctypes.data_as(FP), pix.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(npts),
                                         None, None, None, None)
    assert rc == 0 and npts.value == n
    xr.assert_same(dict(depth=depth, cloud=cloud[:n], cloud_pixel=pix[:n], n_points=npts.value), ref, ("depth", "cloud", "cloud_pixel"), "synchronous")


def mesh_case(gpu, reg, small, filt, pose, use_filtered, scale=1.25):
    g, tris, Kinv = small
    reg.interpolate_mesh_begin(tris, 240, 320, graph_scale=scale)
    reg.mesh_outputs_begin(None, Kinv, 240, 320, graph_scale=scale, filter=gpu.MeshFilterParams(**filt), want_filtered_map=True)
    reg.metric_outputs_begin(Kinv, 240, 320, pose=pose, params=gpu.MetricParams(want_mesh=True, use_filtered_map=use_filtered))
    dense, _ = reg.interpolate_mesh_end()
    mo = reg.mesh_outputs_end()
    got = reg.metric_outputs_end()
    x = reg.download_state(("x",))["x"]
    ref = xr.metric_points(mo["filtered_map"] if use_filtered else dense, Kinv, pose)
    ref.update(xr.metric_mesh(g["pos"], x, scale, Kinv, mo["normals"], tris, mo["tri_valid"], pose))
    return got, ref, mo, dense


@pytest.mark.gpu
def test_gpu_mesh_with_no_some_and_all_triangles_valid_and_either_map(gpu, reg, small):
    g, tris, Kinv = small
    all_off = mr.params(do_oblique_triangle_filter=False, do_edge_length_filter=False, do_idepth_triangle_filter=False)
    seen = {}
    for name, filt in (("some", mr.params()), ("all", all_off), ("none", mr.params(min_triangle_idepth=INF))):
        for pose in (None, POSE):
            for use_filtered in (False, True):
                what = f"{name} valid, pose={pose is not None}, filtered map={use_filtered}"
                got, ref, mo, dense = mesh_case(gpu, reg, small, filt, pose, use_filtered)
                xr.assert_same(got, ref, xr.POINT_KEYS + xr.MESH_KEYS, what)
                assert got["n_valid"] == mo["n_valid"] == len(got["mesh_triangles"]), what
                assert (got["V"], got["T"]) == (g["V"], len(tris))
                seen[name, use_filtered] = (got["n_valid"], got["n_points"])
                if use_filtered:
                    assert np.array_equal(np.isnan(got["depth"]), np.isnan(mo["filtered_map"])), what
                else:
                    assert np.array_equal(np.isnan(got["depth"]), np.isnan(dense)), what
    # copy_out = 0 with the mesh: every array, the mesh's too, fetched through the view's device pointers
    mesh_case(gpu, reg, small, mr.params(), POSE, True)  # (the default filters again: some triangles valid)
    first = reg.metric_outputs(Kinv, 240, 320, pose=POSE, params=gpu.MetricParams(want_mesh=True, use_filtered_map=True))
    dev_only = reg.metric_outputs(Kinv, 240, 320, pose=POSE, params=gpu.MetricParams(want_mesh=True, use_filtered_map=True, copy_out=False))
    assert not set(dev_only) & set(xr.POINT_KEYS + xr.MESH_KEYS) and set(dev_only["device"]) == set(xr.POINT_KEYS + xr.MESH_KEYS)
    n, nv, V, dev = dev_only["n_points"], dev_only["n_valid"], g["V"], dev_only["device"]
    shapes = dict(depth=((240, 320), F), depth_mm=((240, 320), np.uint16), organized=((240, 320, 3), F), cloud=((n, 3), F),
                  cloud_pixel=((n,), np.uint32), mesh_vertices=((V, 3), F), mesh_normals=((V, 3), F), mesh_triangles=((nv, 3), np.int32))
    fetched = {k: fetch(dev[k], *shapes[k]) for k in shapes}
    fetched.update(n_points=n, n_valid=nv)
    xr.assert_same(fetched, first, xr.POINT_KEYS + xr.MESH_KEYS, "mesh and points through the device pointers")
    assert 0 < nv < len(tris) and n > 1000
    T = len(tris)
    assert seen["none", True] == (0, 0) and seen["all", True][0] == T and 0 < seen["some", True][0] < T
    # the filtered map has holes the unfiltered one has not: the two settings follow different maps
    assert seen["some", True][1] < seen["some", False][1] == seen["all", True][1] == seen["none", False][1]


@pytest.mark.gpu
def test_gpu_every_error_leaves_the_previous_view_and_a_repeat_gives_the_same_bytes(gpu, small):
    g, tris, Kinv = small
    lib = gpu.load_library()
    FP = C.POINTER(C.c_float)
    kp = Kinv.ctypes.data_as(FP)
    with gpu.Regularizer(0) as reg:
        p = gpu.MetricParams()
        assert lib.flame_nltgv2_metric_outputs_begin(reg._ctx, kp, None, C.byref(p), 240, 320) == -4  # no graph
        reg.upload_graph(g)
        for params in (gpu.MetricParams(), gpu.MetricParams(use_filtered_map=True), gpu.MetricParams(want_mesh=True, want_cloud=False)):
            with pytest.raises(gpu.NLTGV2Error) as ei:  # nothing resident yet
                reg.metric_outputs_begin(Kinv, 240, 320, params=params)
            assert ei.value.status == -1
        with pytest.raises(gpu.NLTGV2Error):
            reg.metric_outputs_end()  # no begin has succeeded
        reg.interpolate_mesh(tris, 240, 320)
        with pytest.raises(gpu.NLTGV2Error):  # a map, but no filtered one and no mesh buffers
            reg.metric_outputs_begin(Kinv, 240, 320, params=gpu.MetricParams(use_filtered_map=True))
        with pytest.raises(gpu.NLTGV2Error):
            reg.metric_outputs_begin(Kinv, 240, 320, params=gpu.MetricParams(want_mesh=True))
        reg.mesh_outputs(None, Kinv, 240, 320, want_filtered_map=True)
        full = gpu.MetricParams(want_mesh=True)
        first = reg.metric_outputs(Kinv, 240, 320, pose=POSE, params=full)
        again = reg.metric_outputs(Kinv, 240, 320, pose=POSE, params=full)  # unchanged state: identical bytes
        keys = xr.POINT_KEYS + xr.MESH_KEYS
        xr.assert_same(again, first, keys, "a repeated begin")
        assert (again["n_points"], again["n_valid"]) == (first["n_points"], first["n_valid"]) and first["n_points"] > 0 < first["n_valid"]
        view = reg.metric_outputs_end(copy=False)  # (a second _end of the same begin: the same view)
        xr.assert_same(view, first, keys, "a second _end")
        bad_calls = [lambda: reg.metric_outputs_begin(Kinv, 241, 320, params=full),   # another size than the resident map's
                     lambda: reg.metric_outputs_begin(Kinv, 240, 319, params=full),
                     lambda: reg.metric_outputs_begin(Kinv, 0, 320, params=full),
                     lambda: reg.metric_outputs_begin(Kinv, 240, -1, params=full),
                     lambda: reg.metric_outputs_begin(Kinv, 65536, 65536, params=full),
                     lambda: reg.metric_outputs_begin(Kinv, 120, 160, params=gpu.MetricParams(use_filtered_map=True))]
        for call in bad_calls:
            with pytest.raises(gpu.NLTGV2Error) as ei:
                call()
            assert ei.value.status == -1
        assert lib.flame_nltgv2_metric_outputs_begin(reg._ctx, None, None, C.byref(full), 240, 320) == -1
        assert lib.flame_nltgv2_metric_outputs_begin(reg._ctx, kp, None, None, 240, 320) == -1
        assert lib.flame_nltgv2_metric_outputs_end(reg._ctx, None) == -1
        # stale mesh buffers: another upload of the triangles, and the validity speaks of the list before
        reg.interpolate_mesh_begin(tris, 240, 320)
        with pytest.raises(gpu.NLTGV2Error) as ei:
            reg.metric_outputs_begin(Kinv, 240, 320, params=full)
        assert ei.value.status == -1
        reg.interpolate_mesh_end()
        kept = reg.metric_outputs_end()
        xr.assert_same(kept, first, keys, "after the errors")
        assert (kept["n_points"], kept["n_valid"]) == (first["n_points"], first["n_valid"])
        # ... the points alone need no mesh buffers
        pts = reg.metric_outputs(Kinv, 240, 320, pose=POSE)
        xr.assert_same(pts, first, xr.POINT_KEYS, "points without the mesh")
        # a new topology: the mesh buffers belong to the old one
        reg.mesh_outputs(None, Kinv, 240, 320)
        reg.metric_outputs(Kinv, 240, 320, params=full)
        reg.upload_graph(synth.make_graph("320x240", seed=10))
        with pytest.raises(gpu.NLTGV2Error):
            reg.metric_outputs_begin(Kinv, 240, 320, params=full)
