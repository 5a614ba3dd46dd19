"""flame_nltgv2_volume_shift* / _window / _follow through the C-ABI against the checker tests/volume_window_ref.py, bit for bit: the
shifted volume and its counters on both paths of the kernel, integration and raycast at a base that is not zero (near and far), the mesh
across a shift, every error before anything is enqueued, determinism, and a shift beside a running solver."""
import ctypes as C

import numpy as np
import pytest

from flame_amd import synth
from tests import test_volume_window_ref as cpu
from tests import volume_mesh_ref as vmr
from tests import volume_ref as vr
from tests import volume_window_ref as wr
from tests.metric_helpers import on_device

F = np.float32
SHIFTS = [(3, -2, 1), (2, 0, 0), (-5, 0, 0), (0, 0, 4), (0, 0, -3), (16, 0, 0), (0, 0, 0)]
SMALL = {"15x7x5": dict(nx=15, ny=7, nz=5, voxel_size=0.1, origin=(-0.7, -0.3, 0.7), trunc=0.3, max_weight=2.0),
         "2x1x1": dict(nx=2, ny=1, nz=1, voxel_size=0.1, origin=(-0.05, 0.0, 1.0), trunc=0.3, max_weight=2.0)}
STATE = ("x", "w1", "w2", "x_bar", "w1_bar", "w2_bar", "q1", "q2", "q3")


@pytest.fixture(scope="module")
def gpu(built):
    import torch  # noqa: F401

    import flame_amd

    assert hasattr(flame_amd.load_library(), "flame_nltgv2_volume_shift_begin")
    return flame_amd


@pytest.fixture(scope="module")
def reg(gpu):
    with gpu.Regularizer(0) as r:
        yield r


def create(gpu, reg, **params):
    reg.volume_create(gpu.VolumeParams(**params))
    return wr.Volume(**params)


def integrate(gpu, reg, ref, m, K, T, what, **kw):
    m = np.ascontiguousarray(m, F)
    keep = on_device(m)
    got = reg.volume_integrate(K, T, *m.shape, gpu.IntegrateParams(map_device=keep.data_ptr(), **kw))
    with np.errstate(all="ignore"):
        want = ref.integrate(m, K, T, **kw)
    print(what, got["counts"].tolist())
    vr.assert_same_counts(got, want, vr.INTEGRATE_COUNTERS, what)
    vr.assert_same_volume(reg.volume_download(), ref, what)
    return got


def shift(reg, ref, s, what, record_bytes=None):
    """One shift on the device and in the checker: the counters, the window, the path, then both arrays."""
    got = reg.volume_shift(s)
    want = ref.shift(s)
    print(what, tuple(s), got["counts"].tolist(), "record_bytes", got["record_bytes"], "device_ms %.3f" % got["device_ms"])
    wr.assert_same_counts(got, want, what)
    n = ref.nx * ref.ny * ref.nz
    assert got["kept"] + got["entered"] == n and got["counts"][4:].tolist() == [0, 0, 0, 0]
    assert got["shift"].tolist() == list(s) and got["base"].tolist() == ref.base.tolist() == reg.volume_window().tolist()
    if record_bytes is not None:
        assert got["record_bytes"] == record_bytes, what
    vr.assert_same_volume(reg.volume_download(), ref, what)
    return got, want


def raycast(gpu, reg, ref, Kinv, T, what):
    got = reg.volume_raycast(Kinv, T, vr.SCENE_ROWS, vr.SCENE_COLS, gpu.RaycastParams(**vr.SCENE_RAYCAST))
    want = ref.raycast(Kinv, T, vr.SCENE_ROWS, vr.SCENE_COLS, **vr.SCENE_RAYCAST)
    print(what, got["counts"].tolist())
    vr.assert_same_counts(got, want, vr.RAYCAST_COUNTERS, what)
    vr.assert_same_map(got["map"], want["map"], what)
    return got, want


# ---- 1: the shift against the checker ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("s", SHIFTS)
def test_gpu_a_shift_of_the_scene_equals_the_checkers(gpu, reg, s):
    ref = create(gpu, reg, **vr.SCENE)
    integrate(gpu, reg, ref, vr.scene_map(), vr.SCENE_K, vr.IDENTITY, "the scene")
    assert np.count_nonzero(ref.weight > 0) == 1278
    info = reg.volume_info()
    delta = (s[2] * 12 + s[1]) * 16 + s[0]
    got, want = shift(reg, ref, s, "the scene shifted", record_bytes=0 if s == (0, 0, 0) else 16 if delta % 2 == 0 else 8)
    if s == (3, -2, 1):
        assert (want["kept_seen"], want["lost_seen"]) == (912, 366) and got["record_bytes"] == 8
    if s == (2, 0, 0):
        assert (want["kept_seen"], want["lost_seen"]) == (1179, 99) and got["record_bytes"] == 16
    assert want["kept_seen"] + want["lost_seen"] == 1278 and (want["lost_seen"] > 0) == (s != (0, 0, 0))
    assert (want["kept_seen"] > 0) == (s != (16, 0, 0))
    # the second buffer exists from the first shift that moves anything
    assert reg.volume_info()["device_bytes"] in ((info["device_bytes"],) if s == (0, 0, 0) else (2 * 8 * 1920,))
    assert info["device_bytes"] in (8 * 1920, 2 * 8 * 1920)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SMALL))
def test_gpu_shifts_of_an_odd_row_length_and_of_two_voxels(gpu, reg, name):
    for s in ((1, 1, 1), (2, 0, 0)):
        ref = create(gpu, reg, **SMALL[name])
        integrate(gpu, reg, ref, vr.scene_map(), vr.SCENE_K, vr.IDENTITY, name)
        seen = np.count_nonzero(ref.weight > 0)
        assert seen > 0
        even = ref.nx % 2 == 0 and ((s[2] * ref.ny + s[1]) * ref.nx + s[0]) % 2 == 0
        got, want = shift(reg, ref, s, name, record_bytes=16 if even else 8)
        assert want["kept_seen"] + want["lost_seen"] == seen
        if name == "15x7x5":
            assert want["kept_seen"] > 0 and want["lost_seen"] > 0


@pytest.mark.gpu
def test_gpu_special_values_survive_both_paths(gpu, reg):
    rng = np.random.default_rng(3)
    for s, record_bytes in (((3, -2, 1), 8), ((2, 0, 0), 16), ((-4, 2, -2), 16)):
        ref = create(gpu, reg, **vr.SCENE)
        t = rng.uniform(-1, 1, ref.tsdf.shape).astype(F).view(np.uint32)
        w = rng.uniform(0, 2, ref.weight.shape).astype(F).view(np.uint32)
        special_t = np.array([0x7FC12345, 0xFFC00001, 0x7FFFFFFF, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000], np.uint32)
        special_w = np.array([0x80000000, 0x00000001, 0x007FFFFF, 0x7F800000, 0x00000000], np.uint32)  # (an upload wants weight >= 0)
        t.reshape(-1)[rng.choice(t.size, 400, replace=False)] = np.resize(special_t, 400)
        w.reshape(-1)[rng.choice(w.size, 400, replace=False)] = np.resize(special_w, 400)
        ref.tsdf, ref.weight = t.view(F).copy(), w.view(F).copy()
        reg.volume_upload(ref.tsdf, ref.weight)
        vr.assert_same_volume(reg.volume_download(), ref, "special values up and down")
        before = ref.copy()
        got, want = shift(reg, ref, s, "special values", record_bytes=record_bytes)
        # the checker's own claim, by hand: destination (i, j, k) holds the bytes of source (i, j, k) + s
        down = reg.volume_download()
        i, j, k = 5, 4, 3
        for name, arr in (("tsdf", before.tsdf), ("weight", before.weight)):
            assert vr.bits(down[name])[k, j, i] == vr.bits(arr)[k + s[2], j + s[1], i + s[0]]
        kept_special = np.isin(vr.bits(down["tsdf"]), special_t[:3])
        assert np.count_nonzero(kept_special) > 20  # NaN payloads arrived


# ---- 2: integration after a shift -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_integration_into_a_shifted_window_is_a_crop_of_the_fixed_volume(gpu, reg):
    cpu.test_integration_into_a_moving_window_is_a_crop_of_integration_into_a_fixed_volume()  # the checker alone first
    s = (3, -2, 1)
    fixed, _ = cpu.fixed_and_window(s)
    ref = create(gpu, reg, **vr.SCENE)
    m = vr.scene_map()
    integrate(gpu, reg, ref, m, vr.SCENE_K, vr.IDENTITY, "before the shift")
    shift(reg, ref, s, "between")
    got = integrate(gpu, reg, ref, m, vr.SCENE_K, vr.shifted_pose(0.3), "after the shift", weight=0.5)
    assert got["updated"] > 0
    down = reg.volume_download()
    lo = [max(0, s[a]) for a in range(3)]
    hi = [min(ref.dims[a], ref.dims[a] + s[a]) for a in range(3)]
    g = tuple(slice(lo[a], hi[a]) for a in (2, 1, 0))
    loc = tuple(slice(lo[a] - s[a], hi[a] - s[a]) for a in (2, 1, 0))
    assert np.count_nonzero(fixed.weight[g] == F(1.5)) > 100
    assert np.array_equal(vr.bits(down["tsdf"][loc]), vr.bits(fixed.tsdf[g])), "not a crop of the fixed volume: has the origin moved?"
    assert np.array_equal(vr.bits(down["weight"][loc]), vr.bits(fixed.weight[g]))


# ---- 3: the raycast at a base that is not zero ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_raycast_near_and_far(gpu, reg):
    ref = create(gpu, reg, **vr.SCENE)
    m = vr.scene_map()
    integrate(gpu, reg, ref, m, vr.SCENE_K, vr.IDENTITY, "before the shift")
    shift(reg, ref, (3, -2, 1), "near")
    integrate(gpu, reg, ref, m, vr.SCENE_K, vr.shifted_pose(0.3), "after the shift", weight=0.5)
    for T in (vr.shifted_pose(0.3), vr.shifted_pose(0.15)):
        got, want = raycast(gpu, reg, ref, vr.SCENE_KINV, T, "near")
        assert want["hits"] > 0
    # a far window: everything leaves, the camera goes along
    far = (1000, -2000, 4000)
    got, want = shift(reg, ref, far, "far")
    assert want["kept"] == 0 and ref.base.tolist() == [1003, -2002, 4001]
    T_world_cam = vr.IDENTITY.copy()
    T_world_cam[3], T_world_cam[7], T_world_cam[11] = [F(ref.base[a] * 0.1) for a in range(3)]
    T_cam_world = vr.IDENTITY.copy()
    T_cam_world[3], T_cam_world[7], T_cam_world[11] = -T_world_cam[3], -T_world_cam[7], -T_world_cam[11]
    got = integrate(gpu, reg, ref, m, vr.SCENE_K, T_cam_world, "far")
    assert got["updated"] > 500
    got, want = raycast(gpu, reg, ref, vr.SCENE_KINV, T_world_cam, "far")
    assert want["hits"] > 0 and want["empty"] < vr.SCENE_ROWS * vr.SCENE_COLS


# ---- 4: the mesh across a shift ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_the_mesh_of_the_kept_box_keeps_its_bytes_across_a_shift(gpu, reg):
    s = (3, -2, 1)
    ref = create(gpu, reg, **vr.SCENE)
    integrate(gpu, reg, ref, vr.scene_map(), vr.SCENE_K, vr.IDENTITY, "the scene")
    T = vr.IDENTITY.copy()
    T[3], T[7], T[11] = 0.35, -0.25, 1.15  # (3.5, -2.5, 1.5) voxels off the middle voxel
    plan = reg.volume_follow(T, gpu.FollowParams(step=1))
    want_plan = wr.follow(ref, T, step=1)
    assert plan["shift"].tolist() == want_plan["shift"] == list(s)
    assert plan["kept"] == tuple(want_plan["kept"]) and plan["leaving"] == want_plan["leaving"] and len(plan["leaving"]) == 3
    whole = reg.volume_mesh()
    vmr.assert_same_mesh(whole, wr.extract(ref), "the whole window before")
    parts = []
    for lo, hi in plan["leaving"] + [plan["kept"]]:
        parts.append(reg.volume_mesh(lo=lo, hi=hi))
        vmr.assert_same_mesh(parts[-1], wr.extract(ref, lo, hi), "box %r %r" % (lo, hi))
    assert whole["n_triangles"] > 0 and sum(p["n_triangles"] for p in parts) == whole["n_triangles"]
    before = parts[-1]
    shift(reg, ref, s, "between the meshes")
    after = reg.volume_mesh()
    want = wr.extract(ref)
    vmr.assert_same_mesh(after, want, "the whole window after")
    assert after["n_triangles"] == before["n_triangles"] > 0 and np.array_equal(after["triangles"], before["triangles"])
    assert np.array_equal(vr.bits(after["vertices"]), vr.bits(before["vertices"])), "a kept vertex moved"
    same = wr.normals_untouched(ref, want["keys"], s)
    assert 0 < np.count_nonzero(same) < same.size
    assert np.array_equal(vr.bits(after["normals"][same]), vr.bits(before["normals"][same]))


# ---- 5: errors --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_every_error_comes_before_anything_is_enqueued(gpu):
    lib = gpu.load_library()
    with gpu.Regularizer(0) as reg:
        for call in (lambda: reg.volume_shift_begin((1, 0, 0)), reg.volume_window, lambda: reg.volume_follow(vr.IDENTITY), reg.volume_shift_end):
            with pytest.raises(gpu.NLTGV2Error) as ei:
                call()  # no volume
            assert ei.value.status == -1
        ref = create(gpu, reg, **vr.SCENE)
        integrate(gpu, reg, ref, vr.scene_map(), vr.SCENE_K, vr.IDENTITY, "the scene")
        with pytest.raises(gpu.NLTGV2Error):
            reg.volume_shift_end()  # no begin yet
        shift(reg, ref, (1, 0, -1), "a good shift")
        reg.volume_shift_begin((0, 2, 0))  # pending while the errors come
        pending = ref.shift((0, 2, 0))
        plan = gpu.FollowPlan()
        fp = np.ascontiguousarray(vr.IDENTITY).ctypes.data_as(C.POINTER(C.c_float))
        bad = [lambda: lib.flame_nltgv2_volume_shift_begin(reg._ctx, None), lambda: lib.flame_nltgv2_volume_shift(reg._ctx, None, None),
               lambda: lib.flame_nltgv2_volume_window(reg._ctx, None),
               lambda: lib.flame_nltgv2_volume_follow(reg._ctx, None, C.byref(gpu.FollowParams()), C.byref(plan)),
               lambda: lib.flame_nltgv2_volume_follow(reg._ctx, fp, None, C.byref(plan)),
               lambda: lib.flame_nltgv2_volume_follow(reg._ctx, fp, C.byref(gpu.FollowParams()), None),
               lambda: lib.flame_nltgv2_volume_follow(reg._ctx, fp, C.byref(gpu.FollowParams(step=0)), C.byref(plan)),
               lambda: lib.flame_nltgv2_volume_follow(reg._ctx, fp, C.byref(gpu.FollowParams(step=-8)), C.byref(plan)),
               lambda: lib.flame_nltgv2_volume_follow(reg._ctx, fp, C.byref(gpu.FollowParams(focus_depth=float("nan"))), C.byref(plan)),
               lambda: lib.flame_nltgv2_volume_shift_begin(reg._ctx, (C.c_int32 * 3)(wr.MAX_BASE, 0, 0)),
               lambda: lib.flame_nltgv2_volume_shift_begin(reg._ctx, (C.c_int32 * 3)(0, 0, -wr.MAX_BASE)),
               lambda: lib.flame_nltgv2_volume_shift_begin(reg._ctx, (C.c_int32 * 3)(0, 2**31 - 1, 0)),
               lambda: lib.flame_nltgv2_volume_shift_begin(reg._ctx, (C.c_int32 * 3)(-2**31, 0, 0))]
        for T in (np.where(np.arange(12) == 7, np.nan, vr.IDENTITY), np.where(np.arange(12) == 3, np.inf, vr.IDENTITY),
                  np.where(np.arange(12) == 11, 1e9, vr.IDENTITY)):
            t = np.ascontiguousarray(T, F)
            bad.append(lambda t=t: lib.flame_nltgv2_volume_follow(reg._ctx, t.ctypes.data_as(C.POINTER(C.c_float)), C.byref(gpu.FollowParams()), C.byref(plan)))
        for n, call in enumerate(bad):
            assert call() == -1, n
            assert reg.volume_window().tolist() == ref.base.tolist() == [1, 2, -1], n
        # the rule reads t and the third column of R, the literal product included: 0 * NaN is a NaN
        for at, status in ((0, 0), (5, 0), (2, -1)):
            t = np.ascontiguousarray(np.where(np.arange(12) == at, np.nan, vr.IDENTITY), F)
            assert lib.flame_nltgv2_volume_follow(reg._ctx, t.ctypes.data_as(C.POINTER(C.c_float)), C.byref(gpu.FollowParams()), C.byref(plan)) == status
        got = reg.volume_shift_end()  # the pending end still answers its own call
        wr.assert_same_counts(got, pending, "the pending end")
        assert got["shift"].tolist() == [0, 2, 0] and got["base"].tolist() == [1, 2, -1]
        vr.assert_same_volume(reg.volume_download(), ref, "after the refused calls")
        # up to the limit and no further
        shift(reg, ref, (wr.MAX_BASE - 1, -wr.MAX_BASE - 2, 0), "to the limit")
        assert ref.base.tolist() == [wr.MAX_BASE, -wr.MAX_BASE, -1]
        for s in ((1, 0, 0), (0, -1, 0)):
            with pytest.raises(gpu.NLTGV2Error) as ei:
                reg.volume_shift(s)
            assert ei.value.status == -1 and reg.volume_window().tolist() == ref.base.tolist()
        # reset and upload leave the window; create puts it back to zero
        reg.volume_reset()
        assert reg.volume_window().tolist() == ref.base.tolist()
        reg.volume_upload(ref.tsdf, ref.weight)
        assert reg.volume_window().tolist() == ref.base.tolist()
        reg.volume_create(gpu.VolumeParams(**vr.SCENE))
        assert reg.volume_window().tolist() == [0, 0, 0]
    with gpu.Regularizer(0) as fresh:
        fresh.volume_create(gpu.VolumeParams(**vr.SCENE))
        with pytest.raises(gpu.NLTGV2Error) as ei:
            fresh.volume_shift_end()  # _end without _begin
        assert ei.value.status == -1


# ---- 6: determinism ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_the_same_sequence_twice_gives_the_same_bytes(gpu, reg):
    runs = []
    for _ in range(2):
        ref = create(gpu, reg, **vr.SCENE)
        m = vr.scene_map()
        out = []
        for n, s in enumerate(((3, -2, 1), (2, 0, 0), (-4, 1, 0), (0, 0, 0), (1, 1, -2))):
            integrate(gpu, reg, ref, m, vr.SCENE_K, vr.shifted_pose(0.1 * n), "call %d" % n, weight=0.5)
            got, _ = shift(reg, ref, s, "shift %d" % n)
            d = reg.volume_download()
            out.append((got["counts"].tobytes(), d["tsdf"].tobytes(), d["weight"].tobytes()))
        runs.append(out)
    assert runs[0] == runs[1]


# ---- 7: beside the solver ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_a_shift_beside_a_running_solver_leaves_its_result_alone(gpu):
    steps = 60
    g = synth.make_graph("320x240", seed=9)
    with gpu.Regularizer(0) as alone:
        alone.upload_graph(g)
        alone.run(gpu.Params(), steps)
        state_alone = alone.download_state()
    with gpu.Regularizer(0) as reg:
        ref = create(gpu, reg, **vr.SCENE)
        integrate(gpu, reg, ref, vr.scene_map(), vr.SCENE_K, vr.IDENTITY, "the scene")
        reg.upload_graph(g)
        reg.run_async(gpu.Params(), steps)
        reg.volume_shift_begin((3, -2, 1))
        first = reg.volume_shift_end()
        reg.volume_shift_begin((2, 0, 0))
        reg.sync()
        second = reg.volume_shift_end()
        state = reg.download_state()
        wr.assert_same_counts(first, ref.shift((3, -2, 1)), "the first shift beside the solver")
        wr.assert_same_counts(second, ref.shift((2, 0, 0)), "the second")
        vr.assert_same_volume(reg.volume_download(), ref, "two shifts beside the solver")
    for k in STATE:
        assert np.array_equal(state[k], state_alone[k]), k
