"""flame_nltgv2_volume_mesh_* through the C-ABI against the checker tests/volume_mesh_ref.py, bit for bit: vertices and normals as
uint32, triangles, every counter.  The volumes of tests/test_gpu_volume.py (smaller than a wave, x rows that end inside a wave and span
more than two, an axis of one voxel) after their integrations, the volume untouched and the same call twice the same bytes; an uploaded
sphere, random signs with unobserved pockets; the capacities; no normals; nothing but the counters on their way; the synchronous call;
every error before anything is enqueued.  (Zeros and non-finite values, the checkerboard, the volume past 1024 workgroups and the boxes:
tests/test_gpu_volume_mesh_edges.py.)"""
import ctypes as C

import numpy as np
import pytest

from tests import test_volume_mesh_ref as cpu
from tests import volume_mesh_ref as mr
from tests import volume_ref as vr
from tests.metric_helpers import fetch, on_device
from tests.test_gpu_volume import VOLUMES, turned_pose

F = np.float32


@pytest.fixture(scope="module")
def gpu(built):
    import torch  # noqa: F401

    import flame_amd

    assert hasattr(flame_amd.load_library(), "flame_nltgv2_volume_mesh_begin")
    return flame_amd


@pytest.fixture(scope="module")
def reg(gpu):
    with gpu.Regularizer(0) as r:
        yield r


def create(gpu, reg, **params):
    reg.volume_create(gpu.VolumeParams(**params))
    return vr.Volume(**params)


def uploaded(gpu, reg, tsdf, weight=None, voxel_size=0.1, origin=(-0.3, 0.2, 0.5)):
    """A volume with these values on the device and in the checker."""
    nz, ny, nx = tsdf.shape
    ref = create(gpu, reg, nx=nx, ny=ny, nz=nz, voxel_size=voxel_size, origin=origin, trunc=0.3, max_weight=2.0)
    ref.tsdf = np.ascontiguousarray(tsdf, F)
    ref.weight = np.ones(tsdf.shape, F) if weight is None else np.ascontiguousarray(weight, F)
    reg.volume_upload(ref.tsdf, ref.weight)
    return ref


def mesh(gpu, reg, ref, what, lo=(0, 0, 0), hi=(0, 0, 0), want_normals=True):
    """A count query, then the call with exactly the counts it gave: both against the checker."""
    want = mr.extract(ref, lo, hi, want_normals=want_normals)
    q = reg.volume_mesh(gpu.VolumeMeshParams(lo, hi, 0, 0, want_normals, True))
    empty = want["n_vertices"] == 0 and want["n_triangles"] == 0
    for k in mr.MESH_COUNTERS[:4]:
        assert q[k] == want[k], f"{what}, the count query: {k} {q[k]} vs the checker's {want[k]}"
    assert q["overflow"] == (0 if empty else 1) and q["counts"][5:].tolist() == [0, 0, 0]
    got = reg.volume_mesh(gpu.VolumeMeshParams(lo, hi, want["n_vertices"], want["n_triangles"], want_normals, True))
    print(what, got["counts"].tolist(), "device_ms %.3f" % got["device_ms"], "passes", got["pass_ms"].round(3).tolist())
    mr.assert_same_mesh(got, want, what, normals=want_normals)
    assert ("normals" in got) == want_normals and got["counts"][5:].tolist() == [0, 0, 0]
    return got, want


def integrate_both(gpu, reg, ref, m, K, T, **kw):
    m = np.ascontiguousarray(m, F)
    keep = on_device(m)
    reg.volume_integrate(K, T, *m.shape, gpu.IntegrateParams(map_device=keep.data_ptr(), **kw))
    with np.errstate(all="ignore"):
        ref.integrate(m, K, T, **kw)
    vr.assert_same_volume(reg.volume_download(), ref, "the integration before the extraction")


# ---- small volumes after their integrations ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VOLUMES))
def test_gpu_the_volumes_around_a_wave_after_their_integrations(gpu, reg, name):
    ref = create(gpu, reg, **VOLUMES[name])
    m = vr.scene_map()
    integrate_both(gpu, reg, ref, m, vr.SCENE_K, vr.IDENTITY)
    integrate_both(gpu, reg, ref, (m * F(0.97)).astype(F), vr.SCENE_K, turned_pose(), weight=0.5)
    before = reg.volume_download()
    got, want = mesh(gpu, reg, ref, name)
    if min(ref.nx, ref.ny, ref.nz) == 1:
        assert [got[k] for k in mr.MESH_COUNTERS] == [0, 0, 0, 0, 0]
    else:
        assert got["n_triangles"] > 0 and got["live_cubes"] > got["surface_cubes"] > 0 and got["device_ms"] > 0
    after = reg.volume_download()
    for k in ("tsdf", "weight"):
        assert np.array_equal(vr.bits(before[k]), vr.bits(after[k])), "the extraction wrote the volume's " + k
    again = reg.volume_mesh(gpu.VolumeMeshParams(max_vertices=want["n_vertices"], max_triangles=want["n_triangles"]))
    for k in ("vertices", "normals", "triangles", "counts"):
        assert again[k].tobytes() == got[k].tobytes(), "the same call twice: " + k


# ---- uploaded contents ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_an_uploaded_sphere(gpu, reg):
    cpu.test_a_sphere_is_closed_of_genus_zero_and_faces_outwards()  # the checker alone first
    s = cpu.sphere()
    ref = uploaded(gpu, reg, s.tsdf, voxel_size=1.0, origin=(0, 0, 0))
    got, _ = mesh(gpu, reg, ref, "the sphere")
    assert got["live_cubes"] == 13 ** 3 and got["n_vertices"] - 3 * got["n_triangles"] // 2 + got["n_triangles"] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("dims,seed,unseen", [((6, 7, 8), 11, 9), ((70, 9, 5), 3, 200), ((130, 3, 2), 4, 30), ((5, 3, 7), 5, 6)])
def test_gpu_random_signs_with_unobserved_pockets(gpu, reg, dims, seed, unseen):
    tsdf, weight = mr.random_signs(*dims, seed, unseen)
    ref = uploaded(gpu, reg, tsdf, weight)
    got, want = mesh(gpu, reg, ref, "random signs %dx%dx%d" % dims)
    assert 0 < got["live_cubes"] < (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1) and got["n_triangles"] > 0


# ---- capacity, variants -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_capacities_no_normals_and_nothing_but_the_counters(gpu, reg):
    tsdf, weight = mr.random_signs(16, 12, 10, 8, 25)
    ref = uploaded(gpu, reg, tsdf, weight)
    P = gpu.VolumeMeshParams
    exact, want = mesh(gpu, reg, ref, "exact capacity")
    nv, nt = want["n_vertices"], want["n_triangles"]
    for mv, mt in ((nv - 1, nt), (nv, nt - 1), (0, 0), (0, nt), (nv, 0)):
        got = reg.volume_mesh(P(max_vertices=mv, max_triangles=mt))
        assert got["overflow"] == 1 and "vertices" not in got and "triangles" not in got
        assert [got[k] for k in mr.MESH_COUNTERS[:4]] == [want[k] for k in mr.MESH_COUNTERS[:4]]
    roomy = reg.volume_mesh(P(max_vertices=2 ** 31 - 1, max_triangles=2 ** 31 - 1))
    mr.assert_same_mesh(roomy, want, "more room than the box can fill")
    mesh(gpu, reg, ref, "without normals", want_normals=False)
    # the convenience call: a count query, then exactly the counts
    auto = reg.volume_mesh()
    mr.assert_same_mesh(auto, want, "volume_mesh() without params")
    # copy_out = 0: only counters travel, the arrays are on the device
    reg.volume_mesh_begin(P(max_vertices=nv, max_triangles=nt, copy_out=False))
    dev = reg.volume_mesh_end()
    assert "vertices" not in dev and "normals" not in dev and "triangles" not in dev and dev["overflow"] == 0
    got = dict(dev, vertices=fetch(dev["device"]["vertices"], (nv, 3), F), normals=fetch(dev["device"]["normals"], (nv, 3), F),
               triangles=fetch(dev["device"]["triangles"], (nt, 3), np.int32))
    mr.assert_same_mesh(got, want, "the arrays on the device")
    # the synchronous call into the caller's arrays
    lib = gpu.load_library()
    v, n, t = np.zeros((nv, 3), F), np.zeros((nv, 3), F), np.zeros((nt, 3), np.int32)
    c = gpu.VolumeMeshCounts()
    p = P(max_vertices=nv, max_triangles=nt, copy_out=False, want_normals=False)  # (both are forced)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    assert lib.flame_nltgv2_volume_mesh(reg._ctx, C.byref(p), fp(v), fp(n), t.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(c)) == 0
    mr.assert_same_mesh(dict(vertices=v, normals=n, triangles=t, **{k: getattr(c, k) for k in mr.MESH_COUNTERS}), want, "flame_nltgv2_volume_mesh")
    assert lib.flame_nltgv2_volume_mesh(reg._ctx, C.byref(p), None, None, None, C.byref(c)) == 0 and c.n_vertices == nv and c.overflow == 0
    d = P()
    lib.flame_nltgv2_default_volume_mesh_params(C.byref(d))
    assert bytes(d) == bytes(P())


# ---- errors -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_every_error_comes_before_anything_is_enqueued(gpu):
    lib = gpu.load_library()
    P = gpu.VolumeMeshParams
    with gpu.Regularizer(0) as reg:
        with pytest.raises(gpu.NLTGV2Error) as ei:
            reg.volume_mesh_begin(P())  # no volume
        assert ei.value.status == -1
        with pytest.raises(gpu.NLTGV2Error):
            reg.volume_mesh_end()  # nothing pending
        tsdf, weight = mr.random_signs(16, 12, 10, 8, 25)
        ref = uploaded(gpu, reg, tsdf, weight)
        want = mr.extract(ref)
        reg.volume_mesh_begin(P(max_vertices=want["n_vertices"], max_triangles=want["n_triangles"]))  # pending while the errors come
        bad = [P(hi=(17, 12, 10)), P(hi=(16, 0, 10)), P(lo=(-1, 0, 0), hi=(16, 12, 10)), P(lo=(4, 0, 0), hi=(4, 12, 10)), P(lo=(5, 0, 0), hi=(4, 12, 10)),
               P(lo=(16, 0, 0)), P(max_vertices=-1), P(max_triangles=-1), P(lo=(0, 12, 0), hi=(16, 13, 10))]
        for p in bad:
            with pytest.raises(gpu.NLTGV2Error) as ei:
                reg.volume_mesh_begin(p)
            assert ei.value.status == -1
        assert lib.flame_nltgv2_volume_mesh_begin(reg._ctx, None) == -1
        assert lib.flame_nltgv2_volume_mesh_end(reg._ctx, None) == -1
        got = reg.volume_mesh_end()
        mr.assert_same_mesh(got, want, "the pending end after the errors")
        for p in bad[:3]:
            with pytest.raises(gpu.NLTGV2Error):
                reg.volume_mesh_begin(p)
        again = reg.volume_mesh_end()  # the view is still there
        mr.assert_same_mesh(again, want, "the earlier view after more errors")
        vr.assert_same_volume(reg.volume_download(), ref, "the volume after the errors")
        reg.volume_destroy()
        with pytest.raises(gpu.NLTGV2Error):
            reg.volume_mesh_begin(P())
        # a box over 2^26 voxels needs a volume over 2^26 voxels: created and filled (545 MB on the device), never downloaded or meshed
        reg.volume_create(gpu.VolumeParams(nx=1024, ny=1024, nz=65))
        for p in (P(), P(hi=(1024, 1024, 65)), P(lo=(0, 0, 0), hi=(1024, 1024, 65), max_vertices=0)):
            with pytest.raises(gpu.NLTGV2Error) as ei:
                reg.volume_mesh_begin(p)
            assert ei.value.status == -1
        reg.volume_destroy()
