"""flame_nltgv2_volume_* past one grid and off the axes, with the cases and preconditions of tests/test_volume_edges_ref.py: volumes whose
integration takes a second and a third round of the grid-stride loop, with a partial last workgroup; raycast targets past the sixteen
partial counter sets; a camera with a skew and a general bottom row under a rotation about no axis of the volume -- all bit for bit against
tests/volume_ref.py through the helpers of tests/test_gpu_volume.py -- and the device against the float64 restatement
tests/volume_ref64.py within propagated bounds."""
import numpy as np
import pytest

from tests import test_gpu_volume as tv
from tests import test_volume_edges_ref as cpu
from tests import volume_ref as vr
from tests import volume_ref64 as v64


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


# ---- A: volumes past one grid ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cpu.BIG))
def test_gpu_volumes_past_one_grid(gpu, reg, name):
    """67x63x63: 15 workgroups take a second round, the last one 195 voxels of it; 131x65x62: three rounds, the last workgroup ends inside
    its first wave; 1024x1x300: nx at its maximum, ny == 1, a second round of full workgroups.  Past 1024 workgroups the counters of a
    workgroup add up over its rounds, with the lanes past n in the ballots, and the counter slot is that of the capped grid."""
    cpu.check_big(name)  # the checker alone first: every round has updated, behind and outside voxels, the partial workgroup updated ones
    ref = tv.create(gpu, reg, **cpu.BIG[name])
    m = vr.scene_map()
    got = [tv.integrate(gpu, reg, ref, m, cpu.GENERAL_K, cpu.GENERAL_POSE, "%s, call %d" % (name, i), **kw)[0]
           for i, kw in enumerate(cpu.BIG_CALLS)]
    assert got[0]["updated"] == sum(r[0] for r in cpu.big_rounds(name)[0]) and got[0]["saturated"] == 0
    assert got[1]["saturated"] == got[1]["updated"] > 0
    rows, cols = cpu.BIG_TARGET
    view, _ = tv.raycast(gpu, reg, ref, cpu.general_kinv(rows, cols), cpu.GENERAL_BACK, rows, cols, name + " seen again", **cpu.CAST)
    assert view["hits"] > 0 or min(ref.nx, ref.ny, ref.nz) == 1


# ---- B: targets past sixteen workgroups ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["scene", "random"])
def test_gpu_raycast_into_targets_past_sixteen_workgroups(gpu, reg, which):
    """96 x 128: 48 full workgroups, the 16 partial counter sets wrap three times; 97 x 131: the last of 50 workgroups ends inside its
    third wave; hits, back and empty rays side by side, so the waves leave the step loop at different steps."""
    cpu.check_large(which)  # the checker alone first: hits, back and empty all above zero
    if which == "scene":
        ref = tv.create(gpu, reg, **vr.SCENE)
        for _ in range(2):
            tv.integrate(gpu, reg, ref, vr.scene_map(), vr.SCENE_K, vr.IDENTITY, "the scene")
    else:
        ref = cpu.random_volume()
        tv.create(gpu, reg, nx=9, ny=7, nz=11, voxel_size=0.1, origin=(-0.4, -0.3, 0.6), trunc=0.3, max_weight=8.0)
        reg.volume_upload(ref.tsdf, ref.weight)
        vr.assert_same_volume(reg.volume_download(), ref, "the random volume")
    want = iter(cpu.large_counts(which))
    for rows, cols in cpu.LARGE_TARGETS:
        for Kinv, T, what in cpu.large_views(rows, cols):
            got, _ = tv.raycast(gpu, reg, ref, Kinv, T, rows, cols, "%s into %dx%d from %s" % (which, rows, cols, what), **cpu.LARGE_CAST)
            assert {k: got[k] for k in vr.RAYCAST_COUNTERS} == next(want)[3]


# ---- C: the general camera and pose, and D: the device against float64 ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(cpu.GENERAL_VOLUMES))
def test_gpu_general_camera_and_pose(gpu, reg, name):
    """K with a skew and the bottom row 0.01 -0.02 1, a rotation by 17 degrees about (1, 2, 3): every entry of K, Kinv and both poses
    takes part in the sums, whose order then shows in the bits (with the older cases' matrices it does not).  Each integration is also
    compared with the float64 rules, within the bounds they carry."""
    if name == cpu.GENERAL_VOLUMES[0]:
        cpu.test_the_general_camera_shows_the_order_of_every_sum()  # the checker alone first: the case is sensitive to what it is for
    ref = tv.create(gpu, reg, **tv.VOLUMES[name])
    for call, (m, K, T, kw) in enumerate(cpu.general_calls()):
        before = reg.volume_download()
        want = v64.integrate(ref.nx, ref.ny, ref.nz, ref.voxel_size, ref.origin, ref.trunc, ref.max_weight, before["tsdf"], before["weight"],
                             m, K, T, **kw)
        got, _ = tv.integrate(gpu, reg, ref, m, K, T, "%s, call %d" % (name, call), **kw)
        assert got["updated"] > 0 and got["saturated"] == 0
        after = reg.volume_download()
        # (nothing saturates, so W > w_old: a voxel was updated iff its weight changed)
        updated = vr.bits(after["weight"]) != vr.bits(before["weight"])
        assert int(np.count_nonzero(updated)) == got["updated"]
        cpu.compare_integration(want, after["tsdf"], after["weight"], updated, "%s, call %d, the device" % (name, call))
    for rows, cols in tv.TARGETS:
        tv.raycast(gpu, reg, ref, cpu.general_kinv(rows, cols), cpu.GENERAL_BACK, rows, cols, "%s into %dx%d" % (name, rows, cols), **cpu.CAST)


@pytest.mark.gpu
def test_gpu_raycast_of_a_tilted_plane_is_the_ray_plane_intersection(gpu, reg):
    """A volume whose tsdf is an exact plane tilted against every axis, seen from a rotated camera with the general K: trilinear
    interpolation reproduces a linear field, so every hit is the float64 ray-plane intersection within c (EPS M / slope + EPS z), c
    derived in tests/volume_ref64.py (ray_plane) by counting the roundings.  The intersection does not say which rays hit: the counts
    and the map are the checker's."""
    cpu.test_the_checkers_raycast_of_a_tilted_plane_is_the_ray_plane_intersection()
    want, plane = cpu.plane_case()
    ref = cpu.plane_volume()
    tv.create(gpu, reg, max_weight=8.0, **cpu.PLANE)
    reg.volume_upload(ref.tsdf, ref.weight)
    rows, cols = cpu.PLANE_TARGET
    got, _ = tv.raycast(gpu, reg, ref, cpu.general_kinv(rows, cols), cpu.PLANE_BACK, rows, cols, "the plane", **cpu.PLANE_CAST)
    assert (got["hits"], got["back"], got["empty"]) == (want["hits"], want["back"], want["empty"])
    cpu.compare_plane(got["map"], plane, "the device")
