"""The loop the window is for, eight frames of a camera that flies 0.25 m per frame along x past the scene's window (2.5 voxels per frame,
followed in steps of 2 voxels around a point 1 m ahead):

    volume_follow -> volume_mesh of each leaving box -> volume_shift -> volume_integrate -> volume_raycast

Every output of every frame equals the checker's (tests/volume_window_ref.py) bit for bit; the shifts mix 0, 2 and 4 voxels, the meshes
streamed out are not empty, and at the end the window has moved by its own width."""
import numpy as np
import pytest

from tests import volume_mesh_ref as vmr
from tests import volume_ref as vr
from tests import volume_window_ref as wr
from tests.metric_helpers import on_device

F = np.float32
FRAMES, STEP, FOCUS = 8, 2, 1.0


@pytest.mark.gpu
def test_gpu_the_window_follows_a_camera_for_eight_frames(built):
    import torch  # noqa: F401

    import flame_amd as fa

    assert hasattr(fa.load_library(), "flame_nltgv2_volume_follow")
    ref = wr.scene_volume()
    m = vr.scene_map()
    keep = on_device(m)
    shifts, streamed = [], 0
    with fa.Regularizer(0) as reg:
        reg.volume_create(fa.VolumeParams(**vr.SCENE))
        for f in range(FRAMES):
            T_world_cam = vr.shifted_pose(0.25 * f)
            T_cam_world = vr.shifted_pose(-0.25 * f)
            what = "frame %d" % f
            plan = reg.volume_follow(T_world_cam, fa.FollowParams(focus_depth=FOCUS, step=STEP))
            want = wr.follow(ref, T_world_cam, focus_depth=FOCUS, step=STEP)
            assert plan["shift"].tolist() == want["shift"] and plan["leaving"] == want["leaving"], what
            assert (plan["kept"] is None) == (want["kept"] is None) and (plan["kept"] is None or plan["kept"] == tuple(want["kept"])), what
            for lo, hi in plan["leaving"]:  # the map streamed out before it is lost
                mesh = reg.volume_mesh(lo=lo, hi=hi)
                vmr.assert_same_mesh(mesh, wr.extract(ref, lo, hi), what + " leaving %r %r" % (lo, hi))
                streamed += mesh["n_triangles"]
            got = reg.volume_shift(plan["shift"])
            wr.assert_same_counts(got, ref.shift(want["shift"]), what)
            assert got["base"].tolist() == ref.base.tolist() == reg.volume_window().tolist(), what
            got = reg.volume_integrate(vr.SCENE_K, T_cam_world, *m.shape, fa.IntegrateParams(map_device=keep.data_ptr()))
            vr.assert_same_counts(got, ref.integrate(m, vr.SCENE_K, T_cam_world), vr.INTEGRATE_COUNTERS, what)
            assert got["updated"] > 1000, what  # the window is where the camera looks
            vr.assert_same_volume(reg.volume_download(), ref, what)
            got = reg.volume_raycast(vr.SCENE_KINV, T_world_cam, vr.SCENE_ROWS, vr.SCENE_COLS, fa.RaycastParams(**vr.SCENE_RAYCAST))
            ray = ref.raycast(vr.SCENE_KINV, T_world_cam, vr.SCENE_ROWS, vr.SCENE_COLS, **vr.SCENE_RAYCAST)
            vr.assert_same_counts(got, ray, vr.RAYCAST_COUNTERS, what)
            vr.assert_same_map(got["map"], ray["map"], what)
            assert ray["hits"] > 400, what
            shifts.append(tuple(want["shift"]))
            print(what, shifts[-1], ref.base.tolist(), "hits", ray["hits"])
    assert {s[0] for s in shifts} == {0, 2, 4} and all(s[1:] == (0, 0) for s in shifts)
    assert streamed > 500 and ref.base[0] >= 16
