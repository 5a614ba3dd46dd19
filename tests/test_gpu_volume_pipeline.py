"""The volumetric map behind the solver, at 320x240 with a 64x48x32 volume: for four poses

    synth graph -> upload_graph -> run -> interpolate_mesh -> volume_integrate_begin (the resident map)

then a raycast at a fifth pose with copy_out = 0, the last frame's mesh rendered into that pose, and map_error (TRUTH) of the rendered map
against the raycast, both on the device.  Every stage must equal the chained checkers bit for bit: oracle.run and the raster oracle for
the map, tests/volume_ref.py for the volume after every call and for the raycast, tests/view_ref.py and tests/map_error_ref.py behind
them.  The volume outlives the four topologies."""
import numpy as np
import pytest

from flame_amd import synth
from tests import map_error_ref as er
from tests import view_ref as viewref
from tests import volume_ref as vr
from tests.metric_helpers import fetch

F = np.float32
W, H = 320, 240
K = np.array([250, 0, 160, 0, 250, 120, 0, 0, 1], F)
KINV = np.array([1 / 250, 0, -160 / 250, 0, 1 / 250, -120 / 250, 0, 0, 1], np.float64).astype(F)
VOLUME = dict(nx=64, ny=48, nz=32, voxel_size=0.04, origin=(-1.28, -0.96, 0.5), trunc=0.12, max_weight=3.0)
CENTRES = [(0.0, 0.0, 0.0), (0.03, 0.0, 0.0), (0.0, 0.02, 0.01), (-0.03, 0.01, 0.0), (0.015, -0.01, 0.005)]  # the cameras in the world
STEPS = 20


def world_cam(c):
    return np.array([1, 0, 0, c[0], 0, 1, 0, c[1], 0, 0, 1, c[2]], F)


def cam_world(c):
    return np.array([1, 0, 0, -c[0], 0, 1, 0, -c[1], 0, 0, 1, -c[2]], F)


@pytest.mark.gpu
def test_gpu_four_frames_integrated_and_a_fifth_pose_raycast(built):
    import torch  # noqa: F401

    import flame_amd as fa
    from oracle import capi as oracle

    ref = vr.Volume(**VOLUME)
    with fa.Regularizer(0) as reg:
        reg.volume_create(fa.VolumeParams(**VOLUME))
        for k in range(4):
            g = synth.make_graph("320x240", seed=40 + k)
            tris = synth.delaunay_triangles_scipy(g["pos"])
            reg.upload_graph(g)
            reg.run(fa.Params(), STEPS)
            dense, _ = reg.interpolate_mesh(tris, H, W)
            reg.volume_integrate_begin(K, cam_world(CENTRES[k]), H, W)  # the resident map
            host = synth.copy_graph(g)
            oracle.run(host, STEPS)
            want_map = oracle.raster_interpolate_mesh(tris, g["pos"], host["x"], H, W)
            vr.assert_same_map(dense, want_map, "frame %d: the dense map" % k)
            want = ref.integrate(want_map, K, cam_world(CENTRES[k]))
            got = reg.volume_integrate_end()
            print("frame %d:" % k, got["counts"].tolist(), "device_ms %.3f" % got["device_ms"])
            vr.assert_same_counts(got, want, vr.INTEGRATE_COUNTERS, "frame %d" % k)
            vr.assert_same_volume(reg.volume_download(), ref, "frame %d" % k)
            assert want["updated"] > 5000 and want["behind"] > 0 and (want["saturated"] > 0) == (k == 3)
        # the fifth pose: the volume's view and the last mesh's view, compared on the device
        rc = dict(z_near=0.4, dz=0.03, n_steps=48)
        reg.volume_raycast_begin(KINV, world_cam(CENTRES[4]), H, W, fa.RaycastParams(copy_out=False, **rc))
        t = (np.asarray(CENTRES[3], np.float64) - np.asarray(CENTRES[4], np.float64)).astype(F)
        reg.render_view_begin(fa.ViewParams(Kinv_src=KINV, K_dst=K, t=t, copy_out=False, want_tri_index=False), H, W)
        ray, view = reg.volume_raycast_end(), reg.render_view_end()
        assert "map" not in ray and "map" not in view
        reg.map_error_begin(fa.MapErrorParams(source=fa.MAP_ERROR_TRUTH, map_device=view["device"]["map"], truth_device=ray["device"]["map"],
                                              relative=True, win_size=1), H, W)
        err = reg.map_error_end()
        want_ray = ref.raycast(KINV, world_cam(CENTRES[4]), H, W, **rc)
        vr.assert_same_counts(ray, want_ray, vr.RAYCAST_COUNTERS, "the raycast")
        vr.assert_same_map(fetch(ray["device"]["map"], (H, W), F), want_ray["map"], "the raycast")
        want_view = viewref.render_view(tris, g["pos"], host["x"], KINV, K, np.eye(3, dtype=F), t, H, W)
        vr.assert_same_map(fetch(view["device"]["map"], (H, W), F), want_view["map"], "the last mesh in the fifth camera")
        er.assert_same(err, er.map_error(want_view["map"], er.TRUTH, truth=want_ray["map"], relative=True, win_size=1), "the mesh against the volume")
        print("raycast:", ray["counts"].tolist(), "device_ms %.3f; against the mesh: n_valid %d median_bin %d" % (ray["device_ms"], err["n_valid"], err["median_bin"]))
        assert want_ray["hits"] > 20000 and err["n_valid"] > 10000
