"""The surface extraction beside a running solver: a wall integrated into the scene's volume, then, while a 320x240 graph iterates on
the solver's stream,

    run_async -> volume_mesh_begin (count query) -> volume_mesh_begin (exact) -> sync -> volume_mesh_end

The mesh equals the checker's bit for bit, every vertex lies within one voxel_size of the wall's depth along z, and the solver's state
is bit-identical to a run without the stage and to the CPU checker."""
import numpy as np
import pytest

from flame_amd import synth
from tests import volume_mesh_ref as mr
from tests import volume_ref as vr
from tests.metric_helpers import on_device

F = np.float32
STEPS = 60
WALL_DEPTH = 1.0
STATE = ("x", "w1", "w2", "x_bar", "w1_bar", "w2_bar", "q1", "q2", "q3")


@pytest.mark.gpu
def test_gpu_the_wall_meshed_beside_a_running_solver(built):
    import torch  # noqa: F401

    import flame_amd as fa
    from oracle import capi as oracle

    assert hasattr(fa.load_library(), "flame_nltgv2_volume_mesh_begin")
    g = synth.make_graph("320x240", seed=9)
    host = synth.copy_graph(g)
    oracle.run(host, STEPS)
    with fa.Regularizer(0) as alone:
        alone.upload_graph(g)
        alone.run(fa.Params(), STEPS)
        state_alone = alone.download_state()
    wall = np.full((vr.SCENE_ROWS, vr.SCENE_COLS), 1.0 / WALL_DEPTH, F)
    ref = vr.scene_volume()
    with fa.Regularizer(0) as reg:
        reg.volume_create(fa.VolumeParams(**vr.SCENE))
        keep = on_device(wall)
        for _ in range(2):
            got = reg.volume_integrate(vr.SCENE_K, vr.IDENTITY, *wall.shape, fa.IntegrateParams(map_device=keep.data_ptr()))
            vr.assert_same_counts(got, ref.integrate(wall, vr.SCENE_K, vr.IDENTITY), vr.INTEGRATE_COUNTERS, "the wall")
        vr.assert_same_volume(reg.volume_download(), ref, "the wall, twice")
        want = mr.extract(ref)
        reg.upload_graph(g)
        reg.run_async(fa.Params(), STEPS)
        reg.volume_mesh_begin(fa.VolumeMeshParams(copy_out=False))  # a count query beside the solver ...
        q = reg.volume_mesh_end()
        reg.volume_mesh_begin(fa.VolumeMeshParams(max_vertices=q["n_vertices"], max_triangles=q["n_triangles"]))  # ... and the mesh
        reg.sync()
        mesh = reg.volume_mesh_end()
        state = reg.download_state()
        vr.assert_same_volume(reg.volume_download(), ref, "the volume after the extraction")
    print("the wall:", mesh["counts"].tolist(), "device_ms %.3f" % mesh["device_ms"])
    assert q["overflow"] == 1 and q["n_vertices"] == want["n_vertices"] and q["n_triangles"] == want["n_triangles"]
    mr.assert_same_mesh(mesh, want, "the wall beside the solver")
    assert mesh["n_triangles"] > 100 and mesh["surface_cubes"] > 50
    z = mesh["vertices"][:, 2].astype(np.float64)
    assert np.all(np.abs(z - WALL_DEPTH) <= float(ref.voxel_size)), "a vertex %.4f from the wall" % np.abs(z - WALL_DEPTH).max()
    assert np.all(mesh["normals"][:, 2] < -0.9), "the normals face the camera, where tsdf grows"
    for k in STATE:
        assert np.array_equal(state[k], state_alone[k]), "the solver's %s differs from a run without the stage" % k
        assert np.array_equal(state[k], host[k]), "the solver's %s differs from the CPU checker" % k
