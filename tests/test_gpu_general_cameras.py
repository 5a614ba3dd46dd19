"""Every stage that takes a camera matrix or a pose, on the device, with the general matrices of tests/test_general_cameras_ref.py: bit for
bit against the float32 checkers, which that file shows to depend on every entry the stage reads.  A kernel, a host-side copy or a
binding that drops an entry or takes it from another index fails here and nowhere among the pinhole cases.  Each stage on the smallest
shape its own tests use; and one general Kinv handed over as a non-contiguous view and as float64."""
import numpy as np
import pytest

from oracle import stereo_capi as so
from tests import fuse_ref as fr
from tests import input_ref as ir
from tests import mesh_ref as mr
from tests import metric_ref as xr
from tests import test_general_cameras_ref as cpu
from tests import test_gpu_fuse_views as tf
from tests import test_gpu_render_view as tg
from tests import test_mesh_outputs as tm
from tests import view_ref as vr
from tests.metric_helpers import on_device

F = np.float32
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(built):
    import torch  # noqa: F401

    import flame_amd

    return flame_amd


@pytest.fixture(scope="module")
def reg(gpu):
    with gpu.Regularizer(0) as r:
        yield r


# ---- metric outputs ------------------------------------------------------------------------------------------------------------------------
def test_gpu_metric_points_general_kinv_and_pose(gpu, reg):
    v = cpu.metric_map()
    rows, cols = v.shape
    d = on_device(v.copy())  # (the shared map is read-only)
    finite = int(np.isfinite(v).sum())
    reg.upload_graph(cpu.mesh_scene()[0])
    for lo, hi in cpu.METRIC_WINDOWS:
        for pose in (cpu.METRIC_POSE, None):
            what = "general Kinv, pose=%s, window (%s, %s)" % (pose is not None, lo, hi)
            got = reg.metric_outputs(cpu.METRIC_KINV, rows, cols, pose=pose, params=gpu.MetricParams(min_depth=lo, max_depth=hi, map_device=d.data_ptr()))
            xr.assert_same(got, xr.metric_points(v, cpu.METRIC_KINV, pose, lo, hi), xr.POINT_KEYS, what)
            assert 0 < got["n_points"] <= finite and (got["n_points"] < finite or hi == cpu.INF), what
    # the paths around the kernel: the same matrices as views that are not contiguous, and as float64
    first = reg.metric_outputs(cpu.METRIC_KINV, rows, cols, pose=cpu.METRIC_POSE, params=gpu.MetricParams(min_depth=0.5, max_depth=3.0, map_device=d.data_ptr()))
    assert 0 < first["n_points"] < finite
    strided_k, strided_p = cpu.METRIC_KINV.T.copy().T, cpu.METRIC_POSE.T.copy().T
    assert not strided_k.flags["C_CONTIGUOUS"] and not strided_p.flags["C_CONTIGUOUS"]
    for Kinv, pose, what in ((strided_k, strided_p, "non-contiguous views"), (cpu.METRIC_KINV.astype(np.float64), cpu.METRIC_POSE.astype(np.float64), "float64")):
        got = reg.metric_outputs(Kinv, rows, cols, pose=pose, params=gpu.MetricParams(min_depth=0.5, max_depth=3.0, map_device=d.data_ptr()))
        xr.assert_same(got, first, xr.POINT_KEYS, what)


def test_gpu_mesh_outputs_and_metric_mesh_general_kinv_and_pose(gpu, reg):
    g, tris = cpu.mesh_scene()
    Kinv, pose, scale = cpu.MESH_KINV, cpu.MESH_POSE, cpu.MESH_SCALE
    reg.upload_graph(g)
    # the mesh outputs with the default filters: validity, normals and the filtered map
    mo, ref = tm.check_outputs(gpu, reg, g["pos"], tris, Kinv, 240, 320, scale, what="general Kinv")
    assert 0 < mo["n_valid"] < len(tris)
    t = mr.filter_tests(g["pos"], ref["vtx_idepth"], tris, Kinv, 320)
    assert t["angle"].any() and not t["angle"].all() and t["edge"].any() and not t["edge"].all()
    for K in (Kinv.T.copy().T, Kinv.astype(np.float64)):
        again = reg.mesh_outputs(tris, K, 240, 320, graph_scale=scale, want_filtered_map=True)
        for k in ("tri_valid", "normals", "filtered_map"):
            assert again[k].tobytes() == mo[k].tobytes(), k
    # the metric mesh: vertices posed, normals rotated by R only
    reg.interpolate_mesh_begin(tris, 240, 320, graph_scale=scale)
    reg.mesh_outputs_begin(None, Kinv, 240, 320, graph_scale=scale, want_filtered_map=True)
    reg.metric_outputs_begin(Kinv, 240, 320, pose=pose, params=gpu.MetricParams(want_mesh=True, use_filtered_map=True))
    reg.interpolate_mesh_end()
    mo = reg.mesh_outputs_end()
    got = reg.metric_outputs_end()
    x = reg.download_state(("x",))["x"]
    want = xr.metric_points(mo["filtered_map"], Kinv, pose)
    want.update(xr.metric_mesh(g["pos"], x, scale, Kinv, mo["normals"], tris, mo["tri_valid"], pose))
    xr.assert_same(got, want, xr.POINT_KEYS + xr.MESH_KEYS, "general Kinv and pose, mesh")
    assert 0 < got["n_valid"] < len(tris) and got["n_points"] > 1000
    unposed = xr.metric_mesh(g["pos"], x, scale, Kinv, mo["normals"], tris, mo["tri_valid"], None)
    seen = np.unique(tris)
    assert (xr.bits(got["mesh_normals"])[seen] != xr.bits(unposed["mesh_normals"])[seen]).any(axis=1).mean() > 0.9  # (the pose does turn them)


# ---- the view renderer and the fusion --------------------------------------------------------------------------------------------------------
def test_gpu_render_view_general_cameras_and_pose(gpu, reg):
    c = cpu.general_view()
    got, want = tg.both_forms(gpu, reg, c, "general cameras")
    assert got["tris_drawn"] > 0 and got["tris_culled_facing"] > 0 and got["coverage"] > 1000
    # non-contiguous and float64 matrices through ViewParams
    other = dict(c, Kinv_src=c["Kinv_src"].T.copy().T, K_dst=c["K_dst"].reshape(3, 3).T.copy().T, R=c["R"].astype(np.float64), t=c["t"].astype(np.float64))
    again = reg.render_view(tg.view_params(gpu, other), c["rows"], c["cols"])
    vr.assert_same(again, want, "non-contiguous and float64 matrices")


def test_gpu_fuse_views_four_general_sources(gpu, reg):
    sources = cpu.fuse_scene()
    got, want = tf.fuse_kept(gpu, reg, sources, *cpu.VIEW_SRC, min_support=2, rel_tol=cpu.FUSE_REL_TOL, K_dst=cpu.FUSE_K_DST, what="four general sources")
    for s, r in enumerate(want["renders"]):
        assert (vr.bits(got["layers"][s]) == vr.bits(r["map"])).all() and got["present"][s] == r["coverage"] > 0 and r["tris_drawn"] > 0
    assert got["coverage"] == want["coverage"] > 1500


# ---- the raw-frame input stage ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,pad", cpu.INPUT_FORMATS)
def test_gpu_add_raw_frame_general_working_camera_and_skewed_raw_camera(built, fmt, pad):
    from flame_amd.stereo import FeatureTracker
    from tests.test_feature_frontend import PAD

    w, h, K, Kinv, p = cpu.input_case()
    raw, (grey, n_outside) = cpu.input_expected(fmt, pad)
    assert raw.strides[0] == p["raw_width"] * ir.BYTES[fmt] + pad and 0 < n_outside < w * h
    want = so.make_frame(grey, PAD)
    planes = []
    for Kin, Kr in ((Kinv, p["K_raw"]), (Kinv.T.copy().T, p["K_raw"].astype(np.float64))):
        with FeatureTracker(K, Kin, w, h, border=PAD) as tr:
            tr.set_input(format=fmt, **dict(p, K_raw=Kr))
            assert tr.add_raw_frame(10, raw) == dict(n_outside=n_outside)
            got = tr.download_frame(10)
            for name, a, b in zip(("img_pad", "gradx_pad", "grady_pad"), got, want):
                assert a.tobytes() == b.tobytes(), "format %d: %s differs at %d places" % (fmt, name, int((a != b).sum()))
            planes.append(got)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*planes))


# ---- the selection of the graph's vertices ------------------------------------------------------------------------------------------------------
def test_gpu_select_graph_features_general_kinv_and_poses(built):
    from flame_amd.stereo import FeatureTracker
    from tests import select_ref as sr
    from tests import test_select_graph_features as ts

    c = cpu.select_case()
    sc = c["sc"]
    taken = failed_height = 0
    for Kinv in (c["Kinv"], c["Kinv"].T.copy().T, c["Kinv"].astype(np.float64)):
        with FeatureTracker(c["K64"].astype(F), Kinv, sc.width, sc.height, border=ts.PAD) as tr:
            for gp, scale in ((dict(), 1.0), (dict(min_height=-0.5, max_height=1.5, adaptive_data_weights=1), 0.37)):
                rc_c, ref = sr.select(c["feats"], c["proj"], c["Kinv"], c["world"], scale, gp)
                rc, got = ts._gpu_select(tr, c["world"], gp, scale, c["feats"], c["proj"])
                assert rc == rc_c == 0
                ts.assert_same_result(got, ref, "general Kinv and poses, %r scale %g" % (gp, scale))
                taken, failed_height = taken + got["V"], failed_height + got["num_fail_height"]
    assert taken > 0 and failed_height > 0
