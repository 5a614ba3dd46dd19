"""DeviceGraph::metricOutputsBegin / End (include/flame_hip/nltgv2_l1_graph_regularizer.hpp): the program
tests/cpp/metric_outputs_test.cc compiles as C++11 against include/ and, on a GPU, reproduces byte for byte the outputs the Python
mirror obtained for the same graph, triangles, pose and depth window (dumped to a temporary file)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from flame_amd import synth
from tests.conftest import HAS_GPU, ROOT
from tests.metric_helpers import POSE, kinv_for

ROWS, COLS, SCALE = 240, 320, 1.25


def build_program(tmp_path):
    exe = str(tmp_path / "metric_outputs_test")
    lib_dir = os.path.join(ROOT, "flame_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "metric_outputs_test.cc"), "-o", exe, "-L", lib_dir, "-lflame_nltgv2_hip",
        f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_metric_outputs_facade_compiles_and_fails_loudly_without_a_device(built, tmp_path):
    exe = build_program(tmp_path)
    if not HAS_GPU:
        r = subprocess.run([exe, "/dev/null"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no usable HIP device" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("use_filtered,posed", [(0, 1), (1, 0)])
def test_metric_outputs_facade_round_trip(built, tmp_path, use_filtered, posed):
    import torch  # noqa: F401

    import flame_amd

    g = synth.make_graph("320x240", seed=9)
    tris = synth.delaunay_triangles_scipy(g["pos"])
    Kinv = kinv_for(COLS, ROWS)
    lo, hi = (0.0, float("inf")) if posed else (0.6, 2.5)
    with flame_amd.Regularizer(0) as reg:
        reg.upload_graph(g)
        reg.interpolate_mesh_begin(tris, ROWS, COLS, graph_scale=SCALE)
        reg.mesh_outputs_begin(None, Kinv, ROWS, COLS, graph_scale=SCALE, want_filtered_map=True)
        reg.metric_outputs_begin(Kinv, ROWS, COLS, pose=POSE if posed else None,
                                 params=flame_amd.MetricParams(min_depth=lo, max_depth=hi, use_filtered_map=use_filtered, want_mesh=True))
        reg.interpolate_mesh_end()
        reg.mesh_outputs_end()
        out = reg.metric_outputs_end()
    assert out["n_points"] > 1000 and out["n_valid"] > 10
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(b"MET1" + struct.pack("<9i", g["V"], g["E"], len(tris), ROWS, COLS, use_filtered, posed, out["n_points"], out["n_valid"]))
        f.write(struct.pack("<3f", SCALE, lo, hi))
        for a, t in ((Kinv, "<f4"), (POSE, "<f4"), (g["pos"], "<f4"), (g["x"], "<f4"), (g["src"], "<i4"), (g["dst"], "<i4"),
                     (g["alpha"], "<f4"), (g["beta"], "<f4"), (tris, "<i4"), (out["depth"], "<f4"), (out["depth_mm"], "<u2"),
                     (out["organized"], "<f4"), (out["cloud"], "<f4"), (out["cloud_pixel"], "<u4"), (out["mesh_vertices"], "<f4"),
                     (out["mesh_normals"], "<f4"), (out["mesh_triangles"], "<i4")):
            f.write(np.ascontiguousarray(a, t).tobytes())
    r = subprocess.run([build_program(tmp_path), path], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count(": ok") == 4 and "FAIL" not in r.stdout, r.stdout + r.stderr
