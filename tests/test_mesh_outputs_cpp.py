"""DeviceGraph::meshOutputsBegin / End and struct MeshOutputs (include/flame_hip/nltgv2_l1_graph_regularizer.hpp): the program
tests/cpp/mesh_outputs_test.cc compiles as C++11 against include/ and, on a GPU, reproduces bit for bit the outputs the Python
mirror obtained for the same graph (dumped to a temporary file)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from flame_amd import synth
from tests.conftest import HAS_GPU, ROOT


def build_program(tmp_path):
    exe = str(tmp_path / "mesh_outputs_test")
    lib_dir = os.path.join(ROOT, "flame_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "mesh_outputs_test.cc"), "-o", exe, "-L", lib_dir, "-lflame_nltgv2_hip",
        f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_mesh_outputs_facade_compiles_and_fails_loudly_without_a_device(built, tmp_path):
    exe = build_program(tmp_path)
    if not HAS_GPU:
        r = subprocess.run([exe, "/dev/null"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no usable HIP device" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_mesh_outputs_facade_round_trip(built, tmp_path):
    import torch  # noqa: F401

    import flame_amd
    from tests.test_mesh_outputs import kinv_for

    g = synth.make_graph("320x240", seed=12)
    tris = synth.delaunay_triangles_scipy(g["pos"])
    Kinv = kinv_for(320, 240)
    rows, cols, scale = 240, 320, 1.25
    filt = flame_amd.MeshFilterParams(min_triangle_idepth=0.6)
    with flame_amd.Regularizer(0) as reg:
        reg.upload_graph(g)
        out = reg.mesh_outputs(tris, Kinv, rows, cols, graph_scale=scale, filter=filt, want_filtered_map=True)
    assert 0 < out["n_valid"] < len(tris)
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(b"MSH1" + struct.pack("<6i", g["V"], g["E"], len(tris), rows, cols, out["n_valid"]))
        f.write(struct.pack("<fi", scale, out["filtered_coverage"]) + bytes(filt))
        for a, t in ((Kinv, "<f4"), (g["pos"], "<f4"), (g["x"], "<f4"), (g["src"], "<i4"), (g["dst"], "<i4"), (g["alpha"], "<f4"),
                     (g["beta"], "<f4"), (tris, "<i4"), (out["vtx_idepth"], "<f4"), (out["normals"], "<f4"), (out["tri_valid"], "u1"),
                     (out["filtered_map"], "<f4")):
            f.write(np.ascontiguousarray(a, t).tobytes())
    r = subprocess.run([build_program(tmp_path), path], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count(": ok") == 3 and "FAIL" not in r.stdout, r.stdout + r.stderr
