"""DeviceGraph::volumeMeshBegin / volumeMeshEnd (include/flame_hip/nltgv2_l1_graph_regularizer.hpp): the program
tests/cpp/volume_mesh_test.cc compiles as C++11 against include/ and, on a GPU, reproduces byte for byte what the Python mirror
obtained for the same volume and box (dumped to a temporary file)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import volume_mesh_ref as mr
from tests import volume_ref as vr
from tests.conftest import HAS_GPU, ROOT

F = np.float32


def build_program(tmp_path):
    exe = str(tmp_path / "volume_mesh_test")
    lib_dir = os.path.join(ROOT, "flame_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "volume_mesh_test.cc"), "-o", exe, "-L", lib_dir, "-lflame_nltgv2_hip",
        f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_volume_mesh_facade_compiles_and_fails_loudly_without_a_device(built, tmp_path):
    exe = build_program(tmp_path)
    if not HAS_GPU:
        r = subprocess.run([exe, "/dev/null"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no usable HIP device" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_volume_mesh_facade_round_trip(built, tmp_path):
    import torch  # noqa: F401

    import flame_amd

    assert hasattr(flame_amd.load_library(), "flame_nltgv2_volume_mesh_begin")
    vol = dict(nx=20, ny=9, nz=11, voxel_size=0.1, origin=(-1.0, -0.4, 1.0), trunc=0.4, max_weight=2.5)
    lo, hi = (1, 0, 2), (20, 9, 10)
    tsdf, weight = mr.random_signs(vol["nx"], vol["ny"], vol["nz"], 31, 40)
    ref = vr.Volume(**vol)
    ref.tsdf, ref.weight = tsdf, weight
    want = mr.extract(ref, lo, hi)
    with flame_amd.Regularizer(0) as reg:
        reg.volume_create(flame_amd.VolumeParams(**vol))
        reg.volume_upload(tsdf, weight)
        got = reg.volume_mesh(lo=lo, hi=hi)
    mr.assert_same_mesh(got, want, "the Python mirror")
    assert got["n_triangles"] > 100
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(b"VMS1" + struct.pack("<9i", vol["nx"], vol["ny"], vol["nz"], *lo, *hi))
        par = np.array([vol["voxel_size"], *vol["origin"], vol["trunc"], vol["max_weight"]], F)
        for a, t in ((got["counts"], "<i4"), (par, "<f4"), (tsdf, "<f4"), (weight, "<f4"), (got["vertices"], "<f4"), (got["normals"], "<f4"),
                     (got["triangles"], "<i4")):
            f.write(np.ascontiguousarray(a, t).tobytes())
    r = subprocess.run([build_program(tmp_path), path], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count(": ok") == 5 and "FAIL" not in r.stdout, r.stdout + r.stderr
