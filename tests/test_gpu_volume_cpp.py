"""DeviceGraph::volumeCreate / volumeIntegrateBegin / End / volumeRaycastBegin / End / ... (include/flame_hip/nltgv2_l1_graph_regularizer.hpp):
the program tests/cpp/volume_test.cc compiles as C++11 against include/ and, on a GPU, reproduces byte for byte what the Python mirror
obtained for the same graph, triangles, volume and cameras (dumped to a temporary file)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import test_fuse_views_ref as fref
from tests import test_gpu_render_view as tg
from tests import test_gpu_volume as tv
from tests import volume_ref as vr
from tests.conftest import HAS_GPU, ROOT

F = np.float32


def build_program(tmp_path):
    exe = str(tmp_path / "volume_test")
    lib_dir = os.path.join(ROOT, "flame_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "volume_test.cc"), "-o", exe, "-L", lib_dir, "-lflame_nltgv2_hip",
        f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_volume_facade_compiles_and_fails_loudly_without_a_device(built, tmp_path):
    exe = build_program(tmp_path)
    if not HAS_GPU:
        r = subprocess.run([exe, "/dev/null"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no usable HIP device" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_volume_facade_round_trip(built, tmp_path):
    import torch  # noqa: F401

    import flame_amd

    mesh = fref.plane_source(2)
    tris = mesh["tris"]
    rows, cols = fref.SRC
    trows, tcols = 37, 53
    vol = dict(nx=24, ny=20, nz=24, voxel_size=0.1, origin=(-1.2, -1.0, 1.0), trunc=0.4, max_weight=2.5)
    K, Kinv = fref.K, tv.target_kinv(trows, tcols)
    poses, weights = [vr.IDENTITY, tv.turned_pose()], [1.0, 2.0]
    T_world_cam = vr.shifted_pose(0.1)
    rc = dict(z_near=0.5, dz=0.05, n_steps=60)
    g = tg.graph_of(mesh["pos"], mesh["idepth"], tris)
    ref = vr.Volume(**vol)
    with flame_amd.Regularizer(0) as reg:
        reg.volume_create(flame_amd.VolumeParams(**vol))
        reg.upload_graph(g)
        dense = reg.interpolate_mesh(tris, rows, cols)[0]
        counts = []
        for T, w in zip(poses, weights):
            got = reg.volume_integrate(K, T, rows, cols, flame_amd.IntegrateParams(weight=w))
            vr.assert_same_counts(got, ref.integrate(dense, K, T, weight=w), vr.INTEGRATE_COUNTERS, "weight %r" % w)
            counts.append(got["counts"])
        down = reg.volume_download()
        vr.assert_same_volume(down, ref, "two integrations")
        out = reg.volume_raycast(Kinv, T_world_cam, trows, tcols, flame_amd.RaycastParams(**rc))
    want = ref.raycast(Kinv, T_world_cam, trows, tcols, **rc)
    vr.assert_same_map(out["map"], want["map"], "the raycast")
    assert want["hits"] > 500 and counts[1][5] > 0  # (hits; saturated on the second call)
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(b"VOL1" + struct.pack("<11i", g["V"], g["E"], len(tris), rows, cols, vol["nx"], vol["ny"], vol["nz"], trows, tcols, rc["n_steps"]))
        par = np.concatenate([np.array([vol["voxel_size"], *vol["origin"], vol["trunc"], vol["max_weight"]], F), np.asarray(K, F).reshape(-1),
                              np.asarray(Kinv, F).reshape(-1), *poses, np.array(weights, F), T_world_cam, np.array([rc["z_near"], rc["dz"]], F)])
        assert par.size == 64
        for a, t in ((par, "<f4"), (g["pos"], "<f4"), (g["x"], "<f4"), (g["src"], "<i4"), (g["dst"], "<i4"), (g["alpha"], "<f4"), (g["beta"], "<f4"),
                     (tris, "<i4"), (np.concatenate(counts), "<i4"), (down["tsdf"], "<f4"), (down["weight"], "<f4"), (out["counts"], "<i4"),
                     (out["map"], "<f4")):
            f.write(np.ascontiguousarray(a, t).tobytes())
    r = subprocess.run([build_program(tmp_path), path], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count(": ok") == 5 and "FAIL" not in r.stdout, r.stdout + r.stderr
