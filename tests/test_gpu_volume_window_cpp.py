"""DeviceGraph::volumeFollow / volumeShiftBegin / End / volumeWindow (include/flame_hip/nltgv2_l1_graph_regularizer.hpp): the program
tests/cpp/volume_window_test.cc compiles as C++11 against include/ and, on a GPU, reproduces byte for byte what the Python mirror
obtained for the same volume and camera (dumped to a temporary file)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import volume_mesh_ref as vmr
from tests import volume_ref as vr
from tests import volume_window_ref as wr
from tests.conftest import HAS_GPU, ROOT
from tests.metric_helpers import on_device

F = np.float32


def build_program(tmp_path):
    exe = str(tmp_path / "volume_window_test")
    lib_dir = os.path.join(ROOT, "flame_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "volume_window_test.cc"), "-o", exe, "-L", lib_dir, "-lflame_nltgv2_hip",
        f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_volume_window_facade_compiles_and_fails_loudly_without_a_device(built, tmp_path):
    exe = build_program(tmp_path)
    if not HAS_GPU:
        r = subprocess.run([exe, "/dev/null"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no usable HIP device" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_volume_window_facade_round_trip(built, tmp_path):
    import torch  # noqa: F401

    import flame_amd

    vol = dict(vr.SCENE)
    rows, cols = vr.SCENE_ROWS, vr.SCENE_COLS
    T_world_cam = vr.IDENTITY.copy()
    T_world_cam[3], T_world_cam[7] = 0.35, -0.25
    focus, step = 1.15, 1  # the point followed lies (3.5, -2.5, 1.5) voxels off the middle voxel
    rc = dict(vr.SCENE_RAYCAST)
    ref = wr.Volume(**vol)
    m = vr.scene_map()
    keep = on_device(m)
    with flame_amd.Regularizer(0) as reg:
        reg.volume_create(flame_amd.VolumeParams(**vol))
        reg.volume_integrate(vr.SCENE_K, vr.IDENTITY, rows, cols, flame_amd.IntegrateParams(map_device=keep.data_ptr()))
        ref.integrate(m, vr.SCENE_K, vr.IDENTITY)
        before = reg.volume_download()
        vr.assert_same_volume(before, ref, "before")
        plan = reg.volume_follow(T_world_cam, flame_amd.FollowParams(focus_depth=focus, step=step))
        assert plan["shift"].tolist() == wr.follow(ref, T_world_cam, focus_depth=focus, step=step)["shift"] == [3, -2, 1]
        shifted = reg.volume_shift(plan["shift"])
        wr.assert_same_counts(shifted, ref.shift(plan["shift"]), "the shift")
        after = reg.volume_download()
        vr.assert_same_volume(after, ref, "after")
        ray = reg.volume_raycast(vr.SCENE_KINV, T_world_cam, rows, cols, flame_amd.RaycastParams(**rc))
        vr.assert_same_map(ray["map"], ref.raycast(vr.SCENE_KINV, T_world_cam, rows, cols, **rc)["map"], "the raycast")
        mesh = reg.volume_mesh(want_normals=False)
        vmr.assert_same_mesh(mesh, wr.extract(ref, want_normals=False), "the mesh", normals=False)
    assert ray["hits"] > 0 and mesh["n_triangles"] > 0 and shifted["kept_seen"] == 912
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(b"VWN1" + struct.pack("<8i", vol["nx"], vol["ny"], vol["nz"], rows, cols, rc["n_steps"], mesh["n_vertices"], mesh["n_triangles"]))
        par = np.concatenate([np.array([vol["voxel_size"], *vol["origin"], vol["trunc"], vol["max_weight"]], F), vr.SCENE_KINV, T_world_cam,
                              np.array([rc["z_near"], rc["dz"], focus], F)])
        ints = np.concatenate([np.array([step], np.int32), np.frombuffer(bytes(plan["plan"]), np.int32), shifted["counts"], shifted["base"],
                               np.array([shifted["record_bytes"]], np.int32)])
        assert par.size == 30 and ints.size == 45
        for a, t in ((par, "<f4"), (ints, "<i4"), (before["tsdf"], "<f4"), (before["weight"], "<f4"), (after["tsdf"], "<f4"), (after["weight"], "<f4"),
                     (ray["counts"], "<i4"), (ray["map"], "<f4"), (mesh["vertices"], "<f4"), (mesh["triangles"], "<i4")):
            f.write(np.ascontiguousarray(a, t).tobytes())
    r = subprocess.run([build_program(tmp_path), path], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count(": ok") == 5 and "FAIL" not in r.stdout, r.stdout + r.stderr
