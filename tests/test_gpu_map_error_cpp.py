"""DeviceGraph::mapErrorBegin / End (include/flame_hip/nltgv2_l1_graph_regularizer.hpp): the program tests/cpp/map_error_test.cc
compiles as C++11 against include/ and, on a GPU, reproduces byte for byte what the Python mirror obtained for the same graph,
triangles, images and true map from both sources (dumped to a temporary file)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from flame_amd import synth
from tests import map_error_ref as er
from tests.conftest import HAS_GPU, ROOT

ROWS, COLS, BORDER, WIN = 240, 320, 4, 5
KRKINV = np.array([[1, 0.01, 1.5], [-0.01, 1, -0.75], [0, 0, 1]], np.float32)
KT = np.array([6.0, 2.0, 0.01], np.float32)


def build_program(tmp_path):
    exe = str(tmp_path / "map_error_test")
    lib_dir = os.path.join(ROOT, "flame_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "map_error_test.cc"), "-o", exe, "-L", lib_dir, "-lflame_nltgv2_hip",
        f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_map_error_facade_compiles_and_fails_loudly_without_a_device(built, tmp_path):
    exe = build_program(tmp_path)
    if not HAS_GPU:
        r = subprocess.run([exe, "/dev/null"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no usable HIP device" in r.stdout, r.stdout + r.stderr


def stats_bytes(flame_amd, out):
    st = flame_amd.MapErrorStats()
    C.memmove(st.hist, out["hist"].ctypes.data, 1024)
    st.n_valid, st.median_bin, st.ptile_bin, st.mean, st.sum = out["n_valid"], out["median_bin"], out["ptile_bin"], float(out["mean"]), out["sum"]
    return bytes(st)


@pytest.mark.gpu
def test_map_error_facade_round_trip(built, tmp_path):
    import torch  # noqa: F401

    import flame_amd

    g = synth.make_graph("320x240", seed=9)
    tris = synth.delaunay_triangles_scipy(g["pos"])
    rng = np.random.default_rng(12)
    ref, cmp = (rng.integers(0, 256, (ROWS, COLS), dtype=np.uint8) for _ in range(2))
    truth = rng.uniform(0.2, 2.0, (ROWS, COLS)).astype(np.float32)
    truth[rng.random((ROWS, COLS)) < 0.1] = 0
    with flame_amd.Regularizer(0) as reg:
        reg.upload_graph(g)
        dense, _ = reg.interpolate_mesh(tris, ROWS, COLS)
        reg.photo_set_images(ref, cmp)
        photo = reg.map_error(flame_amd.MapErrorParams(KRKinv=KRKINV, Kt=KT, border=BORDER, win_size=WIN, want_image=True, max_error=48.0), ROWS, COLS)
        true = reg.map_error(flame_amd.MapErrorParams(source=flame_amd.MAP_ERROR_TRUTH, truth=truth, win_size=WIN, want_image=True, max_error=0.75,
                                                      gray=ref, flip=True), ROWS, COLS)
    er.assert_same(photo, er.map_error(dense, er.PHOTO, KRKINV, KT, ref, cmp, BORDER, win_size=WIN, max_error=48.0, want_image=True), "photo")
    er.assert_same(true, er.map_error(dense, er.TRUTH, truth=truth, win_size=WIN, gray=ref, max_error=0.75, flip=True, want_image=True), "truth")
    assert photo["n_valid"] > 1000 and true["n_valid"] > 1000
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(b"MER1" + struct.pack("<7i", g["V"], g["E"], len(tris), ROWS, COLS, BORDER, WIN) + struct.pack("<2f", 48.0, 0.75))
        for a, t in ((KRKINV, "<f4"), (KT, "<f4"), (g["pos"], "<f4"), (g["x"], "<f4"), (g["src"], "<i4"), (g["dst"], "<i4"), (g["alpha"], "<f4"),
                     (g["beta"], "<f4"), (tris, "<i4"), (ref, "u1"), (cmp, "u1"), (truth, "<f4")):
            f.write(np.ascontiguousarray(a, t).tobytes())
        for out in (photo, true):
            f.write(np.ascontiguousarray(out["error_map"], "<f4").tobytes())
            f.write(stats_bytes(flame_amd, out))
            f.write(np.ascontiguousarray(out["image"], "u1").tobytes())
    r = subprocess.run([build_program(tmp_path), path], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count(": ok") == 4 and "FAIL" not in r.stdout, r.stdout + r.stderr
