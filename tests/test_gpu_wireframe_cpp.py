"""DeviceGraph::debugWireframeBegin / End (include/flame_hip/): the program tests/cpp/wireframe_test.cc compiles as C++11 against
include/ and, on a GPU, reproduces byte for byte the pictures the Python mirror obtained for the same graph, triangles and image
(dumped to a temporary file)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.conftest import HAS_GPU, ROOT
from tests.test_debug_images import scene  # noqa: F401  (the scene of the debug image tests, as a fixture)


def build_program(tmp_path):
    exe = str(tmp_path / "wireframe_test")
    lib_dir = os.path.join(ROOT, "flame_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "wireframe_test.cc"), "-o", exe, "-L", lib_dir, "-lflame_nltgv2_hip",
        f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_wireframe_facade_compiles_and_fails_loudly_without_a_device(built, tmp_path):
    exe = build_program(tmp_path)
    if not HAS_GPU:
        r = subprocess.run([exe, "/dev/null"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no usable HIP device" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [0, 1])
def test_wireframe_facade_round_trip(built, tmp_path, scene, flip):
    import torch  # noqa: F401

    import flame_amd
    from tests.test_debug_images import COLOR_SCALE, COLS, GRAPH_SCALE, ROWS

    s = scene
    g, tris = s["g"], s["tris"]
    third = np.ones(len(tris), np.uint8)
    third[::3] = 0
    with flame_amd.Regularizer(0) as reg:
        reg.upload_graph(g)
        reg.interpolate_mesh(tris, ROWS, COLS, graph_scale=GRAPH_SCALE)
        every = reg.debug_wireframe(s["img"], ROWS, COLS, GRAPH_SCALE, flame_amd.WireframeParams(scene_color_scale=COLOR_SCALE, flip=flip))
        masked = reg.debug_wireframe(s["img"], ROWS, COLS, GRAPH_SCALE,
                                     flame_amd.WireframeParams(scene_color_scale=COLOR_SCALE, flip=flip, validity=1), tri_valid=third)
    assert every["lines_drawn"] == 3 * len(tris) and masked["lines_drawn"] == 3 * int(third.sum())
    assert not np.array_equal(every["wireframe_img"], masked["wireframe_img"])
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(b"WIR1" + struct.pack("<9i", g["V"], g["E"], len(tris), ROWS, COLS, s["buf"].shape[1], flip, every["lines_drawn"],
                                      masked["lines_drawn"]))
        f.write(struct.pack("<2f", GRAPH_SCALE, COLOR_SCALE))
        for a, t in ((g["pos"], "<f4"), (g["x"], "<f4"), (g["src"], "<i4"), (g["dst"], "<i4"), (g["alpha"], "<f4"), (g["beta"], "<f4"),
                     (tris, "<i4"), (s["buf"], "u1"), (third, "u1"), (every["wireframe_img"], "u1"), (masked["wireframe_img"], "u1")):
            f.write(np.ascontiguousarray(a, t).tobytes())
    r = subprocess.run([build_program(tmp_path), path], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count(": ok") == 3 and "FAIL" not in r.stdout, r.stdout + r.stderr
