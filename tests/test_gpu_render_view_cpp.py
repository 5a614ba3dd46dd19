"""DeviceGraph::renderViewBegin / End (include/flame_hip/nltgv2_l1_graph_regularizer.hpp): the program tests/cpp/render_view_test.cc
compiles as C++11 against include/ and, on a GPU, reproduces byte for byte what the Python mirror obtained for the same graph,
triangles, validity mask and camera (dumped to a temporary file)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import test_gpu_render_view as tg
from tests import test_render_view_ref as cases
from tests import view_ref as vr
from tests.conftest import HAS_GPU, ROOT

F = np.float32


def build_program(tmp_path):
    exe = str(tmp_path / "render_view_test")
    lib_dir = os.path.join(ROOT, "flame_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "render_view_test.cc"), "-o", exe, "-L", lib_dir, "-lflame_nltgv2_hip",
        f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_render_view_facade_compiles_and_fails_loudly_without_a_device(built, tmp_path):
    exe = build_program(tmp_path)
    if not HAS_GPU:
        r = subprocess.run([exe, "/dev/null"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no usable HIP device" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_render_view_facade_round_trip(built, tmp_path):
    rows, cols = 75, 100
    c = tg.mesh_case(21, K_dst=cases.camera(90.0, 50.0, 37.5)[0], R=cases.rotation_y(12.0), t=np.array([-0.4, 0.05, 0.1], F), near_depth=0.25,
                     rows=rows, cols=cols)
    round_trip(tmp_path, c, rows, cols)


@pytest.mark.gpu
def test_render_view_facade_round_trip_with_general_cameras(built, tmp_path):
    """Kinv_src, K_dst and R without a zero (tests/test_general_cameras_ref.py): what ViewParams carries through the facade, entry by entry."""
    from tests import test_general_cameras_ref as general_cases

    c = dict(general_cases.general_view(), near_depth=0.25)
    round_trip(tmp_path, c, c["rows"], c["cols"])


def round_trip(tmp_path, c, rows, cols):
    import torch  # noqa: F401

    import flame_amd

    tris = c["tris"]
    mask = (np.arange(len(tris)) % 4 != 1).astype(np.uint8)
    g = tg.graph_of(c["pos"], c["idepth"], tris)
    with flame_amd.Regularizer(0) as reg:
        reg.upload_graph(g)
        reg.interpolate_mesh(tris, *tg.SRC)
        everything = reg.render_view(tg.view_params(flame_amd, c), rows, cols)
        masked = reg.render_view(tg.view_params(flame_amd, c, validity=1), rows, cols, tri_valid=mask)
    vr.assert_same(everything, cases.render(c), "all valid")
    vr.assert_same(masked, cases.render(c, tri_valid=mask), "masked")
    assert everything["coverage"] > 1000 and masked["coverage"] < everything["coverage"]
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(b"RVW1" + struct.pack("<7i", g["V"], g["E"], len(tris), *tg.SRC, rows, cols))
        camera = np.concatenate([np.asarray(c[k], F).reshape(-1) for k in ("Kinv_src", "K_dst", "R", "t")] + [np.array([c["near_depth"]], F)])
        for a, t in ((camera, "<f4"), (g["pos"], "<f4"), (g["x"], "<f4"), (g["src"], "<i4"), (g["dst"], "<i4"), (g["alpha"], "<f4"), (g["beta"], "<f4"),
                     (tris, "<i4"), (mask, "u1")):
            f.write(np.ascontiguousarray(a, t).tobytes())
        for out in (everything, masked):
            f.write(np.ascontiguousarray(out["map"], "<f4").tobytes())
            f.write(np.ascontiguousarray(out["tri_index"], "<i4").tobytes())
            f.write(struct.pack("<4i", *(out[k] for k in vr.COUNT_KEYS)))
    r = subprocess.run([build_program(tmp_path), path], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count(": ok") == 4 and "FAIL" not in r.stdout, r.stdout + r.stderr
