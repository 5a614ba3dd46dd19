"""DeviceGraph::debugImagesBegin / End, FeatureTracker::drawFeatures and ::frameImageDevice (include/flame_hip/): the program
tests/cpp/debug_images_test.cc compiles as C++11 against include/ and, on a GPU, reproduces byte for byte the pictures the Python
mirror obtained for the same graph, image and features (dumped to a temporary file)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.conftest import HAS_GPU, ROOT
from tests.test_debug_images import scene  # noqa: F401  (the scene of the debug image tests, as a fixture)


def build_program(tmp_path):
    exe = str(tmp_path / "debug_images_test")
    lib_dir = os.path.join(ROOT, "flame_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "debug_images_test.cc"), "-o", exe, "-L", lib_dir, "-lflame_nltgv2_hip",
        f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_debug_images_facade_compiles_and_fails_loudly_without_a_device(built, tmp_path):
    exe = build_program(tmp_path)
    if not HAS_GPU:
        r = subprocess.run([exe, "/dev/null"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no usable HIP device" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [0, 1])
def test_debug_images_facade_round_trip(built, tmp_path, scene, flip):
    import torch  # noqa: F401

    import flame_amd
    from flame_amd.stereo import FeatureTracker, StereoParams
    from tests.test_debug_images import COLOR_SCALE, COLS, GRAPH_SCALE, ROWS, feature_set

    s = scene
    g, tris, K = s["g"], s["tris"], s["K"]
    Kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    p = flame_amd.DebugImageParams(scene_color_scale=COLOR_SCALE, flip=flip)
    with flame_amd.Regularizer(0) as reg:
        reg.upload_graph(g)
        reg.interpolate_mesh(tris, ROWS, COLS, graph_scale=GRAPH_SCALE)
        out = reg.debug_images(s["img"], K, ROWS, COLS, p)
    feats = feature_set()
    with FeatureTracker(K, Kinv, COLS, ROWS) as tr:
        tr.add_frame(11, np.ascontiguousarray(s["img"]))
        tr.set_features(feats)
        tr.project_features(StereoParams(do_letterbox=0), 11, [dict(id=10, q_to_new=[1, 0, 0, 0], t_to_new=[0, 0, 0])])
        thr = 0.01
        fimg, nc, nu = tr.draw_features(11, thr, COLOR_SCALE, bool(flip))
    assert nc > 5 and nu > 5
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(b"DBG1" + struct.pack("<10i", g["V"], g["E"], len(tris), ROWS, COLS, s["buf"].shape[1], len(feats), flip, nc, nu))
        f.write(struct.pack("<3f", GRAPH_SCALE, COLOR_SCALE, thr))
        for a, t in ((K, "<f4"), (Kinv, "<f4"), (g["pos"], "<f4"), (g["x"], "<f4"), (g["w1"], "<f4"), (g["w2"], "<f4"), (g["src"], "<i4"),
                     (g["dst"], "<i4"), (g["alpha"], "<f4"), (g["beta"], "<f4"), (tris, "<i4"), (s["buf"], "u1")):
            f.write(np.ascontiguousarray(a, t).tobytes())
        f.write(feats.tobytes())
        for a, t in ((out["idepthmap_img"], "u1"), (out["normals_img"], "u1"), (out["w1_map"], "<f4"), (out["w2_map"], "<f4"), (fimg, "u1")):
            f.write(np.ascontiguousarray(a, t).tobytes())
    r = subprocess.run([build_program(tmp_path), path], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count(": ok") == 4 and "FAIL" not in r.stdout, r.stdout + r.stderr

