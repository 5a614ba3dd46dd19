"""FeatureTracker::recordMatches / getDebugImageMatches (include/flame_hip/feature_tracker.hpp): the program tests/cpp/matches_test.cc
compiles as C++11 against include/ and, on a GPU, reproduces byte for byte the records, the picture and the counters the sequential
checker tests/matches_ref.py obtained for the same case (dumped to a temporary file)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.conftest import HAS_GPU, ROOT
from tests.test_matches import case, reference, run_checker


def build_program(tmp_path):
    exe = str(tmp_path / "matches_test")
    lib_dir = os.path.join(ROOT, "flame_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "matches_test.cc"), "-o", exe, "-L", lib_dir, "-lflame_nltgv2_hip",
        f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_matches_facade_compiles_and_fails_loudly_without_a_device(built, tmp_path):
    exe = build_program(tmp_path)
    if not HAS_GPU:
        r = subprocess.run([exe, "/dev/null"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no usable HIP device" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name,flip", [("textureless", 0), ("move", 1)])
def test_matches_facade_round_trip(built, tmp_path, name, flip):
    import torch  # noqa: F401

    from flame_amd.stereo import FeatureTracker, StereoParams

    c, ref = case(name), reference(name)
    img = run_checker(c, flip=True)["img"] if flip else ref["img"]
    ids = sorted(c["imgs"])
    poses = FeatureTracker._poses(c["poses"])
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(b"MAT1" + struct.pack("<9i", c["width"], c["height"], c["pad"], len(ids), len(c["poses"]), c["feats"].shape[0],
                                      c["new"], c["curr_pf"], flip))
        f.write(np.ascontiguousarray(c["K"], "<f4").tobytes() + np.ascontiguousarray(c["Kinv"], "<f4").tobytes())
        f.write(bytes(StereoParams(**c["pkw"])))
        f.write(np.asarray(ids, "<u4").tobytes())
        for i in ids:
            f.write(np.ascontiguousarray(c["imgs"][i], np.uint8).tobytes())
        f.write(bytes(poses)[:len(c["poses"]) * C.sizeof(poses._type_)])
        f.write(c["feats"].tobytes() + ref["feats"].tobytes() + np.ascontiguousarray(img).tobytes())
        f.write(np.asarray(ref["kind_count"] + [ref["lines_drawn"], ref["lines_skipped"], ref["rings_skipped"], ref["entries"]],
                           "<i4").tobytes())
    r = subprocess.run([build_program(tmp_path), path], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count(": ok") == 3 and "FAIL" not in r.stdout, r.stdout + r.stderr
