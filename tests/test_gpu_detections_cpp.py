"""FeatureTracker::drawDetections / getDebugImageDetections (include/flame_hip/feature_tracker.hpp): the program
tests/cpp/detections_test.cc compiles as C++11 against include/ and, on a GPU, draws nothing with debug_draw_detections off and
reproduces byte for byte what flame_stereo_draw_detections gives for the same 160x96 case with it on."""
import os
import subprocess

import pytest

from tests.conftest import HAS_GPU, ROOT


def build_program(tmp_path):
    exe = str(tmp_path / "detections_test")
    lib_dir = os.path.join(ROOT, "flame_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "detections_test.cc"), "-o", exe, "-L", lib_dir, "-lflame_nltgv2_hip",
        f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_detections_facade_compiles_and_fails_loudly_without_a_device(built, tmp_path):
    exe = build_program(tmp_path)
    if not HAS_GPU:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no usable HIP device" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_detections_facade_round_trip(built, tmp_path):
    r = subprocess.run([build_program(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count(": ok") == 4 and "FAIL" not in r.stdout, r.stdout + r.stderr
