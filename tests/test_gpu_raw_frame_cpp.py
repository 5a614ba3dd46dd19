"""FeatureTracker::setInput / addRawFrame (include/flame_hip/feature_tracker.hpp): the program tests/cpp/raw_frame_test.cc
compiles as C++11 against include/ and, on a GPU, reproduces byte for byte the frames the checker expects for the exact-shift
case and the pincushion case (BGR8, padded odd stride), from host and from device memory, and throws without setInput."""
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import HAS_GPU, ROOT


def build_program(tmp_path):
    exe = str(tmp_path / "raw_frame_test")
    lib_dir = os.path.join(ROOT, "flame_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "raw_frame_test.cc"), "-o", exe, "-L", lib_dir, "-lflame_nltgv2_hip",
        "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def write_fixture(path, general=False):
    from oracle import stereo_capi as so
    from tests import input_ref as ir
    from tests import raw_frame_cases as rc
    from tests.test_feature_frontend import PAD

    cases = [(rc.EXACT_SHIFT, ir.GREY8, 0), ("pincushion", ir.BGR8, 5)]
    if general:  # a working camera whose K and Kinv are no pinhole's and a raw camera with a skew (tests/test_general_cameras_ref.py)
        from tests import test_general_cameras_ref as general_cases

        cases = [("general", ir.BGR8, 5)]
    with open(path, "wb") as f:
        np.int32([len(cases)]).tofile(f)
        for case, fmt, pad in cases:
            w, h, K, Kinv, p = general_cases.input_case() if general else rc.setup(case)
            raw = rc.raw_bytes(p["raw_width"], p["raw_height"], fmt, pad)
            grey, n_outside = ir.rectify(raw, fmt, p, K, Kinv, w, h)
            if case is rc.EXACT_SHIFT:
                assert n_outside == 0 and grey.tobytes() == raw[2:39, 3:64].tobytes()
            np.int32([w, h, PAD, p["raw_width"], p["raw_height"], fmt, raw.strides[0], n_outside]).tofile(f)
            for a in (K, Kinv, p["K_raw"], p["dist"]):
                np.ascontiguousarray(a, np.float32).tofile(f)
            raw.tofile(f)
            for plane in so.make_frame(grey, PAD):
                plane.tofile(f)


def test_raw_frame_facade_compiles_and_fails_loudly_without_a_device(built, tmp_path):
    exe = build_program(tmp_path)
    if not HAS_GPU:
        write_fixture(str(tmp_path / "fixture.bin"))
        r = subprocess.run([exe, str(tmp_path / "fixture.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no usable HIP device" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_raw_frame_facade_round_trip(built, tmp_path):
    write_fixture(str(tmp_path / "fixture.bin"))
    r = subprocess.run([build_program(tmp_path), str(tmp_path / "fixture.bin")], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count(": ok") == 3 and "FAIL" not in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_raw_frame_facade_round_trip_with_a_general_camera(built, tmp_path):
    """The constructor copies K(r, c) and Kinv(r, c) element by element: with matrices that differ from their transposes, and with K_raw[1]
    set, the frame is still the checker's."""
    write_fixture(str(tmp_path / "general.bin"), general=True)
    r = subprocess.run([build_program(tmp_path), str(tmp_path / "general.bin")], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count(": ok") == 2 and "FAIL" not in r.stdout, r.stdout + r.stderr
