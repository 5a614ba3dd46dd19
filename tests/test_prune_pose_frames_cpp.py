"""FeatureTracker::prunePoseFrames (include/flame_hip/feature_tracker.hpp): the program tests/cpp/prune_pose_frames_test.cc
compiles as C++11 against include/ and, on a GPU, reproduces bit for bit the result the Python mirror obtained for the same
case (dumped to a temporary file) through both reference-shaped calls, is refused when the current pose-frame is not kept,
and erases the dropped entries from the caller's map."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import prune_cases as pc
from tests.conftest import HAS_GPU, ROOT


def build_program(tmp_path):
    exe = str(tmp_path / "prune_pose_frames_test")
    lib_dir = os.path.join(ROOT, "flame_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-invalid-offsetof", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "prune_pose_frames_test.cc"), "-o", exe, "-L", lib_dir, "-lflame_nltgv2_hip",
        f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_prune_facade_compiles_and_fails_loudly_without_a_device(built, tmp_path):
    exe = build_program(tmp_path)
    if not HAS_GPU:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no usable HIP device" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["vga", "vga-letterbox"])
def test_prune_facade_reproduces_the_mirror(built, tmp_path, name):
    import torch  # noqa: F401

    from flame_amd.stereo import FEATURE_DTYPE, FeatureTracker, StereoParams

    case = pc.make(name)
    sc, feats = case["sc"], case["feats"]
    n, first_new, target = feats.shape[0], feats.shape[0] // 3, case["target"]
    dropped = pc.dropped_poses(sc, case["dropped"], target)
    with FeatureTracker(sc.K32, sc.Kinv32, sc.width, sc.height, border=5) as tr:
        tr.set_features(np.ascontiguousarray(feats).view(FEATURE_DTYPE))
        st = tr.prune_pose_frames(StereoParams(do_letterbox=case["letterbox"]), target, case["keep"], dropped, first_new)
        out = tr.get_features()
    assert st["num_moved"] > n // 5 and st["num_removed"] > 0 and st["num_invalidated"] > 0
    # the target pose-frame at the identity, every other pose-frame at its pose relative to the target
    poses = {target: (np.float32([1, 0, 0, 0]), np.float32([0, 0, 0]))}
    for a in pc.PF_IDS:
        if a != target:
            poses[a] = sc.relative(a, target)
    keep_list = [999] + list(case["keep"]) + [case["keep"][0]]  # an id that is not a pose-frame, and a repeated one
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(b"PRN1" + struct.pack("<9i", sc.width, sc.height, n, first_new, len(poses), len(keep_list), target,
                                      case["letterbox"], out.shape[0]))
        f.write(np.ascontiguousarray(sc.K32, "<f4").tobytes() + np.ascontiguousarray(sc.Kinv32, "<f4").tobytes())
        f.write(np.asarray(sorted(poses), "<u4").tobytes())
        for a in sorted(poses):
            f.write(np.asarray(poses[a][0], "<f4").tobytes() + np.asarray(poses[a][1], "<f4").tobytes())
        f.write(np.asarray(keep_list, "<u4").tobytes())
        f.write(np.ascontiguousarray(feats).tobytes() + np.ascontiguousarray(out).tobytes())
        f.write(struct.pack("<7i", *[st[k] for k in ("num_examined", "num_moved", "num_invalidated", "num_removed",
                                                     "num_features", "num_frames_dropped", "error_feature")]))
    r = subprocess.run([build_program(tmp_path), path], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count(": ok") == 3 and "FAIL" not in r.stdout, r.stdout + r.stderr
