"""FeatureTracker::buildPyramid / alignLinearize / alignFrame (include/flame_hip/feature_tracker.hpp): the program
tests/cpp/align_test.cc compiles as C++11 against include/ and, on a GPU, dumps what the facade returns for the one-chunk linearisation
and for the driver's scene of tests/test_gpu_align.py; the dump must hold the same bytes as the Python mirror's results on the same
cases."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import align_cases as ac
from tests.conftest import HAS_GPU, ROOT

CAM_BORDER = 3


def build_program(tmp_path):
    exe = str(tmp_path / "align_test")
    lib_dir = os.path.join(ROOT, "flame_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "align_test.cc"), "-o", exe, "-L", lib_dir, "-lflame_nltgv2_hip",
        "-L/opt/rocm/lib", "-lamdhip64", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def cases():
    """(w, h, K, kind, n_levels, level, params dict, q, t, ref, new, map): case 2 and case 6 of tests/test_gpu_align.py."""
    from tests.test_gpu_align import IDENT, _scene

    ref, new, d = _scene(33, 17, 5)
    q, t = ac.small_pose()
    one = (33, 17, (32.0, 32.0, 16.0, 8.0), 0, 1, 0, dict(border=1, huber_k=10.0), q, t, ref, new, d)
    ref, new, d, _, _ = ac.driver_scene()
    drv = (ac.DRIVER_W, ac.DRIVER_H, ac.DRIVER_K, 1, 3, 0, ac.DRIVER_PARAMS, IDENT[0], IDENT[1], ref, new, d)
    return [one, drv]


def write_fixture(path):
    from flame_amd.stereo import AlignParams

    cs = cases()
    with open(path, "wb") as f:
        np.int32([len(cs)]).tofile(f)
        for w, h, K, kind, n_levels, level, pk, q, t, ref, new, d in cs:
            Km, Ki = ac.K_matrices(K)
            np.int32([w, h, CAM_BORDER, kind, n_levels, level]).tofile(f)
            Km.tofile(f)
            Ki.tofile(f)
            f.write(bytes(AlignParams(**pk)))
            np.asarray(q, np.float64).tofile(f)
            np.asarray(t, np.float64).tofile(f)
            for a in (ref, new, d):
                np.ascontiguousarray(a).tofile(f)


def test_align_facade_compiles_and_fails_loudly_without_a_device(built, tmp_path):
    exe = build_program(tmp_path)
    if not HAS_GPU:
        write_fixture(str(tmp_path / "fixture.bin"))
        r = subprocess.run([exe, str(tmp_path / "fixture.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no usable HIP device" in r.stdout, r.stdout + r.stderr


def _same_system(s, got, what):
    assert np.array(list(s.H) + list(s.b) + [s.cost], np.float64).tobytes() == got["sums"].tobytes(), what
    from flame_amd.stereo import ALIGN_COUNTS

    assert all(int(getattr(s, n)) == got[n] for n in ALIGN_COUNTS), what


@pytest.mark.gpu
def test_align_facade_gives_the_bytes_of_the_python_mirror(built, tmp_path):
    from flame_amd.stereo import AlignParams, FeatureTracker, _AlignResult, _AlignSystem, _AlignTrace

    write_fixture(str(tmp_path / "fixture.bin"))
    r = subprocess.run([build_program(tmp_path), str(tmp_path / "fixture.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "align facade: ran" in r.stdout and "FAIL" not in r.stdout, r.stdout + r.stderr
    blob = open(str(tmp_path / "out.bin"), "rb").read()
    pos = 0
    for w, h, K, kind, n_levels, level, pk, q, t, ref, new, d in cases():
        Km, Ki = ac.K_matrices(K)
        with FeatureTracker(Km, Ki, w, h, border=CAM_BORDER) as tr:
            tr.add_frame(1, ref)
            tr.add_frame(2, new)
            tr.build_pyramid(1, n_levels)
            tr.build_pyramid(2, n_levels)
            if kind == 0:
                got = tr.align_linearize(AlignParams(**pk), 1, 2, level, d, q, t)
                s = _AlignSystem.from_buffer_copy(blob, pos)
                pos += C.sizeof(_AlignSystem)
                assert got["n_used"] > 300
                _same_system(s, got, "the linearisation")
                continue
            got = tr.align_frame(AlignParams(**pk), 1, 2, d, q, t, max_trace=64)
        res = _AlignResult.from_buffer_copy(blob, pos)
        pos += C.sizeof(_AlignResult)
        n = int(np.frombuffer(blob, np.int32, 1, pos)[0])
        pos += 4
        assert n == got["n_evals"] == len(got["trace"]) >= 6
        assert (res.status, res.flags, res.n_evals, list(res.iters)) == (got["status"], got["flags"], got["n_evals"], got["iters"])
        for name in ("q", "t", "q_f32", "t_f32", "R_f32"):
            assert bytes(getattr(res, name)) == got[name].tobytes(), name
        assert np.float64(res.first_mean_cost).tobytes() == np.float64(got["first_mean_cost"]).tobytes()
        assert np.float64(res.last_mean_cost).tobytes() == np.float64(got["last_mean_cost"]).tobytes()
        for k in range(n):
            e = _AlignTrace.from_buffer_copy(blob, pos)
            pos += C.sizeof(_AlignTrace)
            g = got["trace"][k]
            assert (e.level, e.accepted) == (g["level"], g["accepted"]), k
            assert bytes(e.q) == g["q"].tobytes() and bytes(e.t) == g["t"].tobytes() and bytes(e.delta) == g["delta"].tobytes(), k
            _same_system(e.sys, g, "evaluation %d" % k)
    assert pos == len(blob)
