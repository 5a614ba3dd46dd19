"""The checker of the raw-frame input stage (tests/input_ref.py), anchored without a device and independently of the kernel:
the grey formula, a case whose map is exact in float32, the float32 map against a float64 evaluation of the same formula, and
the sizes of the two new structs against the ctypes mirror."""
import os
import subprocess

import numpy as np
import pytest

from tests import input_ref as ir
from tests import raw_frame_cases as rc
from tests.conftest import ROOT


def test_grey_formula():
    v = np.arange(256)
    assert 4899 + 9617 + 1868 == 16384
    assert (ir.grey_of(v, v, v) == v).all()
    assert [int(ir.grey_of(*c)) for c in ((255, 0, 0), (0, 255, 0), (0, 0, 255))] == [76, 150, 29]
    # the byte order of every format: the same pixel (R, G, B) = (200, 100, 50) written five ways
    want = int(ir.grey_of(200, 100, 50))
    for fmt, px in ((ir.BGR8, [50, 100, 200]), (ir.RGB8, [200, 100, 50]), (ir.BGRA8, [50, 100, 200, 7]),
                    (ir.RGBA8, [200, 100, 50, 7]), (ir.GREY8, [want])):
        raw = np.array([px * 2, px * 2], np.uint8)
        assert (ir.grey_plane(raw, fmt, 2) == want).all(), fmt


def test_exact_shifted_crop():
    """Power-of-two focal lengths, no distortion: every product and quotient of the map is exact, every xs and ys an integer,
    every weight 1 or 0 -- the rectified image is a crop of the raw one, byte for byte."""
    w, h, K, Kinv, p = rc.setup(rc.EXACT_SHIFT)
    assert (w, h, p["raw_width"], p["raw_height"]) == (61, 37, 67, 41)
    xs, ys, inside = ir.source_map(p["K_raw"], p["dist"], Kinv, w, h, 67, 41)
    assert (xs == np.arange(61, dtype=np.float32)[None, :] + 3).all() and (ys == np.arange(37, dtype=np.float32)[:, None] + 2).all()
    raw = rc.raw_bytes(67, 41, ir.GREY8)
    got, n_outside = ir.rectify(raw, ir.GREY8, p, K, Kinv, w, h)
    assert n_outside == 0 and got.tobytes() == raw[2:39, 3:64].tobytes()


@pytest.mark.parametrize("case", sorted(rc.CASES))
def test_float32_map_against_float64(case):
    """Both evaluations of the header's formula agree on `inside` everywhere and differ by less than 1e-3 px wherever both are
    inside: 1e-3 is about 9x the largest difference measured (1.1e-4 px at 752x480 -> 640x480, two ulp of a coordinate near
    512) and 500x below what a wrong coefficient order produces.  The counts are the ones worked out with the cases."""
    w, h, K, Kinv, p = rc.setup(case)
    args = (p["K_raw"], p["dist"], Kinv, w, h, p["raw_width"], p["raw_height"])
    xs, ys, inside = ir.source_map(*args)
    xd, yd, inside64 = ir.source_map(*args, dtype=np.float64)
    assert xs.dtype == np.float32 and xd.dtype == np.float64
    assert (inside == inside64).all()
    want_inside = rc.CASES[case][5]
    assert int(inside.sum()) == (w * h if want_inside is None else want_inside)
    diff = max(np.abs(xs[inside] - xd[inside]).max(), np.abs(ys[inside] - yd[inside]).max())
    print("%s: largest difference %.2e px" % (case, diff))
    assert diff < 1e-3


def test_the_edge_cases_are_what_they_claim():
    """denominator_zero: four pixels divide by exactly 0; overflow: one pixel inside (the principal point), 1132 non-finite."""
    w, h, K, Kinv, p = rc.setup("denominator_zero")
    xs, ys, inside = ir.source_map(p["K_raw"], p["dist"], Kinv, w, h, p["raw_width"], p["raw_height"])
    bad = ~np.isfinite(xs) | ~np.isfinite(ys)
    assert int(bad.sum()) == 4 and not inside[bad].any()
    w, h, K, Kinv, p = rc.setup("overflow")
    xs, ys, inside = ir.source_map(p["K_raw"], p["dist"], Kinv, w, h, p["raw_width"], p["raw_height"])
    bad = ~np.isfinite(xs) | ~np.isfinite(ys)
    assert int(bad.sum()) == 1132 and int(inside.sum()) == 1 and inside[18, 30]
    # an outside pixel is 0 whatever the raw frame holds
    raw, (grey, n_outside) = rc.expected("overflow")
    assert n_outside == 2256 and int((grey != 0).sum()) <= 1


def test_input_params_under_the_sanitizers(tmp_path):
    """tests/cpp/input_params_test.cc: a stand-alone program over the pure host part (flame_amd/csrc/input_params.hpp), compiled
    with AddressSanitizer and UndefinedBehaviorSanitizer and run directly.  Nothing is loaded into Python."""
    exe = str(tmp_path / "input_params_test")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "flame_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "input_params_test.cc"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "240 frames and 12 grids walked, 0 violations" in r.stdout, r.stdout + r.stderr


def test_struct_sizes_match_the_ctypes_mirror(built, tmp_path):
    import ctypes as C

    from flame_amd.stereo import InputParams, _InputStats

    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "flame_stereo.h"\nint main(void){printf("%d %d %d\\n", '
                   '(int)sizeof(flame_stereo_input_params), (int)sizeof(flame_stereo_input_stats), FLAME_STEREO_FMT_RGBA8);'
                   ' return 0;}\n')
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe])
    sizes = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert sizes == [C.sizeof(InputParams), C.sizeof(_InputStats), 4] and sizes[0] == 84
    p = InputParams()
    assert (p.format, p.remap, p.raw_width, p.raw_height) == (0, 0, 0, 0)
    assert list(p.K_raw) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(p.dist) == [0] * 8
