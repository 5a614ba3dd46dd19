"""The map error (include/flame_nltgv2.h, flame_nltgv2_map_error_begin): known answers for the checker tests/map_error_ref.py, a
property that shows the measurement means something, and the new symbols and structs of the C-ABI.  No GPU here; the device is compared
with the checker in tests/test_gpu_map_error*.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from flame_amd import synth_stereo as ss
from tests import map_error_ref as er
from tests.conftest import ROOT

F = np.float32
NAN, INF = F(np.nan), F(np.inf)
NAMES = ("flame_nltgv2_default_map_error_params", "flame_nltgv2_map_error_begin", "flame_nltgv2_map_error_end", "flame_nltgv2_map_error")


@pytest.fixture(scope="module", autouse=True)
def stage(built):
    """The checker describes a stage of the library: without its entry points there is nothing these tests speak of."""
    import flame_amd

    lib = flame_amd.load_library()
    for n in NAMES:
        assert hasattr(lib, n), n
    return lib


def random_errors(shape, seed, p_nan=0.4):
    rng = np.random.default_rng(seed)
    e = rng.uniform(0.0, 40.0, shape).astype(F)
    e[rng.random(shape) < p_nan] = NAN
    return e


# ---- self-consistency of the checker ---------------------------------------------------------------------------------------------
def test_window_of_one_is_the_identity():
    e = random_errors((13, 17), 1)
    e[3, 4] = F(-0.0)  # (what |d| leaves for d = +0)
    out, cnt = er.box_mean(e, 1)
    assert np.array_equal(er.bits(out), er.bits(e)) and np.array_equal(cnt, ~np.isnan(e))


@pytest.mark.parametrize("win", [3, 5, 11, 31])
def test_a_constant_error_image_keeps_its_value_under_any_window(win):
    # 6.5 * count is exact for every count up to 31 * 31, so sum / count is 6.5 again -- also at the rim and beside the holes
    e = np.full((37, 29), 6.5, F)
    e[10:14, 5:25] = NAN
    e[0, 0] = e[36, 28] = NAN
    out, cnt = er.box_mean(e, win)
    ok = ~np.isnan(e)
    assert np.array_equal(np.isnan(out), ~ok) and (out[ok] == F(6.5)).all()
    assert cnt.max() <= win * win and cnt[ok].min() >= 1
    if win == 3:
        assert cnt[25, 14] == 9 and cnt[0, 1] == 5 and cnt[9, 14] == 6  # interior; a corner beside a hole; above the band of holes


@pytest.mark.parametrize("win", [1, 3, 11])
def test_a_single_valid_pixel_keeps_its_value_with_count_one(win):
    for at in ((0, 0), (36, 28), (17, 13)):
        e = np.full((37, 29), NAN, F)
        e[at] = F(3.3)
        out, cnt = er.box_mean(e, win)
        assert cnt[at] == 1 and out[at] == F(3.3) and np.isnan(out).sum() == e.size - 1


def test_the_histogram_counts_every_valid_pixel_once():
    e = random_errors((50, 70), 2)
    e[0, :5] = [INF, 0.0, 254.49, 254.5, 1e-40]
    for scale in (1.0, 7.0, 1000.0):
        st = er.statistics(e, scale)
        assert st["hist"].sum() == st["n_valid"] == (~np.isnan(e)).sum()
        assert st["hist"].dtype == np.int32 and st["hist"].shape == (256,)
    st = er.statistics(np.full((4, 4), NAN, F), 1.0)
    assert (st["n_valid"], st["median_bin"], st["ptile_bin"], st["sum"], st["mean"]) == (0, -1, -1, 0.0, 0.0)


def test_the_box_sum_is_taken_in_the_stated_order():
    """A window whose float sum depends on the order: 2^24 + 1 + 1 ... is 2^24 if the ones come one by one after it, more if they come
    first."""
    big = F(2.0 ** 24)
    e = np.zeros((3, 3), F)
    e[0] = [big, 1, 1]      # row sum left to right: (2^24 + 1) + 1 = 2^24
    e[1] = [1, 1, big]      # (1 + 1) + 2^24 = 2^24 + 2
    e[2] = [1, 1, 1]
    out, cnt = er.box_mean(e, 3)
    want = F(F(F(big + F(big + F(2))) + F(3)) / F(9))  # rows top to bottom: (2^24 + (2^24 + 2)) + 3
    assert cnt[1, 1] == 9 and out[1, 1] == want
    assert out[1, 1] != F(np.float64(e.astype(np.float64).sum()) / 9)  # (the exact sum differs: the order shows)


def test_the_sum_is_taken_in_the_stated_order():
    rng = np.random.default_rng(3)
    e = rng.uniform(0, 100, 5000).astype(F)
    e[rng.random(5000) < 0.3] = NAN
    # the definition, spelled out with loops
    terms = [0.0 if np.isnan(v) else float(v) for v in e] + [0.0] * (5 * 1024 - 5000)
    partials = []
    for c in range(5):
        p = terms[c * 1024:(c + 1) * 1024]
        s = 512
        while s >= 1:
            for t in range(s):
                p[t] += p[t + s]
            s //= 2
        partials.append(p[0])
    q = [0.0] * 1024
    for t, b in enumerate(partials):
        q[t] += b
    s = 512
    while s >= 1:
        for t in range(s):
            q[t] += q[t + s]
        s //= 2
    assert er.ordered_sum(e) == q[0]
    assert abs(q[0] - np.nansum(e.astype(np.float64))) < 1e-6 * q[0]
    # more partials than one round of the second level: 1025 blocks
    big = np.ones(1025 * 1024, F)
    assert er.ordered_sum(big) == 1025.0 * 1024.0
    assert er.ordered_sum(np.array([1.0, INF, NAN], F)) == np.inf


# ---- the rank rules on hand-made histograms --------------------------------------------------------------------------------------
def hist_of(**bins):
    h = np.zeros(256, np.int32)
    for k, v in bins.items():
        h[int(k[1:])] = v
    return h


def test_rank_rules():
    assert er.ranks(hist_of(b7=1)) == (1, 7, 7)                       # n = 1
    assert er.ranks(hist_of(b2=2, b9=2)) == (4, 9, 9)                 # a tie exactly at 2 * cum == n: the next occupied bin
    assert er.ranks(hist_of(b2=2, b5=0, b9=2), 50, 100) == (4, 9, 9)  # the percentile rule at the same tie
    assert er.ranks(hist_of(b2=3, b9=2)) == (5, 2, 9)
    assert er.ranks(hist_of(b0=1000)) == (1000, 0, 0)                 # all mass in bin 0
    assert er.ranks(hist_of(b255=17)) == (17, 255, 255)               # all mass in bin 255
    assert er.ranks(hist_of(b3=1, b4=998, b200=1)) == (1000, 4, 4)    # median and percentile in one bin
    assert er.ranks(hist_of(b3=1, b4=990, b200=9)) == (1000, 4, 4)    # 100 * 991 > 99 * 1000: still bin 4
    assert er.ranks(hist_of(b3=1, b4=989, b200=10)) == (1000, 4, 200)  # 100 * 990 == 99 * 1000, a tie: the next occupied bin
    assert er.ranks(hist_of(b1=50, b2=49, b3=1)) == (100, 2, 3)       # 100 * 99 > 99 * 100 is false: the last pixel's bin
    assert er.ranks(hist_of(b1=5), 0, 100) == (5, 1, 1)
    assert er.ranks(hist_of(b1=5, b2=5), 100, 100) == (10, 2, -1)     # no m has den * cum > num * n
    assert er.ranks(np.zeros(256, np.int32)) == (0, -1, -1)
    # 64-bit: counts whose products pass 2^31
    assert er.ranks(hist_of(b10=2_000_000_000, b20=20_202_021), 99, 100) == (2_020_202_021, 10, 20)
    assert er.ranks(hist_of(b10=2_000_000_000, b20=20_202_020), 99, 100) == (2_020_202_020, 10, 10)


# ---- bin edges -------------------------------------------------------------------------------------------------------------------
def test_bin_edges():
    # err * scale exactly k + 0.5: (int)(k + 1.0f) = k + 1 -- halves go up, this is not rintf
    for k in (0, 1, 2, 7, 100, 253):
        assert er.bin_of(F(k + 0.5), 1.0) == k + 1
        # the float below k + 0.5 stays in bin k -- except below 0.5 itself: (0.5 - 2^-25) + 0.5f is a tie between 1 - 2^-24 and 1.0f
        # and rounds to 1.0f, so that float is in bin 1 already.  The rule is (int)(s + 0.5f) as written, with this consequence
        assert er.bin_of(np.nextafter(F(k + 0.5), F(0)), 1.0) == (k if k > 0 else 1)
        assert F((k + 0.5) / 8) * F(8) == F(k + 0.5) and er.bin_of(F((k + 0.5) / 8), 8.0) == k + 1
    assert er.bin_of(F(254.5), 1.0) == 255                       # (int)(255.0f)
    assert er.bin_of(np.nextafter(F(254.5), F(0)), 1.0) == 254
    assert er.bin_of(F(255.0), 1.0) == 255 and er.bin_of(F(1e30), 1.0) == 255 and er.bin_of(F(3e38), 1000.0) == 255
    assert er.bin_of(INF, 1.0) == 255 and er.bin_of(INF, 1000.0) == 255
    assert er.bin_of(F(6e-39), 1.0) == 0 and er.bin_of(F(1e-45), 1000.0) == 0 and er.bin_of(F(-0.0), 1.0) == 0
    assert er.bin_of(F(0.2549), 1000.0) == 255 and er.bin_of(F(0.0125), 1000.0) in (12, 13)
    got = er.bin_of(np.array([0.0, 0.49, 0.5, 1.49, 254.4, 254.6, 300.0], F), 1.0)
    assert got.tolist() == [0, 0, 1, 1, 254, 255, 255]


def test_truth_error_holes_and_overflow():
    v = np.array([[0.5, NAN, 0.5, 0.5, 0.5, 0.5, 3e38, 0.5, -1.0, INF]], F)
    t = np.array([[0.25, 0.5, NAN, 0.0, -1.0, INF, 6e-39, 6e-39, 1.0, 1.0]], F)
    rel, ab = er.truth_error(v, t, True), er.truth_error(v, t, False)
    assert np.isnan(rel[0, 1:5]).all() and np.isnan(ab[0, 1:5]).all()       # NaN v; NaN, zero, negative t
    assert rel[0, 0] == F(1.0) and ab[0, 0] == F(0.25)
    assert np.isnan(rel[0, 5]) and ab[0, 5] == INF                          # t = +inf is > 0: |v - inf| = inf, inf / inf = NaN
    assert rel[0, 6] == INF and ab[0, 6] == F(3e38)                         # 3e38 / 6e-39 overflows
    assert rel[0, 7] == INF or rel[0, 7] > F(8e37)                          # 0.5 / 6e-39
    assert rel[0, 8] == F(2.0) and rel[0, 9] == INF                         # a negative v is an error like any other here
    st = er.statistics(rel, 1000.0)
    assert st["sum"] == np.inf and st["hist"][255] >= 3


# ---- a property that shows the measurement means something -----------------------------------------------------------------------
def small_scene():
    sc = ss.PlaneScene(160, 120, seed=5, normal=(0.2, -0.1, 1.0), distance=2.2)
    sc.add_camera(0, np.eye(3), [0, 0, 0])
    sc.add_camera(1, ss.rot([0.1, 1, 0.05], 0.01), [-0.12, -0.01, -0.02])
    R, t = sc.cams[1]
    KRKinv = (sc.K32 @ R.astype(F) @ sc.Kinv32).astype(F)
    Kt = (sc.K32 @ t.astype(F)).astype(F)
    ys, xs = np.mgrid[0:120, 0:160]
    truth = sc.true_idepth(0, np.stack([xs.ravel(), ys.ravel()], 1).astype(F)).reshape(120, 160).astype(F)
    return sc, KRKinv, Kt, truth


def test_a_wrong_map_has_a_larger_photometric_error_than_the_true_one():
    sc, KRKinv, Kt, truth = small_scene()
    ref, cmp = sc.render(0), sc.render(1)
    res = {}
    for win in (1, 5):
        for name, s in (("true", 1.0), ("high", 1.15), ("low", 0.85)):
            r = er.map_error((truth * F(s)).astype(F), er.PHOTO, KRKinv, Kt, ref, cmp, border=3, win_size=win)
            res[name, win] = (r["median_bin"], float(r["mean"]), r["n_valid"])
    print(res)
    # Measured with this checker (median_bin, mean) at win_size 1 / 5:
    #   the true map   3, 4.18 / 4, 4.18
    #   truth * 1.15  16, 19.10 / 18, 19.11
    #   truth * 0.85  16, 19.04 / 18, 19.06
    # The factor 2 asserted below is a margin under the measured factor of 4 to 5.
    for win in (1, 5):
        m0, mean0, n0 = res["true", win]
        assert n0 > 0.8 * 114 * 154 and 1 <= m0 <= 6
        for name in ("high", "low"):
            m, mean, n = res[name, win]
            assert m >= 2 * m0 and mean >= 2 * mean0, (name, win, res)
        assert abs(res["high", win][0] - res["low", win][0]) <= 1  # the two wrong maps agree within one bin
    # against the true map itself the TRUTH source reads the scaling back: 15 % is bin 150 of the 0.1 % bins
    r = er.map_error((truth * F(1.15)).astype(F), er.TRUTH, truth=truth, relative=True, win_size=1)
    assert r["median_bin"] in (149, 150, 151) and r["n_valid"] == truth.size and abs(float(r["mean"]) - 0.15) < 1e-3


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported_and_the_abi_version_stays(stage):
    import flame_amd
    from flame_amd.regularizer import ABI_SYMBOLS

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flame_nltgv2.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", header), n
        assert n in ABI_SYMBOLS and hasattr(stage, n), n
    assert re.search(r"#define FLAME_NLTGV2_ABI_VERSION 7\b", header) and stage.flame_nltgv2_abi_version() == 7
    for name in ("map_error", "map_error_begin", "map_error_end"):
        assert callable(getattr(flame_amd.Regularizer, name))
    p = flame_amd.MapErrorParams(source=flame_amd.MAP_ERROR_TRUTH, border=9, relative=False, win_size=7, hist_scale=3.0, ptile_num=1, ptile_den=2,
                                 max_error=1.0, flip=True, want_stats=False, want_error_map=False, want_image=True, copy_out=False,
                                 map_device=64, ref_device=64, cmp_device=64, truth_device=64, gray_device=64, image_step_bytes=5,
                                 gray_step_bytes=6, KRKinv=np.arange(9), Kt=np.arange(3), use_filtered_map=True)
    stage.flame_nltgv2_default_map_error_params(C.byref(p))
    d = flame_amd.MapErrorParams()
    for name, typ in flame_amd.MapErrorParams._fields_:
        a, b = getattr(p, name), getattr(d, name)
        if name in ("KRKinv", "Kt"):
            a, b = list(a), list(b)
        elif name == "truth_host":
            a, b = bool(a), bool(b)
        assert a == b, name
    assert (p.source, p.border, p.relative, p.win_size, p.hist_scale, p.ptile_num, p.ptile_den) == (0, 3, 1, 0, 0.0, 99, 100)
    assert (p.want_stats, p.want_error_map, p.want_image, p.copy_out, p.max_error) == (1, 1, 0, 1, 32.0)
    assert list(p.KRKinv) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and p.map_device is None and p.truth_device is None


def test_new_declarations_compile_as_c_and_cpp_with_the_mirrors_sizes(stage, tmp_path):
    import flame_amd
    from flame_amd.regularizer import _MapErrorView

    sizes = (C.sizeof(flame_amd.MapErrorParams), C.sizeof(flame_amd.MapErrorStats), C.sizeof(_MapErrorView))
    assert sizes == (168, 1048, 72)
    src = tmp_path / "t.c"
    src.write_text(
        '#include <stddef.h>\n#include "flame_nltgv2.h"\n'
        "typedef int (*begin_fn)(flame_nltgv2_ctx*, const flame_nltgv2_map_error_params*, int, int);\n"
        "typedef int (*end_fn)(flame_nltgv2_ctx*, flame_nltgv2_map_error_view*);\n"
        "typedef int (*sync_fn)(flame_nltgv2_ctx*, const flame_nltgv2_map_error_params*, int, int, float*, uint8_t*, flame_nltgv2_map_error_stats*);\n"
        "int main(void) {\n"
        "  begin_fn b = flame_nltgv2_map_error_begin; end_fn e = flame_nltgv2_map_error_end; sync_fn s = flame_nltgv2_map_error;\n"
        "  flame_nltgv2_map_error_params p; flame_nltgv2_default_map_error_params(&p);\n"
        "  (void)b; (void)e; (void)s;\n"
        f"  return (sizeof(flame_nltgv2_map_error_params) == {sizes[0]} && sizeof(flame_nltgv2_map_error_stats) == {sizes[1]} &&"
        f" sizeof(flame_nltgv2_map_error_view) == {sizes[2]} &&"
        f" offsetof(flame_nltgv2_map_error_params, source) == {flame_amd.MapErrorParams.source.offset} &&"
        f" offsetof(flame_nltgv2_map_error_params, copy_out) == {flame_amd.MapErrorParams.copy_out.offset} &&"
        f" offsetof(flame_nltgv2_map_error_stats, sum) == {flame_amd.MapErrorStats.sum.offset} &&"
        f" offsetof(flame_nltgv2_map_error_view, stats) == {_MapErrorView.stats.offset} &&"
        " p.ptile_num == 99 && p.want_stats == 1 && FLAME_NLTGV2_MAP_ERROR_TRUTH == 1 && FLAME_NLTGV2_ABI_VERSION == 7) ? 0 : 1;\n"
        "}\n")
    lib_dir = os.path.join(ROOT, "flame_amd")
    link = ["-L", lib_dir, "-lflame_nltgv2_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"]
    inc = ["-I", os.path.join(ROOT, "include")]
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", *inc, str(src), "-o", str(tmp_path / "t_c"), *link])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-x", "c++", *inc, str(src), "-o", str(tmp_path / "t_cpp"), *link])
    assert subprocess.run([str(tmp_path / "t_c")], timeout=60).returncode == 0
    assert subprocess.run([str(tmp_path / "t_cpp")], timeout=60).returncode == 0


def test_map_error_layout_under_the_sanitizers(tmp_path):
    """tests/cpp/map_error_layout_test.cc: a stand-alone program that walks the layout function; nothing is loaded into Python."""
    exe = str(tmp_path / "map_error_layout_test")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "flame_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "map_error_layout_test.cc"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "384 layouts walked, 0 violations" in r.stdout, r.stdout + r.stderr
