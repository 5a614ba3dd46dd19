"""The window that follows the camera (include/flame_nltgv2.h, THE WINDOW, flame_nltgv2_volume_shift_begin, flame_nltgv2_volume_follow):
the checker tests/volume_window_ref.py on its own -- integration into a moving window is a crop of integration into a larger fixed
volume, follow's hysteresis and its boxes -- and the new symbols and structs of the C-ABI.  No GPU here; the device is compared with the
checker in tests/test_gpu_volume_window*.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import volume_mesh_ref as vmr
from tests import volume_ref as vr
from tests import volume_window_ref as wr
from tests.conftest import ROOT

F = np.float32
NAMES = ("flame_nltgv2_default_follow_params", "flame_nltgv2_volume_window", "flame_nltgv2_volume_shift_begin", "flame_nltgv2_volume_shift_end",
         "flame_nltgv2_volume_shift", "flame_nltgv2_volume_follow")


def fixed_and_window(shift=(3, -2, 1)):
    """SCENE's map from two poses into the unchanged checker's fixed 32 x 24 x 20 volume and into a 16 x 12 x 10 window shifted between
    the calls -> (fixed, window)."""
    big = dict(vr.SCENE, nx=32, ny=24, nz=20)
    fixed, win = vr.Volume(**big), wr.scene_volume()
    m = vr.scene_map()
    for v in (fixed, win):
        v.integrate(m, vr.SCENE_K, vr.IDENTITY)
    win.shift(shift)
    for v in (fixed, win):
        v.integrate(m, vr.SCENE_K, vr.shifted_pose(0.3), weight=0.5)
    return fixed, win


def test_integration_into_a_moving_window_is_a_crop_of_integration_into_a_fixed_volume():
    s = (3, -2, 1)
    fixed, win = fixed_and_window(s)
    assert win.base.tolist() == list(s)
    # the voxels inside the window during both calls, as global index ranges: they all lie in the fixed volume
    lo = [max(0, s[a]) for a in range(3)]
    hi = [min(win.dims[a], win.dims[a] + s[a]) for a in range(3)]
    g = tuple(slice(lo[a], hi[a]) for a in (2, 1, 0))
    loc = tuple(slice(lo[a] - s[a], hi[a] - s[a]) for a in (2, 1, 0))
    assert np.count_nonzero(win.weight[loc] == F(1.5)) > 100  # (seen by both calls)
    assert np.array_equal(vr.bits(win.tsdf[loc]), vr.bits(fixed.tsdf[g]))
    assert np.array_equal(vr.bits(win.weight[loc]), vr.bits(fixed.weight[g]))
    # what the rule is for: moving origin instead changes float32 bits of voxel positions
    moved = 0
    for a, n in enumerate(win.dims):
        idx = np.arange(n)
        anchored = (win.origin[a] + ((s[a] + idx).astype(F) * win.voxel_size).astype(F)).astype(F)
        origin_moved = F(win.origin[a] + F(F(s[a]) * win.voxel_size))
        moved += np.count_nonzero(vr.bits(anchored) != vr.bits((origin_moved + (idx.astype(F) * win.voxel_size).astype(F)).astype(F)))
    assert moved == 12


def test_with_base_zero_the_checker_is_the_unchanged_one():
    a, b = vr.scene_volume(), wr.scene_volume()
    m = vr.scene_map()
    for T in (vr.IDENTITY, vr.shifted_pose(0.15)):
        assert a.integrate(m, vr.SCENE_K, T) == b.integrate(m, vr.SCENE_K, T)
    assert np.array_equal(vr.bits(a.tsdf), vr.bits(b.tsdf)) and np.array_equal(vr.bits(a.weight), vr.bits(b.weight))
    ra = a.raycast(vr.SCENE_KINV, vr.shifted_pose(0.15), vr.SCENE_ROWS, vr.SCENE_COLS, **vr.SCENE_RAYCAST)
    rb = b.raycast(vr.SCENE_KINV, vr.shifted_pose(0.15), vr.SCENE_ROWS, vr.SCENE_COLS, **vr.SCENE_RAYCAST)
    assert np.array_equal(vr.bits(ra["map"]), vr.bits(rb["map"])) and ra["hits"] == rb["hits"] > 0
    ma, mb = vmr.extract(a), wr.extract(b)
    assert ma["n_vertices"] > 0 and np.array_equal(vr.bits(ma["vertices"]), vr.bits(mb["vertices"]))


def test_the_shifts_counters_and_the_scenes_counts():
    v = wr.scene_volume()
    v.integrate(vr.scene_map(), vr.SCENE_K, vr.IDENTITY)
    assert np.count_nonzero(v.weight > 0) == 1278
    for s, kept_seen, lost_seen in (((3, -2, 1), 912, 366), ((2, 0, 0), 1179, 99)):
        w = v.copy()
        c = w.shift(s)
        assert (c["kept_seen"], c["lost_seen"]) == (kept_seen, lost_seen) and c["kept"] + c["entered"] == 1920
        assert np.count_nonzero(w.weight > 0) == kept_seen and w.base.tolist() == list(s)
        # destination (i, j, k) holds source (i, j, k) + s
        assert vr.bits(w.tsdf[2, 5, 4]) == vr.bits(v.tsdf[2 + s[2], 5 + s[1], 4 + s[0]])
    w = v.copy()
    assert w.shift((16, 0, 0)) == dict(kept=0, kept_seen=0, lost_seen=1278, entered=1920) and not w.weight.any()
    w = v.copy()
    assert w.shift((0, 0, 0)) == dict(kept=1920, kept_seen=1278, lost_seen=0, entered=0)
    assert w.shift((wr.MAX_BASE + 1, 0, 0)) is None and w.base.tolist() == [0, 0, 0]
    assert w.shift((wr.MAX_BASE, 0, 0)) is not None and w.shift((1, 0, 0)) is None


def test_follow_has_hysteresis_and_truncates_towards_zero():
    v = wr.scene_volume()  # the middle voxel (8, 6, 5) lies at (0, 0, 1)
    step = 4
    for off, want in ((step - 1, 0), (step, step), (2 * step - 1, step), (-(step - 1), 0), (-step, -step), (-(2 * step - 1), -step), (-2 * step, -2 * step)):
        T = vr.IDENTITY.copy()
        T[3], T[7], T[11] = F(0.1 * off + 0.01 * np.sign(off)), 0.0, 1.0
        assert wr.follow(v, T, step=step)["shift"] == [want, 0, 0], off
    v.shift((4, 0, 0))  # the middle moves with the base
    T = vr.IDENTITY.copy()
    T[3], T[11] = F(0.41), 1.0
    assert wr.follow(v, T, step=step)["shift"] == [0, 0, 0]
    assert wr.follow(v, T, step=0) is None
    T[7] = np.nan
    assert wr.follow(v, T, step=step) is None


def rotated_pose():
    """A rotation with no zero entry (about the axis (1, 2, 3) by 0.7 rad) and a translation."""
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(0.7) * Kx + (1 - np.cos(0.7)) * Kx @ Kx
    T = np.concatenate([R, np.array([[0.3], [-0.2], [0.4]])], axis=1).astype(F)
    assert np.all(T != 0)
    return T.reshape(-1)


def test_follow_with_a_focus_depth_reads_the_optical_axis_of_a_rotated_pose():
    v = wr.scene_volume()
    T = rotated_pose()
    R = T.reshape(3, 4)
    got = wr.follow(v, T, focus_depth=1.5, step=2)
    c = R[:, 3].astype(np.float64) + 1.5 * R[:, 2].astype(np.float64)
    g = (c - v.origin.astype(np.float64)) / float(v.voxel_size)
    want = [int(np.trunc((g[a] - (v.dims[a] // 2)) / 2)) * 2 for a in range(3)]
    assert got["shift"] == want and all(s != 0 for s in want), (got, want)
    assert wr.follow(v, T, focus_depth=0.0, step=2)["shift"] != got["shift"]


@pytest.mark.parametrize("shift", [(3, -2, 1), (2, 0, 0), (0, 0, -3), (-5, 4, 0), (15, -11, 9), (0, 0, 0), (16, 0, 0), (1, 1, -10)])
def test_the_leaving_boxes_and_the_kept_box_tile_the_windows_cubes(shift):
    n = (16, 12, 10)
    p = wr.plan(n, list(shift))
    boxes = list(p["leaving"]) + ([p["kept"]] if p["kept"] else [])
    assert len(p["leaving"]) == (1 if p["kept"] is None else sum(1 for s in shift if s != 0))
    sets = [wr.box_cubes(n, lo, hi) for lo, hi in boxes]
    for lo, hi in boxes:
        assert vmr.box_ok(n, lo, hi) is not None
    assert sum(len(s) for s in sets) == len(set().union(*sets)) == 15 * 11 * 9
    assert set().union(*sets) == wr.box_cubes(n, (0, 0, 0), n)
    if p["kept"]:
        lo, hi = p["kept"]
        assert lo == [max(0, s) for s in shift] and hi == [min(n[a], n[a] + shift[a]) for a in range(3)]


def test_the_leaving_and_kept_meshes_add_up_to_the_whole_extraction():
    v = wr.scene_volume()
    v.integrate(vr.scene_map(), vr.SCENE_K, vr.IDENTITY)
    whole = wr.extract(v)
    p = wr.plan(v.dims, [3, -2, 1])
    parts = [wr.extract(v, lo, hi) for lo, hi in list(p["leaving"]) + [p["kept"]]]
    assert whole["n_triangles"] > 0 and sum(m["n_triangles"] for m in parts) == whole["n_triangles"]
    # a kept cube's vertices keep their bytes across the shift, triangles their indices
    before = parts[-1]
    w = v.copy()
    w.shift((3, -2, 1))
    after = wr.extract(w)
    assert after["n_triangles"] == before["n_triangles"] > 0 and np.array_equal(after["triangles"], before["triangles"])
    assert np.array_equal(vr.bits(after["vertices"]), vr.bits(before["vertices"]))
    same = wr.normals_untouched(w, after["keys"], (3, -2, 1))
    assert 0 < np.count_nonzero(same) < same.size
    assert np.array_equal(vr.bits(after["normals"][same]), vr.bits(before["normals"][same]))


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(built):
    import flame_amd

    return flame_amd.load_library()


def test_new_symbols_are_declared_and_exported_and_the_abi_version_stays(lib):
    import flame_amd
    from flame_amd.regularizer import ABI_SYMBOLS

    text = open(os.path.join(ROOT, "include", "flame_nltgv2.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", header), n
        assert n in ABI_SYMBOLS and hasattr(lib, n), n
    assert re.search(r"#define FLAME_NLTGV2_ABI_VERSION 7\b", header) and lib.flame_nltgv2_abi_version() == 7
    assert "a volume that moves with the camera" not in text
    for name in ("volume_window", "volume_shift_begin", "volume_shift_end", "volume_shift", "volume_follow"):
        assert callable(getattr(flame_amd.Regularizer, name))
    p = flame_amd.FollowParams()
    C.memset(C.byref(p), 0x5A, C.sizeof(p))
    lib.flame_nltgv2_default_follow_params(C.byref(p))
    assert bytes(p) == bytes(flame_amd.FollowParams()) and (p.focus_depth, p.step) == (0.0, 8)


def test_new_declarations_compile_as_c_and_cpp_with_the_mirrors_sizes(lib, tmp_path):
    import flame_amd
    from flame_amd.regularizer import _ShiftView

    sizes = (C.sizeof(flame_amd.ShiftCounts), C.sizeof(_ShiftView), C.sizeof(flame_amd.FollowParams), C.sizeof(flame_amd.FollowPlan))
    assert sizes == (32, 64, 8, 128)
    src = tmp_path / "t.c"
    src.write_text(
        '#include <stddef.h>\n#include "flame_nltgv2.h"\n'
        "typedef int (*win_fn)(flame_nltgv2_ctx*, int32_t*);\n"
        "typedef int (*sb_fn)(flame_nltgv2_ctx*, const int32_t*);\n"
        "typedef int (*se_fn)(flame_nltgv2_ctx*, flame_nltgv2_shift_view*);\n"
        "typedef int (*s_fn)(flame_nltgv2_ctx*, const int32_t*, flame_nltgv2_shift_counts*);\n"
        "typedef int (*f_fn)(flame_nltgv2_ctx*, const float*, const flame_nltgv2_follow_params*, flame_nltgv2_follow_plan*);\n"
        "int main(void) {\n"
        "  win_fn w = flame_nltgv2_volume_window; sb_fn sb = flame_nltgv2_volume_shift_begin; se_fn se = flame_nltgv2_volume_shift_end;\n"
        "  s_fn s = flame_nltgv2_volume_shift; f_fn f = flame_nltgv2_volume_follow;\n"
        "  flame_nltgv2_follow_params fp;\n"
        "  flame_nltgv2_default_follow_params(&fp);\n"
        "  (void)w; (void)sb; (void)se; (void)s; (void)f;\n"
        f"  return (sizeof(flame_nltgv2_shift_counts) == {sizes[0]} && sizeof(flame_nltgv2_shift_view) == {sizes[1]} &&"
        f" sizeof(flame_nltgv2_follow_params) == {sizes[2]} && sizeof(flame_nltgv2_follow_plan) == {sizes[3]} &&"
        f" offsetof(flame_nltgv2_shift_view, base) == {_ShiftView.base.offset} &&"
        f" offsetof(flame_nltgv2_shift_view, counts) == {_ShiftView.counts.offset} &&"
        f" offsetof(flame_nltgv2_shift_counts, entered) == {flame_amd.ShiftCounts.entered.offset} &&"
        f" offsetof(flame_nltgv2_follow_plan, kept_lo) == {flame_amd.FollowPlan.kept_lo.offset} &&"
        f" offsetof(flame_nltgv2_follow_plan, leaving_lo) == {flame_amd.FollowPlan.leaving_lo.offset} &&"
        f" offsetof(flame_nltgv2_follow_plan, leaving_hi) == {flame_amd.FollowPlan.leaving_hi.offset} &&"
        " fp.focus_depth == 0.0f && fp.step == 8 && FLAME_NLTGV2_ABI_VERSION == 7) ? 0 : 1;\n"
        "}\n")
    lib_dir = os.path.join(ROOT, "flame_amd")
    link = ["-L", lib_dir, "-lflame_nltgv2_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"]
    inc = ["-I", os.path.join(ROOT, "include")]
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", *inc, str(src), "-o", str(tmp_path / "t_c"), *link])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-x", "c++", *inc, str(src), "-o", str(tmp_path / "t_cpp"), *link])
    assert subprocess.run([str(tmp_path / "t_c")], timeout=60).returncode == 0
    assert subprocess.run([str(tmp_path / "t_cpp")], timeout=60).returncode == 0


def test_window_plan_under_the_sanitizers(tmp_path):
    """tests/cpp/volume_window_layout_test.cc: a stand-alone program that walks side_stage.hpp's window functions against what this
    checker says (passed as text); nothing is loaded into Python."""
    exe = str(tmp_path / "volume_window_layout_test")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall",
                           "-Wextra", "-Werror", "-I", os.path.join(ROOT, "flame_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "volume_window_layout_test.cc"), "-o", exe])
    n = (16, 12, 10)
    lines = []
    for shift in [(3, -2, 1), (2, 0, 0), (0, 0, -3), (-5, 4, 0), (15, -11, 9), (0, 0, 0), (16, 0, 0), (1, 1, -10), (-2000000000, 5, 5)]:
        p = wr.plan(n, list(shift))
        words = list(shift) + [len(p["leaving"]), 1 if p["kept"] else 0]
        words += (p["kept"][0] + p["kept"][1]) if p["kept"] else [0] * 6
        for lo, hi in p["leaving"]:
            words += lo + hi
        lines.append(" ".join(str(w) for w in words))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 violations" in r.stdout and f"{len(lines)} plans" in r.stdout, r.stdout + r.stderr
