"""The volumetric map (include/flame_nltgv2.h, flame_nltgv2_volume_create): the checker tests/volume_ref.py on its own -- the scene the
GPU tests share has every counter of both stages above zero, the order of two integrations is part of the result, the raycast of a plane
gives the plane's depth, the borders of the rules fall where the header puts them -- and the new symbols and structs of the C-ABI.  No
GPU here; the device is compared with the checker in tests/test_gpu_volume*.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import volume_ref as vr
from tests.conftest import ROOT

F = np.float32
NAMES = ("flame_nltgv2_default_volume_params", "flame_nltgv2_default_integrate_params", "flame_nltgv2_default_raycast_params",
         "flame_nltgv2_volume_create", "flame_nltgv2_volume_reset", "flame_nltgv2_volume_destroy", "flame_nltgv2_volume_info",
         "flame_nltgv2_volume_download", "flame_nltgv2_volume_upload", "flame_nltgv2_volume_integrate_begin", "flame_nltgv2_volume_integrate_end",
         "flame_nltgv2_volume_integrate", "flame_nltgv2_volume_raycast_begin", "flame_nltgv2_volume_raycast_end", "flame_nltgv2_volume_raycast")


def test_the_scene_has_every_counter_of_both_stages_above_zero():
    v, m = vr.scene_volume(), vr.scene_map()
    calls = [v.integrate(m, vr.SCENE_K, vr.IDENTITY) for _ in range(3)]
    for c in calls:
        assert c["front"] == 16 * 12 * 10 and c["front"] > c["in_image"] > c["valid"] > c["updated"] > 0 and c["behind"] > 0
        assert c["updated"] == c["valid"] - c["behind"]
    assert calls[0]["saturated"] == calls[1]["saturated"] == 0 and calls[2]["saturated"] == calls[2]["updated"] > 0
    assert np.all(v.weight[v.weight > 0] == F(2.0)) and np.count_nonzero(v.weight) == calls[0]["updated"]
    assert np.all(v.tsdf[v.weight == 0] == F(1.0)) and v.tsdf.min() >= F(-1.0)
    for T in (vr.IDENTITY, vr.shifted_pose(0.15)):
        r = v.raycast(vr.SCENE_KINV, T, vr.SCENE_ROWS, vr.SCENE_COLS, **vr.SCENE_RAYCAST)
        assert r["hits"] > 0 and r["back"] > 0 and r["empty"] > 0, r
        assert r["hits"] == np.count_nonzero(~np.isnan(r["map"])) and np.all(vr.bits(r["map"][np.isnan(r["map"])]) == 0x7FC00000)
        # the wall and the step behind it: every hit lies between the two inverse depths
        assert r["map"][~np.isnan(r["map"])].min() > 0.75 and r["map"][~np.isnan(r["map"])].max() < 1.05


def test_the_order_of_two_integrations_is_part_of_the_result():
    a, b = vr.scene_map(), (vr.scene_map() * F(0.9)).astype(F)
    # (a + b == b + a in float32, so two calls that stay below max_weight commute up to the first call's s * w / w; here the heavier call
    # saturates the voxel and the lighter one meets another w_old in the two orders)
    ab, ba = vr.scene_volume(), vr.scene_volume()
    ab.integrate(a, vr.SCENE_K, vr.IDENTITY, weight=0.5), ab.integrate(b, vr.SCENE_K, vr.shifted_pose(-0.05), weight=3.0)
    ba.integrate(b, vr.SCENE_K, vr.shifted_pose(-0.05), weight=3.0), ba.integrate(a, vr.SCENE_K, vr.IDENTITY, weight=0.5)
    assert np.array_equal(ab.weight > 0, ba.weight > 0)
    assert np.count_nonzero(vr.bits(ab.tsdf) != vr.bits(ba.tsdf)) > 0


def test_the_raycast_of_a_plane_gives_its_depth_within_one_step():
    v = vr.Volume(32, 24, 24, 0.05, (-0.8, -0.6, 0.4), 0.2, 100.0)
    rows, cols = 24, 32
    col, row = np.meshgrid(np.arange(cols), np.arange(rows))
    depth = 1.0 + 0.2 * (col - 16) / 20.0  # a plane tilted about the vertical axis
    v.integrate((1.0 / depth).astype(F), vr.SCENE_K, vr.IDENTITY)
    dz = 0.03
    r = v.raycast(vr.SCENE_KINV, vr.IDENTITY, rows, cols, 0.3, dz, 60)
    hit = ~np.isnan(r["map"])
    assert r["hits"] > 0.5 * rows * cols
    assert np.abs(1.0 / r["map"][hit].astype(np.float64) - depth[hit]).max() < dz


def test_the_borders_of_the_integration_fall_where_the_header_puts_them():
    # one row of voxels along x at z = 1 in front of a camera with f = 1: u == x + c exactly
    K = np.array([1, 0, 0.5, 0, 1, 0, 0, 0, 1], F)
    v = vr.Volume(4, 1, 1, 1.0, (-1.0, 0.0, 1.0), 0.5, 8.0)
    c = v.integrate(np.full((1, 2), 1.0, F), K, vr.IDENTITY)
    # u = -0.5 (in), 0.5, 1.5 == cols - 0.5 (out), 2.5
    assert (c["front"], c["in_image"], c["updated"]) == (4, 2, 2) and v.weight.reshape(-1).tolist() == [1.0, 1.0, 0.0, 0.0]
    # P.z == near_depth is skipped
    assert vr.Volume(4, 1, 1, 1.0, (-1.0, 0.0, 1.0), 0.5, 8.0).integrate(np.full((1, 2), 1.0, F), K, vr.IDENTITY, near_depth=1.0)["front"] == 0
    # sdf == -trunc is updated with tsdf -1, one ulp below is left alone
    # (zm = 1 / 2 and P.z = 1 are exact: sdf == -0.5; with trunc one ulp below 0.5, -0.5 is one ulp below -trunc)
    for trunc, updated in ((F(0.5), 1), (np.nextafter(F(0.5), F(0)), 0)):
        w = vr.Volume(1, 1, 1, 1.0, (0.0, 0.0, 1.0), trunc, 8.0)
        c = w.integrate(np.full((1, 1), 2.0, F), np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], F), vr.IDENTITY)
        assert (c["valid"], c["behind"], c["updated"]) == (1, 1 - updated, updated)
        assert w.tsdf.item() == (-1.0 if updated else 1.0)
    # +inf, a denormal, NaN, 0 and negative values are holes; min_depth and max_depth cut
    for d, kw, valid in ((np.inf, {}, 0), (1e-40, {}, 0), (6e-39, {}, 1), (6e-39, dict(max_depth=1e38), 0), (np.nan, {}, 0), (0.0, {}, 0), (-1.0, {}, 0), (1.0, {}, 1),
                         (1.0, dict(min_depth=1.0), 0), (1.0, dict(max_depth=1.0), 0), (1.0, dict(min_depth=0.5, max_depth=1.5), 1)):
        w = vr.Volume(1, 1, 1, 1.0, (0.0, 0.0, 1.0), 0.5, 8.0)
        with np.errstate(all="ignore"):
            c = w.integrate(np.full((1, 1), d, F), np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], F), vr.IDENTITY, **kw)
        assert (c["in_image"], c["valid"]) == (1, valid), (d, kw, c)


def test_the_raycast_on_hand_made_volumes():
    K1 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], F)  # pixel (0, 0) looks along +z

    def cast(tsdf_of_k, weight=None, nz=8, **kw):
        v = vr.Volume(2, 2, nz, 1.0, (-0.5, -0.5, 0.0), 1.0, 8.0)  # the ray x = y = 0 runs through the middle of the column
        v.tsdf = np.broadcast_to(np.asarray(tsdf_of_k, F)[:, None, None], (nz, 2, 2)).copy()
        v.weight = np.ones((nz, 2, 2), F) if weight is None else np.asarray(weight, F)
        args = dict(z_near=0.0, dz=0.5, n_steps=15)
        args.update(kw)
        return v.raycast(K1, vr.IDENTITY, 1, 1, **args)

    ramp = [3, 2, 1, 0, -1, -2, -3, -4]  # the surface at z = 3, a crossing with f_cur == 0 when a sample falls on it
    r = cast(ramp)
    assert (r["hits"], r["back"], r["empty"]) == (1, 0, 0) and r["map"].item() == F(1.0) / F(3.0)
    r = cast(ramp, dz=0.4, n_steps=19)  # between two samples: linear in a linear field
    assert r["hits"] == 1 and abs(1.0 / r["map"].item() - 3.0) < 1e-5
    assert cast(ramp, z_near=4.0)["back"] == 1 and cast(ramp, z_near=3.0)["back"] == 1  # starts inside / on the surface
    assert cast([-1, -1, 0, 1, 2, 3, 4, 5])["back"] == 1  # met from behind
    r = cast(ramp, z_near=-2.0)  # enters late: four samples in front of the volume
    assert (r["hits"], r["empty"]) == (1, 0) and r["map"].item() == F(1.0) / F(3.0)
    r = cast(ramp, z_near=8.0)  # never enters
    assert (r["hits"], r["back"], r["empty"]) == (0, 0, 1) and vr.bits(r["map"]).item() == 0x7FC00000
    r = cast([5, 4, 3, 2, 1, 0.5, 0.25, 0.125])  # never ends, with valid samples
    assert (r["hits"], r["back"], r["empty"]) == (0, 0, 0) and np.isnan(r["map"].item())
    w = np.ones((8, 2, 2), F)
    w[3, 1, 1] = 0  # a weight-0 voxel among the eight of the cells 2 and 3: the crossing's sample is not valid, the next one has no valid neighbour
    assert cast(ramp, weight=w)["back"] == 1
    r = cast([7, 6, 5, 4, 3, 2, 1, -1], dz=1.0, n_steps=8)  # g == n_axis - 1 exactly: f == 1 in the last cell
    assert r["hits"] == 1 and r["map"].item() == F(1.0) / (F(6.0) + F(1.0) * (F(1.0) / (F(1.0) - F(-1.0))))
    assert cast(ramp, n_steps=1)["hits"] == 0 and cast(ramp, dz=0.001, n_steps=4096)["hits"] == 1
    # an axis of one voxel has no valid sample
    v = vr.Volume(4, 1, 4, 1.0, (0.0, 0.0, 0.0), 1.0, 8.0)
    v.weight[:] = 1
    assert v.raycast(K1, vr.IDENTITY, 3, 5, 0.0, 0.5, 8)["empty"] == 15


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(built):
    import flame_amd

    return flame_amd.load_library()


def test_new_symbols_are_declared_and_exported_and_the_abi_version_stays(lib):
    import flame_amd
    from flame_amd.regularizer import ABI_SYMBOLS

    assert hasattr(lib, "flame_nltgv2_volume_create")
    text = open(os.path.join(ROOT, "include", "flame_nltgv2.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", header), n
        assert n in ABI_SYMBOLS and hasattr(lib, n), n
    assert re.search(r"#define FLAME_NLTGV2_ABI_VERSION 7\b", header) and lib.flame_nltgv2_abi_version() == 7
    for name in ("volume_create", "volume_reset", "volume_destroy", "volume_info", "volume_download", "volume_upload", "volume_integrate_begin",
                 "volume_integrate_end", "volume_integrate", "volume_raycast_begin", "volume_raycast_end", "volume_raycast"):
        assert callable(getattr(flame_amd.Regularizer, name))
    for cls, default in ((flame_amd.VolumeParams, lib.flame_nltgv2_default_volume_params),
                         (flame_amd.IntegrateParams, lib.flame_nltgv2_default_integrate_params),
                         (flame_amd.RaycastParams, lib.flame_nltgv2_default_raycast_params)):
        p = cls()
        C.memset(C.byref(p), 0x5A, C.sizeof(p))
        default(C.byref(p))
        assert bytes(p) == bytes(cls()), cls.__name__
    p = flame_amd.VolumeParams()
    assert (p.nx, p.ny, p.nz, list(p.origin)) == (64, 64, 64, [0, 0, 0]) and p.voxel_size == F(0.05) and p.trunc == F(0.15) and p.max_weight == 64
    i = flame_amd.IntegrateParams()
    assert (i.weight, i.near_depth, i.min_depth, i.max_depth, i.use_filtered_map, i.map_device) == (1, 0, 0, np.inf, 0, None)
    r = flame_amd.RaycastParams()
    assert (r.n_steps, r.copy_out) == (64, 1) and r.z_near == F(0.1) and r.dz == F(0.05)


def test_new_declarations_compile_as_c_and_cpp_with_the_mirrors_sizes(lib, tmp_path):
    import flame_amd
    from flame_amd.regularizer import _IntegrateView, _RaycastView

    sizes = (C.sizeof(flame_amd.VolumeParams), C.sizeof(flame_amd.IntegrateParams), C.sizeof(flame_amd.IntegrateCounts), C.sizeof(_IntegrateView),
             C.sizeof(flame_amd.RaycastParams), C.sizeof(flame_amd.RaycastCounts), C.sizeof(_RaycastView))
    assert sizes == (36, 32, 32, 48, 16, 16, 48)
    src = tmp_path / "t.c"
    src.write_text(
        '#include <stddef.h>\n#include "flame_nltgv2.h"\n'
        "typedef int (*create_fn)(flame_nltgv2_ctx*, const flame_nltgv2_volume_params*);\n"
        "typedef int (*ctx_fn)(flame_nltgv2_ctx*);\n"
        "typedef int (*info_fn)(flame_nltgv2_ctx*, flame_nltgv2_volume_params*, int64_t*);\n"
        "typedef int (*down_fn)(flame_nltgv2_ctx*, float*, float*);\n"
        "typedef int (*up_fn)(flame_nltgv2_ctx*, const float*, const float*);\n"
        "typedef int (*ib_fn)(flame_nltgv2_ctx*, const float*, const float*, const flame_nltgv2_integrate_params*, int, int);\n"
        "typedef int (*ie_fn)(flame_nltgv2_ctx*, flame_nltgv2_integrate_view*);\n"
        "typedef int (*i_fn)(flame_nltgv2_ctx*, const float*, const float*, const flame_nltgv2_integrate_params*, int, int, flame_nltgv2_integrate_counts*);\n"
        "typedef int (*rb_fn)(flame_nltgv2_ctx*, const float*, const float*, const flame_nltgv2_raycast_params*, int, int);\n"
        "typedef int (*re_fn)(flame_nltgv2_ctx*, flame_nltgv2_raycast_view*);\n"
        "typedef int (*r_fn)(flame_nltgv2_ctx*, const float*, const float*, const flame_nltgv2_raycast_params*, int, int, float*, flame_nltgv2_raycast_counts*);\n"
        "int main(void) {\n"
        "  create_fn c = flame_nltgv2_volume_create; ctx_fn rs = flame_nltgv2_volume_reset; ctx_fn d = flame_nltgv2_volume_destroy;\n"
        "  info_fn i = flame_nltgv2_volume_info; down_fn dn = flame_nltgv2_volume_download; up_fn up = flame_nltgv2_volume_upload;\n"
        "  ib_fn ib = flame_nltgv2_volume_integrate_begin; ie_fn ie = flame_nltgv2_volume_integrate_end; i_fn ii = flame_nltgv2_volume_integrate;\n"
        "  rb_fn rb = flame_nltgv2_volume_raycast_begin; re_fn re = flame_nltgv2_volume_raycast_end; r_fn rr = flame_nltgv2_volume_raycast;\n"
        "  flame_nltgv2_volume_params vp; flame_nltgv2_integrate_params ip; flame_nltgv2_raycast_params rp;\n"
        "  flame_nltgv2_default_volume_params(&vp); flame_nltgv2_default_integrate_params(&ip); flame_nltgv2_default_raycast_params(&rp);\n"
        "  (void)c; (void)rs; (void)d; (void)i; (void)dn; (void)up; (void)ib; (void)ie; (void)ii; (void)rb; (void)re; (void)rr;\n"
        f"  return (sizeof(flame_nltgv2_volume_params) == {sizes[0]} && sizeof(flame_nltgv2_integrate_params) == {sizes[1]} &&"
        f" sizeof(flame_nltgv2_integrate_counts) == {sizes[2]} && sizeof(flame_nltgv2_integrate_view) == {sizes[3]} &&"
        f" sizeof(flame_nltgv2_raycast_params) == {sizes[4]} && sizeof(flame_nltgv2_raycast_counts) == {sizes[5]} &&"
        f" sizeof(flame_nltgv2_raycast_view) == {sizes[6]} &&"
        f" offsetof(flame_nltgv2_volume_params, origin) == {flame_amd.VolumeParams.origin.offset} &&"
        f" offsetof(flame_nltgv2_volume_params, max_weight) == {flame_amd.VolumeParams.max_weight.offset} &&"
        f" offsetof(flame_nltgv2_integrate_params, map_device) == {flame_amd.IntegrateParams.map_device.offset} &&"
        f" offsetof(flame_nltgv2_integrate_counts, saturated) == {flame_amd.IntegrateCounts.saturated.offset} &&"
        f" offsetof(flame_nltgv2_integrate_view, counts) == {_IntegrateView.counts.offset} &&"
        f" offsetof(flame_nltgv2_raycast_view, counts) == {_RaycastView.counts.offset} &&"
        f" offsetof(flame_nltgv2_raycast_view, map_device) == {_RaycastView.map_device.offset} &&"
        " vp.nx == 64 && ip.weight == 1.0f && ip.map_device == NULL && rp.n_steps == 64 && rp.copy_out == 1 &&"
        " FLAME_NLTGV2_ABI_VERSION == 7) ? 0 : 1;\n"
        "}\n")
    lib_dir = os.path.join(ROOT, "flame_amd")
    link = ["-L", lib_dir, "-lflame_nltgv2_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"]
    inc = ["-I", os.path.join(ROOT, "include")]
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", *inc, str(src), "-o", str(tmp_path / "t_c"), *link])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-x", "c++", *inc, str(src), "-o", str(tmp_path / "t_cpp"), *link])
    assert subprocess.run([str(tmp_path / "t_c")], timeout=60).returncode == 0
    assert subprocess.run([str(tmp_path / "t_cpp")], timeout=60).returncode == 0


def test_volume_layout_under_the_sanitizers(tmp_path):
    """tests/cpp/volume_layout_test.cc: a stand-alone program that walks the layout functions; nothing is loaded into Python."""
    exe = str(tmp_path / "volume_layout_test")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "flame_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "volume_layout_test.cc"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 violations" in r.stdout, r.stdout + r.stderr
