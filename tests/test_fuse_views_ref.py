"""The fusion of views (include/flame_nltgv2.h, flame_nltgv2_fuse_views_begin): known answers for the checker tests/fuse_ref.py on
hand-made layer stacks (rules C - F), the scene the GPU tests share -- four views of one plane with planted outliers -- with what it
must contain asserted on the checker alone, and the new symbols and structs of the C-ABI.  No GPU here; the device is compared with
the checker in tests/test_gpu_fuse_views*.py."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import fuse_ref as fr
from tests import test_render_view_ref as cases
from tests import view_ref as vr
from tests.conftest import ROOT

F = np.float32
EYE = np.eye(3, dtype=F)
NAN = np.uint32(0x7FC00000).view(F)
NAMES = ("flame_nltgv2_keep_mesh", "flame_nltgv2_keep_mesh_arrays", "flame_nltgv2_drop_mesh", "flame_nltgv2_kept_mesh_info",
         "flame_nltgv2_get_kept_mesh", "flame_nltgv2_default_fuse_params", "flame_nltgv2_fuse_views_begin", "flame_nltgv2_fuse_views_end",
         "flame_nltgv2_fuse_views")

# ---- the scene ---------------------------------------------------------------------------------------------------------------------
SRC = (48, 64)
K, KINV = cases.camera(60.0, 32.0, 24.0)
PLANE_N, PLANE_D = np.array([0.1, -0.05, 1.0]), 2.0  # n . P = 2 in the target's frame
POSES = [(EYE, np.zeros(3, F)),
         (cases.rotation_y(4.0), np.array([-0.15, 0, 0.02], F)),
         (cases.rotation_y(-6.0), np.array([0.25, 0.03, 0], F)),
         (EYE, np.array([0, -0.3, 0.1], F)),
         # four more for the eight-source case
         (cases.rotation_y(2.0), np.array([0.1, 0.1, 0], F)),
         (cases.rotation_y(-3.0), np.array([-0.1, 0.2, 0.05], F)),
         (EYE, np.array([0.3, 0, -0.05], F)),
         (cases.rotation_y(5.0), np.array([-0.3, -0.1, 0], F))]
WEIGHTS = [1.0, 0.3, 1.7, 0.9, 0.5, 2.0, 1.1, 0.7]
REL_TOL = 0.02


def plane_source(s, step=6, outliers=None, seed=None):
    """Source s of the scene: a jittered grid whose vertices lie on the plane as pose s sees it; in sources 1 and 3 one vertex in eight has
    its inverse depth multiplied by 0.7 or 1.4."""
    R, t = POSES[s]
    pos, tris = cases.grid_mesh(*SRC, step, seed=30 + s if seed is None else seed)
    q = KINV.astype(np.float64) @ np.stack([pos[:, 0], pos[:, 1], np.ones(len(pos))])
    idepth = (PLANE_N @ (R.astype(np.float64) @ q)) / (PLANE_D - PLANE_N @ t.astype(np.float64))
    if s in (1, 3) if outliers is None else outliers:
        v = np.arange(len(pos))
        idepth = np.where(v % 8 == s, idepth * np.where((v // 8) % 2 == 0, 0.7, 1.4), idepth)
    return dict(tris=tris, pos=pos, idepth=idepth.astype(F), Kinv_src=KINV, R=R, t=t, weight=WEIGHTS[s])


@functools.lru_cache(maxsize=None)
def scene(n=4):
    return tuple(plane_source(s) for s in range(n))


@functools.lru_cache(maxsize=None)
def scene_fused(min_support, n=4, rows=SRC[0], cols=SRC[1]):
    return fr.fuse_sources(scene(n), K, rows, cols, REL_TOL, min_support)


def stack(*pixels):
    """Hand-made layers: one row, a pixel per argument, each a list of N values (None: a hole) -> (N, 1, len(pixels)) f32."""
    return np.array([[NAN if v is None else F(v) for v in p] for p in pixels], F).T.reshape(len(pixels[0]), 1, len(pixels))


def one(values, weights=None, rel_tol=0.1, min_support=1):
    r = fr.fuse_views(stack(values), weights or [1.0] * len(values), rel_tol, min_support)
    return {k: (v[0, 0] if isinstance(v, np.ndarray) and v.ndim == 2 else v) for k, v in r.items()}


# ---- known answers: rules C - F ------------------------------------------------------------------------------------------------------
def test_one_source_fuses_to_itself_and_a_hole_stays_a_hole():
    r = fr.fuse_views(stack([0.75], [None]), [1.0], 0.0, 1)
    assert vr.bits(r["fused"]).tolist() == [[vr.bits(F(0.75))[()], fr.HOLE]] and vr.bits(r["spread"]).tolist() == [[0, fr.HOLE]]
    assert r["present_mask"].tolist() == [[1, 0]] and r["inlier_mask"].tolist() == [[1, 0]]
    assert (r["coverage"], r["support_hist"][:2], r["present"][0], r["inlier"][0]) == (1, [1, 1], 1, 1)
    assert r["counts"][27:].tolist() == [0] * 5 and r["counts"].dtype == np.int32


def test_of_two_that_disagree_the_nearer_is_the_reference():
    for values in ([0.5, 1.0], [1.0, 0.5]):
        r = one(values, rel_tol=0.1)
        near = values.index(1.0)
        assert r["fused"] == F(1.0) and r["inlier_mask"] == 1 << near and r["present_mask"] == 3 and r["support_hist"][1] == 1
    # ... and within the tolerance of the nearer both count: |0.95 - 1| <= 0.1 * 1
    r = one([0.95, 1.0], rel_tol=0.1)
    assert r["inlier_mask"] == 3 and r["fused"] == F(F(F(0.95) + F(1.0)) / F(2.0)) and r["spread"] == F(F(1.0) - F(0.95))
    # of three the middle one, of four the upper of the two in the middle
    assert one([0.3, 0.9, 0.6], rel_tol=0.0)["inlier_mask"] == 0b100
    assert one([0.3, 0.9, 0.6, 0.7], rel_tol=0.0)["inlier_mask"] == 0b1000
    assert one([0.3, None, 0.6, 0.7], rel_tol=0.0)["inlier_mask"] == 0b100  # (a hole takes no rank)


def test_equal_bit_patterns_tie_by_source_index_and_both_are_inliers_at_zero_tolerance():
    r = one([0.8, 0.8], rel_tol=0.0)
    assert r["inlier_mask"] == 3 and r["support_hist"][2] == 1 and r["fused"] == F(0.8) and r["spread"] == F(0.0)
    # three present, two of them equal: the ranks are (0.5, s0) < (0.8, s1) < (0.8, s3): m is index 1, either way 0.8
    r = one([0.5, 0.8, None, 0.8], rel_tol=0.0, min_support=2)
    assert r["present_mask"] == 0b1011 and r["inlier_mask"] == 0b1010 and r["fused"] == F(0.8)


def test_zero_tolerance_with_unequal_values_leaves_the_reference_alone():
    lo = F(0.8)
    hi = np.nextafter(lo, F(1))
    r = one([lo, hi], rel_tol=0.0)
    assert r["inlier_mask"] == 2 and r["support_hist"][1] == 1 and vr.bits(r["fused"]) == vr.bits(hi) and r["spread"] == F(0.0)
    assert one([lo, hi], rel_tol=0.0, min_support=2)["coverage"] == 0


def test_min_support_from_one_to_n():
    # supports 1, 2, 3, 4 and a pixel nobody sees
    layers = stack([1.0, 0.5, 0.25, 0.125], [1.0, 1.0, 0.5, 0.25], [1.0, 1.0, 1.0, 0.5], [1.0, 1.0, 1.0, 1.0], [None] * 4)
    for k in (1, 2, 3, 4):
        r = fr.fuse_views(layers, [1.0] * 4, 0.01, k)
        assert r["support_hist"][:5] == [1, 1, 1, 1, 1]  # (the histogram does not depend on min_support)
        assert (~np.isnan(r["fused"])).tolist() == [[s >= k for s in (1, 2, 3, 4)] + [False]] and r["coverage"] == 5 - k
    with pytest.raises(AssertionError):
        fr.fuse_views(layers, [1.0] * 4, 0.01, 5)


ORDER_VALUES, ORDER_WEIGHTS = [0.70001, 0.70002, 0.70003], [0.3, 1.7, 0.9]


def test_weights_are_applied_left_to_right_in_ascending_source_index():
    v, w = [F(x) for x in ORDER_VALUES], [F(x) for x in ORDER_WEIGHTS]
    r = one(ORDER_VALUES, ORDER_WEIGHTS, rel_tol=0.01)
    assert r["inlier_mask"] == 7
    p = [F(v[i] * w[i]) for i in range(3)]
    num, den = F(F(p[0] + p[1]) + p[2]), F(F(w[0] + w[1]) + w[2])
    assert vr.bits(r["fused"]) == vr.bits(F(num / den))
    # another order of the same sums gives other bits for these values: the test would be testing nothing otherwise
    other = F(F(p[0] + F(p[1] + p[2])) / F(w[0] + F(w[1] + w[2])))
    assert vr.bits(other) != vr.bits(F(num / den))
    # a source that is no inlier is left out of both sums
    r = one([ORDER_VALUES[0], 0.2, ORDER_VALUES[2]], ORDER_WEIGHTS, rel_tol=0.01)
    assert r["inlier_mask"] == 5 and vr.bits(r["fused"]) == vr.bits(F(F(p[0] + p[2]) / F(w[0] + w[2])))


def test_an_unfused_pixel_keeps_its_masks_and_its_spread():
    r = one([0.5, 1.0, 0.99], rel_tol=0.02, min_support=3)
    assert np.isnan(r["fused"]) and vr.bits(r["fused"]) == fr.HOLE and r["coverage"] == 0
    assert r["present_mask"] == 7 and r["inlier_mask"] == 6 and r["present_mask"] & ~r["inlier_mask"] == 1
    assert r["spread"] == F(F(1.0) - F(0.99)) and r["support_hist"][2] == 1 and (r["present"][:3], r["inlier"][:3]) == ([1, 1, 1], [0, 1, 1])
    assert vr.bits(one([None, None])["spread"]) == fr.HOLE


# ---- the scene: what it must contain, on the checker alone -----------------------------------------------------------------------------
def test_the_scene_has_every_support_outliers_ties_and_a_coverage_that_falls():
    runs = {k: scene_fused(k) for k in (1, 2, 3)}
    r = runs[1]
    assert all(x["tris_drawn"] == len(scene()[0]["tris"]) == 140 for x in r["renders"]) and r["tris_drawn"] == 4 * 140
    assert all(r["support_hist"][k] > 0 for k in range(5)) and sum(r["support_hist"][5:]) == 0, r["support_hist"]
    assert ((r["present_mask"] & ~r["inlier_mask"]) != 0).sum() > 100  # pixels with a present outlier
    b = vr.bits(r["layers"])
    ties = sum(((b[i] == b[j]) & (b[i] != fr.HOLE)).sum() for i in range(4) for j in range(i + 1, 4))
    assert ties > 0
    assert runs[1]["coverage"] > runs[2]["coverage"] > runs[3]["coverage"] > 0
    # the clean layers agree: sources 0 and 2 see the same plane
    both = ~np.isnan(r["layers"][0]) & ~np.isnan(r["layers"][2])
    assert both.sum() > 1000 and np.abs(r["layers"][0][both] / r["layers"][2][both] - 1).max() < 1e-3
    # fused pixels lie on the plane: id = n . ray / 2
    cols, rows = np.meshgrid(np.arange(SRC[1]), np.arange(SRC[0]))
    truth = PLANE_N @ (KINV.astype(np.float64) @ np.stack([cols.ravel(), rows.ravel(), np.ones(cols.size)])) / PLANE_D
    ok = ~np.isnan(runs[3]["fused"]).ravel()
    assert np.abs(runs[3]["fused"].ravel()[ok] / truth[ok] - 1).max() < REL_TOL


# ---- the C-ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stage(built):
    import flame_amd

    return flame_amd.load_library()


def test_new_symbols_are_declared_and_exported_and_the_abi_version_stays(stage):
    import flame_amd
    from flame_amd.regularizer import ABI_SYMBOLS, FUSE_SOURCES, KEPT_MESHES

    text = open(os.path.join(ROOT, "include", "flame_nltgv2.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", header), n
        assert n in ABI_SYMBOLS and hasattr(stage, n), n
    assert re.search(r"#define FLAME_NLTGV2_ABI_VERSION 7\b", header) and stage.flame_nltgv2_abi_version() == 7
    assert re.search(r"#define FLAME_NLTGV2_KEPT_MESHES %d\b" % KEPT_MESHES, header) and KEPT_MESHES == 16
    assert re.search(r"#define FLAME_NLTGV2_FUSE_SOURCES %d\b" % FUSE_SOURCES, header) and FUSE_SOURCES == fr.SOURCES == 8
    for name in ("keep_mesh", "keep_mesh_arrays", "drop_mesh", "kept_mesh_info", "get_kept_mesh", "fuse_views_begin", "fuse_views_end", "fuse_views"):
        assert callable(getattr(flame_amd.Regularizer, name))
    p = flame_amd.FuseParams(sources=[flame_amd.FuseSource(slot=3, Kinv_src=np.arange(9), R=np.arange(9), t=np.arange(3), weight=2, graph_scale=3,
                                                           validity=2)] * 8, K_dst=np.arange(9), near_depth=3.0, rel_tol=0.5, min_support=4,
                             want_fused=False, want_masks=False, want_spread=False, want_layers=True, copy_out=False)
    assert p.n_sources == 8 and p.sources[7].slot == 3
    stage.flame_nltgv2_default_fuse_params(C.byref(p))
    d = flame_amd.FuseParams()
    assert bytes(p) == bytes(d)
    assert (p.n_sources, p.min_support, p.want_fused, p.want_masks, p.want_spread, p.want_layers, p.copy_out) == (1, 1, 1, 1, 1, 0, 1)
    assert list(p.K_dst) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and p.rel_tol == F(0.05) and p.near_depth == 0.0
    for s in p.sources:
        assert (s.slot, s.validity, s.graph_scale, s.weight) == (-1, 0, 1.0, 1.0) and list(s.R) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(s.t) == [0, 0, 0]


def test_new_declarations_compile_as_c_and_cpp_with_the_mirrors_sizes(stage, tmp_path):
    import flame_amd
    from flame_amd.regularizer import _FuseOutputsView

    sizes = (C.sizeof(flame_amd.FuseSource), C.sizeof(flame_amd.FuseParams), C.sizeof(flame_amd.FuseCounts), C.sizeof(_FuseOutputsView))
    assert sizes == (100, 872, 128, 224)
    src = tmp_path / "t.c"
    src.write_text(
        '#include <stddef.h>\n#include "flame_nltgv2.h"\n'
        "typedef int (*keep_fn)(flame_nltgv2_ctx*, int32_t, float, int32_t);\n"
        "typedef int (*keep_arrays_fn)(flame_nltgv2_ctx*, int32_t, const int32_t*, int32_t, const float*, const float*, int32_t, const uint8_t*);\n"
        "typedef int (*drop_fn)(flame_nltgv2_ctx*, int32_t);\n"
        "typedef int (*info_fn)(flame_nltgv2_ctx*, int32_t, int32_t*, int32_t*, int32_t*);\n"
        "typedef int (*get_fn)(flame_nltgv2_ctx*, int32_t, float*, float*, int32_t*, uint8_t*);\n"
        "typedef int (*begin_fn)(flame_nltgv2_ctx*, const flame_nltgv2_fuse_params*, int, int);\n"
        "typedef int (*end_fn)(flame_nltgv2_ctx*, flame_nltgv2_fuse_outputs_view*);\n"
        "typedef int (*sync_fn)(flame_nltgv2_ctx*, const flame_nltgv2_fuse_params*, int, int, float*, uint8_t*, uint8_t*, float*, float*,"
        " flame_nltgv2_fuse_counts*);\n"
        "int main(void) {\n"
        "  keep_fn k = flame_nltgv2_keep_mesh; keep_arrays_fn ka = flame_nltgv2_keep_mesh_arrays; drop_fn d = flame_nltgv2_drop_mesh;\n"
        "  info_fn i = flame_nltgv2_kept_mesh_info; get_fn g = flame_nltgv2_get_kept_mesh;\n"
        "  begin_fn b = flame_nltgv2_fuse_views_begin; end_fn e = flame_nltgv2_fuse_views_end; sync_fn s = flame_nltgv2_fuse_views;\n"
        "  flame_nltgv2_fuse_params p; flame_nltgv2_default_fuse_params(&p);\n"
        "  (void)k; (void)ka; (void)d; (void)i; (void)g; (void)b; (void)e; (void)s;\n"
        f"  return (sizeof(flame_nltgv2_fuse_source) == {sizes[0]} && sizeof(flame_nltgv2_fuse_params) == {sizes[1]} &&"
        f" sizeof(flame_nltgv2_fuse_counts) == {sizes[2]} && sizeof(flame_nltgv2_fuse_outputs_view) == {sizes[3]} &&"
        f" offsetof(flame_nltgv2_fuse_source, Kinv_src) == {flame_amd.FuseSource.Kinv_src.offset} &&"
        f" offsetof(flame_nltgv2_fuse_params, K_dst) == {flame_amd.FuseParams.K_dst.offset} &&"
        f" offsetof(flame_nltgv2_fuse_params, copy_out) == {flame_amd.FuseParams.copy_out.offset} &&"
        f" offsetof(flame_nltgv2_fuse_counts, tris_drawn) == {flame_amd.FuseCounts.tris_drawn.offset} &&"
        f" offsetof(flame_nltgv2_fuse_outputs_view, counts) == {_FuseOutputsView.counts.offset} &&"
        f" offsetof(flame_nltgv2_fuse_outputs_view, layers_device) == {_FuseOutputsView.layers_device.offset} &&"
        " p.sources[7].R[4] == 1.0f && p.sources[7].slot == -1 && p.want_fused == 1 && p.min_support == 1 &&"
        " FLAME_NLTGV2_KEPT_MESHES == 16 && FLAME_NLTGV2_FUSE_SOURCES == 8 && FLAME_NLTGV2_ABI_VERSION == 7) ? 0 : 1;\n"
        "}\n")
    lib_dir = os.path.join(ROOT, "flame_amd")
    link = ["-L", lib_dir, "-lflame_nltgv2_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"]
    inc = ["-I", os.path.join(ROOT, "include")]
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", *inc, str(src), "-o", str(tmp_path / "t_c"), *link])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-x", "c++", *inc, str(src), "-o", str(tmp_path / "t_cpp"), *link])
    assert subprocess.run([str(tmp_path / "t_c")], timeout=60).returncode == 0
    assert subprocess.run([str(tmp_path / "t_cpp")], timeout=60).returncode == 0


def test_fuse_layout_under_the_sanitizers(tmp_path):
    """tests/cpp/fuse_layout_test.cc: a stand-alone program that walks the layout function; nothing is loaded into Python."""
    exe = str(tmp_path / "fuse_layout_test")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "flame_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "fuse_layout_test.cc"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "layouts walked, 0 violations" in r.stdout, r.stdout + r.stderr
