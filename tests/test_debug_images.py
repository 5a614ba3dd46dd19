"""The debug images on the device (flame_nltgv2_debug_images*: drawInverseDepthMap, w1_map_ / w2_map_, drawNormals;
flame_stereo_draw_features: drawFeatures): the CPU part.  Known answers that pin the checker tests/debug_ref.py by hand, the
mirror's defaults, a compile check of the new declarations, and the scene of the GPU tests with the conditions they rely on
(70 x 50 pixels -- no multiple of 4 or 64 --, a mesh of 42 vertices from flame_delaunay_triangulate, x, w1 and w2 chosen).

The GPU part is tests/test_gpu_debug_images.py (with _cpp and _pipeline beside it): files that are collected after
tests/test_frames_*.py, like tests/test_gpu_parity.py.  Those tests time the result gather beside the solver in child processes, and
a pytest process that has created a solver context before them -- created and closed is enough -- makes that measurement fail
(gather tax 2.5 instead of < 0.2 with 8 and 4 hardware queues); so no test that creates one may be collected before them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from flame_amd import synth
from oracle import capi as oracle
from tests import debug_ref as dr
from tests import mesh_ref as mr
from tests.conftest import ROOT

F = np.float32
ROWS, COLS = 50, 70


def camera(fx=525.0, fy=520.0, cx=34.5, cy=25.25):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F)


# ---- CPU: known answers for the checker ------------------------------------------------------------------------------------------
def test_checker_jet_known_answers():
    want = {0.0: (255, 0, 0), 0.5: (255, 255, 0), 1.0: (0, 255, 0), 1.5: (0, 255, 255), 2.0: (0, 0, 255)}
    for v, c in want.items():
        assert tuple(dr.jet(v, 0, 2)[0]) == c, v
    # below 0 and above 2 clamp to the ends
    for v in (-1e-6, -3.0, -np.inf):
        assert tuple(dr.jet(v, 0, 2)[0]) == want[0.0], v
    for v in (2.0000002, 7.0, np.inf):
        assert tuple(dr.jet(v, 0, 2)[0]) == want[2.0], v
    # inside the branches: 255 * (4 v / 2) etc., truncated
    assert tuple(dr.jet(0.25, 0, 2)[0]) == (255, 127, 0)      # 255 * 0.5 = 127.5
    assert tuple(dr.jet(0.75, 0, 2)[0]) == (127, 255, 0)      # 255 * (1 + 4 (0.5 - 0.75) / 2) = 127.5
    assert tuple(dr.jet(1.25, 0, 2)[0]) == (0, 255, 127)
    assert tuple(dr.jet(1.75, 0, 2)[0]) == (0, 127, 255)
    assert tuple(dr.jet(np.nan, 0, 2)[0]) == (0, 0, 255)      # the library's (unpinned) colour for a NaN
    assert dr.jet(np.zeros((3, 4), F)).shape == (3, 4, 3)


def test_checker_normal_map_known_answers():
    assert tuple(dr.normal_map(0, 0, 1)[0]) == (254, 127, 127)
    assert tuple(dr.normal_map(1, -1, 0)[0]) == (127, 0, 255)
    assert tuple(dr.normal_map(-1, 1, 0.5)[0]) == (190, 255, 0)


def flat_scene(idepth=0.5):
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (ROWS, COLS), dtype=np.uint8)
    m = np.full((ROWS, COLS), idepth, F)
    m[:3] = np.nan  # uncovered rows
    return img, m


def test_checker_fronto_parallel_case_is_all_grey_in_the_normals_image():
    """w = 0: a = 0, b = idepth^2, the normal is (0, 0, 1) before the negation, so nz < 0 and nothing is painted; the idepth image is
    jet(idepth) where the map is covered and grey elsewhere."""
    img, m = flat_scene()
    K = camera()
    z = np.zeros_like(m)
    z[:3] = np.nan
    n = dr.plane_param_to_normal(K, 3.0, 4.0, F(0.5), F(0), F(0))
    assert [float(c) for c in n] == [0.0, 0.0, -1.0]
    grey = np.repeat(img[:, :, None], 3, axis=2)
    assert np.array_equal(dr.draw_normals(img, K, m, z, z), grey)
    idm = dr.draw_inverse_depth_map(img, m, scene_color_scale=1.0)
    assert np.array_equal(idm[:3], grey[:3]) and (idm[3:] == np.array([255, 255, 0], np.uint8)).all()
    assert (dr.draw_inverse_depth_map(img, m, scene_color_scale=2.0)[3:] == np.array([0, 255, 0], np.uint8)).all()
    # flip: reversed linear pixel order
    f = dr.draw_inverse_depth_map(img, m, flip=True)
    assert np.array_equal(f.reshape(-1, 3), idm.reshape(-1, 3)[::-1]) and np.array_equal(f[-3:, ::-1], grey[:3][::-1])


def test_checker_normals_are_painted_where_a_exceeds_the_idepth():
    """w1 = -0.004 at u = (25, 10) with fx = 525: a = w1 (25 - 525) = 2 > idepth 0.5, so nz = -(idepth - a) d > 0 and the pixel is
    painted with normalMap of the unit normal; by hand in float64."""
    K = camera()
    w1, w2, idepth = F(-0.004), F(0.0), F(0.5)
    a = float(F(F(w1 * F(25.0)) - F(w1 * F(525.0))))
    assert abs(a - 2.0) < 1e-5
    n = dr.plane_param_to_normal(K, 25.0, 10.0, idepth, w1, w2)
    v = np.array([525.0 * float(w1), 0.0, 0.5 - a])
    v = -v / np.linalg.norm(v)
    assert np.allclose([float(c) for c in n], v, atol=1e-6) and n[2] > 0
    img, m = flat_scene()
    w1m = np.full_like(m, w1)
    painted, _ = dr.normals_painted(K, m, w1m, np.zeros_like(m))
    assert painted[3:].all() and not painted[:3].any()  # (the NaN rows of the map stay grey)
    out = dr.draw_normals(img, K, m, w1m, np.zeros_like(m))
    assert tuple(out[10, 25]) == tuple(dr.normal_map(n[0], n[1], n[2])[0]) and np.array_equal(out[0, 0], [img[0, 0]] * 3)
    # a NaN w leaves the grey pixel
    w1m[20, 30] = np.nan
    assert np.array_equal(dr.draw_normals(img, K, m, w1m, np.zeros_like(m))[20, 30], [img[20, 30]] * 3)


def test_checker_draw_features_fill_order_clipping_and_counters():
    from flame_amd.stereo import FEATURE_DTYPE

    img = np.full((ROWS, COLS), 9, np.uint8)
    f = np.zeros(4, FEATURE_DTYPE)
    f["x"], f["y"] = [10.4, 12.6, 0.2, 40.0], [10.5, 11.0, 49.4, 20.0]
    f["idepth_mu"] = [0.0, 1.0, 2.0, 0.5]
    f["idepth_var"] = [0.1, 0.1, 0.1, 0.2]
    out, nc, nu = dr.draw_features(img, f, 0.2)
    assert (nc, nu) == (3, 1)
    assert tuple(out[11, 10]) == (255, 0, 0) and tuple(out[11, 11]) == (0, 255, 0)  # (10, 11) + (13, 11): the later feature on top
    assert tuple(out[49, 0]) == (0, 0, 255) and tuple(out[47, 2]) == (0, 0, 255) and tuple(out[46, 2]) == (9, 9, 9)
    assert tuple(out[20, 40]) == (9, 9, 9)  # var == threshold: not drawn
    assert (out != 9).any(axis=2).sum() == 25 + 25 - 10 + 9


def test_mirror_exposes_the_debug_images_with_the_reference_defaults(built):
    import flame_amd
    from flame_amd.regularizer import ABI_SYMBOLS
    from flame_amd.stereo import STEREO_ABI_SYMBOLS, FeatureTracker

    for name in ("debug_images", "debug_images_begin", "debug_images_end"):
        assert callable(getattr(flame_amd.Regularizer, name))
        assert "flame_nltgv2_" + name in ABI_SYMBOLS
    for name in ("draw_features", "frame_image_device"):
        assert callable(getattr(FeatureTracker, name))
        assert "flame_stereo_" + name in STEREO_ABI_SYMBOLS
    p = flame_amd.DebugImageParams()
    c = flame_amd.DebugImageParams(0, 1, 0, 0)
    flame_amd.load_library().flame_nltgv2_default_debug_image_params(C.byref(c))
    for q in (p, c):
        assert [getattr(q, n) for n, _ in flame_amd.DebugImageParams._fields_] == [F(1.0), 0, 1, 1]
    assert flame_amd.load_library().flame_nltgv2_abi_version() == 7  # (additive entry points)


def test_new_declarations_compile_as_c_and_cpp_with_the_mirrors_sizes(built, tmp_path):
    import flame_amd
    from flame_amd.regularizer import _DebugImagesView

    src = tmp_path / "t.c"
    src.write_text(
        '#include "flame_nltgv2.h"\n#include "flame_stereo.h"\n'
        "typedef int (*begin_fn)(flame_nltgv2_ctx*, const uint8_t*, const void*, int, const float*, const flame_nltgv2_debug_image_params*, int, int);\n"
        "typedef int (*end_fn)(flame_nltgv2_ctx*, flame_nltgv2_debug_images_view*);\n"
        "typedef int (*sync_fn)(flame_nltgv2_ctx*, const uint8_t*, const void*, int, const float*, const flame_nltgv2_debug_image_params*, int, int,"
        " uint8_t*, uint8_t*, float*, float*);\n"
        "typedef int (*draw_fn)(flame_stereo_ctx*, uint32_t, float, float, int, uint8_t*, int32_t*, int32_t*);\n"
        "typedef int (*img_fn)(flame_stereo_ctx*, uint32_t, const void**, int*);\n"
        "int main(void) {\n"
        "  begin_fn b = flame_nltgv2_debug_images_begin; end_fn e = flame_nltgv2_debug_images_end; sync_fn s = flame_nltgv2_debug_images;\n"
        "  draw_fn d = flame_stereo_draw_features; img_fn i = flame_stereo_frame_image_device;\n"
        "  flame_nltgv2_debug_image_params p; flame_nltgv2_default_debug_image_params(&p);\n"
        "  (void)b; (void)e; (void)s; (void)d; (void)i;\n"
        f"  return (sizeof(flame_nltgv2_debug_image_params) == {C.sizeof(flame_amd.DebugImageParams)} &&"
        f" sizeof(flame_nltgv2_debug_images_view) == {C.sizeof(_DebugImagesView)} && p.want_normals == 1 && FLAME_NLTGV2_ABI_VERSION == 7) ? 0 : 1;\n"
        "}\n")
    lib_dir = os.path.join(ROOT, "flame_amd")
    link = ["-L", lib_dir, "-lflame_nltgv2_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"]
    inc = ["-I", os.path.join(ROOT, "include")]
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", *inc, str(src), "-o", str(tmp_path / "t_c"), *link])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-x", "c++", *inc, str(src), "-o", str(tmp_path / "t_cpp"), *link])
    assert subprocess.run([str(tmp_path / "t_c")], timeout=60).returncode == 0
    assert subprocess.run([str(tmp_path / "t_cpp")], timeout=60).returncode == 0


# ---- the scene of the GPU tests (built on the CPU, once) -------------------------------------------------------------------------
GRAPH_SCALE, COLOR_SCALE = 0.25, 2.0  # x * 0.25 * 2: exact in float, so x = 2 v puts v on the jet's breakpoints


@pytest.fixture(scope="module")
def scene(built):
    """42 vertices at integer pixels inside the image (rows and columns at its rim stay uncovered), triangulated by the library's
    host triangulator; x, w1, w2 chosen; a grey image inside a wider buffer (step_bytes 96 > cols)."""
    import flame_amd

    rng = np.random.default_rng(17)
    gx, gy = np.meshgrid(np.arange(7), np.arange(6))
    pos = np.stack([5 + 9 * gx.ravel() + rng.integers(0, 5, 42), 4 + 8 * gy.ravel() + rng.integers(0, 4, 42)], axis=1).astype(F)
    tris, edges = flame_amd.delaunay(pos)
    V = len(pos)
    x = (rng.random(V) * 5.5 - 0.5).astype(F)  # x / 2 in [-0.25, 2.5]: below 0, the four branches, above 2
    x[[8, 9, 10, 11, 12]] = F([0.0, 1.0, 2.0, 3.0, 4.0])  # the map AT these vertices' pixels: exactly 0, 0.5, 1, 1.5, 2 after the scales
    x[13], x[14] = F(-1.0), F(4.5)
    g = synth.assemble_graph(pos, x, edges)
    g["w1"] = ((rng.random(V) - 0.5) * 0.012).astype(F)  # around +-0.006: a = w1 (u - 525) + w2 (v - 520) crosses the idepths
    g["w2"] = ((rng.random(V) - 0.5) * 0.012).astype(F)
    buf = rng.integers(0, 256, (ROWS, 96), dtype=np.uint8)
    img = buf[:, 7:7 + COLS]
    K = camera()
    idepth = mr.vertex_idepths(x, GRAPH_SCALE)
    dense = oracle.raster_interpolate_mesh(tris, pos, idepth, ROWS, COLS)
    w1m = oracle.raster_interpolate_mesh(tris, pos, g["w1"], ROWS, COLS)
    w2m = oracle.raster_interpolate_mesh(tris, pos, g["w2"], ROWS, COLS)
    return dict(g=g, pos=pos, tris=np.ascontiguousarray(tris, np.int32), edges=edges, buf=buf, img=img, K=K, dense=dense, w1m=w1m, w2m=w2m)


def test_scene_meets_the_conditions_the_gpu_tests_rely_on(scene):
    s = scene
    dense, tris, pos = s["dense"], s["tris"], s["pos"]
    covered = ~np.isnan(dense)
    assert 0.5 < covered.mean() < 0.95 and len(pos) == 42 and len(tris) > 50  # uncovered pixels are present
    v = (dense[covered] * F(COLOR_SCALE)).astype(F)
    for exact in (0.0, 0.5, 1.0, 1.5, 2.0):
        assert (v == F(exact)).any(), exact
    assert (v < 0).any() and (v > 2).any()
    for lo, hi in ((0, 0.5), (0.5, 1.0), (1.0, 1.5), (1.5, 2.0)):
        assert ((v > lo) & (v < hi)).sum() > 20, (lo, hi)
    # the normals image: at least 10 % of the covered pixels painted and at least 10 % not
    painted, _ = dr.normals_painted(s["K"], dense, s["w1m"], s["w2m"])
    frac = painted[covered].mean()
    assert 0.1 <= frac <= 0.9, frac
    assert not painted[~covered].any()
    # the triangles overlap on shared edges: pixels that more than one triangle draws
    count = np.zeros((ROWS, COLS), int)
    for t in range(len(tris)):
        one = np.zeros(len(tris), np.uint8)
        one[t] = 1
        count += ~np.isnan(oracle.raster_interpolate_mesh(tris, pos, np.ones(len(pos), F), ROWS, COLS, tri_valid=one))
    assert (count > 1).sum() > 100 and np.array_equal(count > 0, covered)


# ---- helpers of the GPU tests (tests/test_gpu_debug_images*.py) ------------------------------------------------------------------
def first_difference(got, ref):
    bad = np.argwhere((got != ref).any(axis=2))
    return f"{len(bad)} pixels differ, first {bad[:4].tolist()}: {[got[tuple(b)].tolist() for b in bad[:4]]} vs {[ref[tuple(b)].tolist() for b in bad[:4]]}"


def assert_image(got, ref, what):
    assert got.shape == ref.shape and got.dtype == np.uint8, what
    assert np.array_equal(got, ref), what + ": " + first_difference(got, ref)


def feature_set():
    from flame_amd.stereo import FEATURE_DTYPE

    rng = np.random.default_rng(23)
    n = 64
    f = np.zeros(n, FEATURE_DTYPE)
    f["id"] = np.arange(n) + 100
    f["frame_id"] = 10
    f["x"] = (rng.random(n) * 60 + 5).astype(F)
    f["y"] = (rng.random(n) * 40 + 5).astype(F)
    f["idepth_mu"] = (rng.random(n) * 2.4 + 0.05).astype(F)
    f["idepth_var"] = (rng.random(n) * 0.015 + 0.002).astype(F)
    f["valid"] = 1
    # rectangles cut by the four borders, and a cluster of overlapping ones
    f["x"][:4], f["y"][:4] = [1.2, 68.4, 30.0, 31.0], [25.0, 26.0, 1.3, 48.2]
    f["x"][4:8], f["y"][4:8] = [20.0, 21.4, 22.6, 20.5], [20.0, 21.0, 20.4, 22.5]
    f["idepth_var"][:8] = 0.001
    # sixteen consecutive floats as variances of features that share position and idepth (projectFeatures scales a variance by
    # (idepth_cur / idepth_ref)^4, the same factor for all of them): the projected set then holds a value with both its
    # neighbours, which becomes the threshold; and a NaN
    f["x"][8:24], f["y"][8:24], f["idepth_mu"][8:24] = 40.3, 30.2, 0.8
    f["idepth_var"][8:24] = F(0.01) + np.arange(16, dtype=F) * np.spacing(F(0.01))
    f["idepth_var"][24] = np.nan
    return f
