"""The view renderer (include/flame_nltgv2.h, flame_nltgv2_render_view_begin): known answers for the checker tests/view_ref.py -- a
plane, the identity view, a box in front of a plane, ties, and one triangle per rule on an 8x8 target -- and the new symbols and
structs of the C-ABI.  No GPU here; the device is compared with the checker in tests/test_gpu_render_view*.py, which draw the same
cases (one_triangle_cases, grid_mesh, box_scene)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import view_ref as vr
from tests.conftest import ROOT

F = np.float32
EYE = np.eye(3, dtype=F)
NAMES = ("flame_nltgv2_default_view_params", "flame_nltgv2_render_view_begin", "flame_nltgv2_render_view_end", "flame_nltgv2_render_view",
         "flame_nltgv2_render_view_arrays")


@pytest.fixture(scope="module")
def stage(built):
    import flame_amd

    return flame_amd.load_library()


def camera(f, cx, cy):
    K = np.array([[f, 0, cx], [0, f, cy], [0, 0, 1]], F)
    Kinv = np.array([[1 / f, 0, -cx / f], [0, 1 / f, -cy / f], [0, 0, 1]], F)
    return K, Kinv


def rotation_y(degrees):
    a = np.deg2rad(degrees)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], F)


def grid_mesh(rows, cols, step, seed, jitter=1.5):
    """A jittered grid over rows x cols, two triangles per cell -> (pos (V, 2) f32, tris (T, 3) i32)."""
    rng = np.random.default_rng(seed)
    ny, nx = (rows - 1) // step + 1, (cols - 1) // step + 1
    jj, ii = np.meshgrid(np.arange(nx), np.arange(ny))
    pos = np.stack([jj.ravel() * step, ii.ravel() * step], 1).astype(F)
    pos += rng.uniform(-jitter, jitter, pos.shape).astype(F)
    tris = []
    for i in range(ny - 1):
        for j in range(nx - 1):
            v = i * nx + j
            tris += [(v, v + 1, v + nx), (v + 1, v + nx + 1, v + nx)]
    return pos, np.array(tris, np.int32)


def box_scene():
    """A near box (id 1) in front of a far plane (id 0.25) on a jittered 6-pixel grid, 64x48, seen after t = (0.5, 0, 0)."""
    K, Kinv = camera(60.0, 32.0, 24.0)
    pos, tris = grid_mesh(48, 64, 6, seed=5)
    near = (np.abs(pos[:, 0] - 32) < 10) & (np.abs(pos[:, 1] - 24) < 8)
    idepth = np.where(near, F(1.0), F(0.25)).astype(F)
    return dict(tris=tris, pos=pos, idepth=idepth, Kinv_src=Kinv, K_dst=K, R=EYE, t=np.array([0.5, 0, 0], F), rows=48, cols=64), near


def render(c, **over):
    a = dict(c, **over)
    return vr.render_view(a["tris"], a["pos"], a["idepth"], a.get("Kinv_src", EYE), a.get("K_dst", EYE), a.get("R", EYE), a.get("t", np.zeros(3, F)),
                          a.get("rows", 8), a.get("cols", 8), a.get("near_depth", 0.0), a.get("tri_valid"))


def one_triangle_cases():
    """One triangle per rule on an 8x8 target, with the identity camera unless the case says otherwise (id = 1: P = (x, y, 1), so the
    target position is the source position exactly).  expect: (coverage, drawn, culled_vertex, culled_facing)."""
    tri = np.array([[0, 1, 2]], np.int32)
    one = np.ones(3, F)
    base = np.array([[1, 1], [5, 1], [1, 5]], F)

    def case(name, pos, idepth=one, expect=None, **cam):
        return dict(name=name, tris=tri, pos=np.array(pos, F), idepth=np.array(idepth, F), expect=expect, **cam)

    return [
        case("vertices_on_pixel_centres", base, expect=(15, 1, 0, 0)),
        # 16 * 2.03125 = 32.5 -> 32 and 16 * 2.09375 = 33.5 -> 34: the first edge lies on column 2, the second right of it
        case("tie_rounds_to_even_down", [[2.03125, 1], [5, 1], [2.03125, 4]], expect=(4 + 3 + 2 + 1, 1, 0, 0)),
        case("tie_rounds_to_even_up", [[2.09375, 1], [5, 1], [2.09375, 4]], expect=(3 + 2 + 1 + 0, 1, 0, 0)),
        case("zero_area_in_both_views", [[1, 1], [3, 3], [5, 5]], expect=(0, 0, 0, 1)),
        case("zero_area_in_the_target_view", base, K_dst=np.array([[1, 0, 0], [1, 0, 0], [0, 0, 1]], F), expect=(0, 0, 0, 1)),
        case("flipped_orientation", base, K_dst=np.array([[-1, 0, 7], [0, 1, 0], [0, 0, 1]], F), expect=(0, 0, 0, 1)),
        case("idepth_zero", base, idepth=[1, 0, 1], expect=(0, 0, 1, 0)),
        case("idepth_negative", base, idepth=[1, 1, -1], expect=(0, 0, 1, 0)),
        case("idepth_nan", base, idepth=[np.nan, 1, 1], expect=(0, 0, 1, 0)),
        case("depth_at_near_depth", base, near_depth=1.0, expect=(0, 0, 1, 0)),
        case("depth_beyond_near_depth", base, near_depth=0.5, expect=(15, 1, 0, 0)),
        case("vertex_on_the_coordinate_bound", [[1, 1], [65536, 1], [1, 5]], expect=None),
        case("vertex_past_the_coordinate_bound", [[1, 1], [65537, 1], [1, 5]], expect=(0, 0, 1, 0)),
        case("source_past_the_bound_target_within", [[1, 1], [65537, 1], [1, 5]], K_dst=np.diag([0.5, 0.5, 1]).astype(F), expect=(0, 0, 1, 0)),
        case("wholly_outside", [[10, 10], [14, 10], [10, 14]], expect=(0, 1, 0, 0)),
        case("half_outside", [[4, 4], [12, 4], [4, 12]], expect=(16, 1, 0, 0)),
        case("whole_target", [[-20, -20], [40, -20], [-20, 40]], idepth=[0.5, 1, 2], expect=(64, 1, 0, 0)),
    ]


def counts(r):
    return tuple(r[k] for k in vr.COUNT_KEYS)


# ---- known answers ---------------------------------------------------------------------------------------------------------------
def test_a_plane_seen_after_a_sideways_translation_renders_its_idepth_exactly():
    K, Kinv = camera(60.0, 32.0, 24.0)
    pos, tris = grid_mesh(48, 64, 6, seed=3)
    r = vr.render_view(tris, pos, np.full(len(pos), 0.5, F), Kinv, K, EYE, np.array([0.5, 0, 0], F), 48, 64)
    covered = r["tri_index"] >= 0
    assert r["coverage"] == covered.sum() > 1500 and r["tris_drawn"] == len(tris)
    assert (vr.bits(r["map"])[covered] == vr.bits(F(0.5))).all()
    assert (vr.bits(r["map"])[~covered] == vr.HOLE).all()


def test_the_identity_view_draws_every_triangle_and_culls_none():
    K, Kinv = camera(60.0, 32.0, 24.0)
    pos, tris = grid_mesh(48, 64, 6, seed=4)
    idepth = np.random.default_rng(4).uniform(0.2, 2.0, len(pos)).astype(F)
    r = vr.render_view(tris, pos, idepth, Kinv, K, EYE, np.zeros(3, F), 48, 64)
    assert (r["tris_drawn"], r["tris_culled_vertex"], r["tris_culled_facing"]) == (len(tris), 0, 0)
    m = r["map"][r["tri_index"] >= 0]
    assert idepth.min() * F(0.999) <= m.min() and m.max() <= idepth.max() * F(1.001)


def test_a_near_box_occludes_the_far_plane_and_its_flanks_are_culled():
    c, near = box_scene()
    tris = c["tris"]
    full = render(c)
    assert full["tris_culled_facing"] > 0 and full["tris_culled_vertex"] == 0
    assert full["tris_drawn"] + full["tris_culled_facing"] == len(tris)
    n_near = near[tris].sum(1)
    layers = [render(c, tri_valid=(n_near == 3)), render(c, tri_valid=(n_near == 0)), render(c, tri_valid=(n_near % 3 != 0))]
    front, back = layers[0], layers[1]
    both = (front["tri_index"] >= 0) & (back["tri_index"] >= 0)
    assert both.sum() > 50
    # where both layers cover a pixel the near one owns it, unless a flank drawn between them is nearer still
    owner_near = n_near[full["tri_index"][both]]
    assert (owner_near > 0).all() and (full["map"][both] >= front["map"][both]).all() and (front["map"][both] > back["map"][both]).all()
    # the depth test is a maximum: the full picture is the per-pixel maximum of the three layers
    stack = np.stack([np.where(np.isnan(l["map"]), F(0), l["map"]) for l in layers])
    want = stack.max(0)
    assert (np.where(np.isnan(full["map"]), F(0), full["map"]) == want).all()


def test_bit_equal_values_give_the_larger_triangle_index():
    K, Kinv = camera(60.0, 32.0, 24.0)
    pos, tris = grid_mesh(48, 64, 6, seed=3)
    twice = np.concatenate([tris, tris])
    r = vr.render_view(twice, pos, np.full(len(pos), 0.5, F), Kinv, K, EYE, np.zeros(3, F), 48, 64)
    covered = r["tri_index"] >= 0
    assert covered.sum() > 1500 and (r["tri_index"][covered] >= len(tris)).all()
    # a shared edge of the plane: both triangles give 0.5 there, the later one of the list owns it
    pos, tris = grid_mesh(48, 64, 6, seed=3, jitter=0.0)  # (edges through pixel centres)
    once = vr.render_view(tris, pos, np.full(len(pos), 0.5, F), EYE, EYE, EYE, np.zeros(3, F), 48, 64)
    rev = vr.render_view(tris[::-1], pos, np.full(len(pos), 0.5, F), EYE, EYE, EYE, np.zeros(3, F), 48, 64)
    shared = (once["tri_index"] >= 0) & (once["tri_index"] != len(tris) - 1 - rev["tri_index"])
    assert shared.sum() > 300 and (once["tri_index"][shared] > len(tris) - 1 - rev["tri_index"][shared]).all()


@pytest.mark.parametrize("case", one_triangle_cases(), ids=lambda c: c["name"])
def test_one_triangle_per_rule(case):
    r = render(case)
    if case["expect"] is not None:
        assert counts(r) == case["expect"], (case["name"], counts(r))
    assert r["coverage"] == (r["tri_index"] == 0).sum() == (~np.isnan(r["map"])).sum()


def test_one_triangle_details():
    cases = {c["name"]: c for c in one_triangle_cases()}
    r = render(cases["vertices_on_pixel_centres"])
    want = np.zeros((8, 8), bool)
    for row in range(1, 6):
        want[row, 1:7 - row] = True  # the corners (1, 1), (5, 1), (1, 5) and the hypotenuse col + row == 6 included
    assert ((r["tri_index"] == 0) == want).all() and (vr.bits(r["map"])[want] == vr.bits(F(1.0))).all()
    assert vr.transform_vertex((2.03125, 1), 1, EYE, EYE, EYE, np.zeros(3), 0)[1:5] == (32, 16, 32, 16)
    assert vr.transform_vertex((2.09375, 1), 1, EYE, EYE, EYE, np.zeros(3), 0)[1:5] == (34, 16, 34, 16)
    assert (render(cases["tie_rounds_to_even_down"])["tri_index"][1:5, 2] == 0).all()
    assert (render(cases["tie_rounds_to_even_up"])["tri_index"][:, 2] == -1).all()
    assert render(cases["vertex_on_the_coordinate_bound"])["tris_drawn"] == 1
    r = render(cases["whole_target"])
    # id' interpolates linearly on the target: 0.5 + 0.5 (col + 20) / 60 + 1.5 (row + 20) / 60
    cols, rows = np.meshgrid(np.arange(8), np.arange(8))
    assert np.allclose(r["map"], 0.5 + 0.5 * (cols + 20) / 60 + 1.5 * (rows + 20) / 60, rtol=1e-6)


def test_a_rotated_and_rescaled_camera_sees_the_plane_where_geometry_puts_it():
    """The checker against float64 geometry: a fronto-parallel plane at depth 2 through a camera turned by 20 degrees with other
    intrinsics and a larger target; every covered pixel's inverse depth is that of the plane along the pixel's ray."""
    K, Kinv = camera(60.0, 32.0, 24.0)
    K2, K2inv = camera(90.0, 50.0, 37.5)
    R, t = rotation_y(20.0), np.array([-0.6, 0.05, 0.1], F)
    pos, tris = grid_mesh(48, 64, 6, seed=6)
    r = vr.render_view(tris, pos, np.full(len(pos), 0.5, F), Kinv, K2, R, t, 75, 100)
    assert r["coverage"] > 1000 and r["tris_culled_facing"] == 0
    # the plane z = 2 of the source, n . P = 2 with n = (0, 0, 1), is (R n) . (P' - t) = 2 in the target
    n = R.astype(np.float64) @ np.array([0, 0, 1.0])
    rows, cols = np.nonzero(r["tri_index"] >= 0)
    rays = K2inv.astype(np.float64) @ np.stack([cols, rows, np.ones(len(cols))])
    z = (2.0 + n @ t.astype(np.float64)) / (n @ rays)
    # vertices are snapped to 1/16 pixel: the plane moves by a fraction of that times the depth gradient
    assert np.abs(r["map"][rows, cols] * z - 1).max() < 2e-3


# ---- the C-ABI -------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported_and_the_abi_version_stays(stage):
    import flame_amd
    from flame_amd.regularizer import ABI_SYMBOLS

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flame_nltgv2.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", header), n
        assert n in ABI_SYMBOLS and hasattr(stage, n), n
    assert re.search(r"#define FLAME_NLTGV2_ABI_VERSION 7\b", header) and stage.flame_nltgv2_abi_version() == 7
    for name in ("render_view", "render_view_begin", "render_view_end", "render_view_arrays"):
        assert callable(getattr(flame_amd.Regularizer, name))
    p = flame_amd.ViewParams(Kinv_src=np.arange(9), K_dst=np.arange(9), R=np.arange(9), t=np.arange(3), near_depth=3.0, validity=2, want_map=False,
                             want_tri_index=False, copy_out=False)
    stage.flame_nltgv2_default_view_params(C.byref(p))
    d = flame_amd.ViewParams()
    for name, typ in flame_amd.ViewParams._fields_:
        a, b = getattr(p, name), getattr(d, name)
        if name in ("Kinv_src", "K_dst", "R", "t"):
            a, b = list(a), list(b)
        assert a == b, name
    assert list(p.R) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(p.t) == [0, 0, 0]
    assert (p.near_depth, p.validity, p.want_map, p.want_tri_index, p.copy_out) == (0.0, 0, 1, 1, 1)


def test_new_declarations_compile_as_c_and_cpp_with_the_mirrors_sizes(stage, tmp_path):
    import flame_amd
    from flame_amd.regularizer import _ViewOutputsView

    sizes = (C.sizeof(flame_amd.ViewParams), C.sizeof(flame_amd.ViewCounts), C.sizeof(_ViewOutputsView))
    assert sizes == (140, 16, 64)
    src = tmp_path / "t.c"
    src.write_text(
        '#include <stddef.h>\n#include "flame_nltgv2.h"\n'
        "typedef int (*begin_fn)(flame_nltgv2_ctx*, const flame_nltgv2_view_params*, const uint8_t*, int, int, float);\n"
        "typedef int (*end_fn)(flame_nltgv2_ctx*, flame_nltgv2_view_outputs_view*);\n"
        "typedef int (*sync_fn)(flame_nltgv2_ctx*, const flame_nltgv2_view_params*, const uint8_t*, int, int, float, float*, int32_t*,"
        " flame_nltgv2_view_counts*);\n"
        "typedef int (*arrays_fn)(flame_nltgv2_ctx*, const flame_nltgv2_view_params*, const int32_t*, int32_t, const float*, const float*, int32_t,"
        " const uint8_t*, int, int, float*, int32_t*, flame_nltgv2_view_counts*);\n"
        "int main(void) {\n"
        "  begin_fn b = flame_nltgv2_render_view_begin; end_fn e = flame_nltgv2_render_view_end; sync_fn s = flame_nltgv2_render_view;\n"
        "  arrays_fn a = flame_nltgv2_render_view_arrays;\n"
        "  flame_nltgv2_view_params p; flame_nltgv2_default_view_params(&p);\n"
        "  (void)b; (void)e; (void)s; (void)a;\n"
        f"  return (sizeof(flame_nltgv2_view_params) == {sizes[0]} && sizeof(flame_nltgv2_view_counts) == {sizes[1]} &&"
        f" sizeof(flame_nltgv2_view_outputs_view) == {sizes[2]} &&"
        f" offsetof(flame_nltgv2_view_params, near_depth) == {flame_amd.ViewParams.near_depth.offset} &&"
        f" offsetof(flame_nltgv2_view_params, copy_out) == {flame_amd.ViewParams.copy_out.offset} &&"
        f" offsetof(flame_nltgv2_view_outputs_view, device_ms) == {_ViewOutputsView.device_ms.offset} &&"
        f" offsetof(flame_nltgv2_view_outputs_view, tri_index_device) == {_ViewOutputsView.tri_index_device.offset} &&"
        " p.R[4] == 1.0f && p.want_map == 1 && p.validity == 0 && FLAME_NLTGV2_ABI_VERSION == 7) ? 0 : 1;\n"
        "}\n")
    lib_dir = os.path.join(ROOT, "flame_amd")
    link = ["-L", lib_dir, "-lflame_nltgv2_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"]
    inc = ["-I", os.path.join(ROOT, "include")]
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", *inc, str(src), "-o", str(tmp_path / "t_c"), *link])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-x", "c++", *inc, str(src), "-o", str(tmp_path / "t_cpp"), *link])
    assert subprocess.run([str(tmp_path / "t_c")], timeout=60).returncode == 0
    assert subprocess.run([str(tmp_path / "t_cpp")], timeout=60).returncode == 0


def test_view_layout_under_the_sanitizers(tmp_path):
    """tests/cpp/view_layout_test.cc: a stand-alone program that walks the layout function; nothing is loaded into Python."""
    exe = str(tmp_path / "view_layout_test")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "flame_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "view_layout_test.cc"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "48 layouts walked, 0 violations" in r.stdout, r.stdout + r.stderr
