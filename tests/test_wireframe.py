"""The wireframe image on the device (flame_nltgv2_debug_wireframe*: drawWireframe, flame.cc:2414-2457): the CPU part.  Known answers
that pin the checker tests/wireframe_ref.py by hand, the mirror's defaults, a compile check of the new declarations, and the cases of
the GPU tests with the conditions they rely on.  No solver context is created here.

The GPU part is tests/test_gpu_wireframe.py (with _cpp and _pipeline beside it): files that are collected after tests/test_frames_*.py
(tests/test_debug_images.py says why)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from flame_amd import synth
from tests import mesh_ref as mr
from tests import wireframe_ref as wr
from tests.conftest import ROOT
from tests.test_debug_images import COLOR_SCALE, COLS, GRAPH_SCALE, ROWS, camera
from tests.test_debug_images import scene  # noqa: F401  (the 70 x 50 scene of the debug image tests, as a fixture)

F = np.float32


# ---- CPU: known answers for the checker ------------------------------------------------------------------------------------------
def test_checker_walk_known_answers():
    want = {
        ((0, 0), (5, 2)): [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)],
        ((0, 0), (2, 1)): [(0, 0), (1, 0), (2, 1)],
        ((2, 1), (0, 0)): [(2, 1), (1, 1), (0, 0)],
        ((0, 0), (1, 3)): [(0, 0), (0, 1), (1, 2), (1, 3)],
        ((4, 0), (0, 1)): [(4, 0), (3, 0), (2, 0), (1, 1), (0, 1)],
        ((3, 3), (3, 3)): [(3, 3)],
    }
    for (a, b), px in want.items():
        assert wr.walk(a, b) == px, (a, b)
    # every walk starts at its first point, ends at its second, has max(|dx|, |dy|) + 1 pixels, none of them twice, all in the box
    rng = np.random.default_rng(4)
    for _ in range(300):
        a, b = tuple(rng.integers(0, 20, 2)), tuple(rng.integers(0, 20, 2))
        px = wr.walk(a, b)
        assert px[0] == a and px[-1] == b and len(px) == max(abs(b[0] - a[0]), abs(b[1] - a[1])) + 1 and len(set(px)) == len(px)
        assert all(min(a[0], b[0]) <= x <= max(a[0], b[0]) and min(a[1], b[1]) <= y <= max(a[1], b[1]) for x, y in px)


def test_checker_rounds_half_to_even():
    assert [wr.cv_round(v) for v in (2.5, 3.5, 0.5, 1.5, -0.5, 2.4999, 2.5001)] == [2, 4, 0, 2, 0, 2, 3]
    assert wr.endpoint((15.5, 0.5), 12, 16) is None  # 15.5 -> 16 = cols
    assert wr.endpoint((14.5, 10.5), 12, 16) == (14, 10) and wr.endpoint((15.4, 11.4), 12, 16) == (15, 11)
    assert wr.endpoint((-0.5, 0), 12, 16) == (0, 0) and wr.endpoint((-0.6, 0), 12, 16) is None
    assert wr.endpoint((np.nan, 0), 12, 16) is None and wr.endpoint((3, np.inf), 12, 16) is None


def test_checker_blend_by_hand():
    """grey 9, then (255, 0, 0) and (0, 255, 0): 255 * 0.5f + 9 * 0.5f = 132, 0 * 0.5f + 9 * 0.5f = 4.5 -> 4, so (132, 4, 4); then
    (66, 129.5 -> 129, 2).  The other order: (4, 132, 4), then (129.5 -> 129, 66, 2)."""
    a, b = (255, 0, 0), (0, 255, 0)
    g = np.array([9, 9, 9])
    assert tuple(wr.blend(g, a)) == (132, 4, 4) and tuple(wr.blend(g, b)) == (4, 132, 4)
    assert tuple(wr.blend(wr.blend(g, a), b)) == (66, 129, 2)
    assert tuple(wr.blend(wr.blend(g, b), a)) == (129, 66, 2)
    for old in range(256):  # the float expression of the reference, truncated, against the shift
        for col in (0, 1, 127, 128, 254, 255):
            assert int(F(F(col) * F(0.5)) + F(F(old) * F(0.5))) == (col + old) >> 1
    # ... and through draw_wireframe: two one-pixel triangles over one pixel, values 0 (jet: (255, 0, 0)) and 1 ((0, 255, 0)); each
    # draws the pixel three times with its colour
    img = np.full((4, 6), 9, np.uint8)
    pos = F([[1, 1]] * 6)
    for order in ((0, 1), (1, 0)):
        tris = np.array([[0, 0, 0], [3, 3, 3]])[list(order)]
        out, nd, ns = wr.draw_wireframe(img, tris, pos, F([0, 0, 0, 1, 1, 1]))
        assert (nd, ns) == (6, 0)
        c = g
        for k in order:
            for _ in range(3):
                c = wr.blend(c, (a, b)[k])
        assert tuple(out[1, 1]) == tuple(c) and (out[0] == 9).all()
    # by hand: red 9 -> 132 -> 193 -> 224 -> 112 -> 56 -> 28, green 9 -> 4 -> 2 -> 1 -> 128 -> 191 -> 223, blue 9 -> 4 -> 2 -> 1 -> 0
    assert tuple(wr.draw_wireframe(img, [[0, 0, 0], [3, 3, 3]], pos, F([0, 0, 0, 1, 1, 1]))[0][1, 1]) == (28, 223, 0)


def test_checker_slope_divides_by_count_so_b_is_never_reached():
    v = wr.line_values(0.0, 1.0, 5)  # a line of five pixels: 0, 0.2, ..., 0.8
    assert len(v) == 5 and v[0] == F(0) and v[-1] == F(F(4) * F(F(1) / F(5))) and v[-1] < F(1)
    assert wr.line_values(0.7, 0.1, 1) == [F(0.7)]  # one pixel: A's value
    img = np.full((3, 8), 9, np.uint8)
    out, _, _ = wr.draw_wireframe(img, [[0, 1, 1]], F([[1, 1], [5, 1]]), F([0.0, 2.0]))
    # line 0 -> 1 has 5 pixels, values 0 .. 1.6; pixel (5, 1) gets jet(1.6), then twice more jet(2.0) from 1 -> 1, and jet(0 + 4 * 0.4) again
    from tests.debug_ref import jet

    c = np.array([9, 9, 9])
    for val in (F(F(4) * F(F(2) / F(5))), F(2), F(F(4) * F(F(2) / F(5)))):
        c = wr.blend(c, jet(val)[0])
    assert tuple(out[1, 5]) == tuple(c)
    assert tuple(out[1, 1]) == tuple(wr.blend(wr.blend([9, 9, 9], jet(F(0))[0]), jet(F(0))[0]))


def test_mirror_exposes_the_wireframe_with_the_reference_defaults(built):
    import flame_amd
    from flame_amd.regularizer import ABI_SYMBOLS

    for name in ("debug_wireframe", "debug_wireframe_begin", "debug_wireframe_end"):
        assert callable(getattr(flame_amd.Regularizer, name))
        assert "flame_nltgv2_" + name in ABI_SYMBOLS
    p = flame_amd.WireframeParams()
    c = flame_amd.WireframeParams(0, 1, 2)
    flame_amd.load_library().flame_nltgv2_default_wireframe_params(C.byref(c))
    for q in (p, c):
        assert [getattr(q, n) for n, _ in flame_amd.WireframeParams._fields_] == [F(1.0), 0, 0]
    assert flame_amd.load_library().flame_nltgv2_abi_version() == 7  # (additive entry points)


def test_new_declarations_compile_as_c_and_cpp_with_the_mirrors_sizes(built, tmp_path):
    import flame_amd
    from flame_amd.regularizer import _WireframeView

    src = tmp_path / "t.c"
    src.write_text(
        '#include "flame_nltgv2.h"\n'
        "typedef int (*begin_fn)(flame_nltgv2_ctx*, const uint8_t*, const void*, int, const uint8_t*, const flame_nltgv2_wireframe_params*, int, int, float);\n"
        "typedef int (*end_fn)(flame_nltgv2_ctx*, flame_nltgv2_wireframe_view*);\n"
        "typedef int (*sync_fn)(flame_nltgv2_ctx*, const uint8_t*, const void*, int, const uint8_t*, const flame_nltgv2_wireframe_params*, int, int,"
        " float, uint8_t*, int32_t*, int32_t*);\n"
        "int main(void) {\n"
        "  begin_fn b = flame_nltgv2_debug_wireframe_begin; end_fn e = flame_nltgv2_debug_wireframe_end; sync_fn s = flame_nltgv2_debug_wireframe;\n"
        "  flame_nltgv2_wireframe_params p; p.validity = 2; flame_nltgv2_default_wireframe_params(&p);\n"
        "  (void)b; (void)e; (void)s;\n"
        f"  return (sizeof(flame_nltgv2_wireframe_params) == {C.sizeof(flame_amd.WireframeParams)} &&"
        f" sizeof(flame_nltgv2_wireframe_view) == {C.sizeof(_WireframeView)} && p.validity == 0 && p.flip == 0 && FLAME_NLTGV2_ABI_VERSION == 7) ? 0 : 1;\n"
        "}\n")
    lib_dir = os.path.join(ROOT, "flame_amd")
    link = ["-L", lib_dir, "-lflame_nltgv2_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"]
    inc = ["-I", os.path.join(ROOT, "include")]
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", *inc, str(src), "-o", str(tmp_path / "t_c"), *link])
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-x", "c++", *inc, str(src), "-o", str(tmp_path / "t_cpp"), *link])
    assert subprocess.run([str(tmp_path / "t_c")], timeout=60).returncode == 0
    assert subprocess.run([str(tmp_path / "t_cpp")], timeout=60).returncode == 0


# ---- the cases of the GPU tests (tests/test_gpu_wireframe*.py) -------------------------------------------------------------------
def chain_graph(pos, x):
    """A graph over the given vertices whose edges are a chain (the wireframe reads pos and x only; the state is uploaded, not solved
    for, and consecutive vertices never share a position)."""
    pos = np.ascontiguousarray(pos, F)
    edges = np.stack([np.arange(len(pos) - 1), np.arange(1, len(pos))], axis=1).astype(np.int32)
    return synth.assemble_graph(pos, np.ascontiguousarray(x, F), edges)


def grey(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8)


SINGLE_ROWS, SINGLE_COLS = 12, 16
SINGLE = {  # one triangle each, on a 16 x 12 image
    "shallow_and_steep": [(1, 2), (14, 5), (4, 11)],        # (13, 3) and (-10, 6) shallow, (3, 9) steep
    "diagonal_vertical_horizontal": [(2, 1), (10, 9), (10, 1)],
    "horizontal_vertical_anti": [(3, 3), (12, 3), (3, 10)],  # ... and (-9, 7) from right to left
    "two_vertices_one_pixel": [(5.2, 5.3), (4.8, 4.7), (11, 8)],
    "halves": [(2.5, 3.5), (12.5, 0.5), (7.5, 10.5)],       # -> (2, 4), (12, 0), (8, 10)
    "image_corners": [(0, 0), (15, 11), (15, 0)],
}


def single_case():
    pos = np.array([p for tri in SINGLE.values() for p in tri], F)
    x = np.tile(F([0.3, 1.1, 1.9]), len(SINGLE))
    tris = {}
    for i, name in enumerate(SINGLE):
        tris[name] = np.array([[3 * i, 3 * i + 1, 3 * i + 2]], np.int32)
        tris[name + "_reversed"] = np.array([[3 * i + 2, 3 * i + 1, 3 * i]], np.int32)
    return dict(g=chain_graph(pos, x), pos=pos, x=x, tris=tris, img=grey(SINGLE_ROWS, SINGLE_COLS, 41))


def pair_case():
    """A = (0, 1, 2) and B = (2, 1, 3) share the edge 1 - 2, which A walks 1 -> 2 and B 2 -> 1 (a (6, 3) line: the two walks visit
    different pixels); C = (4, 5, 6) lies across A.  Values 0.2 and 1.8."""
    pos = F([[2, 9], [5, 2], [11, 5], [13, 1], [1, 5], [14, 3], [8, 11]])
    x = F([0.2, 1.8, 0.2, 1.8, 1.8, 1.8, 1.8])
    A, B, Cc = [0, 1, 2], [2, 1, 3], [4, 5, 6]
    tris = dict(AB=[A, B], BA=[B, A], AC=[A, Cc], CA=[Cc, A])
    return dict(g=chain_graph(pos, x), pos=pos, x=x, tris={k: np.array(v, np.int32) for k, v in tris.items()}, img=grey(SINGLE_ROWS, SINGLE_COLS, 42))


FAN_ROWS, FAN_COLS = 23, 31


def fan_case():
    """40 triangles (hub, rim i, rim i + 13): every triangle draws two spokes and a long chord."""
    n = 40
    ang = 2 * np.pi * np.arange(n) / n
    rim = np.stack([15 + 14.4 * np.cos(ang), 11 + 10.4 * np.sin(ang)], axis=1)
    pos = np.concatenate([[[15, 11]], rim]).astype(F)
    x = np.concatenate([[1.0], np.where(np.arange(n) % 2 == 0, 0.2, 1.8)]).astype(F)
    tris = np.array([[0, 1 + i, 1 + (i + 13) % n] for i in range(n)], np.int32)
    return dict(g=chain_graph(pos, x), pos=pos, x=x, tris=tris, img=grey(FAN_ROWS, FAN_COLS, 43))


def outside_case():
    """Vertices 1 and 4 round to x = 16 = cols and x = -1: the lines to them are skipped, the other lines of their triangles drawn."""
    pos = F([[3, 2], [15.6, 5], [8, 10], [12, 1], [-0.6, 6], [6, 6], [15.4, 11.4], [-0.4, 0.4]])
    x = F([0.2, 0.6, 1.0, 1.4, 1.8, 0.4, 0.8, 1.2])
    tris = np.array([[0, 1, 2], [3, 4, 5], [0, 2, 5], [6, 7, 3], [1, 4, 2], [1, 4, 4]], np.int32)
    return dict(g=chain_graph(pos, x), pos=pos, x=x, tris=tris, img=grey(SINGLE_ROWS, SINGLE_COLS, 44))


def scene_wireframe(s, tri_valid=None, scale=COLOR_SCALE, flip=False, tris=None, want_counts=False, g=None):
    idepth = mr.vertex_idepths((s["g"] if g is None else g)["x"], GRAPH_SCALE)
    return wr.draw_wireframe(s["img"], s["tris"] if tris is None else tris, s["pos"], idepth, tri_valid, scale, flip, want_counts)


def filter_state(s):
    """The scene's graph with another state: a gentle plane with two spikes and one vertex near zero, which the default filters split
    (the scene's own x is noise, and they reject every triangle of it)."""
    g = synth.copy_graph(s["g"])
    x = (F(2.0) + F(0.01) * s["pos"][:, 0] + F(0.005) * s["pos"][:, 1]).astype(F)
    x[[10, 25]], x[31] = F(6.0), F(0.01)
    for k in ("x", "x_bar", "x_prev", "data_term"):
        g[k] = x.copy()
    return g


def scene_filter_validity(s, g):
    """tri_validity_ of the scene's mesh in state g under the default filters (tests/mesh_ref.py)."""
    Kinv = np.linalg.inv(s["K"].astype(np.float64)).astype(F)
    return Kinv, np.asarray(mr.mesh_outputs(s["pos"], g["x"], s["tris"], Kinv, ROWS, COLS, GRAPH_SCALE)["tri_valid"], np.uint8)


def test_cases_meet_the_conditions_the_gpu_tests_rely_on(scene):
    # single triangles: every kind of line is there, and reversing the vertex order changes the picture of at least one of them
    c = single_case()
    kinds = set()
    changed = 0
    for name, tri in SINGLE.items():
        p = [wr.endpoint(q, SINGLE_ROWS, SINGLE_COLS) for q in tri]
        assert None not in p
        for a, b in ((0, 1), (1, 2), (0, 2)):
            dx, dy = abs(p[b][0] - p[a][0]), abs(p[b][1] - p[a][1])
            kinds.add("point" if dx == dy == 0 else "horizontal" if dy == 0 else "vertical" if dx == 0 else "diagonal" if dx == dy else
                      "shallow" if dx > dy else "steep")
        fwd = wr.draw_wireframe(c["img"], c["tris"][name], c["pos"], c["x"])
        rev = wr.draw_wireframe(c["img"], c["tris"][name + "_reversed"], c["pos"], c["x"])
        assert fwd[1:] == (3, 0) and rev[1:] == (3, 0)
        changed += not np.array_equal(fwd[0], rev[0])
    assert kinds == {"point", "horizontal", "vertical", "diagonal", "shallow", "steep"} and changed >= 4
    assert any(float(v) % 1 == 0.5 for tri in SINGLE.values() for q in tri for v in q)
    # two triangles: the list order matters, and the shared edge is walked in both directions over different pixels
    c = pair_case()
    pic = {k: wr.draw_wireframe(c["img"], t, c["pos"], c["x"])[0] for k, t in c["tris"].items()}
    assert not np.array_equal(pic["AB"], pic["BA"]) and not np.array_equal(pic["AC"], pic["CA"])
    p1, p2 = wr.endpoint(c["pos"][1], 12, 16), wr.endpoint(c["pos"][2], 12, 16)
    assert set(wr.walk(p1, p2)) != set(wr.walk(p2, p1))
    # the fan: a long list at the hub, more entries than a fresh context's buffer holds, order matters
    c = fan_case()
    img, nd, ns, counts = wr.draw_wireframe(c["img"], c["tris"], c["pos"], c["x"], want_counts=True)
    assert (nd, ns) == (120, 0) and counts[11, 15] >= 65 and counts.sum() > 2 * FAN_ROWS * FAN_COLS
    assert not np.array_equal(img, wr.draw_wireframe(c["img"], c["tris"][::-1], c["pos"], c["x"])[0])
    # the scene: short and long lists, order matters, and the default filters remove some triangles but not all
    s = scene
    img, nd, ns, counts = scene_wireframe(s, want_counts=True)
    assert (nd, ns) == (3 * len(s["tris"]), 0)
    assert (counts == 1).any() and (counts == 2).any() and (counts >= 6).any() and (counts == 0).any()
    assert not np.array_equal(img, scene_wireframe(s, tris=s["tris"][::-1])[0])
    g2 = filter_state(s)
    _, valid = scene_filter_validity(s, g2)
    assert 10 < valid.sum() < len(valid) - 10
    assert not np.array_equal(scene_wireframe(s, tri_valid=valid, g=g2)[0], scene_wireframe(s, g=g2)[0])
    third = np.ones(len(s["tris"]), np.uint8)
    third[::3] = 0
    assert not np.array_equal(scene_wireframe(s, tri_valid=third)[0], img)
    # outside: two triangles lose the two lines that end at their outside vertex, two lose all three; two are drawn whole
    c = outside_case()
    img, nd, ns = wr.draw_wireframe(c["img"], c["tris"], c["pos"], c["x"])
    assert (nd, ns) == (1 + 1 + 3 + 3, 2 + 2 + 3 + 3) and wr.endpoint(c["pos"][6], 12, 16) == (15, 11) and wr.endpoint(c["pos"][7], 12, 16) == (0, 0)
    assert camera().shape == (3, 3)
