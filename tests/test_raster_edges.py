"""The mesh rasteriser (k_raster_triangles + k_raster_resolve, nltgv2_kernels.hip) at its edges, on every entry point that
reaches it: flame_nltgv2_interpolate_mesh_arrays, flame_nltgv2_interpolate_mesh and interpolate_mesh_begin / _end.

CPU: the checker (oracle/raster_oracle.c) against an exact statement of the operation (tests/raster_ref_exact.py: coverage and
  the winning triangle in integers, the value in float64) -- covered set, NaN set and coverage count exactly, every finite
  value within 8 * 2^-24 * max|v| (four roundings of a convex combination, doubled).
GPU: the same cases at 37x53 (1961 pixels: less than one workgroup of k_raster_resolve, 2048 pixels) and 61x97 (5917 pixels:
  three workgroups, the last one ragged), bit for bit with the checker (NaN as NaN: the payload of a NaN is not compared, the
  default NaN's sign differs between x86 and the device) and against the exact statement.

The cases: vertices on .5 in both directions of the tie and one ulp either side of it; triangles off each side and each corner
and wholly outside; three identical points (a 4-pixel block of NaN) in the interior and at cols - 2, where the block crosses
the right border; two identical points; collinear triples; both windings; slivers; boxes 4k, 4k + 1 and 4k + 3 wide; one
triangle over the whole image; 60 triangles on one pixel in three orders; NaN over finite and finite over NaN; validity masks
that knock out the winner, all triangles invalid, T = 0; values negative, -0, 1e30, inf, NaN; one context used at one size,
a smaller one and the first again with fewer triangles.

What the device's output cannot show: a pixel covered by a NaN value and a pixel not covered at all are both NaN in the map, so
"covered" is compared on the pixels with a number; the winner is compared through its value (the triangles that share a pixel
carry different values).  With vertices at most 64 px outside these images no weight exceeds 1e5, so the products with 1e30
stay finite in float32 (the value overflows only at image sizes this suite does not run).

LEFT OUT on purpose: non-finite or very large vertex coordinates.  Their conversion to int is not the same in the exact
statement, the checker and the device, and the kernel walks the whole bounding box of a triangle, so a far-away vertex costs
time in proportion to its distance: a documented limit of the call, not a case to run.  Vertex coordinates stay within 64 px
of the image; the one exception is the triangle that covers the whole image, which no triangle inside that margin can:
its far vertices lie cols + 30 and rows + 30 px out.

The reference program itself writes a 4-pixel block without looking at the right border (its images are padded in practice);
the checker and the kernel both write in-image pixels only, and that guarded behaviour is what is tested here."""
import functools

import numpy as np
import pytest

from oracle import capi as oracle
from tests import raster_ref_exact as rex

SIZES = [(37, 53), (61, 97)]  # rows, cols
F = np.float32


class Mesh:
    """Triangles with vertices of their own (so that no two triangles carry the same values), in list order."""

    def __init__(self):
        self.vtx, self.val, self.tris, self.tv, self.vv = [], [], [], [], []

    def add(self, pts, vals, tri_valid=1, vtx_valid=(1, 1, 1)):
        n = len(self.vtx)
        self.vtx += [tuple(p) for p in pts]
        self.val += list(vals)
        self.vv += list(vtx_valid)
        self.tris.append((n, n + 1, n + 2))
        self.tv.append(tri_valid)
        return self

    def done(self, masks=False, order=None):
        tris = np.array(self.tris, np.int32).reshape(-1, 3)
        tv = np.array(self.tv, np.uint8)
        if order is not None:
            tris, tv = tris[order], tv[order]
        out = dict(vtx=np.array(self.vtx, F).reshape(-1, 2), val=np.array(self.val, F), tris=np.ascontiguousarray(tris),
                   tri_valid=np.ascontiguousarray(tv) if masks else None, vtx_valid=np.array(self.vv, np.uint8) if masks else None)
        return out


def _up(v):
    return np.nextafter(F(v), F(np.inf))


def _dn(v):
    return np.nextafter(F(v), F(-np.inf))


def _ccw_for_the_call(pts):
    """The order of pts in which the call fills the triangle's inside (the other order covers its outline only where all
    three weights vanish)."""
    (ax, ay), (bx, by), (cx, cy) = [(round(float(x)), round(float(y))) for x, y in pts]
    centre = ((ax + bx + cx) / 3.0, (ay + by + cy) / 3.0)
    w_c = (ay - by) * (centre[0] - bx) - (ax - bx) * (centre[1] - by)  # E(b, a, centre)
    return list(pts) if w_c >= 0 else [pts[0], pts[2], pts[1]]


def build_cases(rows, cols):
    C, R = cols, rows
    vals = iter(np.random.default_rng(rows * 1000 + cols).uniform(0.2, 3.0, 4000).astype(F))
    v3 = lambda: [next(vals), next(vals), next(vals)]  # noqa: E731
    fill = lambda pts: _ccw_for_the_call(pts)  # noqa: E731
    cases = {}

    m = Mesh()  # ---- .5 vertices in both directions of the tie, and one ulp either side
    m.add(fill([(2.5, 3.5), (14.5, 2.5), (3.5, 12.5)]), v3())       # 2.5 -> 2, 3.5 -> 4, 14.5 -> 14, 12.5 -> 12
    m.add(fill([(-0.5, 20.5), (9.5, 21.5), (-1.5, 30.5)]), v3())    # -0.5 -> 0, -1.5 -> -2, 20.5 -> 20, 21.5 -> 22
    m.add(fill([(_up(20.5), _dn(2.5)), (_dn(30.5), _up(3.5)), (_up(22.5), _dn(12.5))]), v3())
    m.add(fill([(_dn(21.5), _up(14.5)), (_up(31.5), _dn(15.5)), (_dn(24.5), _up(25.5))]), v3())
    m.add(fill([(C - 9.5, R - 10.5), (C - 0.5, R - 8.5), (C - 7.5, R - 0.5)]), v3())
    cases["half_pixels"] = m.done()

    m = Mesh()  # ---- partly off each side and each corner, wholly outside
    m.add(fill([(-20, 10), (6, 14), (-3, 25)]), v3())                # left
    m.add(fill([(C - 6, 8), (C + 30, 12), (C - 2, 24)]), v3())       # right
    m.add(fill([(15, -25), (30, 5), (20, 7)]), v3())                 # top
    m.add(fill([(18, R - 5), (34, R + 40), (25, R - 2)]), v3())      # bottom
    m.add(fill([(-30, -8), (7, -3), (-4, 9)]), v3())                 # corners
    m.add(fill([(C + 25, -12), (C - 8, -2), (C + 3, 10)]), v3())
    m.add(fill([(-12, R + 20), (8, R - 6), (-5, R - 9)]), v3())
    m.add(fill([(C + 50, R + 10), (C - 7, R - 3), (C + 6, R - 12)]), v3())
    m.add(fill([(-60, 5), (-10, 9), (-40, 30)]), v3())               # wholly outside: left, right, above, below, off a corner
    m.add(fill([(C + 5, 5), (C + 60, 9), (C + 40, 30)]), v3())
    m.add(fill([(5, -60), (30, -50), (12, -2)]), v3())
    m.add(fill([(5, R + 60), (30, R + 50), (12, R + 2)]), v3())
    m.add(fill([(C + 1, R + 1), (C + 64, R + 3), (C + 30, R + 64)]), v3())
    m.add(fill([(-64, -64), (-1, -60), (-30, -1)]), v3())
    cases["off_image"] = m.done()

    m = Mesh()  # ---- degenerate and extreme triangles (placed apart: what each one writes is seen on its own)
    m.add(fill([(0, 10), (6, 10), (0, 13)]), v3())                   # (finite pixels at the start of rows 10 and 12: a block that ran on past
                                                                     # the right border would land on them)
    m.add([(10, 6)] * 3, v3())                                       # three identical points: pixels 10..13 of row 6 are NaN
    m.add([(C - 2, 9)] * 3, v3())                                    # ... and a block that crosses the right border
    m.add([(C - 1, 11)] * 3, v3())
    m.add([(20, 4), (20, 4), (27, 9)], v3())                         # two identical points and a third
    m.add([(31, 3), (38, 8), (31, 3)], v3())
    m.add([(3, 14), (9, 14), (17, 14)], v3())                        # collinear: horizontal, vertical, both diagonals
    m.add([(22, 12), (22, 17), (22, 25)], v3())
    m.add([(26, 12), (30, 16), (37, 23)], v3())
    m.add([(48, 12), (44, 16), (40, 20)], v3())
    pts = [(4, 18), (16, 19), (6, 29)]
    m.add(fill(pts), v3())                                           # one winding fills ...
    m.add(fill(pts)[::-1], v3())                    # ... the other covers no more than its outline's zeros
    m.add(fill([(C - 12, 18), (C - 11, 18), (C - 12, R - 3)]), v3())  # slivers one pixel wide / high
    m.add(fill([(3, R - 4), (3, R - 3), (C - 14, R - 3)]), v3())
    m.add(fill([(30, 26), (37, 26), (33, 31)]), v3())                # boxes 8 (4k), 9 (4k + 1) and 11 (4k + 3) pixels wide
    m.add(fill([(39, 26), (47, 26), (43, 31)]), v3())
    m.add(fill([(C - 11, 2), (C - 1, 2), (C - 6, 7)]), v3())         # (11 wide, ending on the last column: the walk goes on to cols + 1)
    cases["degenerate"] = m.done()

    m = Mesh()  # ---- one triangle over the whole image, and a few on top of it
    m.add(fill([(-10, -10), (2 * C + 20, -10), (-10, 2 * R + 20)]), v3())
    m.add(fill([(5, 5), (25, 8), (9, 22)]), v3())
    cases["whole_image"] = m.done()

    # ---- ordering: 60 triangles that all contain one pixel
    m = Mesh()
    cx, cy = C // 2 + 1, R // 2 - 1
    rng = np.random.default_rng(7)
    for i in range(60):
        ang = rng.uniform(0, 2 * np.pi) + np.array([0.0, 2.1, 4.2])
        rad = rng.uniform(3.0, min(C, R) / 2.0 + 20.0, 3)
        m.add(fill([(cx + r * np.cos(a), cy + r * np.sin(a)) for a, r in zip(ang, rad)]), v3())
    cases["sixty_ascending"] = m.done()
    cases["sixty_descending"] = m.done(order=np.arange(60)[::-1])
    cases["sixty_shuffled"] = m.done(order=np.random.default_rng(8).permutation(60))

    for name, first in (("nan_over_finite", True), ("finite_over_nan", False)):
        m = Mesh()
        big = (fill([(5, 5), (40, 9), (12, 30)]), v3())
        dots = [([(15, 12)] * 3, v3()), ([(11, 20), (19, 20), (14, 20)], v3())]  # (a point and a horizontal line inside it)
        for pts, vv in ([big] + dots if first else dots + [big]):
            m.add(pts, vv)
        cases[name] = m.done()

    # ---- validity masks
    m = Mesh()
    m.add(fill([(5, 5), (40, 9), (12, 30)]), v3())
    m.add(fill([(8, 6), (35, 12), (14, 26)]), v3(), tri_valid=0)               # would have won
    m.add(fill([(20, 3), (45, 20), (25, 28)]), v3())
    m.add(fill([(22, 8), (40, 18), (27, 24)]), v3(), vtx_valid=(1, 0, 1))      # would have won
    m.add([(30, 15)] * 3, v3(), tri_valid=0)                                   # a NaN block that must not appear
    cases["masks_knock_out_winner"] = m.done(masks=True)
    m = Mesh()
    m.add(fill([(5, 5), (40, 9), (12, 30)]), v3(), tri_valid=0)
    m.add(fill([(20, 3), (45, 20), (25, 28)]), v3(), tri_valid=0)
    cases["all_invalid"] = m.done(masks=True)
    empty = Mesh().add([(1, 1), (5, 1), (1, 5)], v3()).done()
    empty["tris"] = np.zeros((0, 3), np.int32)
    cases["no_triangles"] = empty

    # ---- vertex values
    m = Mesh()
    m.add(fill([(3, 3), (20, 5), (6, 17)]), [F(-1.5), F(-0.25), F(2.0)])
    m.add(fill([(22, 3), (40, 5), (25, 17)]), [F(-0.0), F(-0.0), F(-0.0)])
    m.add(fill([(42, 3), (C - 2, 6), (44, 16)]), [F(0.0), F(-0.0), F(1.0)])
    m.add(fill([(3, 19), (20, 21), (6, R - 3)]), [F(1e30), F(-1e30), F(3.0)])
    m.add(fill([(22, 19), (40, 21), (25, R - 3)]), [F(np.inf), F(1.0), F(2.0)])
    m.add(fill([(42, 19), (C - 2, 22), (44, R - 4)]), [F(np.inf), F(-np.inf), F(2.0)])
    m.add(fill([(30, 8), (38, 10), (33, 15)]), [F(np.nan), F(1.0), F(2.0)])     # covered, not counted
    cases["special_values"] = m.done()

    # ---- the random mesh: shared vertices, up to 20 px outside, .5 coordinates, two degenerate triangles
    rng = np.random.default_rng(rows + cols)
    vtx = np.stack([rng.uniform(-20, C + 20, 40), rng.uniform(-20, R + 20, 40)], 1)
    vtx[::3] = np.floor(vtx[::3]) + 0.5
    vtx[36:39] = (C - 2, R // 2)
    vtx[33], vtx[34], vtx[35] = (4, 4), (9, 9), (15, 15)
    tris = np.array([rng.choice(33, 3, replace=False) for _ in range(118)] + [[36, 37, 38], [33, 34, 35]], np.int32)
    cases["random"] = dict(vtx=vtx.astype(F), val=rng.uniform(-2, 5, 40).astype(F), tris=tris, tri_valid=None, vtx_valid=None)
    for name, c in cases.items():
        lo, hi = c["vtx"].min(0), c["vtx"].max(0)
        out = np.array([C + 30, R + 30] if name == "whole_image" else [64, 64])
        assert (lo >= -64).all() and (hi <= np.array([C, R]) + out).all(), name
    return cases


CASE_NAMES = sorted(build_cases(*SIZES[0]))
GRAPH_SCALE = F(1.37)


@functools.lru_cache(maxsize=None)
def reference(name, rows, cols, through_graph=False):
    """(case, values, the checker's image, the exact image, the winners, the value bound) -- computed once, shared, read-only.
    through_graph: the values are x * graph_scale as the context-bound call forms them, and there is no vertex mask."""
    c = dict(build_cases(rows, cols)[name])
    values = (c["val"] * GRAPH_SCALE).astype(F) if through_graph else c["val"]
    if through_graph:
        c["vtx_valid"] = None
    want = oracle.raster_interpolate_mesh(c["tris"], c["vtx"], values, rows, cols, tri_valid=c["tri_valid"], vtx_valid=c["vtx_valid"])
    exact, winner = rex.interpolate_mesh_exact(c["tris"], c["vtx"], values, rows, cols, c["tri_valid"], c["vtx_valid"])
    bound = rex.value_bound(c["tris"], values, winner)
    for a in (want, exact, winner, bound):
        a.setflags(write=False)
    return c, values, want, exact, winner, bound


def same_bits(got, want, what):
    """Bit for bit, NaN as NaN (the payload of a NaN is not compared)."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN set", np.argwhere(gn != wn)[:6])
    bad = got.view(np.uint32)[~wn] != want.view(np.uint32)[~wn]
    assert not bad.any(), (what, np.argwhere(~wn)[bad][:6], got[~wn][bad][:6], want[~wn][bad][:6])


def against_exact(img, coverage, exact, winner, bound, what):
    """img (float32, from the checker or the device) against the exact statement; returns the largest |deviation| / bound."""
    assert np.array_equal(np.isnan(img), np.isnan(exact)), (what, "NaN set", np.argwhere(np.isnan(img) != np.isnan(exact))[:6])
    assert not (~np.isnan(exact) & (winner < 0)).any()
    assert coverage == int((~np.isnan(exact)).sum()), (what, coverage, int((~np.isnan(exact)).sum()))
    inf = np.isinf(exact)
    assert np.array_equal(img[inf].astype(np.float64), exact[inf]), (what, "infinite values")
    fin = np.isfinite(exact)
    dev = np.abs(img[fin].astype(np.float64) - exact[fin])
    assert (dev <= bound[fin]).all(), (what, np.argwhere(fin)[dev > bound[fin]][:6], dev.max())
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = dev[bound[fin] > 0] / bound[fin][bound[fin] > 0]
    return float(ratio.max()) if ratio.size else 0.0


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
def test_exact_statement_known_answers():
    """The exact statement itself: answers that a transposed, mirrored or off-by-one statement gets wrong."""
    tris = np.array([[0, 1, 2]], np.int32)
    vtx = np.array([[10, 10], [20, 10], [10, 20]], F)  # (the known answers of the reference's own interpolateMeshTest)
    img, win = rex.interpolate_mesh_exact(tris, vtx, np.array([1.0, 2.0, 3.0], F), 40, 45)
    assert img.shape == (40, 45) and img[10, 10] == 1.0 and img[10, 20] == 2.0 and img[20, 10] == 3.0  # img[row = y, col = x]
    assert img[15, 15] == pytest.approx(2.5, abs=1e-12) and img[12, 17] == pytest.approx(1.0 + 0.7 + 0.4, abs=1e-12)
    assert int((~np.isnan(img)).sum()) == 66 and np.isnan(img[16, 15]) and not np.isnan(img[15, 15])  # x + y <= 30, inclusive
    assert (win[~np.isnan(img)] == 0).all() and (win[np.isnan(img)] == -1).all()
    # the other winding: only where all three weights vanish -- nowhere for a proper triangle
    img2, _ = rex.interpolate_mesh_exact(np.array([[0, 2, 1]], np.int32), vtx, np.ones(3, F), 40, 45)
    assert np.isnan(img2).all()
    # ties go to the even pixel, in both directions and for negative coordinates
    assert [rex.round_half_even(v) for v in (2.5, 3.5, -0.5, -1.5, 0.5, 1.5)] == [2, 4, 0, -2, 0, 2]
    assert rex.round_half_even(_dn(2.5)) == 2 and rex.round_half_even(_up(2.5)) == 3 and rex.round_half_even(_dn(3.5)) == 3
    # three identical points: a block of 4 NaN pixels from the point rightwards, cut at the border, never wrapped into the next row
    for x0, cells in ((10, [10, 11, 12, 13]), (43, [43, 44])):
        img3, win3 = rex.interpolate_mesh_exact(tris, np.array([[x0, 7]] * 3, F), np.ones(3, F), 40, 45)
        assert np.isnan(img3).all() and np.argwhere(win3 == 0).tolist() == [[7, c] for c in cells]
    # the later triangle owns a shared pixel, whatever the order of the indices
    vtx4 = np.array([[10, 10], [30, 10], [10, 30], [25, 28]], F)
    v4 = np.array([1, 1, 1, 9], F)
    ab, wab = rex.interpolate_mesh_exact(np.array([[0, 1, 2], [0, 1, 3]], np.int32), vtx4, v4, 40, 45)
    ba, wba = rex.interpolate_mesh_exact(np.array([[0, 1, 3], [0, 1, 2]], np.int32), vtx4, v4, 40, 45)
    assert wab[14, 15] == 1 and wba[14, 15] == 1 and ab[14, 15] > 1.0 and ba[14, 15] == 1.0


@pytest.mark.parametrize("rows,cols", SIZES)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_checker_against_exact_statement(name, rows, cols):
    """oracle/raster_oracle.c reproduces the covered set, the NaN set and the coverage count exactly and every finite value
    within 8 * 2^-24 * max(|v1|, |v2|, |v3|) of the float64 value -- directly and with the values x * graph_scale."""
    for through_graph in (False, True):
        c, values, want, exact, winner, bound = reference(name, rows, cols, through_graph)
        ratio = against_exact(want, oracle.raster_coverage(want), exact, winner, bound, (name, rows, cols, through_graph))
        print(f"raster checker vs exact: {name} {rows}x{cols} graph={through_graph}: max deviation / bound = {ratio:.3f}")
    if name == "sixty_ascending":
        cx, cy = cols // 2 + 1, rows // 2 - 1
        assert winner[cy, cx] == 59
    if name in ("sixty_descending", "sixty_shuffled"):
        # every triangle contains the pixel: alone it owns it, and its value there is not another one's (so that the value shows the winner)
        cx, cy = cols // 2 + 1, rows // 2 - 1
        alone = [rex.interpolate_mesh_exact(c["tris"][i:i + 1], c["vtx"], values, rows, cols)[0][cy, cx] for i in range(60)]
        assert np.isfinite(alone).all()
        gaps = np.diff(np.sort(alone))
        assert gaps.min() > 2 * bound[cy, cx]
        assert exact[cy, cx] == alone[59] and winner[cy, cx] == 59
    if name == "no_triangles" or name == "all_invalid":
        assert np.isnan(want).all() and (winner == -1).all()
    if name == "degenerate":
        assert (winner[9, cols - 2:] == 2).all() and (winner[10, :2] == 0).all() and winner[11, cols - 1] == 3 and (winner[12, :3] == 0).all()
        assert np.isnan(want[9, cols - 2:]).all() and (winner[6, 10:14] == 1).all()
        assert np.isfinite(want[10, :2]).all() and np.isfinite(want[12, :3]).all()  # the blocks at the border stopped there
    if name == "special_values":
        assert (winner == 6).sum() > 10 and np.isnan(exact[winner == 6]).all()  # the NaN vertex: covered, not counted
        assert np.isinf(exact).sum() > 50 and (np.signbit(want) & (want == 0)).sum() > 50  # inf and -0 come through


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu(built):
    import torch  # noqa: F401

    import flame_amd

    return flame_amd


def graph_of(c):
    """A graph whose positions are the case's vertices and whose x are its values (never solved: edges only where two
    consecutive vertices are apart, so that every edge has a length)."""
    from flame_amd import synth

    V = len(c["vtx"])
    edges = np.array([(i, i + 1) for i in range(V - 1) if (c["vtx"][i] != c["vtx"][i + 1]).any()], np.int32).reshape(-1, 2)
    return synth.assemble_graph(c["vtx"], c["val"], edges)


def check_image(img, cov, name, rows, cols, through_graph, what):
    c, values, want, exact, winner, bound = reference(name, rows, cols, through_graph)
    same_bits(img, want, (what, name, rows, cols))
    assert cov == oracle.raster_coverage(want), (what, name, cov)
    against_exact(img, cov, exact, winner, bound, (what, name, rows, cols))


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", SIZES)
def test_gpu_arrays_path_every_case(gpu, rows, cols):
    """flame_nltgv2_interpolate_mesh_arrays: every case bit for bit with the checker and exact in coverage, winner and NaN
    set, on ONE context (each call also has to leave nothing of the one before)."""
    with gpu.Regularizer(0) as reg:
        for name in CASE_NAMES:
            c = reference(name, rows, cols)[0]
            img, cov = reg.interpolate_mesh_arrays(c["tris"], c["vtx"], c["val"], rows, cols, vtx_valid=c["vtx_valid"],
                                                   tri_valid=c["tri_valid"])
            check_image(img, cov, name, rows, cols, False, "arrays")


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", SIZES)
def test_gpu_graph_paths_every_case(gpu, rows, cols):
    """The same cases with the vertices as a graph's positions and the values as its x, graph_scale 1.37: through
    flame_nltgv2_interpolate_mesh and through interpolate_mesh_begin / _end (no vertex mask on these calls)."""
    for name in CASE_NAMES:
        c = reference(name, rows, cols, True)[0]
        with gpu.Regularizer(0) as reg:
            reg.upload_graph(graph_of(c))
            img, cov = reg.interpolate_mesh(c["tris"], rows, cols, graph_scale=float(GRAPH_SCALE), tri_valid=c["tri_valid"])
            check_image(img, cov, name, rows, cols, True, "interpolate_mesh")
            reg.interpolate_mesh_begin(c["tris"], rows, cols, graph_scale=float(GRAPH_SCALE), tri_valid=c["tri_valid"])
            img, cov = reg.interpolate_mesh_end()
            check_image(img, cov, name, rows, cols, True, "interpolate_mesh_begin/_end")


@pytest.mark.gpu
def test_gpu_context_reuse_across_image_sizes(gpu):
    """One context at 61x97, then 37x53, then 61x97 again with fewer triangles: each result is that of a fresh context (the
    checker's), nothing of the earlier image or of its keys survives -- on all three entry points."""
    big, small = SIZES[1], SIZES[0]
    seq = [("sixty_shuffled", big, slice(None)), ("whole_image", small, slice(None)), ("degenerate", big, slice(0, 6)),
           ("no_triangles", big, slice(None)), ("random", small, slice(0, 40))]

    def expect(name, size, keep, through_graph):
        c = dict(reference(name, *size, through_graph)[0])
        c["tris"] = np.ascontiguousarray(c["tris"][keep])
        values = (c["val"] * GRAPH_SCALE).astype(F) if through_graph else c["val"]
        return c, oracle.raster_interpolate_mesh(c["tris"], c["vtx"], values, *size)

    with gpu.Regularizer(0) as reg:
        for name, size, keep in seq:
            c, want = expect(name, size, keep, False)
            img, cov = reg.interpolate_mesh_arrays(c["tris"], c["vtx"], c["val"], *size)
            same_bits(img, want, ("reuse, arrays", name, size))
            assert cov == oracle.raster_coverage(want)
    with gpu.Regularizer(0) as reg:
        for k, (name, size, keep) in enumerate(seq):
            c, want = expect(name, size, keep, True)
            reg.upload_graph(graph_of(c))
            if k % 2 == 0:
                img, cov = reg.interpolate_mesh(c["tris"], *size, graph_scale=float(GRAPH_SCALE))
            else:
                reg.interpolate_mesh_begin(c["tris"], *size, graph_scale=float(GRAPH_SCALE))
                img, cov = reg.interpolate_mesh_end()
            same_bits(img, want, ("reuse, graph", name, size, k))
            assert cov == oracle.raster_coverage(want)
        # ... and the two entry points one after the other on the same graph, the image shrinking and growing
        c, _ = expect("sixty_shuffled", big, slice(None), True)
        reg.upload_graph(graph_of(c))
        for size, keep in ((big, slice(None)), (small, slice(0, 30)), (big, slice(0, 7))):
            tris = np.ascontiguousarray(c["tris"][keep])
            want = oracle.raster_interpolate_mesh(tris, c["vtx"], (c["val"] * GRAPH_SCALE).astype(F), *size)
            reg.interpolate_mesh_begin(tris, *size, graph_scale=float(GRAPH_SCALE))
            img, cov = reg.interpolate_mesh_end()
            same_bits(img, want, ("reuse, begin/end", size))
            img, cov2 = reg.interpolate_mesh(tris, *size, graph_scale=float(GRAPH_SCALE))
            same_bits(img, want, ("reuse, interpolate_mesh", size))
            assert cov == cov2 == oracle.raster_coverage(want)
