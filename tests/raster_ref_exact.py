"""An exact statement of the mesh -> dense map rasterisation (utils::interpolateMesh drawing each triangle with
utils::DrawShadedTriangleBarycentric: utils/image_utils.cc:373-396, utils/rasterization.cc:164-246), from its definition.

Vertices are rounded to integer pixels, half to even.  For a triangle (a, b, c) of the list and a pixel p the three edge
functions are the signed areas

    E(s, e, p) = (e.y - s.y) (p.x - s.x) - (e.x - s.x) (p.y - s.y)

and the weights of the three vertices are  w_c = E(b, a, p),  w_b = E(a, c, p),  w_a = E(c, b, p)  (each vertex against the
opposite edge, the triangle walked as c, b, a).  These are integers: coverage and the winner are decided exactly, here in
int64 (|E| < 2^33 for coordinates below 2^15, asserted).  A pixel is covered when all three weights are >= 0 -- edges and
vertices included, and for a degenerate triangle every pixel on which all three vanish.  The x walk runs in blocks of 4 pixels
from xmin = min of the three x: the pixels examined are xmin ... xmin + 4 (floor((xmax - xmin) / 4) + 1) - 1 on the rows ymin ...
ymax, so up to 3 pixels right of xmax are examined too (a degenerate triangle covers them), and only pixels inside the image
are written.  Triangles are drawn in list order: the LAST valid triangle that covers a pixel owns it, whatever it writes.

    value = (v_c w_c + v_b w_b + v_a w_a) / (w_c + w_b + w_a)    in float64;  NaN where the sum is 0.

Non-finite or very large vertex coordinates are outside this statement (their conversion to int is not defined here)."""
import numpy as np


def round_half_even(v):
    """Python's round(): exact, ties to the even integer."""
    return round(float(v))


def interpolate_mesh_exact(tris, vtx, values, rows, cols, tri_valid=None, vtx_valid=None):
    """-> (value (rows, cols) float64 with NaN where nothing was written, winner (rows, cols) int64: the index of the
    triangle that owns the pixel, -1 where none does)."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    vtx = np.asarray(vtx, np.float32).reshape(-1, 2)
    val = np.asarray(np.asarray(values, np.float32), np.float64)
    img = np.full((rows, cols), np.nan)
    winner = np.full((rows, cols), -1, np.int64)
    P = [(round_half_even(x), round_half_even(y)) for x, y in vtx]
    for t, (a, b, c) in enumerate(tris):
        if tri_valid is not None and not tri_valid[t]:
            continue
        if vtx_valid is not None and not (vtx_valid[a] and vtx_valid[b] and vtx_valid[c]):
            continue
        pa, pb, pc = P[a], P[b], P[c]
        assert max(abs(v) for p in (pa, pb, pc) for v in p) < 2 ** 15
        xmin, xmax = min(pa[0], pb[0], pc[0]), max(pa[0], pb[0], pc[0])
        ymin, ymax = min(pa[1], pb[1], pc[1]), max(pa[1], pb[1], pc[1])
        xend = xmin + 4 * ((xmax - xmin) // 4 + 1)  # one past the last pixel of the last block of 4
        x0, x1, y0, y1 = max(xmin, 0), min(xend, cols), max(ymin, 0), min(ymax + 1, rows)  # only in-image pixels are written
        if x0 >= x1 or y0 >= y1:
            continue
        py, px = np.mgrid[y0:y1, x0:x1].astype(np.int64)

        def E(s, e):
            return (e[1] - s[1]) * (px - s[0]) - (e[0] - s[0]) * (py - s[1])

        wc, wb, wa = E(pb, pa), E(pa, pc), E(pc, pb)
        cov = (wc >= 0) & (wb >= 0) & (wa >= 0)
        total = wc + wb + wa
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            v = (val[c] * wc + val[b] * wb + val[a] * wa) / np.where(total == 0, np.nan, total)
        img[y0:y1, x0:x1][cov] = v[cov]
        winner[y0:y1, x0:x1][cov] = t
    return img, winner


def value_bound(tris, values, winner):
    """8 * 2^-24 * max(|v_a|, |v_b|, |v_c|) of the triangle that owns each pixel (0 where none does): the float32 evaluation
    of a convex combination -- product, sum, sum, quotient: four roundings of at most 2^-24 max|v| each -- doubled."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    val = np.abs(np.asarray(np.asarray(values, np.float32), np.float64))
    per_tri = val[tris].max(1) if len(tris) else np.zeros(0)
    out = np.zeros(winner.shape)
    own = winner >= 0
    out[own] = 8 * 2.0 ** -24 * per_tri[winner[own]]
    return out
