"""numpy restatement of flame_nltgv2_render_view_begin (include/flame_nltgv2.h states the rules), the checker of the view renderer.
Plain loops over vertices and triangles, a triangle's bounding box as one array; float32 where the device computes in float, no FMA,
every sum of three products left to right; the edge functions in exact integers.  The device must agree bit for bit.

  1 vertex     q = Kinv_src (pos, 1); P = q / id; P' = R P + t; h = K_dst P'; (sx, sy) = 16 (h.x / h.z, h.y / h.z); usable iff id > 0,
               P'.z > near_depth, |sx|, |sy| <= 2^20 and the source position times 16 within the same bound; X, Y, Xs, Ys = rint
  2 triangle   drawn iff valid, all vertices usable, the doubled areas in both views non-zero and of one sign
  3 coverage   pixel centres at (16 col, 16 row); the three weights s * E >= 0
  4 value      (id'a wa + (id'b wb + id'c wc)) / |A|, a candidate iff 0 < val < inf
  5 depth      the largest {bits(val), t + 1} owns the pixel
  6 outputs    map (0x7fc00000 on holes), tri_index (-1 on holes), coverage, drawn / culled_vertex / culled_facing
"""
import numpy as np

F = np.float32
BOUND = F(1048576.0)
HOLE = np.uint32(0x7FC00000)
COUNT_KEYS = ("coverage", "tris_drawn", "tris_culled_vertex", "tris_culled_facing")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _mat(a, n):
    return np.ascontiguousarray(a, F).reshape(n)


def _rint(v):
    return int(np.rint(v))  # ties to even


def transform_vertex(pos, idepth, Kinv_src, K_dst, R, t, near_depth):
    """Rule 1 for one vertex -> (usable, X, Y, Xs, Ys, id')."""
    Ki, K, R, t = _mat(Kinv_src, 9), _mat(K_dst, 9), _mat(R, 9), _mat(t, 3)
    px, py, idv, near = F(pos[0]), F(pos[1]), F(idepth), F(near_depth)
    with np.errstate(all="ignore"):
        q = [F(F(Ki[3 * i] * px) + F(Ki[3 * i + 1] * py)) + F(Ki[3 * i + 2] * F(1.0)) for i in range(3)]
        P = [F(q[i] / idv) for i in range(3)]
        Pd = [F(F(F(F(R[3 * i] * P[0]) + F(R[3 * i + 1] * P[1])) + F(R[3 * i + 2] * P[2])) + t[i]) for i in range(3)]
        h = [F(F(F(K[3 * i] * Pd[0]) + F(K[3 * i + 1] * Pd[1])) + F(K[3 * i + 2] * Pd[2])) for i in range(3)]
        sx, sy = F(F(h[0] / h[2]) * F(16.0)), F(F(h[1] / h[2]) * F(16.0))
        ssx, ssy = F(px * F(16.0)), F(py * F(16.0))
        usable = bool(idv > F(0.0)) and bool(Pd[2] > near) and bool(np.abs(sx) <= BOUND) and bool(np.abs(sy) <= BOUND) \
            and bool(np.abs(ssx) <= BOUND) and bool(np.abs(ssy) <= BOUND)
        if not usable:
            return False, 0, 0, 0, 0, F(0.0)
        return True, _rint(sx), _rint(sy), _rint(ssx), _rint(ssy), F(F(1.0) / Pd[2])


def _area2(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def _edge(xi, yi, xj, yj, col, row):
    return (xj - xi) * (16 * row - yi) - (yj - yi) * (16 * col - xi)


def render_view(triangles, pos, idepths, Kinv_src, K_dst, R, t, rows, cols, near_depth=0.0, tri_valid=None):
    """-> dict(map (rows, cols) f32, tri_index (rows, cols) i32, coverage, tris_drawn, tris_culled_vertex, tris_culled_facing)."""
    tris = np.asarray(triangles, np.int64).reshape(-1, 3)
    pos = np.asarray(pos, F).reshape(-1, 2)
    idepths = np.asarray(idepths, F).reshape(-1)
    verts = [transform_vertex(pos[v], idepths[v], Kinv_src, K_dst, R, t, near_depth) for v in range(len(pos))]
    keys = np.zeros((rows, cols), np.uint64)
    drawn = culled_vertex = culled_facing = 0
    for ti, (a, b, c) in enumerate(tris):
        if tri_valid is not None and not tri_valid[ti]:
            continue
        va, vb, vc = verts[a], verts[b], verts[c]
        if not (va[0] and vb[0] and vc[0]):
            culled_vertex += 1
            continue
        A = _area2(va[1], va[2], vb[1], vb[2], vc[1], vc[2])
        As = _area2(va[3], va[4], vb[3], vb[4], vc[3], vc[4])
        if A == 0 or As == 0 or (A > 0) != (As > 0):
            culled_facing += 1
            continue
        drawn += 1
        s = 1 if A > 0 else -1
        absA = F(np.int64(abs(A)))
        xs, ys = (va[1], vb[1], vc[1]), (va[2], vb[2], vc[2])
        c0, c1 = max(0, -((-min(xs)) // 16)), min(cols - 1, max(xs) // 16)
        r0, r1 = max(0, -((-min(ys)) // 16)), min(rows - 1, max(ys) // 16)
        if c1 < c0 or r1 < r0:
            continue
        # every pixel of the clipped bounding box at once: int64 holds the weights exactly (|w| < 2^44)
        col, row = np.meshgrid(np.arange(c0, c1 + 1, dtype=np.int64), np.arange(r0, r1 + 1, dtype=np.int64))
        wa = s * _edge(vb[1], vb[2], vc[1], vc[2], col, row)
        wb = s * _edge(vc[1], vc[2], va[1], va[2], col, row)
        wc = s * _edge(va[1], va[2], vb[1], vb[2], col, row)
        with np.errstate(all="ignore"):
            fa, fb, fc = wa.astype(F), wb.astype(F), wc.astype(F)  # (round to nearest even)
            val = ((va[5] * fa + (vb[5] * fb + vc[5] * fc)) / absA).astype(F)
            candidate = (wa >= 0) & (wb >= 0) & (wc >= 0) & (val > F(0.0)) & (val < F(np.inf))
        key = (val.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(ti + 1)
        box = keys[r0:r1 + 1, c0:c1 + 1]
        np.maximum(box, np.where(candidate, key, np.uint64(0)), out=box)
    owner = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    hole = owner == 0
    mbits = np.where(hole, HOLE, (keys >> np.uint64(32)).astype(np.uint32)).astype(np.uint32)
    return dict(map=mbits.view(F), tri_index=(owner - 1).astype(np.int32), coverage=int((~hole).sum()), tris_drawn=drawn,
                tris_culled_vertex=culled_vertex, tris_culled_facing=culled_facing)


def assert_same(got, want, what=""):
    """The device's dict (Regularizer.render_view_end) against the checker's, bit for bit; outputs the device did not bring are skipped."""
    for k in COUNT_KEYS:
        assert int(got[k]) == int(want[k]), "%s: %s %d, checker %d" % (what, k, got[k], want[k])
    if "map" in got:
        g, w = bits(got["map"]), bits(want["map"])
        assert g.shape == w.shape, (what, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, "%s: map differs at %d pixels, first (row, col) %s: %#x, checker %#x" % (
            what, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])
    if "tri_index" in got:
        g, w = np.asarray(got["tri_index"], np.int32), want["tri_index"]
        bad = np.argwhere(g != w)
        assert g.shape == w.shape and len(bad) == 0, "%s: tri_index differs at %d pixels, first %s: %d, checker %d" % (
            what, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])
