"""numpy restatement of flame_nltgv2_fuse_views_begin (include/flame_nltgv2.h states the rules), the checker of the fusion stage, over
tests/view_ref.py for the layers.  float32 where the device computes in float, no FMA, Python integers for the ranks; plain loops over
the sources, whole images at once.  The device must agree bit for bit.

  A layers     layer s = view_ref.render_view of source s into the target (holes 0x7fc00000)
  B present    layer s is no hole; n = how many
  C reference  m = the value at index n // 2 of the present values ordered by (bits, source): the upper median, the nearer surface
  D inliers    |v_s - m| <= rel_tol * m; support = how many
  E fused      support >= min_support: ((v_a w_a) + v_b w_b) + ... / (w_a + w_b) + ... over the inliers by ascending source; else a hole
  F outputs    fused, present_mask, inlier_mask (bit s), spread = max inlier - min inlier (NaN where n == 0), 32 counter words
"""
import numpy as np

from tests import view_ref as vr

F = np.float32
HOLE = vr.HOLE
SOURCES = 8
COUNT_WORDS = 32


def fuse_views(layers, weights, rel_tol, min_support, tris_drawn=0):
    """layers (N, rows, cols) f32 with holes as NaN 0x7fc00000 -> dict(fused, present_mask, inlier_mask, spread, coverage,
    support_hist [9], present [8], inlier [8], tris_drawn, counts (32,) i32)."""
    layers = np.ascontiguousarray(layers, F)
    N, rows, cols = layers.shape
    assert 1 <= N <= SOURCES and len(weights) == N and 1 <= min_support <= N
    w = [F(x) for x in weights]
    b = vr.bits(layers).astype(np.int64)                     # (N, rows, cols)
    pr = b != int(HOLE)                                      # rule B (a value is > 0 and finite: never the NaN pattern)
    n = pr.sum(0)
    # rule C: rank_s = #{j present : (bits_j, j) < (bits_s, s)}; the owner of m has rank n // 2
    mbits = np.zeros((rows, cols), np.int64)
    for s in range(N):
        rank = np.zeros((rows, cols), np.int64)
        for j in range(N):
            if j != s:
                rank += pr[j] & ((b[j] < b[s]) | ((b[j] == b[s]) & (j < s)))
        mbits = np.where(pr[s] & (rank == n // 2), b[s], mbits)
    m = mbits.astype(np.uint32).view(F)
    with np.errstate(all="ignore"):
        tol = (F(rel_tol) * m).astype(F)
        inl = np.zeros((N, rows, cols), bool)
        for s in range(N):
            inl[s] = pr[s] & (np.abs((layers[s] - m).astype(F)) <= tol)  # rule D
        support = inl.sum(0)
        num, den = np.zeros((rows, cols), F), np.zeros((rows, cols), F)
        seen = np.zeros((rows, cols), bool)
        hi, lo = np.zeros((rows, cols), np.int64), np.full((rows, cols), 1 << 32, np.int64)
        for s in range(N):  # rule E: ascending source index, left to right; the first inlier starts the sums
            vw = (layers[s] * w[s]).astype(F)
            num = np.where(inl[s], np.where(seen, (num + vw).astype(F), vw), num).astype(F)
            den = np.where(inl[s], np.where(seen, (den + w[s]).astype(F), w[s]), den).astype(F)
            seen |= inl[s]
            hi = np.where(inl[s], np.maximum(hi, b[s]), hi)
            lo = np.where(inl[s], np.minimum(lo, b[s]), lo)
        is_fused = (n > 0) & (support >= min_support)
        fused = np.where(is_fused, (num / np.where(is_fused, den, F(1))).astype(F).view(np.uint32), HOLE).astype(np.uint32).view(F)
        sp = (hi.astype(np.uint32).view(F) - np.where(n > 0, lo, 0).astype(np.uint32).view(F)).astype(F)
        spread = np.where(n > 0, sp.view(np.uint32), HOLE).astype(np.uint32).view(F)
    bit = (1 << np.arange(N, dtype=np.int64))[:, None, None]
    out = dict(fused=fused, present_mask=(pr * bit).sum(0).astype(np.uint8), inlier_mask=(inl * bit).sum(0).astype(np.uint8), spread=spread,
               coverage=int(is_fused.sum()), support_hist=[int((support == k).sum()) for k in range(SOURCES + 1)],
               present=[int(pr[s].sum()) if s < N else 0 for s in range(SOURCES)],
               inlier=[int(inl[s].sum()) if s < N else 0 for s in range(SOURCES)], tris_drawn=int(tris_drawn))
    out["counts"] = np.array([out["coverage"]] + out["support_hist"] + out["present"] + out["inlier"] + [out["tris_drawn"]] + [0] * 5, np.int32)
    assert out["counts"].shape == (COUNT_WORDS,) and sum(out["support_hist"]) == rows * cols
    return out


def fuse_sources(sources, K_dst, rows, cols, rel_tol, min_support, near_depth=0.0):
    """sources: dicts(tris, pos, idepth, Kinv_src, R, t, weight[, tri_valid]) -> fuse_views' dict plus layers (N, rows, cols) and renders
    (view_ref.render_view's dict per source)."""
    eye = np.eye(3, dtype=F)
    renders = [vr.render_view(s["tris"], s["pos"], s["idepth"], s.get("Kinv_src", eye), K_dst, s.get("R", eye), s.get("t", np.zeros(3, F)), rows, cols,
                              near_depth, s.get("tri_valid")) for s in sources]
    layers = np.stack([r["map"] for r in renders]) if renders else np.zeros((0, rows, cols), F)
    out = fuse_views(layers, [s.get("weight", 1.0) for s in sources], rel_tol, min_support, sum(r["tris_drawn"] for r in renders))
    out["layers"], out["renders"] = layers, renders
    return out


def assert_same(got, want, what=""):
    """The device's dict (Regularizer.fuse_views_end) against the checker's, bit for bit; outputs the device did not bring are skipped."""
    g, w = np.asarray(got["counts"], np.int32), want["counts"]
    assert g.shape == w.shape and (g == w).all(), "%s: counters %s, checker %s" % (what, g.tolist(), w.tolist())
    for name in ("fused", "spread", "layers", "present_mask", "inlier_mask"):
        if name not in got:
            continue
        floats = name in ("fused", "spread", "layers")
        g = vr.bits(got[name]) if floats else np.asarray(got[name], np.uint8)
        w = vr.bits(want[name]) if floats else want[name]
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, "%s: %s differs at %d pixels, first %s: %#x, checker %#x" % (
            what, name, len(bad), tuple(bad[0]), g[tuple(bad[0])], w[tuple(bad[0])])
