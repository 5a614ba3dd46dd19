"""CPU restatement of the mesh outputs of Flame::update() (flame.cc:372-407) in numpy float32: the checker of
flame_nltgv2_mesh_outputs (include/flame_nltgv2.h, flame_amd/csrc/mesh_kernels.hip).

  vtx_idepths_ = x * graph_scale                                   flame.cc:377
  obliqueTriangleFilter / edgeLengthFilter / idepthTriangleFilter   flame.cc:2207-2361, in the order of flame.cc:389-407
  getVertexNormals (the triangle-based overload)                    flame.cc:2554-2641

Written as elementwise float32 operations in the reference's order -- never np.dot, np.cross or np.linalg.norm, whose
summation order is not ours.  Eigen is not available here, so what its version decides is fixed by us ("unpinned"):

  * sums of three products (a row of Kinv * p, dot(), squaredNorm()) are taken LEFT TO RIGHT, (a0 b0 + a1 b1) + a2 b2.
    Why: for 3-vectors of floats Eigen does not vectorise (3 floats are no packet) and evaluates the coefficient-based product
    and the reductions with its no-vectorisation unrollers; the product's (etor_product_coeff_impl) accumulates res += a_k b_k for
    k = 0, 1, 2.  The redux unroller splits a range in halves, which for three addends may give a0 + (a1 + a2); we could not
    run Eigen to settle that, so the library's convention everywhere else (flame_nltgv2_project_graph) is kept and stated;
  * normalize() leaves a vector whose squared norm is not > 0 unchanged (Eigen >= 3.3); a NaN squared norm too;
  * `Kinv * p / id` is the full 3x3 product, then a true division of each component (Eigen >= 3.3: scalar_quotient_op);
  * `/ 3` and `count * n`: the int converts to float first;
  * angle = float32(arccos(float64(d))) -- the reference's `fabs(acos(d))`; for |d| > 1 and NaN the angle is NaN and rejects nothing;
  * comparisons with NaN are false: a NaN never clears validity; FLAME_ASSERT(max_id >= min_id) is not reproduced.

The float64 twin (dtype=np.float64) follows the same formulas; it only serves to sanity-check the float32 one.
"""
import numpy as np

DEFAULTS = dict(do_oblique_triangle_filter=True, oblique_normal_thresh=1.39626, oblique_idepth_diff_factor=0.35,
                oblique_idepth_diff_abs=0.1, do_edge_length_filter=True, edge_length_thresh=0.333,
                do_idepth_triangle_filter=True, min_triangle_idepth=0.01)  # params.h:69-85


def params(**kw):
    p = dict(DEFAULTS)
    assert set(kw) <= set(p), set(kw) - set(p)
    p.update(kw)
    return p


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross3(a, b):  # Eigen cross3
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _normalize3(v):
    """MatrixBase::normalize(), elementwise over arrays of vectors: z = squaredNorm(); if (z > 0) v /= sqrt(z)."""
    z = _dot3(v, v)
    with np.errstate(all="ignore"):
        n = np.sqrt(z)
        ok = z > 0
        return [np.where(ok, c / n, c) for c in v]


def vertex_idepths(x, graph_scale):
    with np.errstate(all="ignore"):
        return (np.asarray(x, np.float32) * np.float32(graph_scale)).astype(np.float32)


def backproject(pos, idepth, Kinv, dtype=np.float32):
    """p = Kinv * (pos.x, pos.y, 1) / idepth  (flame.cc:2226-2229) -> three arrays."""
    K = np.asarray(Kinv, dtype).reshape(9)
    px, py = np.asarray(pos, dtype)[:, 0], np.asarray(pos, dtype)[:, 1]
    one = dtype(1)
    idepth = np.asarray(idepth, dtype)
    with np.errstate(all="ignore"):
        h = [(K[3 * r] * px + K[3 * r + 1] * py) + K[3 * r + 2] * one for r in range(3)]
        return [c / idepth for c in h]


def triangle_geometry(pos, idepth, tris, Kinv, dtype=np.float32):
    """Per triangle: d = ray . inward normal, the outward unit normal (3 arrays) and the corner idepths."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    P = backproject(pos, idepth, Kinv, dtype)
    a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
    with np.errstate(all="ignore"):
        p0, p1, p2 = [q[a] for q in P], [q[b] for q in P], [q[c] for q in P]
        delta1 = [p1[i] - p0[i] for i in range(3)]
        delta2 = [p2[i] - p0[i] for i in range(3)]
        normal = _normalize3(_cross3(delta1, delta2))  # inward, flame.cc:2242-2245
        three = dtype(3)
        ray = _normalize3([((p0[i] + p1[i]) + p2[i]) / three for i in range(3)])
        d = _dot3(ray, normal)
        outward = _normalize3(_cross3(delta2, delta1))  # flame.cc:2609-2612
    idepth = np.asarray(idepth, dtype)
    return d, outward, (idepth[a], idepth[b], idepth[c])


def angle_rejects(d, thresh):
    """The literal test of flame.cc:2252-2253 per triangle: float32(arccos(float64(d))) > thresh."""
    with np.errstate(all="ignore"):
        angle = np.abs(np.arccos(np.asarray(d, np.float32).astype(np.float64)).astype(np.float32))
        return angle > np.float32(thresh)


def _ord(f):
    u = int(np.float32(f).view(np.uint32))
    return -(u & 0x7FFFFFFF) - 1 if u & 0x80000000 else u


def _from_ord(o):
    u = ((-(o + 1)) | 0x80000000) if o < 0 else o
    return np.uint32(u).view(np.float32)


def next_float(f, k=1):
    """The float k steps above (k < 0: below) f in numeric order (-0 sits one step below +0)."""
    return _from_ord(_ord(f) + k)


def oblique_cos_bound(thresh):
    """D*: the smallest float in [-1, 1] with float32(arccos(float64(D))) <= thresh (== flame_nltgv2_oblique_cos_bound)."""
    thresh = np.float32(thresh)

    def accepted(dv):
        return np.float32(np.arccos(np.float64(np.float32(dv)))) <= thresh

    if np.isnan(thresh):
        return np.float32(-1)
    if accepted(-1.0):
        return np.float32(-1)
    if not accepted(1.0):
        return np.float32(np.inf)
    lo, hi = _ord(-1.0), _ord(1.0)
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if accepted(_from_ord(mid)):
            hi = mid
        else:
            lo = mid
    return _from_ord(hi)


def bound_rejects(d, bound):
    """The device's form of the angle test."""
    d = np.asarray(d, np.float32)
    with np.errstate(all="ignore"):
        return (d >= np.float32(-1)) & (d <= np.float32(1)) & (d < np.float32(bound))


def filter_tests(pos, idepth, tris, Kinv, cols, p=None, dtype=np.float32):
    """The five comparisons, each as a boolean array `clears validity`, regardless of the do_* switches:
    angle, rel (relative idepth difference), abs, edge (edge length), mean (mean idepth)."""
    p = params() if p is None else p
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    d, _, (id0, id1, id2) = triangle_geometry(pos, idepth, tris, Kinv, dtype)
    out = {}
    with np.errstate(all="ignore"):
        if dtype == np.float32:
            out["angle"] = angle_rejects(d, p["oblique_normal_thresh"])
        else:
            out["angle"] = np.abs(np.arccos(d)) > dtype(p["oblique_normal_thresh"])
        min_id = np.where(id0 < id1, id0, id1)
        min_id = np.where(min_id < id2, min_id, id2)
        max_id = np.where(id0 > id1, id0, id1)
        max_id = np.where(max_id > id2, max_id, id2)
        out["rel"] = (max_id - min_id) / max_id > dtype(p["oblique_idepth_diff_factor"])
        out["abs"] = max_id - min_id > dtype(p["oblique_idepth_diff_abs"])
        thresh2 = dtype(p["edge_length_thresh"]) * dtype(cols)  # flame.cc:2297-2298
        thresh2 = thresh2 * thresh2
        xy = np.asarray(pos, dtype)
        v0, v1, v2 = xy[tris[:, 0]], xy[tris[:, 1]], xy[tris[:, 2]]

        def dist2(u, v):
            dx, dy = u[:, 0] - v[:, 0], u[:, 1] - v[:, 1]
            return dx * dx + dy * dy

        out["edge"] = (dist2(v0, v1) > thresh2) | (dist2(v0, v2) > thresh2) | (dist2(v1, v2) > thresh2)
        out["mean"] = ((id0 + id1) + id2) / dtype(3) < dtype(p["min_triangle_idepth"])
    return out


def triangle_validity(pos, idepth, tris, Kinv, cols, p=None, dtype=np.float32):
    p = params() if p is None else p
    t = filter_tests(pos, idepth, tris, Kinv, cols, p, dtype)
    valid = np.ones(len(t["angle"]), bool)
    if p["do_oblique_triangle_filter"]:
        valid &= ~(t["angle"] | t["rel"] | t["abs"])
    if p["do_edge_length_filter"]:
        valid &= ~t["edge"]
    if p["do_idepth_triangle_filter"]:
        valid &= ~t["mean"]
    return valid.astype(np.uint8)


def vertex_normals(pos, idepth, tris, Kinv, dtype=np.float32):
    """getVertexNormals, flame.cc:2575-2631: a plain loop over the triangles, the running mean per corner."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    V = len(idepth)
    _, outward, (id0, id1, id2) = triangle_geometry(pos, idepth, tris, Kinv, dtype)
    with np.errstate(all="ignore"):
        skip = (id0 <= 0) | (id1 <= 0) | (id2 <= 0)  # flame.cc:2585
    normals = np.zeros((V, 3), dtype)
    counts = np.zeros(V, np.int64)
    on = np.stack(outward, axis=1).astype(dtype)
    zero = dtype(0)
    with np.errstate(all="ignore"):
        for t in range(len(tris)):
            if skip[t]:
                continue
            for v in tris[t]:
                c0, c1 = dtype(counts[v]), dtype(counts[v] + 1)
                n = [(c0 * normals[v, i] + on[t, i]) / c1 for i in range(3)]
                z = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
                if z > zero:
                    s = np.sqrt(z)
                    n = [n[0] / s, n[1] / s, n[2] / s]
                normals[v] = n
                counts[v] += 1
    return normals


def mesh_outputs(pos, x, tris, Kinv, rows, cols, graph_scale=1.0, p=None):
    """All outputs of flame_nltgv2_mesh_outputs except the filtered map (the rasteriser has its own checker)."""
    del rows
    idepth = vertex_idepths(x, graph_scale)
    valid = triangle_validity(pos, idepth, tris, Kinv, cols, p)
    return dict(vtx_idepth=idepth, tri_valid=valid, n_valid=int(valid.sum()), normals=vertex_normals(pos, idepth, tris, Kinv))
