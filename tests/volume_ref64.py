"""A float64 look at the volumetric map (include/flame_nltgv2.h, flame_nltgv2_volume_create), independent of tests/volume_ref.py: that
checker restates the kernels operation for operation, which is right for bit-exactness and blind to a rule mis-stated in both places.
Here the rules of the header are written as plain float64 numpy -- matrix products, one division, np.rint for the nearest pixel -- with
none of the checker's sequence of roundings, and every value carries a bound `e` on how far a float32 evaluation of the same expression
may lie from it.  The bounds follow the rules at the top of tests/stereo_update_ref64.py, vectorised (EPS = 2^-24; the inputs are float32
numbers, so their e = 0):
    x + y, x - y   e = ex + ey + EPS (|x| + |y|)       a sum is charged for the magnitudes of its terms, not of its result, so the bound
                                                       does not depend on the order in which float32 adds them
    M x (+ t)      e_i = sum_j |M_ij| ex_j + EPS sum_j |M_ij x_j| + adds * EPS (sum_j |M_ij x_j| + |t_i|)
    x * y          e = |x| ey + |y| ex + ex ey + EPS |x y|
    x / y          e = (ex + |x / y| ey) / (|y| - ey) + EPS |x / y|       (infinite when y's interval holds 0)
No value of the cases this serves is subnormal.  A decision `x < threshold` is DOUBTFUL when |x - threshold| <= e.

    integrate        one call on a given state of the volume -> the decisions, the new tsdf and weight with their bounds, the doubtful voxels
    plane_volume     a volume whose tsdf is an exact tilted plane, computed in float64 and rounded once; every weight 1
    ray_plane        the float64 intersection of the pixels' rays with that plane, the slope of the field along each ray and the constant
                     c of the bound c (EPS M / slope + EPS z) on the raycast's depth, derived there by counting roundings
"""
import numpy as np

F = np.float32
EPS = 2.0 ** -24
FLT_MAX = 3.4028234663852886e38


def _affine(M, t, x, ex):
    """M (3x3) x + t (t may be None) on three arrays -> three values, three bounds."""
    out, err = [], []
    for i in range(3):
        terms = [M[i, j] * x[j] for j in range(3)]
        mag = sum(np.abs(term) for term in terms)
        v = terms[0] + terms[1] + terms[2]
        e = sum(abs(M[i, j]) * ex[j] for j in range(3)) + EPS * mag
        adds = 2
        if t is not None:
            v, mag, adds = v + t[i], mag + abs(t[i]), 3
        out.append(v)
        err.append(e + adds * EPS * mag)
    return out, err


def _quotient(x, ex, y, ey):
    with np.errstate(all="ignore"):
        r = x / y
        e = (ex + np.abs(r) * ey) / (np.abs(y) - ey) + EPS * np.abs(r)
    return r, np.where(np.abs(y) > ey, e, np.inf)


def integrate(nx, ny, nz, voxel_size, origin, trunc, max_weight, tsdf, weight_old, idepthmap, K, T_cam_world, weight=1.0, near_depth=0.0,
              min_depth=0.0, max_depth=np.inf):
    """Rules 1 - 9 for one call on the state (tsdf, weight_old), both (nz, ny, nx) float32.  -> dict: the float64 decisions front,
    in_image, valid, behind, updated; tsdf and weight after the call with e_tsdf, e_weight; doubt, the voxels one of whose decisions lies
    within its bound of its threshold.  Every parameter is taken as the float32 number the device gets."""
    f8 = np.float64
    vs, tr, mw, wgt = (f8(F(v)) for v in (voxel_size, trunc, max_weight, weight))
    near, dmin, dmax = (f8(F(v)) for v in (near_depth, min_depth, max_depth))
    o = np.asarray(origin, F).astype(f8)
    K = np.asarray(K, F).astype(f8).reshape(3, 3)
    T = np.asarray(T_cam_world, F).astype(f8).reshape(3, 4)
    m = np.asarray(idepthmap, F).astype(f8)
    rows, cols = m.shape
    t_old, w_old = np.asarray(tsdf, F).astype(f8), np.asarray(weight_old, F).astype(f8)
    kk, jj, ii = np.indices((nz, ny, nx)).astype(f8)
    with np.errstate(all="ignore"):
        # 1 centre
        p, ep = [], []
        for a, ind in enumerate((ii, jj, kk)):
            step = ind * vs
            p.append(o[a] + step)
            ep.append(EPS * np.abs(step) + EPS * (abs(o[a]) + np.abs(step)))
        P, eP = _affine(T[:, :3], T[:, 3], p, ep)
        # 2 front
        front = P[2] > near
        doubt = np.abs(P[2] - near) <= eP[2]
        # 3 projection
        q, eq = _affine(K, None, P, eP)
        u, eu = _quotient(q[0], eq[0], q[2], eq[2])
        v, ev = _quotient(q[1], eq[1], q[2], eq[2])
        # 4 in image
        in_image = front & (u >= -0.5) & (u < cols - 0.5) & (v >= -0.5) & (v < rows - 0.5)
        border = (np.abs(u + 0.5) <= eu) | (np.abs(u - (cols - 0.5)) <= eu) | (np.abs(v + 0.5) <= ev) | (np.abs(v - (rows - 0.5)) <= ev)
        doubt |= front & (border | ~np.isfinite(eu) | ~np.isfinite(ev))
        # 5 the nearest pixel: floorf(x + 0.5f) and rint(x) part only at a tie, which is doubtful
        pixel = np.zeros(u.shape, bool)
        idx = []
        for x, ex, n in ((u, eu, cols), (v, ev, rows)):
            xs = np.where(in_image, x, 0.0)
            xh, exh = xs + 0.5, ex + EPS * (np.abs(xs) + 0.5)
            pixel |= np.abs(xh - np.rint(xh)) <= exh
            idx.append(np.clip(np.rint(xs), 0, n - 1).astype(np.int64))
        doubt |= in_image & pixel
        # 6 validity
        d = m[idx[1], idx[0]]
        zm = 1.0 / d
        ezm = EPS * np.abs(zm)
        valid = in_image & (d > 0) & (zm > dmin) & (zm < dmax)
        doubt |= in_image & (d > 0) & ((np.abs(zm - dmin) <= ezm) | (np.abs(zm - dmax) <= ezm) | (zm + ezm >= FLT_MAX))
        # 7 distance
        sdf = zm - P[2]
        esdf = ezm + eP[2] + EPS * (np.abs(zm) + np.abs(P[2]))
        behind = valid & (sdf < -tr)
        doubt |= valid & (np.abs(sdf + tr) <= esdf)
        updated = valid & ~behind
        # 8 truncation
        r = sdf / tr
        er = esdf / tr + EPS * np.abs(r)
        doubt |= updated & (np.abs(r - 1.0) <= er)
        s = np.minimum(r, 1.0)
        # 9 update
        a, b = t_old * w_old, s * wgt
        ea, eb = EPS * np.abs(a), wgt * er + EPS * np.abs(b)
        num, enum = a + b, ea + eb + EPS * (np.abs(a) + np.abs(b))
        W, eW = w_old + wgt, EPS * (np.abs(w_old) + wgt)
        t_new, et = _quotient(num, enum, W, eW)
        w_new = np.minimum(W, mw)
    return dict(front=front, in_image=in_image, valid=valid, behind=behind, updated=updated, doubt=doubt,
                tsdf=np.where(updated, t_new, t_old), e_tsdf=np.where(updated, et, 0.0),
                weight=np.where(updated, w_new, w_old), e_weight=np.where(updated, eW, 0.0))


# ---- the raycast of an exact plane --------------------------------------------------------------------------------------------------------
def plane_volume(nx, ny, nz, voxel_size, origin, trunc, normal, point):
    """-> (tsdf, weight), (nz, ny, nx) float32: tsdf = ((p - point) . n) / trunc at the voxel centres p = origin + index * voxel_size, the
    float32 parameters taken as real numbers, n = normal / |normal|; computed in float64 and rounded once."""
    f8 = np.float64
    vs, tr = f8(F(voxel_size)), f8(F(trunc))
    o = np.asarray(origin, F).astype(f8)
    n = np.asarray(normal, f8) / np.linalg.norm(np.asarray(normal, f8))
    c0 = np.asarray(point, f8)
    kk, jj, ii = np.indices((nz, ny, nx)).astype(f8)
    field = sum(((o[a] + ind * vs) - c0[a]) * n[a] for a, ind in enumerate((ii, jj, kk))) / tr
    return field.astype(F), np.ones((nz, ny, nx), F)


def ray_plane(q, T_world_cam, voxel_size, origin, trunc, normal, point, tsdf, dz):
    """q: the three (rows, cols) float32 arrays Kinv (col, row, 1) as the device forms them (the ray IS that float32 triple); the rest as
    in plane_volume.  -> dict: z, the ray parameter at which p = T_world_cam (q z) meets the plane; slope = |n . (R q)| / trunc, the
    field's derivative in z along the ray; M = max |tsdf|; c (below).

    Trilinear interpolation reproduces a linear field, so the raycast's z* = z_prev + dz (f_prev / (f_prev - f_cur)) is the intersection
    up to rounding: |z* - z| <= c (EPS M / slope + EPS z).  Counting the roundings of the rule, each against its unit:
      the value f of a sample, unit EPS M (every intermediate is at most M in magnitude, and so is every difference b - a of a lerp: both
      are asserted below):
         1   the stored values, rounded once each; a sample is a convex combination of eight of them
         9   the lerps a + t (b - a): three roundings each; seven lerps in three levels, and a level hands the errors of the level
             before on with weights that sum to 1, so three levels count, not seven lerps
         7 r the grid coordinate, per axis q_i z (1), the three products of the pose (1), its three sums (3), minus the origin (1), the
             division (1); f = g - i0 is exact.  Each is at most EPS L in metres, L = sum_j |R_aj q_j| z + |t_a| + |origin_a| at its
             largest over the rays and axes; a shift of the sample by that much along every axis moves the value by at most
             |n|_1 EPS L / trunc = r EPS M with r = |n|_1 L / (trunc M)
      f_prev > 0 >= f_cur, so |d lambda| <= df / (f_prev - f_cur) for lambda = f_prev / (f_prev - f_cur), and f_prev - f_cur = slope dz:
      an error df of both values moves z* by df / slope.  That is (10 + 7 r) EPS M / slope.
      the crossing, unit EPS z (dz <= z):
         3   f_prev - f_cur, the division, the product with dz: relative roundings of a term that is at most dz
         1   the sum z_prev + ...
         4   the samples lie at the float32 numbers z_n = z_near + (float)n dz (two roundings each); z_prev is the same float32 number in
             the crossing, but z_cur - z_prev is dz only within those four roundings
         2   the pixel 1 / (z* q.z): a product and a division, undone here in float64
      That is 10 EPS z.  So c = max(10 + 7 r, 10) = 10 + 7 r."""
    f8 = np.float64
    tr = f8(F(trunc))
    o = np.asarray(origin, F).astype(f8)
    T = np.asarray(T_world_cam, F).astype(f8).reshape(3, 4)
    R, t = T[:, :3], T[:, 3]
    n = np.asarray(normal, f8) / np.linalg.norm(np.asarray(normal, f8))
    c0 = np.asarray(point, f8)
    q = [np.asarray(a, F).astype(f8) for a in q]
    d = [R[a, 0] * q[0] + R[a, 1] * q[1] + R[a, 2] * q[2] for a in range(3)]  # R q
    nd = n[0] * d[0] + n[1] * d[1] + n[2] * d[2]
    with np.errstate(all="ignore"):
        z = np.dot(c0 - t, n) / nd
    t32 = np.asarray(tsdf, F).astype(f8)
    M = np.abs(t32).max()
    steps = max(np.abs(np.diff(t32, axis=a)).max() for a in range(3))
    assert steps <= M, "a lerp's difference b - a is larger than the unit of the count"
    zmax = np.abs(z) + f8(F(dz))
    L = np.maximum.reduce([sum(abs(R[a, j]) * np.abs(q[j]) for j in range(3)) * zmax + abs(t[a]) + abs(o[a]) for a in range(3)])
    return dict(z=z, slope=np.abs(nd) / tr, M=M, L=L, n1=np.abs(n).sum(), trunc=tr)


def crossing_c(plane, hit):
    """The derived constant for the rays `hit` (bool, rows x cols) of a ray_plane result."""
    r = plane["n1"] * plane["L"][hit].max() / (plane["trunc"] * plane["M"])
    return 10.0 + 7.0 * r
