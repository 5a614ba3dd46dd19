"""Float64 statements of the two per-frame graph maintenance operations, written from their definitions.

projectGraph (flame.cc:1888-1905 with EpipolarGeometry::project, stereo/epipolar_geometry.h:152-180).  A vertex at pixel u
with inverse depth idepth = x * graph_scale is taken to the other camera:

    idepth != 0:  P = R (Kinv [u; 1] / idepth) + t,   u_new = (K P)_xy / (K P)_z,   idepth_new = 1 / P_z
    idepth == 0:  h = KRKinv [u; 1],                  u_new = h_xy / h_z,           idepth_new = 0
    x_new = idepth_new / graph_scale
    keep  = u_new in [rx, rx + rw) x [ry, ry + rh)  and not (idepth_new < 0)

R is the rotation matrix of the quaternion q = (w, x, y, z), R = I + 2 w [v]x + 2 [v]x^2 with v = (x, y, z) (what q p q* is for
a unit q; q is used as given, not normalised).  The inputs are the float32 numbers the device gets, every operation on them is
float64; nothing is shared with oracle/photometric_oracle.c (no quaternion product in steps, matrices as matrices).

rescale_data (flame.cc:328-351):

    new_scale = mean(data_term * graph_scale);   x, x_bar, x_prev, data_term *= graph_scale / new_scale
    data_factor *= new_scale / graph_scale

with the mean from math.fsum (correctly rounded)."""
import math

import numpy as np

U32 = 2.0 ** -24  # unit roundoff of float32: one rounding to nearest changes a value by at most U32 * |value|


def rotation_from_quaternion(q):
    w, x, y, z = (float(v) for v in np.asarray(q, np.float32))
    S = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    return np.eye(3) + 2.0 * w * S + 2.0 * (S @ S)


def _f64(a, shape):
    return np.asarray(np.asarray(a, np.float32), np.float64).reshape(shape)


def project64(pos, x, graph_scale, K, Kinv, q, t, KRKinv, region):
    """-> dict(pos (V, 2), x (V,), idepth (V,), z (V,), keep (V,) bool, at_inf (V,) bool), all float64.  z is the third
    coordinate of the point in the other camera (of h for a vertex at infinity): the number u_new was divided by."""
    K, Kinv, M = _f64(K, (3, 3)), _f64(Kinv, (3, 3)), _f64(KRKinv, (3, 3))
    R, t = rotation_from_quaternion(q), _f64(t, (3, 1))
    gs = float(np.float32(graph_scale))
    u = _f64(pos, (-1, 2))
    hom = np.stack([u[:, 0], u[:, 1], np.ones(len(u))])  # (3, V)
    idepth = _f64(x, (-1,)) * gs
    at_inf = idepth == 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        P = R @ ((Kinv @ hom) / np.where(at_inf, 1.0, idepth)) + t
        h = np.where(at_inf, M @ hom, K @ P)
        z = np.where(at_inf, h[2], P[2])
        new_pos = np.stack([h[0] / h[2], h[1] / h[2]], 1)
        new_idepth = np.where(at_inf, 0.0, 1.0 / P[2])
        new_x = new_idepth / gs
    rx, ry, rw, rh = (float(np.float32(r)) for r in region)
    inside = (rx <= new_pos[:, 0]) & (new_pos[:, 0] < rx + rw) & (ry <= new_pos[:, 1]) & (new_pos[:, 1] < ry + rh)
    return dict(pos=new_pos, x=new_x, idepth=new_idepth, z=z, keep=inside & ~(new_idepth < 0), at_inf=at_inf)


def project_bound(pos, x, graph_scale, K, Kinv, q, t, KRKinv):
    """Per-vertex bounds of |float32 evaluation - project64|: (position bound (V, 2) in pixels, bound of x_new (V,), bound of z (V,)).

    Every float32 operation rounds its exact result by at most U32 relative (no operand here is near the denormals).  Written
    e(.) for the error bound and m(.) for a magnitude sum (the sum of the absolute values of the terms a quantity is made of; a
    rounding of a partial sum is at most U32 m), to first order in U32:

      idepth = x * scale, depth = 1 / idepth         2 roundings: e(depth) = 2 U |depth|
      Kinv:  p_i = Kinv_ii u_i + Kinv_i2             2 roundings: e = 2 U m(p_i),  m(p_i) = |Kinv_ii u_i| + |Kinv_i2|;  p_2 = 1
      scale: a_i = p_i depth                         e(a_i) = (2 + 2 + 1) U m(a_i), m(a_i) = m(p_i) |depth|;  e(a_2) = 2 U |depth|
      quaternion rotation  r = a + w (2 v x a) + v x (2 v x a):
        c = v x a     per component two products and a difference: e(c) = |v| x e(a) + 2 U m(c), m(c) = |v| x m(a)   (|.| x |.|:
                      the cross product with every term taken positive); doubling is exact: d = 2 c
        f = v x d     e(f) = |v| x e(d) + 2 U m(f),  m(f) = |v| x m(d)
        r_i = (a_i + w d_i) + f_i                    3 roundings, each of a partial sum: e(r_i) = e(a_i) + |w| e(d_i) + e(f_i) + 3 U m(r_i),
                                                     m(r_i) = m(a_i) + |w| m(d_i) + m(f_i)
      + t:   P_i = r_i + t_i                         e(P_i) = e(r_i) + U m(P_i),  m(P_i) = m(r_i) + |t_i|
      K:     g_i = K_ii P_i + K_i2 P_2  (i = 0, 1)   e(g_i) = |K_ii| e(P_i) + |K_i2| e(P_2) + 2 U (|K_ii| m(P_i) + |K_i2| m(P_2))
      reciprocal  n = 1 / P_2                        e(n) / |n| = e(P_2) / |P_2| + U
      multiply    u_new_i = g_i n                    e(u_new_i) = (e(g_i) + |u_new_i| e(P_2)) / |P_2| + 2 U |u_new_i|
      x_new = n / scale                              e(x_new) = |x_new| (e(P_2) / |P_2| + 2 U)
    and for a vertex at infinity, h_i = (M_i0 u_0 + M_i1 u_1) + M_i2: at most 3 roundings per term, e(h_i) = 3 U m(h_i);
      u_new_i = h_i (1 / h_2): e(u_new_i) = (e(h_i) + |u_new_i| e(h_2)) / |h_2| + 2 U |u_new_i|;  x_new = 0 exactly.

    The bounds returned are these, DOUBLED for margin (the terms of second order).  z is P_2 (h_2 at infinity) with e(P_2)."""
    U = U32
    r = project64(pos, x, graph_scale, K, Kinv, q, t, KRKinv, (0, 0, 1, 1))
    K, Kinv, M = np.abs(_f64(K, (3, 3))), np.abs(_f64(Kinv, (3, 3))), np.abs(_f64(KRKinv, (3, 3)))
    w, vx, vy, vz = (abs(float(v)) for v in np.asarray(q, np.float32))
    t = np.abs(_f64(t, (3,)))
    u = np.abs(_f64(pos, (-1, 2)))
    gs = float(np.float32(graph_scale))

    def cross_abs(a):  # |v| x a with every term positive
        return [vy * a[2] + vz * a[1], vz * a[0] + vx * a[2], vx * a[1] + vy * a[0]]

    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        depth = np.abs(1.0 / (_f64(x, (-1,)) * gs))
        m_p = [Kinv[0, 0] * u[:, 0] + Kinv[0, 2], Kinv[1, 1] * u[:, 1] + Kinv[1, 2]]
        m_a = [m_p[0] * depth, m_p[1] * depth, depth]
        e_a = [5 * U * m_a[0], 5 * U * m_a[1], 2 * U * depth]
        m_c = cross_abs(m_a)
        e_c = [ec + 2 * U * mc for ec, mc in zip(cross_abs(e_a), m_c)]
        m_d, e_d = [2 * v for v in m_c], [2 * v for v in e_c]
        m_f = cross_abs(m_d)
        e_f = [ef + 2 * U * mf for ef, mf in zip(cross_abs(e_d), m_f)]
        m_r = [m_a[i] + w * m_d[i] + m_f[i] for i in range(3)]
        e_r = [e_a[i] + w * e_d[i] + e_f[i] + 3 * U * m_r[i] for i in range(3)]
        m_P = [m_r[i] + t[i] for i in range(3)]
        e_P = [e_r[i] + U * m_P[i] for i in range(3)]
        e_g = [K[i, i] * e_P[i] + K[i, 2] * e_P[2] + 2 * U * (K[i, i] * m_P[i] + K[i, 2] * m_P[2]) for i in range(2)]
        e_h = [3 * U * (M[i, 0] * u[:, 0] + M[i, 1] * u[:, 1] + M[i, 2]) for i in range(3)]
        inf = r["at_inf"]
        e_z = np.where(inf, e_h[2], e_P[2])
        absz, c = np.abs(r["z"]), np.abs(r["pos"])
        b_pos = np.stack([(np.where(inf, e_h[i], e_g[i]) + c[:, i] * e_z) / absz + 2 * U * c[:, i] for i in range(2)], 1)
        b_x = np.where(inf, 0.0, np.abs(r["x"]) * (e_z / absz + 2 * U))
    return 2 * b_pos, 2 * b_x, 2 * e_z


def rescale64(x, x_bar, x_prev, data_term, graph_scale, data_factor, new_scale=None):
    """-> dict(new_scale, x, x_bar, x_prev, data_term, data_factor, mean_abs).  new_scale: the mean, or -- to state the
    arrays for a given (float32) new_scale -- the one passed in.  mean_abs is mean(|data_term * graph_scale|)."""
    gs = float(np.float32(graph_scale))
    d = _f64(data_term, (-1,))
    V = len(d)
    terms = [float(v) * gs for v in d]
    mean = math.fsum(terms) / V
    ns = mean if new_scale is None else float(np.float32(new_scale))
    out = dict(new_scale=mean, mean_abs=math.fsum(abs(v) for v in terms) / V)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for name, a in (("x", x), ("x_bar", x_bar), ("x_prev", x_prev), ("data_term", data_term)):
            out[name] = _f64(a, (-1,)) * gs / ns
        out["data_factor"] = float(np.float32(data_factor)) * (ns / gs)
    return out
