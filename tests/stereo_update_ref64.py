"""Float64 restatements of the stages of the per-feature stereo update that lie around the epipolar walk -- predict, the
search region, the valid rectangle, the measurement model, the fusion, fail_feature -- for
tests/test_stereo_update_edges.py.  Written from the formulas (inverse_depth_filter.cc:36-176, :265-303,
inverse_depth_meas_model.cc:48-154, epipolar_geometry.h:127-405, flame.cc:1538-1752), not from oracle/stereo_oracle.c: the
rotation is a matrix product, the clip is a slab intersection, a quotient is one division.  A Geometry of
oracle.stereo_capi (its fields have known-answer tests of their own, tests/test_stereo.py) and float32 inputs go in; values
and the decision taken come out.

Every value is an R32: a float64 number `v` together with `e`, a running bound on how far a float32 evaluation of the same
expression may lie from v.  The rules (EPS = 2^-24, the float32 unit roundoff; inputs are float32 numbers, so e = 0):
    x + y, x - y   e = ex + ey + EPS (|x| + |y|)        (not EPS |x + y|: then a sum's bound does not depend on the order
                                                         in which float32 adds its terms)
    x * y          e = |x| ey + |y| ex + ex ey + EPS |x y|
    x / y          e = (ex + |x / y| ey) / (|y| - ey) + EPS |x / y|      (infinite when y's interval holds 0)
    sqrt(x)        e = ex / (sqrt(x - ex) + sqrt(x)) + EPS sqrt(x)
    bilinear       e = (ex + ey) * (largest difference of neighbouring pixels around the sample) + 8 EPS max|pixel|;
                   where the position is uncertain by a pixel or more, the spread of the pixels it may touch
plus 2^-149 per operation for results that are subnormal.  The conditioning -- 1 / h2 of a projection, 1 / pc.z,
1 / ATA, 1 / edn^2, 1 / edg^2, the slope of a clipped segment -- enters through the division rule, from the float64
values.  A decision `x < threshold` is doubtful when |x - threshold| <= e; Doubt collects those.  The rules charge a sum
for the magnitudes of its terms, not of its result: that is what leaves room for the float32 code adding in another
order, or splitting a quotient into a reciprocal and a product (one more EPS on a value whose sums were charged double).
"""
from __future__ import annotations

import math

import numpy as np

EPS = 2.0 ** -24
TINY = 2.0 ** -149
INF = float("inf")
FLT_MAX = 3.4028234663852886e38


class R32:
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v, self.e = float(v), float(e)

    @staticmethod
    def of(x):
        return x if isinstance(x, R32) else R32(x)

    def checked(self):
        if not abs(self.v) <= FLT_MAX:      # float32 overflows (or the value is a NaN): nothing is known
            self.e = INF
        return self

    def exact_zero(self):
        return self.v == 0.0 and self.e == 0.0

    def __neg__(self):
        return R32(-self.v, self.e)

    def __abs__(self):
        return R32(abs(self.v), self.e)

    def __add__(self, o):
        o = R32.of(o)
        if o.exact_zero():
            return self
        if self.exact_zero():
            return o
        return R32(self.v + o.v, self.e + o.e + EPS * (abs(self.v) + abs(o.v)) + TINY).checked()

    __radd__ = __add__

    def __sub__(self, o):
        if o is self:
            return R32(0.0)     # x - x of one float32 number is 0 exactly
        return self + (-R32.of(o))

    def __rsub__(self, o):
        return R32.of(o) + (-self)

    def __mul__(self, o):
        o = R32.of(o)
        if o.exact_zero() or self.exact_zero():
            return R32(0.0)
        v = self.v * o.v
        return R32(v, abs(self.v) * o.e + abs(o.v) * self.e + self.e * o.e + EPS * abs(v) + TINY).checked()

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = R32.of(o)
        if self.exact_zero() and o.v != 0.0:
            return R32(0.0)
        if abs(o.v) <= o.e:
            return R32(self.v / o.v if o.v != 0.0 else INF, INF)
        v = self.v / o.v
        return R32(v, (self.e + abs(v) * o.e) / (abs(o.v) - o.e) + EPS * abs(v) + TINY).checked()

    def __rtruediv__(self, o):
        return R32.of(o) / self

    def sqrt(self):
        if self.exact_zero():
            return self
        v = math.sqrt(max(self.v, 0.0))
        lo = math.sqrt(max(self.v - self.e, 0.0))
        return R32(v, (self.e / (lo + v) if lo + v > 0.0 else math.sqrt(self.e)) + EPS * v + TINY)

    def __repr__(self):
        return "R32(%r +- %.3g)" % (self.v, self.e)


class Doubt:
    """Collects the decisions that a float32 evaluation may take the other way.
    decide: {decision name: outcome} for a feature whose inputs were SET ON that decision's threshold: the case states
    what exact arithmetic gives, float64 follows it and goes on, so that the values behind the decision are compared too."""

    def __init__(self, decide=None):
        self.why = []
        self.decide = dict(decide or {})

    def lt(self, a, b, name):
        """a < b, by the float64 values."""
        if name in self.decide:
            return bool(self.decide[name])
        a, b = R32.of(a), R32.of(b)
        d, e = a.v - b.v, a.e + b.e
        if e > 0.0 and abs(d) <= e or math.isnan(d) or math.isinf(e):
            self.why.append(name)
        return d < 0.0

    def flag(self, name):
        self.why.append(name)

    def __bool__(self):
        return bool(self.why)


class Geo64:
    """The fields of a stereo_capi.Geometry as Python floats."""

    def __init__(self, g):
        for n in ("K", "Kinv", "q", "t", "tcr", "KRKinv", "Kt"):
            setattr(self, n, [float(v) for v in getattr(g, n)])
        self.epx, self.epy = float(g.epx), float(g.epy)
        w, x, y, z = self.q
        # rotation matrix of the (unit up to roundoff) quaternion, each entry with its float32 bound
        W, X, Y, Z = R32(w), R32(x), R32(y), R32(z)
        self.R = [[1.0 - 2.0 * (Y * Y + Z * Z), 2.0 * (X * Y - W * Z), 2.0 * (X * Z + W * Y)],
                  [2.0 * (X * Y + W * Z), 1.0 - 2.0 * (X * X + Z * Z), 2.0 * (Y * Z - W * X)],
                  [2.0 * (X * Z - W * Y), 2.0 * (Y * Z + W * X), 1.0 - 2.0 * (X * X + Y * Y)]]
        if (x, y, z) == (0.0, 0.0, 0.0) and w == 1.0:
            self.R = [[R32(float(i == j)) for j in range(3)] for i in range(3)]

    def rotate(self, p):
        return [self.R[i][0] * p[0] + self.R[i][1] * p[1] + self.R[i][2] * p[2] for i in range(3)]


def rect_contains(vx, vy, vw, vh, px, py):
    """cv::Rect(vx, vy, vw, vh).contains(Point2f): the point becomes integer by cvRound, ties to even (Python's round)."""
    ix, iy = round(float(px)), round(float(py))
    return vx <= ix < vx + vw and vy <= iy < vy + vh


def rect_contains_r32(rect, px, py, D, name):
    """rect_contains of a computed point; doubtful when the point's interval reaches across a rounding tie that matters."""
    if name in D.decide:
        return bool(D.decide[name])
    inside = rect_contains(*rect, px.v, py.v)
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            if math.isfinite(px.e + py.e) and rect_contains(*rect, px.v + sx * px.e, py.v + sy * py.e) != inside:
                D.flag(name)
                return inside
    if not math.isfinite(px.e + py.e):
        D.flag(name)
    return inside


def valid_rect(P, width, height):
    row_offset = height // 3 if P.do_letterbox else 0
    border = int(np.float32(np.float32(P.rescale_factor_max) * np.float32(P.win_size)) / np.float32(2) + np.float32(1))
    return border, border + row_offset, width - 2 * border, height - 2 * border - 2 * row_offset


def max_depth_projection64(g, ux, uy):
    M = g.KRKinv
    h = [M[3 * i] * R32(ux) + M[3 * i + 1] * R32(uy) + R32(M[3 * i + 2]) for i in range(3)]
    return h[0] / h[2], h[1] / h[2]


def project64(g, ux, uy, idepth):
    """EpipolarGeometry::project (epipolar_geometry.h:127-143) of an inverse depth > 0, or == 0 exactly."""
    idepth = R32.of(idepth)
    if idepth.exact_zero():
        return max_depth_projection64(g, ux, uy)
    M = g.KRKinv
    depth = 1.0 / idepth
    h = [M[3 * i] * (ux * depth) + M[3 * i + 1] * (uy * depth) + M[3 * i + 2] * depth + g.Kt[i] for i in range(3)]
    return h[0] / h[2], h[1] / h[2]


def predict64(g, process_var_factor, ux, uy, mu, var, D):
    """inverse_depth_filter::predict.  -> dict(decision "assert" | "no" | "yes", x, y, mu_pred, var_pred, forced)."""
    mu, var = float(mu), float(var)
    if not mu >= 0.0:
        return dict(decision="assert")
    forced = mu < 1e-6            # the float32 input against the double constant: exact
    if mu == 0.0:
        x, y = max_depth_projection64(g, ux, uy)
        mu_pred = R32(0.0)
    else:
        depth = 1.0 / R32(mu)
        p = [(g.Kinv[0] * R32(ux) + g.Kinv[2]) * depth, (g.Kinv[4] * R32(uy) + g.Kinv[5]) * depth, depth]
        pc = [a + b for a, b in zip(g.rotate(p), g.t)]
        if pc[2].v == 0.0 and pc[2].e == 0.0:
            return dict(decision="assert")
        if abs(pc[2].v) <= pc[2].e:
            D.flag("pc.z against 0")
        mu_pred = 1.0 / pc[2]
        x = (g.K[0] * pc[0] + g.K[2] * pc[2]) / pc[2]
        y = (g.K[4] * pc[1] + g.K[5] * pc[2]) / pc[2]
    if D.lt(mu_pred, 0.0, "mu_pred < 0"):
        return dict(decision="no", x=x, y=y, mu_pred=R32(0.0), var_pred=R32(1e10), forced=forced)
    if forced:
        f4 = R32(1.0)
    else:
        f = mu_pred / mu
        f = f * f
        f4 = f * f
    return dict(decision="yes", x=x, y=y, mu_pred=mu_pred, var_pred=process_var_factor * f4 * var, forced=forced)


def _clip64(lo, hi, a, b, D, name):
    """The part of the segment a -> b inside [lo.x, hi.x] x [lo.y, hi.y], as a parameter interval (slab form).
    -> None (invisible) or (a', b', sides) with sides the set of box sides that cut it ("left", "right", "top", "bottom")."""
    t0, t1 = R32(0.0), R32(1.0)
    s0 = s1 = None
    for axis, (near, far) in enumerate((("left", "right"), ("top", "bottom"))):
        d = b[axis] - a[axis]
        if d.exact_zero():
            if D.lt(a[axis], lo[axis], name + ": parallel, outside") or D.lt(hi[axis], a[axis], name + ": parallel, outside"):
                return None
            continue
        # an axis along which the whole segment stays inside the slab decides nothing, whatever the sign of d
        if min(a[axis].v - lo[axis], hi[axis] - a[axis].v) - a[axis].e > 1.001 * (abs(d.v) + d.e):
            continue
        if abs(d.v) <= d.e:
            D.flag(name + ": direction")
            if d.v == 0.0:
                continue
        ta, tb = (lo[axis] - a[axis]) / d, (hi[axis] - a[axis]) / d
        (t_in, side_in), (t_out, side_out) = ((ta, near), (tb, far)) if d.v > 0.0 else ((tb, far), (ta, near))
        # the larger entry and the smaller exit: whichever float32 picks where the two are close, the value is the same up
        # to their distance, which joins the bound
        if t_in.v > t0.v:
            t0, s0 = R32(t_in.v, max(t_in.e, t0.e if t_in.v - t0.v <= t_in.e + t0.e else 0.0)), side_in
        elif t0.v - t_in.v <= t_in.e + t0.e:
            t0 = R32(t0.v, max(t_in.e, t0.e) + (t0.v - t_in.v))
        if t_out.v < t1.v:
            t1, s1 = R32(t_out.v, max(t_out.e, t1.e if t1.v - t_out.v <= t_out.e + t1.e else 0.0)), side_out
        elif t_out.v - t1.v <= t_out.e + t1.e:
            t1 = R32(t1.v, max(t_out.e, t1.e) + (t_out.v - t1.v))
    if D.lt(t1, t0, name + ": visible"):
        return None
    out = []
    for t in (t0, t1):
        pt = []
        for axis in range(2):
            c = a[axis] + t * (b[axis] - a[axis])
            pt.append(R32(min(max(c.v, lo[axis]), hi[axis]), c.e))
        out.append(pt)
    return out[0], out[1], {s for s in (s0, s1) if s}


NO_REGION = ("empty idepth window", "zero length", "first clip", "zero length after the clip", "second clip")


def search_region64(P, g, width, height, ux, uy, mu, var, D):
    """inverse_depth_filter::getSearchRegion.  -> dict(exit = index into NO_REGION or None, seg = (sx, sy, ex, ey) R32,
    sides = box sides that cut it in the first clip, padded, cut, sides2 = ... in the second clip)."""
    mu, var = float(mu), float(var)
    lo_p, hi_p = float(P.idepth_min), float(P.idepth_max)
    id_min, id_max = R32(lo_p), R32(hi_p)
    if not (math.isnan(mu) or math.isnan(var)):
        half = P.search_sigma * R32(var).sqrt()
        id_min, id_max = mu - half, mu + half
    if D.lt(id_min, lo_p, "idepth window: lower clamp"):
        id_min = R32(lo_p)
    if D.lt(hi_p, id_max, "idepth window: upper clamp"):
        id_max = R32(hi_p)
    if D.lt(id_max, id_min, "idepth window: empty"):
        return dict(exit=0)
    a, b = project64(g, ux, uy, id_min), project64(g, ux, uy, id_max)
    if id_min.e == 0.0 and id_max.e == 0.0 and id_min.v == id_max.v:
        return dict(exit=1)             # the same float32 input gives the same float32 point: length 0 exactly
    d = (b[0] - a[0], b[1] - a[1])
    length = (d[0] * d[0] + d[1] * d[1]).sqrt()
    if not D.lt(0.0, length, "segment length > 0"):
        return dict(exit=1)
    epi = (d[0] / length, d[1] / length)
    lo, hi = (1.0, 1.0), (float(width - 1), float(height - 1))
    c = _clip64(lo, hi, a, b, D, "first clip")
    if c is None:
        return dict(exit=2)
    a, b, sides = c
    d = (b[0] - a[0], b[1] - a[1])
    length = (d[0] * d[0] + d[1] * d[1]).sqrt()
    if not D.lt(0.0, length, "clipped length > 0"):
        return dict(exit=3)
    padded = D.lt(length, float(P.epilength_min), "padding")
    if padded:
        pad = (P.epilength_min - length) / 2.0
        a = (a[0] - epi[0] * pad, a[1] - epi[1] * pad)
        b = (b[0] + epi[0] * pad, b[1] + epi[1] * pad)
    cut = D.lt(float(P.epilength_max), length, "cut")
    if cut:
        b = (a[0] + epi[0] * P.epilength_max, a[1] + epi[1] * P.epilength_max)
    c = _clip64(lo, hi, a, b, D, "second clip")
    if c is None:
        return dict(exit=4)
    a, b, sides2 = c
    return dict(exit=None, seg=(a[0], a[1], b[0], b[1]), sides=sides, padded=padded, cut=cut, sides2=sides2)


def reference_epiline64(g, ux, uy):
    """epipolar_geometry.h:303-325, unit vector (R32 pair); None where the reference asserts."""
    ax = -g.K[0] * R32(g.tcr[0]) + g.tcr[2] * (R32(ux) - g.K[2])
    ay = -g.K[4] * R32(g.tcr[1]) + g.tcr[2] * (R32(uy) - g.K[5])
    n = (ax * ax + ay * ay).sqrt()
    if not n.v > 0.0:
        return None
    return ax / n, ay / n


def bilinear_r32(img, x, y):
    """Bilinear sample of a 2-D array at an R32 position: the float64 value, and what a float32 evaluation at a position
    (ex, ey) away may differ by."""
    x0, y0 = int(math.floor(x.v)), int(math.floor(y.v))
    dx, dy = x.v - x0, y.v - y0
    f = img[y0:y0 + 2, x0:x0 + 2].astype(np.float64)
    v = (1 - dx) * (1 - dy) * f[0, 0] + dx * (1 - dy) * f[0, 1] + (1 - dx) * dy * f[1, 0] + dx * dy * f[1, 1]
    e = 8 * EPS * float(np.abs(f).max())
    if x.e > 0.0 or y.e > 0.0:
        blk = img[max(y0 - 1, 0):y0 + 3, max(x0 - 1, 0):x0 + 3].astype(np.float64)
        lx = np.abs(np.diff(blk, axis=1)).max() if blk.shape[1] > 1 else 0.0
        ly = np.abs(np.diff(blk, axis=0)).max() if blk.shape[0] > 1 else 0.0
        e += x.e * float(lx) + y.e * float(ly)
        if not (x.e < 1.0 and y.e < 1.0):
            if not math.isfinite(x.e + y.e):
                return R32(v, INF)
            blk = img[max(int(math.floor(y.v - y.e)), 0):int(math.floor(y.v + y.e)) + 2,
                      max(int(math.floor(x.v - x.e)), 0):int(math.floor(x.v + x.e)) + 2]
            e = float(blk.max()) - float(blk.min()) + 8 * EPS * float(np.abs(blk).max())
    return R32(v, e)


def epiline64(g, ux, uy, D):
    """epipolar_geometry.h:239-292.  -> (u_inf.x, u_inf.y, epi.x, epi.y) or None where the reference asserts."""
    ix, iy = max_depth_projection64(g, ux, uy)
    tz = g.t[2]
    if tz > 0.0:
        zx, zy = R32(g.epx), R32(g.epy)
    elif tz == 0.0:
        zx, zy = ix + 1e6 * (g.K[0] * R32(g.t[0])), iy + 1e6 * (g.K[4] * R32(g.t[1]))
    else:
        p = [g.Kinv[0] * R32(ux) + g.Kinv[2], g.Kinv[4] * R32(uy) + g.Kinv[5], R32(1.0)]
        qp = g.rotate(p)
        min_depth = (1.0 - tz) / qp[2]
        c = [min_depth * qp[k] + g.t[k] for k in range(3)]
        if not c[2].v > 0.0:
            return None
        zx, zy = (g.K[0] * c[0] + g.K[2] * c[2]) / c[2], (g.K[4] * c[1] + g.K[5] * c[2]) / c[2]
    dx, dy = zx - ix, zy - iy
    n2 = dx * dx + dy * dy
    if D.lt(1e-10, n2, "epiline norm"):
        n = n2.sqrt()
        dx, dy = dx / n, dy / n
    else:
        dx, dy = R32(0.0), R32(0.0)
    return ix, iy, dx, dy


def disparity_to_idepth64(g, ux, uy, ix, iy, ex, ey, disp):
    """epipolar_geometry.h:389-405: least squares of (Kt - Kt.z u_cmp) idepth = w disp epi.  -> (idepth, ATA)."""
    M = g.KRKinv
    w = M[6] * R32(ux) + M[7] * R32(uy) + M[8]
    ax = g.Kt[0] - g.Kt[2] * (ix + disp * ex)
    ay = g.Kt[1] - g.Kt[2] * (iy + disp * ey)
    wd = w * disp
    bx, by = ex * wd, ey * wd
    ata = ax * ax + ay * ay
    return (ax * bx + ay * by) / ata, ata


MEAS_EXITS = ("disp < 1e-3", "mu < 0", "gnorm < 1e-3", "|edn| < 1e-3")


def meas64(P, g, gradx_pad, grady_pad, ux, uy, cx, cy, D):
    """InverseDepthMeasModel::idepth.  cx, cy: the match in image coordinates (R32).  The gradient images carry the
    frame's border while the sample is offset by z_win_size / 2 + 1 (inverse_depth_meas_model.cc:87-93): as there.
    -> dict(exit = index into MEAS_EXITS or None or "assert", mu, var, and the intermediate values)."""
    el = epiline64(g, ux, uy, D)
    if el is None:
        return dict(exit="assert")
    ix, iy, ex, ey = el
    cx, cy = R32.of(cx), R32.of(cy)
    disp = ex * (cx - ix) + ey * (cy - iy)
    if D.lt(disp, 1e-3, "disp < 1e-3"):
        return dict(exit=0, disp=disp)
    mu, ata = disparity_to_idepth64(g, ux, uy, ix, iy, ex, ey, disp)
    if D.lt(mu, 0.0, "mu_meas < 0"):
        return dict(exit=1, disp=disp)
    off = float(P.z_win_size // 2 + 1)
    sx, sy = cx + off, cy + off
    rows, cols = gradx_pad.shape
    if not (sx.v >= 0 and sy.v >= 0 and sx.v < cols - 1 and sy.v < rows - 1):
        return dict(exit="assert")
    gx, gy = bilinear_r32(gradx_pad, sx, sy), bilinear_r32(grady_pad, sx, sy)
    gnorm = (gx * gx + gy * gy).sqrt()
    if D.lt(gnorm, 1e-3, "gnorm < 1e-3"):
        return dict(exit=2, disp=disp, gnorm=gnorm)
    edn = (gx / gnorm) * ex + (gy / gnorm) * ey
    if D.lt(abs(edn), 1e-3, "|edn| < 1e-3"):
        return dict(exit=3, disp=disp, gnorm=gnorm, edn=edn)
    geo_var = P.epipolar_line_var / (edn * edn)
    edg = gx * ex + gy * ey
    photo_var = 2.0 * P.pixel_var / (edg * edg)
    dmin, dmax = disp - disp / 10.0, disp + disp / 10.0
    idmin, _ = disparity_to_idepth64(g, ux, uy, ix, iy, ex, ey, dmin)
    idmax, _ = disparity_to_idepth64(g, ux, uy, ix, iy, ex, ey, dmax)
    alpha = (idmax - idmin) / (dmax - dmin)
    var = alpha * alpha * (geo_var + photo_var)
    return dict(exit=None, mu=mu, var=var, disp=disp, gnorm=gnorm, edn=edn, edg=edg, ata=ata, alpha=alpha)


def fuse64(mu_pred, var_pred, mu_meas, var_meas, thresh, D):
    """inverse_depth_filter::update.  mu_pred, var_pred: the feature's float32 prior.
    -> dict(outlier, prior (whether the prior took part), mu, var)."""
    mu_pred, var_pred = float(mu_pred), float(var_pred)
    prior = (not math.isnan(mu_pred)) and mu_pred > 0.0
    if prior:
        w = var_pred + var_meas
        mu = (var_meas * mu_pred + var_pred * mu_meas) / w
        var = (var_pred * var_meas) / w
    else:
        mu, var = mu_meas, var_meas
    res = mu_meas - mu_pred
    dist = res * res / var_pred
    t2 = R32(thresh) * thresh
    if D.lt(t2, dist, "outlier gate"):
        return dict(outlier=True, prior=prior)
    if not D.lt(0.0, mu, "mu_post <= 0"):
        mu = R32(0.0)
    return dict(outlier=False, prior=prior, mu=mu, var=var)


def fail64(P, var, num_dropouts, D):
    """fail_feature on a variance (float32 number or R32) and the dropout counter.  -> (bits, var', dropouts'):
    bit 0 = the variance passed idepth_var_max, bit 1 = the dropouts passed max_dropouts (uint32 arithmetic)."""
    v = R32.of(var) * float(P.process_fail_var_factor)
    bits = 1 if D.lt(float(P.idepth_var_max), v, "idepth_var_max") else 0
    n = (int(num_dropouts) + 1) & 0xffffffff
    if n > (int(P.max_dropouts) & 0xffffffff):
        bits |= 2
    return bits, v, n


REACHED_THE_WALK = 100     # stage64 without a walk: the feature passed the gradient gate; the walk decides the rest


def stage64(P, stages, g_new, g_pf, width, height, pad, ref_pad, new_gx, new_gy, f, walk=None, decide=None):
    """One feature through Flame::updateFeatureIDepths / trackFeature (flame.cc:1280-1752) in float64.
    stages: name -> code (oracle.stereo_capi.STAGE).  g_new, g_pf: Geo64 of T_ref_to_new and T_ref_to_newest-pose-frame.
    walk: None, or callable(patch [5 R32], segment [4 R32, image coordinates]) -> (match.x, match.y) R32 in image
    coordinates, or None where the float64 walk's best step is not clear of the others.
    decide: see Doubt.
    -> dict(stage, doubt [names], forced, fail, and the values of the stages passed)."""
    D = Doubt(decide)
    out = dict(forced=0, fail=0, doubt=D.why)

    def done(stage, failed=True, var=None):
        out["stage"] = stage
        if failed:
            out["fail"], out["fail_var"], _ = fail64(P, f["idepth_var"] if var is None else var, f["num_dropouts"], D)
        return out

    t = g_new.t
    baseline = (R32(t[0]) * t[0] + R32(t[1]) * t[1] + R32(t[2]) * t[2]).sqrt()
    if D.lt(baseline, float(P.min_baseline), "baseline"):
        return done(stages["baseline skip"], failed=False)
    ux, uy, mu, var = (float(f[k]) for k in ("x", "y", "idepth_mu", "idepth_var"))
    pr = predict64(g_new, float(P.process_var_factor), ux, uy, mu, var, D)
    out["predict"] = pr
    if pr["decision"] == "assert":
        return done(-1, failed=False)
    if pr["decision"] == "no":
        return done(stages["predict no"])
    out["forced"] = int(pr["forced"])
    rect = valid_rect(P, width, height)
    rescale = R32(1.0)
    if mu > 0.0 and D.lt(0.0, pr["mu_pred"], "idepth_cmp > 0"):
        rescale = pr["mu_pred"] / mu
    if not D.lt(float(P.rescale_factor_min), rescale, "rescale_factor_min") or \
            not D.lt(rescale, float(P.rescale_factor_max), "rescale_factor_max"):
        mv = predict64(g_pf, float(P.process_var_factor), ux, uy, mu, var, D)
        out["move"] = mv
        if mv["decision"] == "assert":
            return done(-1, failed=False)
        if mv["decision"] == "no":
            return done(stages["move failed: predict"])
        if not rect_contains_r32(rect, mv["x"], mv["y"], D, "moved point in the rectangle"):
            return done(stages["move failed: rectangle"])
        if D.lt(mv["mu_pred"], 1e-6, "idepth_pf < 1e-6"):
            v4 = R32(1.0)
            out["forced"] |= 2
        else:
            v = mv["mu_pred"] / mu
            v = v * v
            v4 = v * v
        out["moved_var"] = var * v4
        return done(stages["moved"], var=out["moved_var"])
    sr = search_region64(P, g_new, width, height, ux, uy, mu, var, D)
    out["region"] = sr
    if sr["exit"] is not None:
        return done(stages["no region: empty idepth window"] + sr["exit"])
    if not rect_contains(*rect, ux, uy):
        return done(stages["outside the valid rectangle"])
    epi = reference_epiline64(g_new, ux + float(pad), uy + float(pad))
    if epi is None:
        return done(-1, failed=False)
    px, py = R32(ux) + float(pad), R32(uy) + float(pad)
    patch = [bilinear_r32(ref_pad, px + k * epi[0] * rescale, py + k * epi[1] * rescale) for k in (-2.0, -1.0, 0.0, 1.0, 2.0)]
    diffs = [abs(patch[k] - patch[k - 1]) for k in range(1, 5)]
    gmax = R32(max(d.v for d in diffs), max(d.e for d in diffs))
    out["gmax"] = gmax
    if D.lt(gmax, float(P.min_grad_mag), "min_grad_mag"):
        return done(stages["search status 1"])
    if walk is None:
        return done(REACHED_THE_WALK, failed=False)
    m = walk(patch, sr["seg"])
    if m is None:
        D.flag("walk")
        return done(REACHED_THE_WALK, failed=False)
    out["match"] = m
    ms = meas64(P, g_new, new_gx, new_gy, ux, uy, m[0], m[1], D)
    out["meas"] = ms
    if ms["exit"] == "assert":
        return done(-1, failed=False)
    if ms["exit"] is not None:
        return done(stages["meas: disp < 1e-3"] + ms["exit"])
    fu = fuse64(mu, var, ms["mu"], ms["var"], float(P.outlier_sigma_thresh), D)
    out["fuse"] = fu
    if fu["outlier"]:
        return done(stages["outlier"])
    return done(stages["updated, prior > 0"] if fu["prior"] else stages["updated, prior <= 0"], failed=False)
