"""numpy restatement of the pyramid levels and the direct image alignment of include/flame_stereo.h (flame_stereo_build_pyramid,
flame_stereo_align_linearize, flame_stereo_align_frame state every rule), the checker of that stage.  With dtype float32 every
operation rounds once, in the header's association, and the device must agree bit for bit; with dtype float64 the same code serves
the tests of the formulas' properties.  The 28 sums are float64 in either case.

  pyrDown      out(y, x) = (sum_ij k_i k_j src(r(2y + i), r(2x + j)) + 128) >> 8, k = 1 4 6 4 1, r = BORDER_REFLECT_101 repeated
  gradients    getCentralGradient: 0.5 (right - left) inside, forward / backward differences in the first / last column and row
  sums         flame_nltgv2_map_error's rule on float64 terms: chunks of 1024 pairwise, the partials strided, then pairwise
"""
import numpy as np

CHUNK = 1024
COUNTS = ("n_used", "n_no_depth", "n_behind", "n_outside", "n_huber")
H_PAIRS = [(i, j) for i in range(6) for j in range(i, 6)]  # the upper triangle, row-major
SMALL_ANGLE2 = 1e-10
OK, TOO_FEW = 0, 1
FLAG_NOT_PD, FLAG_REJECTED, FLAG_MAX_ITERS = 1, 2, 4


# ---- pyramid ----
def reflect_101(p, n):
    """cv::borderInterpolate(BORDER_REFLECT_101) repeated until inside, as a closed form: even, period 2 (n - 1)."""
    p = np.asarray(p, np.int64)
    period = 2 * (n - 1)
    m = np.abs(p) % period
    return np.where(m < n, m, period - m)


def pyr_down(img):
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    dh, dw = (h + 1) // 2, (w + 1) // 2
    k = (1, 4, 6, 4, 1)
    src = img.astype(np.int64)
    acc = np.zeros((dh, dw), np.int64)
    ys, xs = 2 * np.arange(dh), 2 * np.arange(dw)
    for i in range(-2, 3):
        rows = src[reflect_101(ys + i, h)]
        for j in range(-2, 3):
            acc += k[i + 2] * k[j + 2] * rows[:, reflect_101(xs + j, w)]
    return ((acc + 128) >> 8).astype(np.uint8)


def central_gradient(img, dtype=np.float32):
    T = dtype
    a = np.asarray(img).astype(T)
    gx, gy = np.empty_like(a), np.empty_like(a)
    gx[:, 1:-1] = T(0.5) * (a[:, 2:] - a[:, :-2])
    gx[:, 0] = a[:, 1] - a[:, 0]
    gx[:, -1] = a[:, -1] - a[:, -2]
    gy[1:-1] = T(0.5) * (a[2:] - a[:-2])
    gy[0] = a[1] - a[0]
    gy[-1] = a[-1] - a[-2]
    return gx, gy


def level_size(w, h, level):
    for _ in range(level):
        w, h = (w + 1) // 2, (h + 1) // 2
    return w, h


def levels_valid(w, h, n_levels):
    if not 1 <= n_levels <= 5:
        return False
    wl, hl = level_size(w, h, n_levels - 1)
    return wl >= 4 and hl >= 4


def build_pyramid(img, n_levels, dtype=np.float32):
    """-> [(img, gradx, grady)] per level; level 0 is the image itself with its central gradients (what add_frame keeps inside its
    padded planes)."""
    out = []
    cur = np.asarray(img, np.uint8)
    for l in range(n_levels):
        if l > 0:
            cur = pyr_down(cur)
        gx, gy = central_gradient(cur, dtype)
        out.append((cur, gx, gy))
    return out


# ---- pose ----
def quat_to_rot(q):
    w, x, y, z = (np.float64(v) for v in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx,
                     1.0 - (txx + tyy)], np.float64)


def pose_floats(q, t, dtype=np.float32):
    """The 12 numbers the kernel sees: R (9, row-major) and t (3), rounded to dtype."""
    return quat_to_rot(q).astype(dtype), np.asarray(t, np.float64).astype(dtype)


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], np.float64)


def exp_left(delta, q, t):
    """T' = exp(delta) T in double, delta = (v, omega); q renormalised."""
    delta = np.asarray(delta, np.float64)
    q, t = np.asarray(q, np.float64), np.asarray(t, np.float64)
    v, o = delta[:3], delta[3:]
    th2 = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]
    if th2 < SMALL_ANGLE2:
        A, B, Cc = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
        Hs, Hc = 0.5 - th2 / 48.0, 1.0 - th2 / 8.0
    else:
        th = np.sqrt(th2)
        s, c = np.sin(th), np.cos(th)
        A, B, Cc = s / th, (1.0 - c) / th2, (th - s) / (th2 * th)
        Hs, Hc = np.sin(0.5 * th) / th, np.cos(0.5 * th)
    ot = _cross(o, t)
    oot = _cross(o, ot)
    ov = _cross(o, v)
    oov = _cross(o, ov)
    t2 = ((t + A * ot) + B * oot) + ((v + B * ov) + Cc * oov)
    a, b, c, d = Hc, Hs * o[0], Hs * o[1], Hs * o[2]
    w, x, y, z = q
    r = np.array([((a * w - b * x) - c * y) - d * z, ((a * x + b * w) + c * z) - d * y, ((a * y - b * z) + c * w) + d * x,
                  ((a * z + b * y) - c * x) + d * w], np.float64)
    n = np.sqrt(((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3])
    return r / n, t2


def full_H(sums):
    H = np.zeros((6, 6), np.float64)
    for k, (i, j) in enumerate(H_PAIRS):
        H[i, j] = H[j, i] = sums[k]
    return H


def solve(sums, lm_lambda=0.0):
    """(H + lambda diag H) delta = -b by Cholesky in double; None when H is not positive definite."""
    H = full_H(sums)
    b = np.asarray(sums[21:27], np.float64)
    A = H + lm_lambda * np.diag(np.diag(H))
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    y = np.linalg.solve(L, -b)
    d = np.linalg.solve(L.T, y)
    return d if np.isfinite(d).all() else None


def accept(cost_new, n_new, cost_old, n_old):
    with np.errstate(all="ignore"):
        return bool(np.float64(cost_new) / np.float64(n_new) < np.float64(cost_old) / np.float64(n_old))


# ---- the sum rule ----
def _pairwise(p):
    s = CHUNK // 2
    with np.errstate(all="ignore"):
        while s >= 1:
            p = p[..., :s] + p[..., s:2 * s]
            s //= 2
    return p[..., 0]


def ordered_sum(terms):
    """float64 terms in linear pixel order -> the sum, in the order of flame_nltgv2_map_error's `sum`."""
    terms = np.asarray(terms, np.float64).reshape(-1)
    chunks = (terms.size + CHUNK - 1) // CHUNK
    padded = np.zeros(chunks * CHUNK, np.float64)
    padded[:terms.size] = terms
    b = _pairwise(padded.reshape(chunks, CHUNK))
    rounds = (chunks + CHUNK - 1) // CHUNK
    bp = np.zeros(rounds * CHUNK, np.float64)
    bp[:chunks] = b
    q = np.zeros(CHUNK, np.float64)
    with np.errstate(all="ignore"):
        for j in range(rounds):
            q = q + bp[j * CHUNK:(j + 1) * CHUNK]
    return np.float64(_pairwise(q))


# ---- the linearisation ----
def _bilinear(plane, x0, y0, w00, w01, w10, w11):
    g00, g01, g10, g11 = plane[y0, x0], plane[y0, x0 + 1], plane[y0 + 1, x0], plane[y0 + 1, x0 + 1]
    return ((w00 * g00 + w01 * g01) + w10 * g10) + w11 * g11


def pixel_terms(ref_img, new_level, idepthmap, level, K, border, huber_k, R, t, dtype=np.float32):
    """Per level pixel: the class masks, r, J [6], wgt, u, v -- the header's steps 1 to 8 in `dtype`.  K = (fx, fy, cx, cy) of level
    0; new_level = (img, gradx, grady) of the new frame's level; R [9], t [3] already in `dtype`."""
    T = dtype
    ref = np.asarray(ref_img).astype(T)
    img, gxp, gyp = (np.asarray(a).astype(T) for a in new_level)
    h, w = ref.shape
    scale = T(1 << level)
    fx, fy, cx, cy = (T(v) / scale for v in K)
    R, t = np.asarray(R, T), np.asarray(t, T)
    d = np.asarray(idepthmap, T)[::1 << level, ::1 << level][:h, :w]
    assert d.shape == (h, w)
    xx, yy = np.meshgrid(np.arange(w), np.arange(h))
    ring = (xx >= border) & (xx < w - border) & (yy >= border) & (yy < h - border)
    fb, k = T(border), T(huber_k)
    with np.errstate(all="ignore"):
        dvalid = (d == d) & (d > T(0)) & (d < T(np.inf))
        no_depth = ring & ~dvalid
        elig = ring & dvalid
        a = (xx.astype(T) - cx) / fx
        b = (yy.astype(T) - cy) / fy
        Xx = ((R[0] * a + R[1] * b) + R[2]) + t[0] * d
        Xy = ((R[3] * a + R[4] * b) + R[5]) + t[1] * d
        Xz = ((R[6] * a + R[7] * b) + R[8]) + t[2] * d
        front = Xz > T(0)
        behind = elig & ~front
        xn, yn, rho = Xx / Xz, Xy / Xz, d / Xz
        u = fx * xn + cx
        v = fy * yn + cy
        ins = (u >= fb) & (v >= fb) & (u < T(w - 1 - border)) & (v < T(h - 1 - border))
        outside = elig & front & ~ins
        used = elig & front & ins
        us, vs = np.where(used, u, fb), np.where(used, v, fb)
        x0, y0 = us.astype(np.int64), vs.astype(np.int64)  # truncation
        dx, dy = us - x0.astype(T), vs - y0.astype(T)
        w11 = dx * dy
        w01, w10 = dx - w11, dy - w11
        w00 = ((T(1) - dx) - dy) + w11
        inew = _bilinear(img, x0, y0, w00, w01, w10, w11)
        gx = _bilinear(gxp, x0, y0, w00, w01, w10, w11)
        gy = _bilinear(gyp, x0, y0, w00, w01, w10, w11)
        r = inew - ref
        Gx, Gy, xy = fx * gx, fy * gy, xn * yn
        J = np.stack([Gx * rho, Gy * rho, -((Gx * xn + Gy * yn) * rho), -(Gx * xy + Gy * (T(1) + yn * yn)),
                      Gx * (T(1) + xn * xn) + Gy * xy, Gy * xn - Gx * yn])
        ar = np.abs(r)
        quad = ar <= k
        wgt = np.where(quad, T(1), k / ar)
    return dict(used=used, no_depth=no_depth, behind=behind, outside=outside, huber=used & ~quad, r=r, J=J, wgt=wgt, u=u, v=v,
                ring=ring)


def linearize(ref_img, new_level, idepthmap, level, K, border, huber_k, q, t, dtype=np.float32):
    """-> dict: sums [28] float64 (H's upper triangle row-major, b, cost), the five counts, and the per-pixel terms under 'px'."""
    R, tf = pose_floats(q, t, dtype)
    px = pixel_terms(ref_img, new_level, idepthmap, level, K, border, huber_k, R, tf, dtype)
    used = px["used"].reshape(-1)
    wgt = px["wgt"].reshape(-1).astype(np.float64)
    J = px["J"].reshape(6, -1).astype(np.float64)
    r = px["r"].reshape(-1).astype(np.float64)
    sums = np.zeros(28, np.float64)
    with np.errstate(all="ignore"):
        wj = [wgt * J[i] for i in range(6)]
        for k, (i, j) in enumerate(H_PAIRS):
            sums[k] = ordered_sum(np.where(used, wj[i] * J[j], 0.0))
        for i in range(6):
            sums[21 + i] = ordered_sum(np.where(used, wj[i] * r, 0.0))
        sums[27] = ordered_sum(np.where(used, (wgt * r) * r, 0.0))
    out = dict(sums=sums, px=px, n_used=int(px["used"].sum()), n_no_depth=int(px["no_depth"].sum()),
               n_behind=int(px["behind"].sum()), n_outside=int(px["outside"].sum()), n_huber=int(px["huber"].sum()))
    return out


def assert_same_system(got, ref, what=""):
    """Bit for bit: the 28 sums as uint64, the five counts equal."""
    for n in COUNTS:
        assert got[n] == ref[n], f"{what}: {n} {got[n]} != {ref[n]}"
    g = np.ascontiguousarray(got["sums"], np.float64).view(np.uint64)
    r = np.ascontiguousarray(ref["sums"], np.float64).view(np.uint64)
    bad = np.flatnonzero(g != r)
    assert bad.size == 0, f"{what}: sums differ at {bad.tolist()}: {got['sums'][bad]} != {ref['sums'][bad]}"


# ---- the driver ----
def align_frame(ref_pyr, new_pyr, idepthmap, K, q_init, t_init, border=2, huber_k=10.0, coarsest_level=2, finest_level=0,
                max_iters_per_level=10, min_pixels=100, min_step=1e-5, lm_lambda=0.0, dtype=np.float32):
    """The loop of flame_stereo_align_frame on two pyramids (build_pyramid).  -> dict: status, flags, q, t, iters, trace (list of dicts:
    level, accepted, q, t, delta, sums, counts), first_mean_cost, last_mean_cost."""
    q = np.asarray(q_init, np.float64)
    q = q / np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    t = np.asarray(t_init, np.float64).copy()
    trace, iters = [], [0] * 5
    status, flags = OK, 0

    def ev(level, eq, et, delta):
        s = linearize(ref_pyr[level][0], new_pyr[level], idepthmap, level, K, border, huber_k, eq, et, dtype)
        s.pop("px")
        s.update(level=level, accepted=1, q=eq.copy(), t=et.copy(), delta=np.asarray(delta, np.float64).copy())
        trace.append(s)
        return s

    sys = None
    for level in range(coarsest_level, finest_level - 1, -1):
        if status != OK:
            break
        sys = ev(level, q, t, np.zeros(6))
        it = 0
        while True:
            if sys["n_used"] < min_pixels:
                status = TOO_FEW
                break
            if it >= max_iters_per_level:
                flags |= FLAG_MAX_ITERS
                break
            delta = solve(sys["sums"], lm_lambda)
            if delta is None:
                flags |= FLAG_NOT_PD
                break
            q2, t2 = exp_left(delta, q, t)
            sys2 = ev(level, q2, t2, delta)
            if not accept(sys2["sums"][27], sys2["n_used"], sys["sums"][27], sys["n_used"]):
                sys2["accepted"] = 0
                flags |= FLAG_REJECTED
                break
            q, t, sys = q2, t2, sys2
            iters[level] += 1
            it += 1
            if np.max(np.abs(delta)) < min_step:
                break
    with np.errstate(all="ignore"):
        first = np.float64(trace[0]["sums"][27]) / np.float64(trace[0]["n_used"])
        last = np.float64(sys["sums"][27]) / np.float64(sys["n_used"])
    return dict(status=status, flags=flags, q=q, t=t, iters=iters, trace=trace, first_mean_cost=float(first),
                last_mean_cost=float(last))


# ---- synthetic scenes ----
def texture_at(w, h, seed, scale, x, y):
    """A smooth, well-textured function of real pixel coordinates (x, y): six sinusoids, their sum inside (-6, 6)."""
    rng = np.random.default_rng(seed)
    v = np.zeros(np.shape(x))
    for _ in range(6):
        fx, fy = rng.uniform(0.02, 0.12, 2) * rng.choice([-1, 1], 2) / scale
        v += rng.uniform(0.5, 1.0) * np.sin(2 * np.pi * (fx * x + fy * y) + rng.uniform(0, 2 * np.pi))
    return v


def make_scene(w, h, K, q_true, t_true, seed=0, idepth=None, scale=1.0):
    """A reference image, a known inverse-depth map and the new image that the true pose T_ref_to_new = (q_true, t_true) predicts: the
    texture is defined in the new camera's pixel coordinates, the reference image is its value at the warp of each reference pixel.
    -> (ref u8, new u8, idepth f32)."""
    fx, fy, cx, cy = K
    if idepth is None:
        yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        idepth = (0.5 + 0.2 * np.sin(xx / w * 3.0) * np.cos(yy / h * 2.0)).astype(np.float32)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    R = quat_to_rot(q_true).reshape(3, 3)
    d = idepth.astype(np.float64)
    a, b = (xx - cx) / fx, (yy - cy) / fy
    X = R[:, 0, None, None] * a + R[:, 1, None, None] * b + R[:, 2, None, None] + np.asarray(t_true)[:, None, None] * d
    u, v = fx * X[0] / X[2] + cx, fy * X[1] / X[2] + cy
    lo, hi = -6.0, 6.0  # the six sinusoids' sum lies inside
    new = texture_at(w, h, seed, scale, xx, yy)
    ref = texture_at(w, h, seed, scale, u, v)
    to8 = lambda z: np.clip(np.rint((z - lo) / (hi - lo) * 255.0), 0, 255).astype(np.uint8)
    return to8(ref), to8(new), idepth


def pose_error(q, t, q_true, t_true):
    """(rotation angle between the two in radians, translation distance)."""
    q, qt = np.asarray(q, np.float64), np.asarray(q_true, np.float64)
    c = abs(float(np.dot(q / np.linalg.norm(q), qt / np.linalg.norm(qt))))
    return 2.0 * float(np.arccos(min(1.0, c))), float(np.linalg.norm(np.asarray(t) - np.asarray(t_true)))
