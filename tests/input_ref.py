"""The checker of the raw-frame input stage (flame_stereo_add_raw_frame): a numpy restatement of the definition in
include/flame_stereo.h -- the integer grey of a tap, the float32 map in the header's association with one rounding per
operation, the inside test on the floats, the reference's bilinear weights (utils/image_utils.h:199-214) and the rounding.
Every array below is float32 and every line holds one operation per rounding, so numpy rounds where the device rounds."""
import numpy as np

GREY8, BGR8, RGB8, BGRA8, RGBA8 = range(5)
BYTES = {GREY8: 1, BGR8: 3, RGB8: 3, BGRA8: 4, RGBA8: 4}
F = np.float32


def cam(fx, fy, cx, cy):
    """(K, Kinv) as float32 row-major 3x3; Kinv is rounded from the float64 inverse once (the caller's business: the
    definition reads whatever Kinv the context was given)."""
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
    Kinv = np.array([[1.0 / fx, 0, -cx / fx], [0, 1.0 / fy, -cy / fy], [0, 0, 1]], np.float64)
    return K.astype(F), Kinv.astype(F)


def grey_of(r, g, b):
    """(4899 R + 9617 G + 1868 B + 8192) >> 14 on integers."""
    r, g, b = (np.asarray(c).astype(np.int64) for c in (r, g, b))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


def grey_plane(raw, fmt, width):
    """The grey of every raw pixel: raw is (rows, >= width * bytes) uint8, any padding behind the pixels is ignored."""
    raw = np.asarray(raw, np.uint8)
    rows = raw.shape[0]
    px = raw.reshape(rows, -1)[:, :width * BYTES[fmt]].reshape(rows, width, BYTES[fmt])
    if fmt == GREY8:
        return px[:, :, 0].copy()
    if fmt in (BGR8, BGRA8):
        return grey_of(px[:, :, 2], px[:, :, 1], px[:, :, 0])
    return grey_of(px[:, :, 0], px[:, :, 1], px[:, :, 2])


def source_map(K_raw, dist, Kinv, w, h, raw_width, raw_height, dtype=np.float32):
    """(xs, ys, inside) of every rectified pixel, (h, w) each, evaluated in `dtype` in the header's association."""
    T = dtype
    Kinv = np.asarray(Kinv, F).reshape(-1).astype(T)
    Kr = np.asarray(K_raw, F).reshape(-1).astype(T)
    d = np.zeros(8, F)
    d[:len(dist)] = np.asarray(dist, F)
    k1, k2, p1, p2, k3, k4, k5, k6 = d.astype(T)
    v, u = np.mgrid[0:h, 0:w]
    u, v = u.astype(T), v.astype(T)
    one, two = T(1), T(2)
    with np.errstate(all="ignore"):
        x = (Kinv[0] * u + Kinv[1] * v) + Kinv[2]
        y = (Kinv[3] * u + Kinv[4] * v) + Kinv[5]
        r2 = x * x + y * y
        r4 = r2 * r2
        r6 = r4 * r2
        num = ((one + k1 * r2) + k2 * r4) + k3 * r6
        den = ((one + k4 * r2) + k5 * r4) + k6 * r6
        rad = num / den
        tx, ty = two * x, two * y
        a1 = tx * y
        a2 = r2 + tx * x
        a3 = r2 + ty * y
        xd = (x * rad + p1 * a1) + p2 * a2
        yd = (y * rad + p1 * a3) + p2 * a1
        xs = (Kr[0] * xd + Kr[1] * yd) + Kr[2]
        ys = Kr[4] * yd + Kr[5]
        inside = (xs >= 0) & (ys >= 0) & (xs < T(raw_width - 1)) & (ys < T(raw_height - 1))
    for a in (x, rad, xd, xs, ys):
        assert a.dtype == T
    return xs, ys, inside


def rectify(raw, fmt, params, K, Kinv, w, h):
    """The definition.  raw: (raw_height, >= raw_width * bytes) uint8 (or (rows, cols, channels)); params: dict with remap,
    raw_width, raw_height, K_raw (9 or 3x3), dist (up to 8).  K is not read (the map starts from Kinv).  Returns
    (grey (h, w) uint8, n_outside)."""
    rw, rh = int(params["raw_width"]), int(params["raw_height"])
    g = grey_plane(np.asarray(raw, np.uint8).reshape(rh, -1), fmt, rw)
    if not params.get("remap", 0):
        assert (rw, rh) == (w, h)
        return g, 0
    xs, ys, inside = source_map(params["K_raw"], params.get("dist", ()), Kinv, w, h, rw, rh)
    xi = np.where(inside, xs, F(0))  # (an outside pixel forms no integer and no address)
    yi = np.where(inside, ys, F(0))
    x0, y0 = xi.astype(np.int32), yi.astype(np.int32)
    dx, dy = xi - x0.astype(F), yi - y0.astype(F)
    w11 = dx * dy
    w01 = dx - w11
    w10 = dy - w11
    w00 = ((F(1) - dx) - dy) + w11
    gf = g.astype(F)
    g00, g01, g10, g11 = gf[y0, x0], gf[y0, x0 + 1], gf[y0 + 1, x0], gf[y0 + 1, x0 + 1]
    value = ((w00 * g00 + w01 * g01) + w10 * g10) + w11 * g11
    assert value.dtype == F
    out = (value + F(0.5)).astype(np.int32).astype(np.uint8)
    out[~inside] = 0
    return out, int((~inside).sum())
