"""A float64 statement of the per-vertex photometric residual (BASELINE config 5), written from the geometry itself.

It shares nothing with oracle/photometric_oracle.c: no KRKinv / Kt, no float32.  A vertex at pixel u with inverse depth
idepth (= x * graph_scale) is back-projected with K^-1, scaled to depth 1 / idepth, moved into the other camera with R, t
and projected with K; at idepth == 0 (a point at infinity) only the rotation acts.  As in the residual's definition
there is no test for points behind the camera: their projection is used as it is.

    err[v] = | I_cmp(project(u_v)) - I_ref(u_v) |,  NaN where idepth is NaN or negative, or where u_v or its projection
             lies outside [border, cols - border) x [border, rows - border).

Images are addressed through an explicit row stride (bytes), as a padded buffer is."""
import numpy as np


def project64(K, R, t, pos, idepth):
    """u (V, 2) and idepth (V,) -> (projected pixel (V, 2), z of the point in the other camera (V,)), float64.
    For idepth == 0 the z returned is that of the unit-depth ray (its sign is the point's side)."""
    K = np.asarray(K, np.float64)
    u = np.asarray(pos, np.float64).reshape(-1, 2)
    idepth = np.asarray(idepth, np.float64)
    ray = np.linalg.solve(K, np.stack([u[:, 0], u[:, 1], np.ones(len(u))]))  # K^-1 [u; 1], depth 1
    rot = np.asarray(R, np.float64) @ ray
    with np.errstate(divide="ignore", invalid="ignore"):
        at_inf = idepth == 0
        pc = np.where(at_inf, rot, rot / np.where(at_inf, 1.0, idepth) + np.asarray(t, np.float64).reshape(3, 1))
        h = K @ pc
        c = np.stack([h[0] / h[2], h[1] / h[2]], 1)
    return c, pc[2]


def bilinear64(flat, step, x, y):
    """Bilinear lookup at (x, y) in a uint8 image stored row after row, `step` bytes apart (x: column, y: row)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    fx, fy = x - x0, y - y0
    at = lambda r, c: flat[r * step + c].astype(np.float64)  # noqa: E731
    return ((1 - fx) * (1 - fy) * at(y0, x0) + fx * (1 - fy) * at(y0, x0 + 1)
            + (1 - fx) * fy * at(y0 + 1, x0) + fx * fy * at(y0 + 1, x0 + 1))


def _flat_step(img):
    """(the bytes of a 2-D uint8 image from its first pixel to its last, its row step).  A view with contiguous rows is read
    in place, padding and all; any other layout is copied into dense rows first."""
    img = np.asarray(img, np.uint8)
    if img.strides[1] != 1 or img.strides[0] < img.shape[1]:
        img = np.ascontiguousarray(img)
    n = (img.shape[0] - 1) * img.strides[0] + img.shape[1]
    return np.lib.stride_tricks.as_strided(img, shape=(n,), strides=(1,)), img.strides[0]


def inside64(x, y, rows, cols, border):
    return (x >= border) & (y >= border) & (x < cols - border) & (y < rows - border)


def residual64(pos, x, graph_scale, K, R, t, ref, cmp, border):
    """(err (V,), projected pixel (V, 2), z in the other camera (V,)) in float64.  ref / cmp: 2-D uint8, rows may be padded."""
    ref, cmp = np.asarray(ref), np.asarray(cmp)
    rows, cols = ref.shape
    u = np.asarray(pos, np.float64).reshape(-1, 2)
    idepth = np.asarray(x, np.float64) * float(graph_scale)
    c, z = project64(K, R, t, u, np.where(np.isnan(idepth), 1.0, idepth))
    ok = ~np.isnan(idepth) & ~(idepth < 0) & inside64(u[:, 0], u[:, 1], rows, cols, border)
    ok &= np.isfinite(c).all(1) & inside64(c[:, 0], c[:, 1], rows, cols, border)
    err = np.full(len(u), np.nan)
    if ok.any():
        a = bilinear64(*_flat_step(cmp), c[ok, 0], c[ok, 1])
        b = bilinear64(*_flat_step(ref), u[ok, 0], u[ok, 1])
        err[ok] = np.abs(a - b)
    return err, c, z


def local_range(img, x, y):
    """max - min of the 4x4 pixels around the cell of (x, y): bounds how much a bilinear lookup can change per pixel of
    movement anywhere within one pixel of (x, y)."""
    img = np.asarray(img)
    rows, cols = img.shape
    x0 = np.clip(np.floor(x).astype(np.int64), 1, cols - 3)
    y0 = np.clip(np.floor(y).astype(np.int64), 1, rows - 3)
    blocks = np.stack([img[y0 + dy, x0 + dx] for dy in (-1, 0, 1, 2) for dx in (-1, 0, 1, 2)], 1).astype(np.float64)
    return blocks.max(1) - blocks.min(1)
