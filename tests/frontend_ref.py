"""CPU checker of projectFeatures and detectFeatures (TEST INFRASTRUCTURE): a vectorised float32 numpy restatement of

    Flame::projectFeatures                         flame.cc:1754-1860
    Flame::detectFeatures (live single-pass part)  flame.cc:822-1058
    the detection loop's feature initialisation    flame.cc:736-757

with the reference's expression order.  numpy's float32 arithmetic is IEEE, correctly rounded and never contracted,
so each step rounds exactly as the reference's scalar float code.  The geometry (tcr, K, KRKinv, ...) comes from
oracle.stereo_capi.load_geometry and the pixel gradients from oracle.stereo_capi.make_frame.

Return codes follow flame_nltgv2_status: 0, INVALID_ARG (-1) or ASSERT (-8).
"""
from __future__ import annotations

import numpy as np

OK, INVALID_ARG, ASSERT = 0, -1, -8
F32 = np.float32


def _g(geo, name):
    return np.array(list(getattr(geo, name)), dtype=np.float32)


def border_of(rescale_factor_max, win_size) -> int:
    """`int border = params.rescale_factor_max * params.fparams.win_size / 2 + 1;` in float (flame.cc:847, 1771)."""
    return int(F32(F32(F32(rescale_factor_max) * F32(win_size)) / F32(2)) + F32(1))


def fast_ceil(r) -> int:
    ret = int(r)
    return ret + 1 if ret < r else ret


def rotate(q, vx, vy, vz):
    """Eigen Quaternionf * Vector3f (_transformVector): v + w uv + u x uv, uv = 2 (u x v)."""
    w, ux, uy, uz = (F32(c) for c in q)
    uvx = uy * vz - uz * vy
    uvy = uz * vx - ux * vz
    uvz = ux * vy - uy * vx
    uvx = uvx + uvx
    uvy = uvy + uvy
    uvz = uvz + uvz
    cx = uy * uvz - uz * uvy
    cy = uz * uvx - ux * uvz
    cz = ux * uvy - uy * uvx
    return (vx + w * uvx) + cx, (vy + w * uvy) + cy, (vz + w * uvz) + cz


def project_idepth(geo, ux, uy, idepth):
    """EpipolarGeometry::project(u_ref, idepth, &u_cmp, &new_idepth) (epipolar_geometry.h:152-180), elementwise.
    Returns (x, y, new_idepth, ok); ok False where the reference asserts."""
    ux, uy, idepth = (np.asarray(a, dtype=np.float32) for a in (ux, uy, idepth))
    K, Ki, M, t = _g(geo, "K"), _g(geo, "Kinv"), _g(geo, "KRKinv"), _g(geo, "t")
    q = _g(geo, "q")
    with np.errstate(all="ignore"):
        # maxDepthProjection (idepth == 0)
        h0 = (M[0] * ux + M[1] * uy) + M[2] * F32(1)
        h1 = (M[3] * ux + M[4] * uy) + M[5] * F32(1)
        h2 = (M[6] * ux + M[7] * uy) + M[8] * F32(1)
        inv = F32(1) / h2
        mx, my = h0 * inv, h1 * inv
        depth = F32(1) / idepth
        px = (Ki[0] * ux + Ki[2]) * depth
        py = (Ki[4] * uy + Ki[5]) * depth
        pz = F32(1) * depth
        rx, ry, rz = rotate(q, px, py, pz)
        pcx, pcy, pcz = rx + t[0], ry + t[1], rz + t[2]
        u0 = K[0] * pcx + K[2] * pcz
        u1 = K[4] * pcy + K[5] * pcz
        nid = F32(1) / pcz
        x, y = u0 * nid, u1 * nid
    zero = idepth == F32(0)
    ok = (idepth >= F32(0)) & (zero | (np.abs(pcz) > F32(0)))
    x = np.where(zero, mx, x).astype(np.float32)
    y = np.where(zero, my, y).astype(np.float32)
    nid = np.where(zero, F32(0), nid).astype(np.float32)
    return x, y, nid, ok


def reference_epiline(geo, ux, uy):
    """EpipolarGeometry::referenceEpiline (epipolar_geometry.h:303-325), elementwise: (ex, ey, ok); ok False where
    the reference asserts (norm2 <= 0 or NaN).  `1.0f / sqrt(norm2)` is the double sqrt."""
    ux, uy = np.asarray(ux, dtype=np.float32), np.asarray(uy, dtype=np.float32)
    K, tcr = _g(geo, "K"), _g(geo, "tcr")
    ex = -K[0] * tcr[0] + tcr[2] * (ux - K[2])
    ey = -K[4] * tcr[1] + tcr[2] * (uy - K[5])
    n2 = ex * ex + ey * ey
    ok = n2 > F32(0)
    with np.errstate(all="ignore"):
        inv = (1.0 / np.sqrt(n2.astype(np.float64))).astype(np.float32)
        return (ex * inv).astype(np.float32), (ey * inv).astype(np.float32), ok


def project_features(feats, geos, cur_frame_id, width, height, rescale_factor_max=1.4, win_size=5, do_letterbox=False):
    """Flame::projectFeatures.  feats: FEATURE_DTYPE array (the resident set); geos: {frame_id: Geometry of
    T_ref_to_cur}.  Returns (rc, error_feature, kept feats, feats_in_curr); on error both arrays are None."""
    n = feats.shape[0]
    border = border_of(rescale_factor_max, win_size)
    row_offset = height // 3 if do_letterbox else 0
    rx, ry = F32(border), F32(border + row_offset)
    rw, rh = F32(width - 2 * border), F32(height - 2 * border - 2 * row_offset)
    known = np.isin(feats["frame_id"], np.array(list(geos.keys()), dtype=np.uint32))
    if not known.all():
        return INVALID_ARG, int(np.nonzero(~known)[0][0]), None, None
    x = np.zeros(n, np.float32)
    y = np.zeros(n, np.float32)
    nid = np.zeros(n, np.float32)
    ok = np.ones(n, bool)
    for fid, geo in geos.items():
        sel = feats["frame_id"] == fid
        if sel.any():
            x[sel], y[sel], nid[sel], ok[sel] = project_idepth(geo, feats["x"][sel], feats["y"][sel], feats["idepth_mu"][sel])
    valid = feats["valid"] != 0
    bad = valid & ~ok
    if bad.any():
        return ASSERT, int(np.nonzero(bad)[0][0]), None, None
    inside = (rx <= x) & (x < rx + rw) & (ry <= y) & (y < ry + rh)
    keep = valid & inside & (nid >= F32(0))
    off = keep & ~((x >= 0) & (x < F32(width)) & (y >= 0) & (y < F32(height)))
    if off.any():
        return ASSERT, int(np.nonzero(off)[0][0]), None, None
    kept = feats[keep].copy()
    cur = np.zeros(kept.shape[0], dtype=feats.dtype)
    cur["id"] = kept["id"]
    cur["frame_id"] = cur_frame_id
    cur["x"], cur["y"] = x[keep], y[keep]
    cur["idepth_mu"] = nid[keep]
    mu = kept["idepth_mu"]
    with np.errstate(all="ignore"):
        v4 = cur["idepth_mu"] / mu
        v4 = v4 * v4
        v4 = v4 * v4
    v4 = np.where(mu.astype(np.float64) < 1e-6, F32(1), v4).astype(np.float32)
    cur["idepth_var"] = v4 * kept["idepth_var"]
    cur["valid"] = 1
    cur["num_updates"] = kept["num_updates"]
    return OK, -1, kept, cur


def detect_features(gx_pad, gy_pad, pad, width, height, geo, ref_frame_id, *, win=16, min_grad_mag=5.0,
                    idepth_init=0.01, idepth_var_init=0.25, rescale_factor_max=1.4, win_size=5, do_letterbox=False,
                    idepthmap=None, mask_xy=None, first_id=0, dtype=None, swap=True):
    """Flame::detectFeatures + the detection loop's initialisation.  geo: Geometry of T_ref_to_prev.  Returns
    (rc, error_pixel, new feats (dtype), number of cells).  swap=False passes (col, row) to referenceEpiline instead of
    the reference's (row, col) -- only for showing that the swap matters."""
    border = border_of(rescale_factor_max, win_size)
    row_offset = height // 3 if do_letterbox else 0
    hc = fast_ceil(F32(height) / F32(win))
    wc = fast_ceil(F32(width) / F32(win))
    g2 = F32(min_grad_mag) * F32(min_grad_mag)
    blocked = np.zeros((hc, wc), bool)
    if mask_xy is not None and len(mask_xy):
        m = np.asarray(mask_xy, np.float32).reshape(-1, 2)
        if not ((m[:, 0] >= 0) & (m[:, 1] >= 0) & (m[:, 0] < width) & (m[:, 1] < height)).all():
            return INVALID_ARG, -1, None, hc * wc
        cx = (m[:, 0] / F32(win)).astype(np.uint32)
        cy = (m[:, 1] / F32(win)).astype(np.uint32)
        if (cx >= wc).any() or (cy >= hc).any():
            return INVALID_ARG, -1, None, hc * wc
        blocked[cy, cx] = True
    r_lo, r_hi, c_lo, c_hi = border + row_offset, height - border - row_offset, border, width - border
    ii, jj = np.mgrid[r_lo:max(r_hi, r_lo), c_lo:max(c_hi, c_lo)]
    ii, jj = ii.ravel(), jj.ravel()
    gx = gx_pad[ii + pad, jj + pad].astype(np.float32)
    gy = gy_pad[ii + pad, jj + pad].astype(np.float32)
    cand = ~(gx * gx + gy * gy < g2)
    ux, uy = (ii, jj) if swap else (jj, ii)
    ex, ey, ok = reference_epiline(geo, ux.astype(np.float32), uy.astype(np.float32))  # (row, col) as (x, y)
    bad = cand & ~ok
    if bad.any():
        return ASSERT, int((ii[bad] * width + jj[bad]).min()), None, hc * wc
    with np.errstate(all="ignore"):
        epigrad = gx * ex + gy * ey
        e2 = epigrad * epigrad
    take = cand & ~(e2 < g2) & (e2 >= 0)
    ci = (ii.astype(np.float32) / F32(win)).astype(np.int64)
    cj = (jj.astype(np.float32) / F32(win)).astype(np.int64)
    cell = ci * wc + cj
    # per cell: the largest score, ties to the last pixel in row-major scan order (the reference's `>=`)
    t = np.nonzero(take)[0]
    order = np.lexsort((t, e2[t], cell[t]))  # by cell, then score, then scan position
    t = t[order]
    last = np.r_[cell[t][1:] != cell[t][:-1], True] if t.size else np.zeros(0, bool)
    win_idx = t[last]
    best = np.zeros(hc * wc, np.float32)
    pos = np.full(hc * wc, -1, np.int64)
    best[cell[win_idx]] = e2[win_idx]
    pos[cell[win_idx]] = win_idx
    emit = np.nonzero((~blocked.ravel()) & (best > 0))[0]
    src = pos[emit]
    out = np.zeros(emit.size, dtype=dtype)
    out["id"] = (first_id + np.arange(emit.size)).astype(np.uint32)
    out["frame_id"] = ref_frame_id
    out["x"], out["y"] = jj[src].astype(np.float32), ii[src].astype(np.float32)
    mu = np.full(emit.size, F32(idepth_init), np.float32)
    if idepthmap is not None:
        d = np.asarray(idepthmap, np.float32)[ii[src], jj[src]]
        mu = np.where(np.isnan(d), mu, d).astype(np.float32)
    out["idepth_mu"] = mu
    out["idepth_var"] = F32(idepth_var_init)
    out["valid"] = 1
    return OK, -1, out, hc * wc


def detect_scan_literal(gx_pad, gy_pad, pad, width, height, geo, win, min_grad_mag, border, row_offset=0):
    """The reference's scan loop (flame.cc:1017-1047) written out pixel by pixel, for small images: {cell: (x, y)}
    of the cells whose best score is > 0.  Used to check the vectorised checker's tie rule."""
    K, tcr = _g(geo, "K"), _g(geo, "tcr")
    hc, wc = fast_ceil(F32(height) / F32(win)), fast_ceil(F32(width) / F32(win))
    g2 = F32(min_grad_mag) * F32(min_grad_mag)
    best = np.zeros((hc, wc), np.float32)
    pxc = {}
    for ii in range(border + row_offset, height - border - row_offset):
        for jj in range(border, width - border):
            gx, gy = F32(gx_pad[ii + pad, jj + pad]), F32(gy_pad[ii + pad, jj + pad])
            if gx * gx + gy * gy < g2:
                continue
            ux, uy = F32(ii), F32(jj)
            ex = -K[0] * tcr[0] + tcr[2] * (ux - K[2])
            ey = -K[4] * tcr[1] + tcr[2] * (uy - K[5])
            inv = F32(1.0 / np.sqrt(np.float64(ex * ex + ey * ey)))
            ex, ey = ex * inv, ey * inv
            epigrad = gx * ex + gy * ey
            e2 = epigrad * epigrad
            if e2 < g2:
                continue
            ci, cj = int(F32(ii) / F32(win)), int(F32(jj) / F32(win))
            if e2 >= best[ci, cj]:
                best[ci, cj] = e2
                pxc[(ci, cj)] = (jj, ii)
    return {c: p for c, p in pxc.items() if best[c] > 0}
