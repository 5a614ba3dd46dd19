"""CPU checker of the detections debug image (getDebugImageDetections; include/flame_stereo.h, flame_stereo_draw_detections)
(TEST INFRASTRUCTURE): a float32 numpy restatement of

    the `score` image of Flame::detectFeatures' scan loop   flame.cc:1212-1251 (written at :1249)
    Flame::drawDetections                                   flame.cc:2363-2412
    utils::applyColorMap                                    utils/visualization.h:272-287

with the reference's expression order.  The epiline and the border come from tests/frontend_ref.py, the colour map from
tests/debug_ref.py (jet(v, 0, max_score)); the gradients from oracle.stereo_capi.make_frame.

UNPINNED (OpenCV is not part of this tree, and the front-end is not pinned to a reference binary): the blend
`0.7 * debug_img + 0.3 * img_rgb` on 8-bit data is read as cv::addWeighted(A, 0.7, B, 0.3, 0): alpha = (float)0.7, beta = (float)0.3,
per channel t = (float)c * alpha + (float)g * beta in float (two rounded products, one rounded sum, no FMA), then
saturate_cast<uchar>(t) = round to nearest, ties to even, clamped to [0, 255].

Return codes follow flame_nltgv2_status: 0 or ASSERT (-8).
"""
from __future__ import annotations

import numpy as np

from tests import debug_ref as dr
from tests import frontend_ref as fr

OK, ASSERT = fr.OK, fr.ASSERT
F32 = np.float32
ALPHA, BETA = F32(0.7), F32(0.3)


def scan_rect(width, height, rescale_factor_max=1.4, win_size=5, do_letterbox=False):
    """(r_lo, r_hi, c_lo, c_hi) of detectFeatures' scan loop (flame.cc:1216-1217)."""
    border = fr.border_of(rescale_factor_max, win_size)
    row_offset = height // 3 if do_letterbox else 0
    return border + row_offset, height - border - row_offset, border, width - border


def num_examined(width, height, **kw):
    r_lo, r_hi, c_lo, c_hi = scan_rect(width, height, **kw)
    return max(r_hi - r_lo, 0) * max(c_hi - c_lo, 0)


def detection_score(gx_pad, gy_pad, pad, width, height, geo, *, min_grad_mag=5.0, rescale_factor_max=1.4, win_size=5,
                    do_letterbox=False, swap=True):
    """The `score` image of detectFeatures, vectorised.  geo: Geometry of T_ref_to_prev.  Returns (rc, error_pixel, score):
    score is (height, width) float32, NaN where the reference leaves its initial NaN; on ASSERT error_pixel is the lowest
    row * width + col whose referenceEpiline asserts after the first gradient test, and such pixels stay NaN.
    swap=False passes (col, row) to referenceEpiline instead of the reference's (row, col), only to show the swap matters."""
    r_lo, r_hi, c_lo, c_hi = scan_rect(width, height, rescale_factor_max, win_size, do_letterbox)
    score = np.full((height, width), np.nan, np.float32)
    g2 = F32(min_grad_mag) * F32(min_grad_mag)
    ii, jj = np.mgrid[r_lo:max(r_hi, r_lo), c_lo:max(c_hi, c_lo)]
    ii, jj = ii.ravel(), jj.ravel()
    gx = gx_pad[ii + pad, jj + pad].astype(np.float32)
    gy = gy_pad[ii + pad, jj + pad].astype(np.float32)
    with np.errstate(all="ignore"):
        cand = ~(gx * gx + gy * gy < g2)
        ux, uy = (ii, jj) if swap else (jj, ii)
        ex, ey, ok = fr.reference_epiline(geo, ux.astype(np.float32), uy.astype(np.float32))  # (row, col) as (x, y)
        epigrad = gx * ex + gy * ey
        e2 = epigrad * epigrad
        take = cand & ok & ~(e2 < g2)
        score[ii[take], jj[take]] = np.abs(epigrad[take])
    bad = cand & ~ok
    if bad.any():
        return ASSERT, int((ii[bad] * width + jj[bad]).min()), score
    return OK, -1, score


def detection_score_literal(gx_pad, gy_pad, pad, width, height, geo, *, min_grad_mag=5.0, rescale_factor_max=1.4, win_size=5,
                            do_letterbox=False):
    """The reference's double loop (flame.cc:1216-1251) written out pixel by pixel, for small images: the score image."""
    K, tcr = fr._g(geo, "K"), fr._g(geo, "tcr")
    border = fr.border_of(rescale_factor_max, win_size)
    row_offset = height // 3 if do_letterbox else 0
    score = np.full((height, width), np.nan, np.float32)
    g2 = F32(min_grad_mag) * F32(min_grad_mag)
    with np.errstate(all="ignore"):
        for ii in range(border + row_offset, height - border - row_offset):
            for jj in range(border, width - border):
                gx, gy = F32(gx_pad[ii + pad, jj + pad]), F32(gy_pad[ii + pad, jj + pad])
                if gx * gx + gy * gy < g2:
                    continue
                ux, uy = F32(ii), F32(jj)
                ex = -K[0] * tcr[0] + tcr[2] * (ux - K[2])
                ey = -K[4] * tcr[1] + tcr[2] * (uy - K[5])
                n2 = ex * ex + ey * ey
                assert n2 > 0, "referenceEpiline asserts at (%d, %d)" % (ii, jj)
                inv = F32(1.0 / np.sqrt(np.float64(n2)))
                ex, ey = ex * inv, ey * inv
                epigrad = gx * ex + gy * ey
                if epigrad * epigrad < g2:
                    continue
                score[ii, jj] = abs(epigrad)
    return score


def blend(c, g):
    """cv::addWeighted(c, 0.7, g, 0.3, 0) on bytes, elementwise (UNPINNED, see the module's docstring)."""
    c, g = np.asarray(c, np.uint8), np.asarray(g, np.uint8)
    t = (c.astype(np.float32) * ALPHA).astype(np.float32) + (g.astype(np.float32) * BETA).astype(np.float32)
    return np.clip(np.rint(t.astype(np.float32)), 0, 255).astype(np.uint8)


def jet_branch(score, max_score):
    """Which branch of utils::jet(v, 0, max_score) each pixel takes: 0 = unscored (NaN), 1..4 = the four branches, with
    debug_ref.jet's comparisons."""
    v = np.asarray(score, np.float32)
    vmax = F32(max_score)
    with np.errstate(all="ignore"):
        c = np.where(v < F32(0), F32(0), v).astype(np.float32)
        c = np.where(c > vmax, vmax, c).astype(np.float64)
        dv = np.float64(F32(vmax - F32(0)))
        b = np.where(c < 0.25 * dv, 1, np.where(c < 0.5 * dv, 2, np.where(c < 0.75 * dv, 3, 4)))
    return np.where(np.isnan(v), 0, b)


def draw_detections(img, score, max_score=0.005, flip=False):
    """Flame::drawDetections (flame.cc:2363-2412) without the text overlay: (height, width, 3) uint8."""
    score = np.asarray(score, np.float32)
    col = np.zeros(score.shape + (3,), np.uint8)
    ok = ~np.isnan(score)
    col[ok] = dr.jet(score[ok], 0.0, max_score)
    out = blend(col, dr._gray3(img))
    return dr._flip(out, flip)
