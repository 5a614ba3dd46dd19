"""The detections picture (getDebugImageDetections; include/flame_stereo.h, flame_stereo_draw_detections) on the CPU: the C-ABI
surface, and the checker tests/detections_ref.py against the reference's loop written out, against the detection checker
(tests/frontend_ref.py) and against the blend's stated rounding.  The GPU side is tests/test_gpu_detections.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from flame_amd import synth_stereo as ss
from oracle import stereo_capi as so
from tests import detections_ref as dt
from tests import frontend_ref as fr
from tests.conftest import ROOT
from tests.test_feature_frontend import PAD, geometry, plane_scene, tie_ramp

F32 = np.float32
NAME = "flame_stereo_draw_detections"


# ---- the scenes the CPU and GPU tests share -----------------------------------------------------------------------------

def scene_case(size):
    """(img, K, Kinv, q, t, geo) of the test sizes: the 160x96 one is the tie ramp with a pure x-translation, the others the
    plane scene's pose-frame 10 against frame 9."""
    w, h = size
    if size == (160, 96):
        img = tie_ramp(w, h)
        K, Kinv = ss.intrinsics(w, h)
        q, t = np.float32([1, 0, 0, 0]), np.float32([0.1, 0, 0])
    else:
        sc = plane_scene(w, h)
        img, K, Kinv = sc.render(10), sc.K32, sc.Kinv32
        q, t = sc.relative(10, 9)
    return img, K, Kinv, q, t, so.load_geometry(K, Kinv, q, t)


def checker_picture(img, geo, *, max_score=0.005, flip=False, min_grad_mag=5.0, do_letterbox=False, swap=True):
    """(rc, error_pixel, score, picture) of the checker on a host image."""
    h, w = img.shape
    _, gx, gy = so.make_frame(img, PAD)
    rc, px, score = dt.detection_score(gx, gy, PAD, w, h, geo, min_grad_mag=min_grad_mag, do_letterbox=do_letterbox, swap=swap)
    return rc, px, score, dt.draw_detections(img, score, max_score, flip)


# ---- the C-ABI surface ---------------------------------------------------------------------------------------------------

def test_symbol_is_exported_declared_and_listed(built):
    import flame_amd
    from flame_amd.stereo import STEREO_ABI_SYMBOLS

    nm = subprocess.check_output(["nm", "-D", "--defined-only", flame_amd.library_path()], text=True)
    assert NAME in STEREO_ABI_SYMBOLS
    assert (" T %s\n" % NAME) in nm
    hdr = open(os.path.join(ROOT, "include", "flame_stereo.h")).read()
    assert NAME + "(" in hdr and "UNPINNED: this reads the MatExpr" in hdr


def test_stats_struct_is_plain_c99_of_12_bytes(built, tmp_path):
    from flame_amd.stereo import _DetectionsStats

    src = tmp_path / "t.c"
    src.write_text('#include "flame_stereo.h"\n'
                   'typedef int (*draw_fn)(flame_stereo_ctx*, const flame_stereo_params*, const flame_stereo_detect_params*,\n'
                   '                       uint32_t, const float*, const float*, float, int, uint8_t*,\n'
                   '                       flame_stereo_detections_stats*);\n'
                   'typedef char size_is_12[sizeof(flame_stereo_detections_stats) == 12 ? 1 : -1];\n'
                   'int main(void) { flame_stereo_detections_stats s; draw_fn d = flame_stereo_draw_detections;\n'
                   '  s.num_scored = 0; s.num_examined = 0; s.error_pixel = -1;\n'
                   '  return d == 0 ? 1 : s.num_scored + s.num_examined + s.error_pixel + 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "t.o")])
    assert C.sizeof(_DetectionsStats) == 12


def test_null_context_is_invalid_arg(built):
    from flame_amd.stereo import DetectParams, StereoParams, _DetectionsStats, _lib

    L = _lib()
    p, dp, st = StereoParams(), DetectParams(), _DetectionsStats()
    q = (C.c_float * 4)(1, 0, 0, 0)
    t = (C.c_float * 3)(0.1, 0, 0)
    img = np.full(12, 0xA5, np.uint8)
    assert L.flame_stereo_draw_detections(None, C.byref(p), C.byref(dp), 1, q, t, C.c_float(0.005), 0, img.ctypes.data,
                                          C.byref(st)) == -1
    assert (img == 0xA5).all()


# ---- the checker checks itself -------------------------------------------------------------------------------------------

def _same_with_nans(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("size,letterbox,mag", [((61, 37), False, 5.0), ((61, 37), True, 5.0), ((61, 37), False, 0.0),
                                                ((160, 96), False, 1.0), ((160, 96), True, 5.0)])
def test_vectorised_score_equals_the_literal_loop(size, letterbox, mag):
    img, K, Kinv, q, t, geo = scene_case(size)
    w, h = size
    _, gx, gy = so.make_frame(img, PAD)
    rc, px, score = dt.detection_score(gx, gy, PAD, w, h, geo, min_grad_mag=mag, do_letterbox=letterbox)
    lit = dt.detection_score_literal(gx, gy, PAD, w, h, geo, min_grad_mag=mag, do_letterbox=letterbox)
    assert (rc, px) == (0, -1)
    # |x| of a non-NaN float has one bit pattern and the NaN written at the start is numpy's in both: compare the bytes
    assert np.array_equal(np.isnan(score), np.isnan(lit))
    assert _same_with_nans(np.nan_to_num(score, nan=-1.0), np.nan_to_num(lit, nan=-1.0))
    r_lo, r_hi, c_lo, c_hi = dt.scan_rect(w, h, do_letterbox=letterbox)
    inside = np.zeros((h, w), bool)
    inside[r_lo:r_hi, c_lo:c_hi] = True
    assert np.isnan(score[~inside]).all() and (~np.isnan(score)).sum() > 0
    assert dt.num_examined(w, h, do_letterbox=letterbox) == inside.sum()


def test_score_of_the_tie_ramp_is_the_gradient():
    """gx = 2 (a central difference of a ramp of slope 2), gy = 0, epiline (+-1, 0): every scored pixel scores 2."""
    img, K, Kinv, q, t, geo = scene_case((160, 96))
    _, gx, gy = so.make_frame(img, PAD)
    _, _, score = dt.detection_score(gx, gy, PAD, 160, 96, geo, min_grad_mag=1.0)
    r_lo, r_hi, c_lo, c_hi = dt.scan_rect(160, 96)
    assert (r_lo, r_hi, c_lo, c_hi) == (4, 92, 4, 156)
    away = np.ones(160, bool)
    away[126:131] = False  # the wrap columns and their neighbours
    away[:c_lo] = away[c_hi:] = False
    assert (score[r_lo:r_hi][:, away] == F32(2)).all()


def test_zero_translation_reports_the_lowest_asserting_pixel():
    img, K, Kinv, q, t, _ = scene_case((61, 37))
    geo = so.load_geometry(K, Kinv, [1, 0, 0, 0], [0, 0, 0])
    _, gx, gy = so.make_frame(img, PAD)
    rc, px, score = dt.detection_score(gx, gy, PAD, 61, 37, geo)
    rc_d, px_d, _, _ = fr.detect_features(gx, gy, PAD, 61, 37, geo, 10, dtype=so.FEATURE_DTYPE)
    assert rc == dt.ASSERT and (rc, px) == (rc_d, px_d) and np.isnan(score).all()


def test_score_is_consistent_with_detection():
    """What the picture shows is what detectFeatures selected from."""
    sc = plane_scene(320, 240)
    img = sc.render(10)
    geo = geometry(sc, 10, 9)
    _, gx, gy = so.make_frame(img, PAD)
    win = 16
    rng = np.random.default_rng(11)
    mask = np.stack([rng.uniform(0, 319.9, 40), rng.uniform(0, 239.9, 40)], 1).astype(np.float32)
    rc, _, feats, ncells = fr.detect_features(gx, gy, PAD, 320, 240, geo, 10, win=win, mask_xy=mask, dtype=so.FEATURE_DTYPE)
    rc2, _, score = dt.detection_score(gx, gy, PAD, 320, 240, geo)
    assert rc == 0 and rc2 == 0 and feats.shape[0] > 100
    fx, fy = feats["x"].astype(np.int64), feats["y"].astype(np.int64)
    assert not np.isnan(score[fy, fx]).any()  # every feature sits on a scored pixel
    wc = fr.fast_ceil(F32(320) / F32(win))
    ii, jj = np.nonzero(~np.isnan(score))
    cell = (ii.astype(np.float32) / F32(win)).astype(np.int64) * wc + (jj.astype(np.float32) / F32(win)).astype(np.int64)
    s2 = score[ii, jj] * score[ii, jj]  # |epigrad|^2 = epigrad * epigrad, bit for bit
    best = np.zeros(ncells, np.float32)
    np.maximum.at(best, cell, s2)
    fcell = (fy.astype(np.float32) / F32(win)).astype(np.int64) * wc + (fx.astype(np.float32) / F32(win)).astype(np.int64)
    assert np.array_equal(score[fy, fx] * score[fy, fx], best[fcell])  # ... the best of its cell
    blocked = np.zeros(ncells, bool)
    blocked[(mask[:, 1] / F32(win)).astype(np.int64) * wc + (mask[:, 0] / F32(win)).astype(np.int64)] = True
    assert blocked[np.unique(cell)].any()  # (the mask does take cells away)
    # a cell with a scored pixel and no mask point emits a feature, and no other cell does
    assert np.array_equal(np.sort(fcell), np.setdiff1d(np.unique(cell), np.nonzero(blocked)[0]))


# ---- the blend -------------------------------------------------------------------------------------------------------------

def test_blend_table_against_float64():
    """All 256 x 256 (c, g) pairs.  The float path makes three roundings of values below 256 (ulp 2^-16): it stays within
    1.5 ulp of the float64 value of 0.7f * c + 0.3f * g, and the byte differs from that value's rounding only where it lies
    within that distance of a tie."""
    c, g = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    got = dt.blend(c.astype(np.uint8), g.astype(np.uint8)).astype(np.float64)
    t64 = np.float64(F32(0.7)) * c + np.float64(F32(0.3)) * g
    tol = 1.5 * 2.0 ** -16
    assert np.abs(got - t64).max() <= 0.5 + tol
    differs = got != np.rint(t64)
    near_tie = np.abs(np.abs(t64 - np.floor(t64)) - 0.5) <= tol
    assert differs.any() and near_tie[differs].all()
    assert got.min() == 0 and got.max() == 255  # (0, 0) and (255, 255): the clamp is never needed


def test_blend_exact_ties_go_to_even():
    # 0.3f = 0.300000011920929: 5 * 0.3f = 1.50000005960464 lies exactly between the floats 1.5 and 1.50000011920929 and rounds
    # to the even mantissa, 1.5: an exact tie in float although the float64 value lies above it
    assert F32(5) * F32(0.3) == F32(1.5)
    for c, g, want in ((0, 5, 2), (0, 15, 4), (0, 255, 76), (1, 6, 2), (3, 8, 4), (0, 65, 20), (2, 7, 4)):
        t = F32(F32(c) * F32(0.7)) + F32(F32(g) * F32(0.3))
        assert t - np.floor(t) == F32(0.5), (c, g, t)
        assert dt.blend(c, g) == want, (c, g)
    # (0, 15): the float64 value 4.50000017881393 and round-half-up would both say 5
    assert np.rint(np.float64(F32(0.3)) * 15) == 5
    # not ties
    assert (dt.blend(0, 100), dt.blend(255, 0), dt.blend(255, 100), dt.blend(255, 255)) == (30, 178, 208, 255)


def test_picture_known_answers():
    """Unscored: rne(g * 0.3f) three times.  A score at or above max_score: jet's last branch at v = vmax, (0, 0, 255).  Score 0:
    the first branch at v = vmin, (255, 0, 0).  Flip reverses the pixel order."""
    img = np.uint8([[100, 0, 200]])
    score = np.float32([[np.nan, 7.0, 0.0]])
    out = dt.draw_detections(img, score, 0.005)
    assert out.tolist() == [[[30, 30, 30], [0, 0, 178], [238, 60, 60]]]
    assert dt.draw_detections(img, score, 0.005, flip=True).tolist() == [[[238, 60, 60], [0, 0, 178], [30, 30, 30]]]
    assert dt.jet_branch(score, 0.005).tolist() == [[0, 4, 1]]


def test_max_scores_and_thresholds_reach_every_branch_of_jet():
    img, K, Kinv, q, t, geo = scene_case((320, 240))
    _, gx, gy = so.make_frame(img, PAD)
    seen, per_case = set(), {}
    for mag in (0.0, 5.0):
        _, _, score = dt.detection_score(gx, gy, PAD, 320, 240, geo, min_grad_mag=mag)
        for max_score in (0.005, 8.0, 64.0, 255.0):
            counts = np.bincount(dt.jet_branch(score, max_score).ravel(), minlength=5)
            per_case[(mag, max_score)] = counts
            seen |= {b for b in range(1, 5) if counts[b]}
            # the branch a pixel is counted in is the branch debug_ref.jet paints it with
            col = dt.dr.jet(np.nan_to_num(score, nan=0.0).ravel(), 0.0, max_score).reshape(240, 320, 3)
            br = dt.jet_branch(score, max_score)
            assert (col[br == 1][:, 2] == 0).all() and (col[br == 1][:, 0] == 255).all()
            assert (col[br == 2][:, 2] == 0).all() and (col[br == 2][:, 1] == 255).all()
            assert (col[br == 3][:, 0] == 0).all() and (col[br == 3][:, 1] == 255).all()
            assert (col[br == 4][:, 0] == 0).all() and (col[br == 4][:, 2] == 255).all()
    assert seen == {1, 2, 3, 4}, per_case
    # the reference's literal with its default threshold: every scored pixel clamps to vmax
    assert per_case[(5.0, 0.005)][1:4].sum() == 0 and per_case[(5.0, 0.005)][4] > 0
    # min_grad_mag = 0 scores the flat pixels (epigrad = 0): the first branch
    assert per_case[(0.0, 64.0)][1] > 0
    assert all(per_case[(0.0, m)][0] == 240 * 320 - dt.num_examined(320, 240) for m in (0.005, 8.0, 64.0, 255.0))
