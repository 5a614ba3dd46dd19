"""CPU checker of prunePoseFrames (TEST INFRASTRUCTURE): the two feature loops of

    Flame::prunePoseFrames                         flame.cc:608-700
    stereo::inverse_depth_filter::predict          inverse_depth_filter.cc:35-63

in numpy float32, one feature at a time in the reference's order.  The projection step is
tests/frontend_ref.project_idepth (EpipolarGeometry::project, elementwise and therefore evaluated for all features
up front: it reads nothing the loop writes); everything after it is scalar float32 code per feature.

What the loops do, as include/flame_stereo.h lists it:
  1. the target is the kept pose-frame with the largest id (`pruned_pfs.crbegin()` of a std::map) -- the caller's job,
     `target_of` does it;
  2. `valid` is not tested;
  3. a feats_ record (index < first_new) is overwritten before the success test;
  4. idepth_var *= (idepth_pf / old)^4 by two squarings, 1 when double(idepth_pf) < 1e-6; var_pred is discarded;
  5. cv::Rect (integers) .contains(cv::Point2f): the point is rounded to nearest, ties to even, first (cvRound).
     UNPINNED: OpenCV is not available to check this reading against.  A NaN (or out-of-int-range) coordinate is
     outside: cvRound gives INT_MIN on x86;
  6. where project asserts: ASSERT with the lowest index, nothing changes;
  7. a failed feats_ record is kept with valid = 0, a failed new_feats_ record (index >= first_new) is removed
     unrewritten.

This is our restatement of the reference, not the reference: parity with its binary is unpinned like the rest of the
front-end.  Return codes follow flame_nltgv2_status: 0, INVALID_ARG (-1) or ASSERT (-8).
"""
from __future__ import annotations

import numpy as np

from tests.frontend_ref import ASSERT, INVALID_ARG, OK, border_of, project_idepth

F32 = np.float32
STAT_NAMES = ("num_examined", "num_moved", "num_invalidated", "num_removed", "num_features", "error_feature")


def target_of(keep_ids) -> int:
    """`pruned_pfs.crbegin()` of a std::map<uint32_t, ...>: the largest kept id."""
    return max(int(k) for k in keep_ids)


def valid_region(width, height, rescale_factor_max=1.4, win_size=5, do_letterbox=False):
    """cv::Rect valid_region(border, border + row_offset, width - 2 border, height - 2 border - 2 row_offset)."""
    border = border_of(rescale_factor_max, win_size)
    row_offset = height // 3 if do_letterbox else 0
    return border, border + row_offset, width - 2 * border, height - 2 * border - 2 * row_offset


def cv_round(v) -> int:
    """cvRound(float): to nearest, ties to even; INT_MIN for NaN and for values outside int (x86 cvtss2si)."""
    v = float(v)
    if v != v or not (-2147483648.0 <= v < 2147483648.0):
        return -2147483648
    r = int(np.rint(np.float64(v)))
    return r if -2147483648 <= r <= 2147483647 else -2147483648


def rect_contains(rect, x, y) -> bool:
    rx, ry, rw, rh = rect
    ix, iy = cv_round(x), cv_round(y)
    return rx <= ix < rx + rw and ry <= iy < ry + rh


def prune_pose_frames(feats, keep_ids, dropped_geos, target_frame_id, width, height, first_new=None,
                      rescale_factor_max=1.4, win_size=5, do_letterbox=False):
    """feats: FEATURE_DTYPE array, [0, first_new) = feats_, [first_new, n) = new_feats_ (None: all feats_).
    dropped_geos: {frame_id: Geometry of target.pose.inverse() * pf.pose}.  Returns (rc, stats dict, pruned array);
    on error the array is None and stats["error_feature"] the lowest offending index."""
    n = feats.shape[0]
    first_new = n if first_new is None else int(first_new)
    keep = set(int(k) for k in keep_ids)
    stats = dict.fromkeys(STAT_NAMES + ("num_behind", "num_outside"), 0)  # (the last two: the checker's own detail)
    stats["num_examined"], stats["num_features"], stats["error_feature"] = n, n, -1
    if (not keep or int(target_frame_id) not in keep or any(int(k) in keep for k in dropped_geos)
            or not 0 <= first_new <= n):
        return INVALID_ARG, stats, None
    rect = valid_region(width, height, rescale_factor_max, win_size, do_letterbox)
    fid = feats["frame_id"]
    orphan = ~np.isin(fid, np.array(sorted(keep), dtype=np.uint32))
    unknown = orphan & ~np.isin(fid, np.array(sorted(dropped_geos.keys()), dtype=np.uint32))
    # EpipolarGeometry::project of every orphan (elementwise; reads only the input records)
    px = np.zeros(n, np.float32)
    py = np.zeros(n, np.float32)
    pd = np.zeros(n, np.float32)
    ok = np.ones(n, bool)
    for f_id, geo in dropped_geos.items():
        sel = orphan & (fid == f_id)
        if sel.any():
            px[sel], py[sel], pd[sel], ok[sel] = project_idepth(geo, feats["x"][sel], feats["y"][sel],
                                                               feats["idepth_mu"][sel])
    if unknown.any():  # pfs_[feat.frame_id] of a frame that is not there
        stats["error_feature"] = int(np.nonzero(unknown)[0][0])
        return INVALID_ARG, stats, None
    if (orphan & ~ok).any():  # FLAME_ASSERT in project (epipolar_geometry.h:128, 139)
        stats["error_feature"] = int(np.nonzero(orphan & ~ok)[0][0])
        return ASSERT, stats, None
    out = feats.copy()
    kept_rows = []
    with np.errstate(all="ignore"):
        for ii in range(n):
            if not orphan[ii]:
                kept_rows.append(ii)
                continue
            feat = out[ii]
            # inverse_depth_filter::predict
            u_x, u_y, idepth_pf = F32(px[ii]), F32(py[ii]), F32(pd[ii])
            move_success = True
            if idepth_pf < F32(0.0):
                idepth_pf = F32(0.0)
                move_success = False
            fine = move_success and rect_contains(rect, u_x, u_y)
            if not move_success:
                stats["num_behind"] += 1
            elif not fine:
                stats["num_outside"] += 1
            if ii >= first_new and not fine:  # new_feats_: `continue` before anything is written (flame.cc:675-678)
                stats["num_removed"] += 1
                continue
            feat["frame_id"] = target_frame_id
            feat["x"], feat["y"] = u_x, u_y
            old_idepth = F32(feat["idepth_mu"])
            feat["idepth_mu"] = idepth_pf
            var_factor4 = F32(idepth_pf / old_idepth)
            var_factor4 = F32(var_factor4 * var_factor4)
            var_factor4 = F32(var_factor4 * var_factor4)
            if float(idepth_pf) < 1e-6:
                var_factor4 = F32(1)
            feat["idepth_var"] = F32(F32(feat["idepth_var"]) * var_factor4)
            if not fine:  # feats_: marked, kept (flame.cc:643-647)
                feat["valid"] = 0
                stats["num_invalidated"] += 1
            else:
                stats["num_moved"] += 1
            kept_rows.append(ii)
    pruned = out[np.array(kept_rows, dtype=np.int64)] if len(kept_rows) != n else out
    stats["num_features"] = pruned.shape[0]
    return OK, stats, pruned


def prune_vectorised(feats, keep_ids, dropped_geos, target_frame_id, width, height, first_new=None,
                     rescale_factor_max=1.4, win_size=5, do_letterbox=False):
    """The same result by whole-array numpy (no error paths): what a host-side caller would write.  Used as the fair
    host baseline of tools/prune_bench.py and checked against prune_pose_frames by the tests."""
    n = feats.shape[0]
    first_new = n if first_new is None else int(first_new)
    rx, ry, rw, rh = valid_region(width, height, rescale_factor_max, win_size, do_letterbox)
    fid = feats["frame_id"]
    orphan = ~np.isin(fid, np.array(sorted(int(k) for k in keep_ids), dtype=np.uint32))
    out = feats.copy()
    idx = np.nonzero(orphan)[0]
    if idx.size == 0:
        return out
    px = np.zeros(idx.size, np.float32)
    py = np.zeros(idx.size, np.float32)
    pd = np.zeros(idx.size, np.float32)
    sub = feats[idx]
    for f_id, geo in dropped_geos.items():
        sel = sub["frame_id"] == f_id
        if sel.any():
            px[sel], py[sel], pd[sel], _ = project_idepth(geo, sub["x"][sel], sub["y"][sel], sub["idepth_mu"][sel])
    with np.errstate(all="ignore"):
        success = ~(pd < F32(0))
        pd = np.where(success, pd, F32(0)).astype(np.float32)
        finite = np.isfinite(px) & np.isfinite(py) & (np.abs(px) < 2.0 ** 31) & (np.abs(py) < 2.0 ** 31)
        ix = np.where(finite, np.rint(px.astype(np.float64)), -2.0 ** 31)
        iy = np.where(finite, np.rint(py.astype(np.float64)), -2.0 ** 31)
        fine = success & (rx <= ix) & (ix < rx + rw) & (ry <= iy) & (iy < ry + rh)
        v4 = pd / sub["idepth_mu"]
        v4 = v4 * v4
        v4 = v4 * v4
        v4 = np.where(pd.astype(np.float64) < 1e-6, F32(1), v4).astype(np.float32)
        new = sub.copy()
        new["frame_id"] = target_frame_id
        new["x"], new["y"], new["idepth_mu"] = px, py, pd
        new["idepth_var"] = sub["idepth_var"] * v4
    new["valid"] = np.where(fine, sub["valid"], 0)
    out[idx] = new
    gone = np.zeros(n, bool)
    gone[idx[~fine & (idx >= first_new)]] = True
    return out[~gone] if gone.any() else out
