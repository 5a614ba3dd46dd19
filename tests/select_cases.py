"""Inputs of the graph-vertex selection tests (TEST INFRASTRUCTURE), built on tests/prune_cases.py: its scene (five
pose-frames 10..22, frames 23 and 24 after them) and its features (anchors drawn at random, 10 % invalid, a few with
idepth_mu 0, 5e-7 and 60), with idepth_var redrawn from U(0.002, 0.02) so that the default threshold 1e-2 splits them.

The projected records (feats_in_curr) are tests/frontend_ref.py's projection into frame 23 where it succeeds and
ZEROED records elsewhere: the rule never tests the projected record's `valid` flag, so such a record can be selected and
its zeros then appear in the output -- that is part of what is compared.  These two arrays go through the form on the
caller's arrays.  For the resident form the same features go through set_features + project_features first (what is
left is all valid); `resident_sets` is the checker's version of that, optionally followed by an in-place prune whose
moves fail, which brings invalid records back.

The world pose (camera -> world) of a camera (R, t) of PlaneScene is (R^T, -R^T t): the scene's cameras map world
points into the camera.  With the default band [0.1, 4] the selected features lie in the upper part of the image
(-world.y is "up").
"""
from __future__ import annotations

import numpy as np

from flame_amd import synth_stereo as ss
from oracle import stereo_capi as so
from tests import frontend_ref as fr
from tests import prune_cases as pc
from tests import prune_ref as pr

CUR = 23  # the frame the features are projected into
SIZES = (1, 64, 255, 256, 257, 1500, 8400, 16000, 61000, 61441)
BANDS = (dict(), dict(min_height=-0.5, max_height=1.5))  # the default band, and one with a negative min_height
SCALES = (1.0, 0.37, 2.5)
PRUNE = ([10, 13, 16], [19, 22], 16)  # (keep ids, dropped ids, target = the largest kept id)
_SCENES = {}
_CASES = {}


def size_of(n):
    return "320x240" if n <= 1500 else ("640x480" if n <= 16000 else "1920x1080")


def scene_for(n):
    size = size_of(n)
    if size not in _SCENES:
        _SCENES[size] = pc.scene(size)
    return _SCENES[size]


def world_poses(sc, ids=pc.PF_IDS):
    out = []
    for k in ids:
        R, t = sc.cams[k]
        out.append(dict(id=k, q=ss.quat_from_rot(R.T).astype(np.float32), t=(-R.T @ t).astype(np.float32)))
    return out


def world_pose64(sc, k):
    R, t = sc.cams[k]
    return R.T, -R.T @ t


def project_geos(sc, ids=pc.PF_IDS, cur=CUR):
    return {a: so.load_geometry(sc.K32, sc.Kinv32, *sc.relative(a, cur)) for a in ids}


def project_poses(sc, ids=pc.PF_IDS, cur=CUR):
    return [dict(id=a, q_to_new=sc.relative(a, cur)[0], t_to_new=sc.relative(a, cur)[1]) for a in ids]


def projected_aligned(sc, feats, cur=CUR):
    """One projected record per feature, index-aligned: projectFeatures' record where the feature is valid and its
    projection stays inside the valid region in front of the camera, a zeroed record elsewhere."""
    n = feats.shape[0]
    out = np.zeros(n, feats.dtype)
    border = fr.border_of(1.4, 5)
    rx, ry = np.float32(border), np.float32(border)
    rw, rh = np.float32(sc.width - 2 * border), np.float32(sc.height - 2 * border)
    for a, geo in project_geos(sc, cur=cur).items():
        sel = np.nonzero(feats["frame_id"] == a)[0]
        if sel.size == 0:
            continue
        f = feats[sel]
        x, y, nid, ok = fr.project_idepth(geo, f["x"], f["y"], f["idepth_mu"])
        with np.errstate(all="ignore"):
            inside = (rx <= x) & (x < rx + rw) & (ry <= y) & (y < ry + rh)
            good = (f["valid"] != 0) & ok & inside & (nid >= np.float32(0))
            v4 = nid / f["idepth_mu"]
            v4 = v4 * v4
            v4 = v4 * v4
        v4 = np.where(f["idepth_mu"].astype(np.float64) < 1e-6, np.float32(1), v4).astype(np.float32)
        rec = np.zeros(sel.size, feats.dtype)
        rec["id"], rec["frame_id"] = f["id"], cur
        rec["x"], rec["y"], rec["idepth_mu"] = x, y, nid
        rec["idepth_var"] = v4 * f["idepth_var"]
        rec["valid"], rec["num_updates"] = 1, f["num_updates"]
        out[sel[good]] = rec[good]
    return out


def make(n):
    """-> dict(sc, feats, proj, world): the inputs of the form on the caller's arrays."""
    if n not in _CASES:
        sc = scene_for(n)
        feats = pc.features(sc, n, seed=300 + SIZES.index(n))
        feats["idepth_var"] = np.random.default_rng(900 + n).uniform(0.002, 0.02, n).astype(np.float32)
        _CASES[n] = dict(sc=sc, feats=feats, proj=projected_aligned(sc, feats), world=world_poses(sc))
    return _CASES[n]


def resident_sets(n, prune: bool = False):
    """The checker's (feats, feats_in_curr) after set_features(make(n).feats) + project_features(CUR): every record is
    valid.  prune=True: then Flame::prunePoseFrames keeps pose-frames 10, 13, 16 and drops 19 and 22 (see PRUNE) with
    every record counted as feats_ (first_new = the count).  The target, 16, looks a quarter of an image away from frame
    23, so many moves leave its valid region; those records stay, marked invalid, and nothing is removed: the two sets
    stay index-aligned and the resident one has invalid records again."""
    case = make(n)
    sc = case["sc"]
    rc, err, kept, cur = fr.project_features(case["feats"], project_geos(sc), CUR, sc.width, sc.height)
    assert rc == 0, (rc, err)
    if prune:
        keep, dropped, target = PRUNE
        rc, st, kept = pr.prune_pose_frames(kept, keep, pc.dropped_geos(sc, dropped, target), target, sc.width, sc.height,
                                            first_new=kept.shape[0])
        assert rc == 0 and st["num_removed"] == 0 and st["num_invalidated"] > 0, st
    return kept, cur
