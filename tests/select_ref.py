"""CPU checker of the graph-vertex selection (TEST INFRASTRUCTURE): the preprocessing of

    Flame::syncGraph                               flame.cc:1954-1980
    and the data-term lines of its vertex loops    flame.cc:2001-2004, 2041-2044

in numpy float32, operation for operation as include/flame_stereo.h states it:

  pix       = (x / mu, y / mu, 1 / mu)                       three true divisions (Eigen >= 3.3)
  xyz       = Kinv * pix                                     the full product, each row (a + b) + c
  R row 1   = (tx*y + tz*w, 1 - (tx*x + tz*z), ty*z - tx*w)  tx = 2x, ty = 2y, tz = 2z (Eigen's toRotationMatrix)
  world.y   = ((R10*X + R11*Y) + R12*Z) + t[1]
  selected  = valid && var < idepth_var_max_graph && -world.y >= min_height && -world.y <= max_height

numpy's float32 arithmetic is IEEE, correctly rounded and never contracted.  The predicate reads the RESIDENT record,
the outputs the PROJECTED record at the same index (its `valid` and `id` are not read).  The assert on idepth_mu and the
pose look-up run for every record, valid or not.  The order of the selected is ascending record index.

`height64` is the float64 statement of the same height straight from K, R, t; `select_sequential` restates the
reference's set logic (feats_to_update, feat_id_to_idx) one record at a time.

This is our restatement of the reference, not the reference: parity with its binary is unpinned like the rest of the
front-end.  Return codes follow flame_nltgv2_status: 0, INVALID_ARG (-1) or ASSERT (-8).
"""
from __future__ import annotations

import numpy as np

from tests.frontend_ref import ASSERT, INVALID_ARG, OK

F32 = np.float32
DEFAULT_GP = dict(idepth_var_max_graph=1e-2, min_height=0.1, max_height=4.0, adaptive_data_weights=0)
COUNTERS = ("num_examined", "num_invalid", "num_fail_var", "num_fail_height", "error_feature")
ARRAYS = ("feat_id", "pos", "data_term", "data_weight", "feat_index")


def rotation_row1(q):
    """Row 1 of Eigen's Quaternion::toRotationMatrix(), q = (w, x, y, z), in float32."""
    w, x, y, z = (F32(c) for c in q)
    tx, ty, tz = F32(2) * x, F32(2) * y, F32(2) * z
    twx, twz = tx * w, tz * w
    txx, txy = tx * x, tx * y
    tyz, tzz = ty * z, tz * z
    return txy + twz, F32(1) - (txx + tzz), tyz - twx


def heights32(feats, Kinv32, world_poses):
    """-> (h = -world.y as float32 [n], known [n]: the record's frame is listed)."""
    n = feats.shape[0]
    Ki = np.asarray(Kinv32, np.float32).reshape(-1)
    mu = feats["idepth_mu"].astype(np.float32)
    r10 = np.zeros(n, np.float32)
    r11 = np.zeros(n, np.float32)
    r12 = np.zeros(n, np.float32)
    ty = np.zeros(n, np.float32)
    known = np.zeros(n, bool)
    for p in reversed(list(world_poses)):  # (the kernel's linear search takes the FIRST entry of an id)
        sel = feats["frame_id"] == np.uint32(p["id"])
        a, b, c = rotation_row1(p["q"])
        r10[sel], r11[sel], r12[sel], ty[sel] = a, b, c, F32(np.asarray(p["t"], np.float32)[1])
        known |= sel
    with np.errstate(all="ignore"):
        px, py, pz = feats["x"] / mu, feats["y"] / mu, F32(1) / mu
        X = (Ki[0] * px + Ki[1] * py) + Ki[2] * pz
        Y = (Ki[3] * px + Ki[4] * py) + Ki[5] * pz
        Z = (Ki[6] * px + Ki[7] * py) + Ki[8] * pz
        wy = ((r10 * X + r11 * Y) + r12 * Z) + ty
        h = (-wy).astype(np.float32)
    return h, known


def classify(feats, Kinv32, world_poses, gp=None):
    """-> (rc, error_feature, cls [n]): 0 selected, 1 invalid, 2 variance, 3 height (the first failing test)."""
    gp = dict(DEFAULT_GP, **(gp or {}))
    n = feats.shape[0]
    h, known = heights32(feats, Kinv32, world_poses)
    mu = feats["idepth_mu"]
    asserts = ~(mu >= F32(0))  # FLAME_ASSERT(idepth >= 0.0f): NaN fails
    bad = asserts | ~known
    if bad.any():  # the loop stops at the first record that fails either; within a record the assert comes first
        i = int(np.nonzero(bad)[0][0])
        return (ASSERT if asserts[i] else INVALID_ARG), i, None
    with np.errstate(all="ignore"):
        valid = feats["valid"] != 0
        var_ok = feats["idepth_var"] < F32(gp["idepth_var_max_graph"])
        band = (h >= F32(gp["min_height"])) & (h <= F32(gp["max_height"]))
    cls = np.full(n, 3, np.uint8)
    cls[band] = 0
    cls[~var_ok] = 2
    cls[~valid] = 1
    return OK, -1, cls


def select(feats, feats_in_curr, Kinv32, world_poses, graph_scale, gp=None):
    """-> (rc, result dict): V, the five arrays (pos as [V, 2]) and the counters.  On error V = 0, empty arrays."""
    gp = dict(DEFAULT_GP, **(gp or {}))
    n = feats.shape[0]
    assert feats_in_curr.shape[0] == n
    res = dict(V=0, num_examined=n, num_invalid=0, num_fail_var=0, num_fail_height=0, error_feature=-1,
               feat_id=np.zeros(0, np.int32), pos=np.zeros((0, 2), np.float32), data_term=np.zeros(0, np.float32),
               data_weight=np.zeros(0, np.float32), feat_index=np.zeros(0, np.int32))
    rc, err, cls = classify(feats, Kinv32, world_poses, gp)
    if rc != OK:
        res["error_feature"] = err
        return rc, res
    idx = np.nonzero(cls == 0)[0]
    big = feats["id"][idx] >= np.uint32(2 ** 31)
    if big.any():
        res["error_feature"] = int(idx[big][0])
        return INVALID_ARG, res
    c = feats_in_curr[idx]
    with np.errstate(all="ignore"):
        res["data_term"] = (c["idepth_mu"] / F32(graph_scale)).astype(np.float32)
        res["data_weight"] = ((F32(1) / c["idepth_var"]) if gp["adaptive_data_weights"] else
                              np.ones(idx.size, np.float32)).astype(np.float32)
    res["V"] = int(idx.size)
    res["feat_id"] = feats["id"][idx].astype(np.int32)
    res["pos"] = np.stack([c["x"], c["y"]], axis=1).astype(np.float32).reshape(-1, 2)
    res["feat_index"] = idx.astype(np.int32)
    res["num_invalid"] = int((cls == 1).sum())
    res["num_fail_var"] = int((cls == 2).sum())
    res["num_fail_height"] = int((cls == 3).sum())
    return OK, res


def height64(feats, K, R, t):
    """-world.y in float64 straight from K (3x3), R (3x3, camera -> world) and t: world = R K^-1 (x, y, 1) / mu + t,
    for records that all live in this one camera."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    R = np.asarray(R, np.float64).reshape(3, 3)
    t = np.asarray(t, np.float64).reshape(3)
    pix = np.stack([feats["x"].astype(np.float64), feats["y"].astype(np.float64), np.ones(feats.shape[0])], axis=0)
    with np.errstate(all="ignore"):
        xyz = np.linalg.solve(K, pix) / feats["idepth_mu"].astype(np.float64)
        world = R @ xyz + t[:, None]
    return -world[1]


def select_sequential(feats, feats_in_curr, heights, graph_scale, gp=None):
    """The reference's set logic written out (flame.cc:1956-1980, 2031-2044) on precomputed heights: feats_to_update
    as a set of ids, feat_id_to_idx as a dict (a later index of the same id wins), then one vertex per id of the set.
    -> {feat_id: (index, x, y, data_term, data_weight)}."""
    gp = dict(DEFAULT_GP, **(gp or {}))
    feats_to_update = set()
    feat_id_to_idx = {}
    for ii in range(feats.shape[0]):
        feat = feats[ii]
        feat_id_to_idx[int(feat["id"])] = ii
        hh = F32(heights[ii])
        with np.errstate(all="ignore"):
            if (feat["valid"] and F32(feat["idepth_var"]) < F32(gp["idepth_var_max_graph"]) and hh >= F32(gp["min_height"])
                    and hh <= F32(gp["max_height"])):
                feats_to_update.add(int(feat["id"]))
    out = {}
    for feat_id in feats_to_update:
        ii = feat_id_to_idx[feat_id]
        c = feats_in_curr[ii]
        with np.errstate(all="ignore"):
            term = F32(c["idepth_mu"]) / F32(graph_scale)
            weight = F32(1) / F32(c["idepth_var"]) if gp["adaptive_data_weights"] else F32(1)
        out[feat_id] = (ii, F32(c["x"]), F32(c["y"]), F32(term), F32(weight))
    return out
