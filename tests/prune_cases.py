"""Inputs of the prunePoseFrames tests (TEST INFRASTRUCTURE): a PlaneScene with five pose-frames and a feature set
anchored in all of them, built so that the prune has real work on every path -- shared by the CPU tests (which assert
the shares on the checker's output), the GPU tests, the C++ test's dump and tools/prune_bench.py.

Pose-frames 10, 13, 16, 19, 22 (a sideways-and-forward dolly, about an eighth of the image per pose-frame); the prune
keeps the last `5 - n_dropped` of them, so the target is 22 and the dropped pose-frames are the oldest.  Features lie on
random points of the whole image (inside the middle third with do_letterbox), with a prior around the true inverse
depth; a few have the special values the loops branch on.
"""
from __future__ import annotations

import numpy as np

from flame_amd import synth_stereo as ss
from oracle import stereo_capi as so

PF_IDS = (10, 13, 16, 19, 22)
SIZES = {"320x240": (320, 240), "640x480": (640, 480), "1920x1080": (1920, 1080)}


def scene(size: str, seed: int = 5):
    w, h = SIZES[size]
    sc = ss.PlaneScene(w, h, seed=seed, normal=(0.2, -0.1, 1.0), distance=2.2)
    for i, k in enumerate(PF_IDS):
        sc.add_camera(k, ss.rot([0.1, 1, 0.05], 0.006 * i), [-0.13 * i, 0.01 * i, -0.05 * i])
    sc.add_camera(23, ss.rot([0.1, 1, 0.05], 0.026), [-0.55, 0.042, -0.21])  # frames after pose-frame 22
    sc.add_camera(24, ss.rot([0.1, 1, 0.05], 0.028), [-0.58, 0.044, -0.22])
    return sc


def features(sc, n: int, seed: int, anchors=PF_IDS, letterbox: bool = False, special: bool = True):
    """n features, anchors drawn at random (so orphans are spread over all indices)."""
    rng = np.random.default_rng(seed)
    f = np.zeros(n, so.FEATURE_DTYPE)
    f["id"] = np.arange(n)
    f["frame_id"] = np.asarray(anchors, np.uint32)[rng.integers(0, len(anchors), n)]
    lo, hi = (sc.height / 3 + 6, 2 * sc.height / 3 - 6) if letterbox else (0.0, float(sc.height))
    f["x"] = rng.uniform(0, sc.width, n).astype(np.float32)
    f["y"] = rng.uniform(lo, hi, n).astype(np.float32)
    xy = np.stack([f["x"], f["y"]], 1)
    for a in set(int(v) for v in f["frame_id"]):
        sel = f["frame_id"] == a
        f["idepth_mu"][sel] = (sc.true_idepth(a, xy[sel]) * (1.0 + 0.08 * rng.uniform(-1, 1, int(sel.sum())))).astype(np.float32)
    f["idepth_var"] = rng.uniform(0.005, 0.05, n).astype(np.float32)
    f["valid"] = (rng.random(n) >= 0.1).astype(np.uint8)
    f["num_updates"] = rng.integers(0, 9, n)
    f["num_dropouts"] = rng.integers(0, 3, n)
    f["search_status"] = rng.integers(0, 4, n)
    if special and n >= 50:
        pick = rng.choice(n, 5 * (n // 50), replace=False).reshape(5, -1)
        f["idepth_mu"][pick[0]] = 0.0    # maxDepthProjection; the variance factor is 0/0 -> replaced by 1
        f["idepth_mu"][pick[1]] = 5e-7   # old idepth below 1e-6: the test is on the NEW value
        f["idepth_mu"][pick[2]] = 60.0   # 17 mm in front of its pose-frame: behind the target camera
        f["x"][pick[3]] = np.rint(f["x"][pick[3]]) + np.float32(0.5)  # ties
        f["y"][pick[4]] = np.rint(f["y"][pick[4]]) + np.float32(0.5)
    return f


def split(n_dropped: int):
    """(keep ids, dropped ids, target id)."""
    keep = PF_IDS[n_dropped:]
    return list(keep), list(PF_IDS[:n_dropped]), max(keep)


def dropped_poses(sc, dropped, target):
    return [dict(id=a, q_to_new=sc.relative(a, target)[0], t_to_new=sc.relative(a, target)[1]) for a in dropped]


def dropped_geos(sc, dropped, target):
    return {a: so.load_geometry(sc.K32, sc.Kinv32, *sc.relative(a, target)) for a in dropped}


# (name, size, n features, do_letterbox, n_dropped pose-frames, anchors of the features or None = all five)
CASES = (
    ("one", "320x240", 1, 0, 1, (10,)),
    ("wave", "320x240", 64, 0, 2, None),
    ("group-1", "320x240", 255, 0, 2, None),
    ("group", "320x240", 256, 0, 2, None),
    ("group+1", "320x240", 257, 1, 2, None),
    ("small", "320x240", 1500, 0, 2, None),
    ("vga", "640x480", 8400, 0, 2, None),
    ("vga-letterbox", "640x480", 8400, 1, 3, None),
    ("vga-four", "640x480", 16000, 0, 4, None),
    ("hd", "1920x1080", 61000, 0, 2, None),
    ("hd-letterbox", "1920x1080", 61441, 1, 3, None),  # 240 full groups + 1 lane
    ("nothing-to-move", "640x480", 1000, 0, 2, (16, 19, 22)),
    ("everything-to-move", "640x480", 3000, 0, 2, (10, 13)),
)
CASE_NAMES = tuple(c[0] for c in CASES)
_SCENES = {}


def make(name):
    """-> dict(sc, feats, keep, dropped, target, letterbox)."""
    _, size, n, letterbox, n_dropped, anchors = CASES[CASE_NAMES.index(name)]
    if size not in _SCENES:
        _SCENES[size] = scene(size)
    sc = _SCENES[size]
    keep, dropped, target = split(n_dropped)
    feats = features(sc, n, seed=100 + CASE_NAMES.index(name), anchors=anchors or PF_IDS, letterbox=bool(letterbox))
    return dict(sc=sc, feats=feats, keep=keep, dropped=dropped, target=target, letterbox=int(letterbox))


def first_new_values(n):
    return sorted(set([0, n // 3, n]))
