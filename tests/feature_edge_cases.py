"""Inputs of tests/test_feature_stage_edges.py (TEST INFRASTRUCTURE): the four stages of flame_amd/csrc/feature_kernels.hip
(projectFeatures, detectFeatures, prunePoseFrames, the graph-vertex selection) past 256 workgroups of 256 and at the
shape, region, mask and map edges of projection and detection.  Every expected result comes from the bit-exact CPU
checkers (tests/frontend_ref.py, tests/prune_ref.py, tests/select_ref.py); inputs and results are built once per process
and shared read-only by the CPU part (which asserts that a case reaches the path it names) and the GPU part.

A: the 1920x1080 scene and the features of tests/prune_cases.py at 65 536, 65 537, 70 001 and 131 073 records (256 full
   workgroups -- the last count at which group_base's loop takes one turn --, 256 + one lane, 274 and 513), and detection
   on seeded random bytes with one cell per pixel (320x240, window 1) or per 2x2 pixels (640x480, window 2): 76 800 cells,
   300 workgroups.
B: projection with 1..513 records and five keep patterns; a camera whose K and Kinv are exact in float, so that an
   identity pose at idepth_mu 0 returns the input point bit for bit and the half-open float rectangle can be probed one
   ulp at a time; the inverse depths the stage branches on; a pose table of 32 entries.
C: detection with windows 1..100 on 61x37, images whose candidate range is empty, mask points on cell boundaries, an
   inverse-depth map with every special value but NaN at winning pixels, thresholds met with equality, ids that wrap.
"""
from __future__ import annotations

import functools

import numpy as np

from flame_amd import synth_stereo as ss
from oracle import stereo_capi as so
from tests import frontend_ref as fr
from tests import prune_cases as pc
from tests import prune_ref as pr
from tests import select_cases as sc_
from tests import select_ref as sr

F32 = np.float32
PAD = 5       # the padding of the resident frames
GROUP = 256   # items per workgroup of the counting and scattering kernels
BORDER = fr.border_of(1.4, 5)  # 4: the default parameters' border of the valid region and of the candidate range


def frozen(a):
    a.setflags(write=False)
    return a


def ulp_down(v):
    return np.nextafter(F32(v), F32(-np.inf))


def ulp_up(v):
    return np.nextafter(F32(v), F32(np.inf))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- A: past 256 workgroups ----------------------------------------------------------------------------------------------

BIG_COUNTS = (65536, 65537, 70001, 131073)
FIRST_PAST = 256 * GROUP  # the first record index or cell of workgroup 256
FLOOR = 1000              # records at or past workgroup 256 that a case's compacted output must hold
# a rule that selects about half of the records (the default one selects 4 %: too few behind workgroup 256 at 70 001)
SELECT_GP = dict(idepth_var_max_graph=0.03, min_height=-100.0, max_height=100.0, adaptive_data_weights=1)
SELECT_SCALE = 0.37


def floor_applies(n):
    """65 536 records fill workgroups 0..255 and nothing else; of 65 537 a single lane lies in workgroup 256."""
    return n >= FIRST_PAST + FLOOR


def hd_scene():
    return sc_.scene_for(61000)  # prune_cases.scene("1920x1080"), built once for all modules


@functools.lru_cache(maxsize=None)
def big_features(n, letterbox=0):
    return frozen(pc.features(hd_scene(), n, seed=700 + BIG_COUNTS.index(n), letterbox=bool(letterbox)))


@functools.lru_cache(maxsize=None)
def big_project(n, letterbox):
    """-> (rc, error index, kept, projected) of the projection into frame 23."""
    sc = hd_scene()
    return fr.project_features(big_features(n, letterbox), sc_.project_geos(sc), sc_.CUR, sc.width, sc.height,
                               do_letterbox=bool(letterbox))


def big_first_new(n):
    return (n, n // 3)  # nothing removed: committed in place; records removed: compacted into the other buffer


@functools.lru_cache(maxsize=None)
def big_prune(n, first_new):
    sc = hd_scene()
    keep, dropped, target = pc.split(2)
    return pr.prune_pose_frames(big_features(n), keep, pc.dropped_geos(sc, dropped, target), target, sc.width, sc.height,
                                first_new=first_new)


@functools.lru_cache(maxsize=None)
def big_survivors(n):
    """n records of prune_cases.features that all survive the projection into frame 23, ids 0..n-1: the resident form of
    the selection runs right after project_features, which must not shrink the set below 257 workgroups."""
    sc = hd_scene()
    pool = pc.features(sc, n + n // 2 + 1000, seed=800 + BIG_COUNTS.index(n))
    rc, _, kept, _ = fr.project_features(pool, sc_.project_geos(sc), sc_.CUR, sc.width, sc.height)
    assert rc == 0 and kept.shape[0] >= n, (rc, kept.shape)
    out = kept[:n].copy()
    out["id"] = np.arange(n)
    return frozen(out)


@functools.lru_cache(maxsize=None)
def big_select_inputs(n, form):
    """-> (feats, feats_in_curr): the caller's arrays (prune_cases.features and their index-aligned projection, zeroed
    where it fails), or what the resident and the projected set hold after set_features(big_survivors) + project."""
    sc = hd_scene()
    if form == "arrays":
        return big_features(n), frozen(sc_.projected_aligned(sc, big_features(n)))
    rc, _, kept, cur = fr.project_features(big_survivors(n), sc_.project_geos(sc), sc_.CUR, sc.width, sc.height)
    assert rc == 0
    return frozen(kept), frozen(cur)


@functools.lru_cache(maxsize=None)
def big_select(n, form):
    sc = hd_scene()
    feats, cur = big_select_inputs(n, form)
    return sr.select(feats, cur, sc.Kinv32, sc_.world_poses(sc), SELECT_SCALE, SELECT_GP)


# detection: (width, height, detection_win_size), both 76 800 cells
BIG_DETECT = ((320, 240, 1), (640, 480, 2))
DETECT_Q = ss.quat_from_rot(ss.rot([0, 1, 0], -0.004)).astype(np.float32)  # a sideways step with a little forward motion
DETECT_T = np.float32([0.03, -0.002, 0.01])
PREFIX_COUNT = 70001


@functools.lru_cache(maxsize=None)
def random_image(w, h, seed=21):
    rng = np.random.RandomState(seed + 131 * w + 7 * h)
    return frozen(rng.randint(0, 256, size=(h, w)).astype(np.uint8))


def detect_ref(img, K, Kinv, q=DETECT_Q, t=DETECT_T, ref_id=7, **kw):
    """tests/frontend_ref.detect_features on an image: (rc, error pixel, new records, number of cells)."""
    h, w = img.shape
    _, gx, gy = so.make_frame(np.ascontiguousarray(img), PAD)
    return fr.detect_features(gx, gy, PAD, w, h, so.load_geometry(K, Kinv, q, t), ref_id, dtype=so.FEATURE_DTYPE, **kw)


@functools.lru_cache(maxsize=None)
def big_detect(w, h, win, first_id):
    K, Kinv = ss.intrinsics(w, h)
    return detect_ref(random_image(w, h), K, Kinv, win=win, first_id=first_id)


def cells_of(out, win, w):
    """The row-major cell index of each detected record."""
    wc = fr.fast_ceil(F32(w) / F32(win))
    return (out["y"].astype(np.int64) // win) * wc + out["x"].astype(np.int64) // win


# ---- B: projection at its shape and region edges ---------------------------------------------------------------------------

PROJECT_COUNTS = (1, 63, 64, 65, 255, 256, 257, 512, 513)
PATTERNS = ("all", "none", "first", "last", "half")
W, H = 320, 240
# a camera whose K and Kinv are exact in float: with the identity pose KRKinv is the identity matrix
K_EXACT = np.float32([256, 0, 160, 0, 256, 120, 0, 0, 1])
KINV_EXACT = np.float32([1 / 256, 0, -160 / 256, 0, 1 / 256, -120 / 256, 0, 0, 1])
IDENT_Q, IDENT_T = np.float32([1, 0, 0, 0]), np.float32([0, 0, 0])


def pose(frame_id, q, t):
    return dict(id=frame_id, q_to_new=np.float32(q), t_to_new=np.float32(t))


def geos_of(poses, K=K_EXACT, Kinv=KINV_EXACT):
    return {p["id"]: so.load_geometry(K, Kinv, p["q_to_new"], p["t_to_new"]) for p in poses}


def plain_features(n, seed, frames, w=W, h=H, margin=40):
    """n valid records well inside the image, at depths of 1.5 to 4 m."""
    rng = np.random.default_rng(seed)
    f = np.zeros(n, so.FEATURE_DTYPE)
    f["id"] = np.arange(n)
    f["frame_id"] = np.asarray(frames, np.uint32)[rng.integers(0, len(frames), n)]
    f["x"] = rng.uniform(margin, w - margin, n).astype(np.float32)
    f["y"] = rng.uniform(margin, h - margin, n).astype(np.float32)
    f["idepth_mu"] = rng.uniform(0.25, 0.65, n).astype(np.float32)
    f["idepth_var"] = rng.uniform(0.005, 0.05, n).astype(np.float32)
    f["valid"] = 1
    f["num_updates"] = rng.integers(0, 9, n)
    f["num_dropouts"] = rng.integers(0, 3, n)
    f["search_status"] = rng.integers(0, 4, n)
    return f


SHAPE_POSES = (pose(10, ss.quat_from_rot(ss.rot([0.1, 1, 0.05], 0.004)), [-0.025, 0.003, -0.01]),
               pose(11, ss.quat_from_rot(ss.rot([0.1, 1, 0.05], 0.007)), [-0.045, 0.004, -0.016]))


@functools.lru_cache(maxsize=None)
def shape_case(n, pattern):
    """-> (feats, checker result): n records that all project inside when valid, with `valid` set by the pattern."""
    f = plain_features(n, 40 + n, (10, 11))
    keep = np.ones(n, bool)
    if pattern == "none":
        keep[:] = False
    elif pattern == "first":
        keep[1:] = False
    elif pattern == "last":
        keep[:-1] = False
    elif pattern == "half":
        keep = np.random.default_rng(90 + n).random(n) < 0.5
    f["valid"] = keep
    return frozen(f), fr.project_features(f, geos_of(SHAPE_POSES), 14, W, H)


def region(letterbox):
    """(x, y, w, h) of projectFeatures' float rectangle for the exact camera."""
    off = H // 3 if letterbox else 0
    return F32(BORDER), F32(BORDER + off), F32(W - 2 * BORDER), F32(H - 2 * BORDER - 2 * off)


RECT_POSES = (pose(10, IDENT_Q, IDENT_T),)


@functools.lru_cache(maxsize=None)
def rect_case(letterbox):
    """-> (feats, inside [n] bool: the known answer of the half-open rule, finite [n] bool).  Records of pose-frame 10
    (identity pose) with idepth_mu 0: the projected point is the record's own."""
    rx, ry, rw, rh = region(letterbox)
    hx, hy = F32(rx + rw), F32(ry + rh)
    mx, my = F32(rx + 8), F32(ry + 8)  # a point well inside
    pts = [(mx, my, True)]
    for lo, hi, other, axis in ((rx, hx, my, 0), (ry, hy, mx, 1)):
        for v, inside in ((lo, True), (ulp_down(lo), False), (ulp_up(lo), True), (hi, False), (ulp_down(hi), True),
                          (ulp_up(hi), False), (F32(np.nan), False), (F32(np.inf), False), (F32(-np.inf), False)):
            pts.append((v, other, inside) if axis == 0 else (other, v, inside))
    pts += [(rx, ry, True), (ulp_down(hx), ulp_down(hy), True), (hx, ry, False), (rx, hy, False), (ulp_down(rx), ry, False),
            (hx, hy, False), (F32(np.nan), F32(np.nan), False)]
    n = len(pts)
    f = np.zeros(n, so.FEATURE_DTYPE)
    f["id"] = 500 + np.arange(n)
    f["frame_id"] = 10
    f["x"] = [p[0] for p in pts]
    f["y"] = [p[1] for p in pts]
    f["idepth_mu"] = 0.0
    f["idepth_var"] = 0.02
    f["valid"] = 1
    f["num_updates"] = 1 + np.arange(n) % 7
    inside = np.array([p[2] for p in pts])
    return frozen(f), inside, np.isfinite(f["x"]) & np.isfinite(f["y"])


E6 = F32(1e-6)  # the float nearest 1e-6: 9.99999997e-7, below 1e-6 as a double; its upper neighbour is above
SUBNORMAL = F32(2.0 ** -127)
# pose-frame 10: the identity; 11: 131 072 m forward and an eighth of a metre sideways, so that an inverse depth around
# 1e-6 changes visibly and +inf (the camera centre itself) lands in front of the target
SPECIAL_POSES = (pose(10, IDENT_Q, IDENT_T), pose(11, IDENT_Q, [0.125, 0, 131072.0]))
SPECIAL_MU = dict(neg_zero=F32(-0.0), e6=E6, e6_lo=ulp_down(E6), e6_hi=ulp_up(E6), subnormal=SUBNORMAL, inf=F32(np.inf))


@functools.lru_cache(maxsize=None)
def special_case():
    """-> (feats, {name: index}): valid records with the special inverse depths and variances between plain ones."""
    f = plain_features(500, 77, (10, 11))
    at = {}
    k = 3
    for frame in (10, 11):
        for name, mu in SPECIAL_MU.items():
            if name == "inf" and frame == 10:
                continue  # the camera centre lies ON the target's camera plane under the identity: see plane_case
            f["frame_id"][k], f["idepth_mu"][k], f["x"][k], f["y"][k] = frame, mu, 100.25, 77.75
            at["%s@%d" % (name, frame)] = k
            k += 37  # spread over waves and both workgroups
    for name, var, mu in (("var_inf", np.inf, 0.5), ("var_nan", np.nan, 0.5), ("var_inf_mu0", np.inf, 0.0),
                          ("var_nan_mu0", np.nan, 0.0)):
        f["frame_id"][k], f["idepth_mu"][k], f["idepth_var"][k] = 10, mu, var
        at[name] = k
        k -= 5
    return frozen(f), at


PLANE_POSES = (pose(10, IDENT_Q, IDENT_T), pose(12, IDENT_Q, [0, 0, -2.0]))
PLANE_AT = (10, 70, 300)  # the first of them invalid: never projected


@functools.lru_cache(maxsize=None)
def plane_case():
    """Records of pose-frame 12 at depth 2 exactly: the target camera stands 2 m further on, the third coordinate of the
    point in it is 2 - 2 = 0 and EpipolarGeometry::project asserts."""
    f = plain_features(400, 78, (10,))
    for i in PLANE_AT:
        f["frame_id"][i], f["idepth_mu"][i] = 12, 0.5
    f["valid"][PLANE_AT[0]] = 0
    return frozen(f)


TABLE_IDS = tuple(range(100, 132))
TABLE_USED = (100, 116, 131)  # the first, a middle and the last entry
TABLE_POSES = tuple(pose(k, ss.quat_from_rot(ss.rot([0.1, 1, 0.05], 0.0004 * (k - 99))),
                         [-0.003 * (k - 99), 0.0003 * (k - 99), -0.001 * (k - 99)]) for k in TABLE_IDS)


@functools.lru_cache(maxsize=None)
def table_case():
    f = plain_features(700, 79, TABLE_USED, margin=2)
    f["valid"][::11] = 0
    K, Kinv = ss.intrinsics(W, H)
    return frozen(f), fr.project_features(f, geos_of(TABLE_POSES, K, Kinv), 200, W, H)


# ---- C: detection at its shape, mask and map edges -------------------------------------------------------------------------

SMALL = (61, 37)
# (width, height, window, do_letterbox, what)
DETECT_SHAPES = (
    (61, 37, 1, 0, "one pixel per cell"),
    (61, 37, 3, 0, ""),
    (61, 37, 7, 0, ""),
    (61, 37, 16, 0, "a pixel row of the cell per 16-lane row"),
    (61, 37, 64, 0, "one cell, walked in 64 turns"),
    (61, 37, 100, 0, "a window larger than the image"),
    (16, 16, 16, 0, "the image is one cell"),
    (9, 9, 3, 0, "one candidate pixel"),
    (8, 8, 4, 0, "no candidate column or row"),
    (61, 24, 7, 1, "r_hi == r_lo"),
    (61, 17, 7, 1, "r_hi < r_lo"),
    (61, 12, 3, 1, "r_hi < r_lo"),
)
EMPTY_RANGE = tuple(s for s in DETECT_SHAPES if s[:2] == (8, 8) or s[3])


def candidate_range(w, h, letterbox):
    off = h // 3 if letterbox else 0
    return BORDER + off, h - BORDER - off, BORDER, w - BORDER


@functools.lru_cache(maxsize=None)
def shape_detect(w, h, win, letterbox):
    K, Kinv = ss.intrinsics(w, h)
    return detect_ref(random_image(w, h), K, Kinv, win=win, do_letterbox=bool(letterbox), first_id=11)


MASK_WINS = (3, 7, 16)
# the exact camera of the small image: the mask points go through project_features unchanged
K_SMALL = np.float32([64, 0, 32, 0, 64, 16, 0, 0, 1])
KINV_SMALL = np.float32([1 / 64, 0, -32 / 64, 0, 1 / 64, -16 / 64, 0, 0, 1])
MASK_T = np.float32([0.125, 0, 0])  # a pure sideways step


def mask_points(win):
    """-> list of (x, y, kind).  "boundary": exactly on a cell boundary in x, in y, and in both; "below": one ulp below
    one; "partial": the last pixel of the partial last cell; "zero": -0.0; "corner": (width - ulp, height - ulp)."""
    w, h = SMALL
    kx, ky = (w // win) // 2, (h // win) // 2  # a cell in the middle of the image
    bx, by = F32(kx * win), F32(ky * win)
    pts = [(bx, F32(by + 1.5), "boundary"), (F32(bx + win + 1.25), by, "boundary"), (F32(bx + 2 * win), F32(by + win), "boundary"),
           (ulp_down(bx), F32(by + 0.5), "below"), (F32(bx + 0.5), ulp_down(by + win), "below")]
    if w % win:
        pts.append((F32(w - 1), F32(by + 2), "partial"))
    if h % win:
        pts.append((F32(bx + 0.75), F32(h - 1), "partial"))
    pts += [(F32(-0.0), F32(-0.0), "zero"), (F32(-0.0), F32(by - win + 0.25), "zero"), (ulp_down(w), ulp_down(h), "corner")]
    return pts


def cell_named(x, y, win, w=SMALL[0]):
    """The cell (uint32)(y / (float)win) * wc + (uint32)(x / (float)win) of a mask point."""
    wc = fr.fast_ceil(F32(w) / F32(win))
    return int(np.uint32(F32(y) / F32(win))) * wc + int(np.uint32(F32(x) / F32(win)))


@functools.lru_cache(maxsize=None)
def mask_detect(win, which):
    """which: None (no mask), "all" (every point), "projected" (the points project_features keeps), or a point's index."""
    pts = np.float32([p[:2] for p in mask_points(win)])
    if which is None:
        m = None
    elif which == "all":
        m = pts
    elif which == "projected":
        m = mask_projected(win)[1]
        m = np.stack([m["x"], m["y"]], 1)
    else:
        m = pts[which:which + 1]
    return detect_ref(random_image(*SMALL), K_SMALL, KINV_SMALL, IDENT_Q, MASK_T, win=win, mask_xy=m, first_id=5)


@functools.lru_cache(maxsize=None)
def mask_projected(win):
    """-> (records carrying the mask points, what the checker's projection keeps of them (the projected set))."""
    pts = mask_points(win)
    f = np.zeros(len(pts), so.FEATURE_DTYPE)
    f["id"] = 900 + np.arange(len(pts))
    f["frame_id"] = 10
    f["x"], f["y"] = [p[0] for p in pts], [p[1] for p in pts]
    f["idepth_var"] = 0.02
    f["valid"] = 1
    rc, _, kept, cur = fr.project_features(f, geos_of(RECT_POSES, K_SMALL, KINV_SMALL), 12, *SMALL)
    assert rc == 0
    return frozen(f), frozen(cur)


MAP_SPECIALS = (F32(0.0), F32(-0.0), F32(-0.75), F32(np.inf), F32(-np.inf), F32(2.0 ** -130), F32(np.nan))


@functools.lru_cache(maxsize=None)
def map_case(win=7):
    """-> (map, winners (row, col) [n, 2], checker result with the map): the specials cycle over the winning pixels."""
    w, h = SMALL
    K, Kinv = ss.intrinsics(w, h)
    rc, _, base, _ = detect_ref(random_image(w, h), K, Kinv, win=win)
    assert rc == 0
    rng = np.random.default_rng(31)
    m = rng.uniform(0.05, 1.5, (h, w)).astype(np.float32)
    rows, cols = base["y"].astype(np.int64), base["x"].astype(np.int64)
    m[rows, cols] = np.array(MAP_SPECIALS, np.float32)[np.arange(rows.size) % len(MAP_SPECIALS)]
    return frozen(m), np.stack([rows, cols], 1), detect_ref(random_image(w, h), K, Kinv, win=win, idepthmap=m)


def ramp_image():
    """I = 2 x: the central difference is gx = 2 exactly away from the two edge columns, gy = 0."""
    w, h = SMALL
    return np.ascontiguousarray(np.tile((2 * np.arange(w)).astype(np.uint8), (h, 1)))


def ramp_detect(min_grad_mag, win=16):
    """With K_SMALL and the step MASK_T the reference epiline is (-+1, 0) exactly: |gradient|^2 = score = 4."""
    return detect_ref(ramp_image(), K_SMALL, KINV_SMALL, IDENT_Q, MASK_T, win=win, min_grad_mag=min_grad_mag)


WRAP_IDS = (2 ** 31 - 2, 2 ** 32 - 2)


@functools.lru_cache(maxsize=None)
def wrap_detect(first_id):
    K, Kinv = ss.intrinsics(*SMALL)
    return detect_ref(random_image(*SMALL), K, Kinv, win=16, first_id=first_id)
