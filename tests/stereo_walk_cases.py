"""Inputs that drive the epipolar walk (line_stereo::match) through the places where a 16-lane form of it can disagree
with the sequential loop: exact cost ties, best steps at either end of a walk and at round joins, walks of one to seven
rounds, neighbouring features whose walks differ by rounds, segments clipped by the image box.

Plain numpy, shared by the CPU and the GPU tests of tests/test_stereo_walk_edges.py.  PlaneScene gives the geometry only
(a fronto-parallel plane, identity rotations); all three frames show the SAME integer-valued pattern image, so equal
costs are equal bits and a period of the pattern is a period of the cost.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import stereo_capi as so

W, H = 160, 120
DISTANCE = 2.0          # plane Z = 2 in the first camera: true inverse depth 0.5 for anchor 10
BASELINE_PX = 26.0      # focal length x baseline: a prior of sigma 0.49 then spans more than epilength_max = 48 px
SAMPLE_DISTS = (0.5, 1.0, 1.5)
VAR_LO, VAR_HI = 1e-6, 0.24

# ---- images ------------------------------------------------------------------------------------------------


def _stripes(w, h, period, direction):
    ys, xs = np.mgrid[0:h, 0:w]
    c = {"v": xs, "h": ys, "d": xs + ys}[direction]
    return np.where((c % period) < period // 2, 40, 200).astype(np.uint8)


def _sawtooth(w, h, period, direction):
    ys, xs = np.mgrid[0:h, 0:w]
    c = {"v": xs, "h": ys, "d": xs + ys}[direction]
    return (20 + (c % period) * (200 // period)).astype(np.uint8)


def _checker(w, h, cell):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.where(((xs // cell) + (ys // cell)) % 2 == 0, 60, 190).astype(np.uint8)


def _step_edge(w, h):
    img = np.full((h, w), 70, np.uint8)
    img[:, w // 2:] = 180
    img[h // 2:, :] += 30   # and a weaker horizontal edge, so that walks along y see a gradient too
    return img


def _saturated_blocks(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.where(((xs // 12) + 2 * (ys // 10)) % 3 == 0, 0, np.where(((xs // 12) + (ys // 10)) % 2 == 0, 255, 128)).astype(np.uint8)


def _constant(w, h):
    return np.full((h, w), 117, np.uint8)


def _dots(w, h):
    img = np.full((h, w), 30, np.uint8)
    img[3::8, 2::8] = 250
    return img


PATTERNS = {}
for _d in "vhd":
    for _p in (4, 6, 8, 16):
        PATTERNS["stripes_%s%d" % (_d, _p)] = functools.partial(_stripes, period=_p, direction=_d)
    PATTERNS["saw_%s12" % _d] = functools.partial(_sawtooth, period=12, direction=_d)
PATTERNS["checker8"] = functools.partial(_checker, cell=8)
PATTERNS["step_edge"] = _step_edge
PATTERNS["saturated"] = _saturated_blocks
PATTERNS["constant"] = _constant
PATTERNS["dots"] = _dots

# ---- motions: direction of the new camera's translation; t.z == 0 except for the last two ---------------------------------
_S = 0.5 ** 0.5
MOTIONS = {
    "+x": (1.0, 0.0, 0.0), "-x": (-1.0, 0.0, 0.0), "+y": (0.0, 1.0, 0.0), "-y": (0.0, -1.0, 0.0),
    "+x+y": (_S, _S, 0.0), "+x-y": (_S, -_S, 0.0), "-x+y": (-_S, _S, 0.0), "-x-y": (-_S, -_S, 0.0),
    # epipole inside the image (K t / t.z is within a few pixels of the centre); rescale factors 0.8 and 1.29
    "forward": (0.02, 0.01, 0.5), "backward": (-0.015, 0.02, -0.45),
}


def ladder(n, lo=VAR_LO, hi=VAR_HI):
    """Geometric ladder of n variances, dealt out so that the four features of a group (one wave of the 16-lane form)
    sit a quarter of the ladder apart: a factor 22 in variance, 4.7 in the length of the search segment."""
    rungs = lo * (hi / lo) ** (np.arange(n) / max(n - 1, 1))
    q = max(n // 4, 1)
    i = np.arange(n)
    stride = max(int(0.382 * q), 1)             # walk each quarter in long strides: any short prefix of the features
    while np.gcd(stride, q) != 1:               # already spans the ladder
        stride += 1
    idx = (i % 4) * q + ((i // 4) * stride) % q
    return rungs[np.minimum(idx, n - 1)].astype(np.float32)


def make_case(pattern="stripes_v8", motion="+x", w=W, h=H, pad=5, nx=20, ny=15, border=6, seed=0, mu_spread=0.3, **pkw):
    """-> dict(sc, imgs, feats, poses, pkw, pad).  Features on an nx x ny grid in each of the anchors 10 and 11 (11 sits
    half way to the new camera 12, so its features see half the baseline)."""
    from flame_amd import synth_stereo as ss

    sc = ss.PlaneScene(w, h, seed=1, normal=(0.0, 0.0, 1.0), distance=DISTANCE, margin=4)   # its texture is not used
    t = np.asarray(MOTIONS[motion], np.float64)
    if t[2] == 0.0:
        t = t * (BASELINE_PX / float(sc.K[0, 0]))
    sc.add_camera(10, np.eye(3), [0, 0, 0])
    sc.add_camera(11, np.eye(3), 0.5 * t)
    sc.add_camera(12, np.eye(3), t)
    img = PATTERNS[pattern](w, h)
    imgs = {10: img, 11: img, 12: img}
    rng = np.random.default_rng(1234 + seed)
    n1 = nx * ny
    feats = np.zeros(2 * n1, so.FEATURE_DTYPE)
    gx = border + (np.arange(nx) + 0.5) * ((w - 2 * border) / nx)
    gy = border + (np.arange(ny) + 0.5) * ((h - 2 * border) / ny)
    x = np.tile(gx, ny) + rng.uniform(-1.5, 1.5, n1)
    y = np.repeat(gy, nx) + rng.uniform(-1.5, 1.5, n1)
    # a third on whole pixels, a third on quarter pixels, the rest anywhere: positions with few mantissa bits keep the
    # cost of a periodic image exactly periodic
    k = np.arange(n1) % 3
    x = np.where(k == 0, np.rint(x), np.where(k == 1, np.rint(4 * x) / 4, x))
    y = np.where(k == 0, np.rint(y), np.where(k == 1, np.rint(4 * y) / 4, y))
    var = ladder(2 * n1)
    for a_i, anchor in enumerate((10, 11)):
        s = slice(a_i * n1, (a_i + 1) * n1)
        xy = np.stack([x, y], 1).astype(np.float32)
        truth = sc.true_idepth(anchor, xy)
        e = rng.uniform(-1.0, 1.0, n1)
        e[::5] = 0.0                                   # every fifth prior is the truth
        feats["frame_id"][s] = anchor
        feats["x"][s], feats["y"][s] = xy[:, 0], xy[:, 1]
        feats["idepth_mu"][s] = (truth * (1.0 + mu_spread * e)).astype(np.float32)
    feats["id"] = np.arange(2 * n1)
    feats["idepth_var"] = var
    feats["valid"] = 1
    pkw = dict(pkw)
    if pattern == "constant":
        pkw.setdefault("min_grad_mag", 0.0)            # reach the walk, then the gnorm < 1e-3 exit of the measurement model
    return dict(sc=sc, imgs=imgs, feats=feats, poses=ss.poses_for(sc, [10, 11], 12, 11), pkw=pkw, pad=pad, name="%s %s %r" % (pattern, motion, pkw))


def run_checker(case, feats=None, trace=True):
    """The sequential checker on a case: (rc, stats[7], records, trace [n, 8] or None)."""
    sc, pad = case["sc"], case["pad"]
    frames = [dict(p, img_pad=so.make_frame(case["imgs"][p["id"]], pad)[0]) for p in case["poses"]]
    out = (case["feats"] if feats is None else feats).copy()
    tr = np.zeros((out.shape[0], len(so.TRACE_COLS)), np.int32) if trace else None
    rc, stats = so.update_feature_idepths(so.Params(**case["pkw"]), sc.K32, sc.Kinv32, sc.width, sc.height, pad, frames,
                                          so.make_frame(case["imgs"][12], pad), 11, out, trace=tr)
    return rc, stats, out, tr


def walk_params(sample_dist):
    return dict(sample_dist=sample_dist, epilength_max=48.0)


def grid_cases(sample_dist):
    """Every pattern x every motion at one sample distance (160 x 120, 600 features each)."""
    for pattern in PATTERNS:
        for motion in MOTIONS:
            yield make_case(pattern, motion, **walk_params(sample_dist))


def tied_case():
    """The case the feature-count sweep takes its first n features from: period-8 stripes, motion along x, half-pixel
    steps; 4800 features, so that one lane per feature fills more than kStatSlots = 64 blocks of 64."""
    return make_case("stripes_v8", "+x", nx=60, ny=40, **walk_params(0.5))


def short_walk_case():
    """epilength_min below one step: walks of one and two steps."""
    return make_case("saw_v12", "-x", sample_dist=1.5, epilength_min=1.0, epilength_max=48.0)


def search_segments(case):
    """stereo_search_region per feature: (rc [n], segment [n, 4] = start.x, start.y, end.x, end.y in image coordinates)."""
    sc, feats = case["sc"], case["feats"]
    P = so.Params(**case["pkw"])
    geos = {p["id"]: so.load_geometry(sc.K32, sc.Kinv32, p["q_to_new"], p["t_to_new"]) for p in case["poses"]}
    rc = np.zeros(feats.shape[0], np.int32)
    seg = np.zeros((feats.shape[0], 4), np.float32)
    for i, f in enumerate(feats):
        r = so.search_region(P, geos[int(f["frame_id"])], sc.width, sc.height, f["x"], f["y"], f["idepth_mu"], f["idepth_var"])
        rc[i], seg[i] = r[0], r[1:5]
    return rc, seg
