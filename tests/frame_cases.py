"""The shapes of tests/test_frame_planes_edges.py: frames from 2x2, borders up to 64 and wider than the frame, padded widths at
the edges of k_frame_pad_gradient's 256-lane row blocks, and flame_stereo_set_camera's largest dimension.  Every case states
what it is there to reach; `check_reaches` asserts that from the checker's index map (tests/frame_ref.py) alone, so a case that
quietly stopped reaching its edge fails on the CPU."""
import functools

import numpy as np

from tests import frame_ref as fr
from tests import input_ref as ir

NONE, ONE, MANY = "no reflection", "one reflection", "two reflections or more"

# (w, h, border): (reflections the farthest padded pixel needs, padded width minus the nearest multiple of 256 or None, note)
FRAME_CASES = {
    # the smallest frame: border 2 is the first a single reflection leaves outside, border 64 takes dozens
    (2, 2, 0): (NONE, None, ""),
    (2, 2, 1): (ONE, None, ""),
    (2, 2, 2): (MANY, None, ""),
    (2, 2, 64): (MANY, None, "dozens"),
    # border == height; border == width; border > 2 (w - 1): the left side needs a second reflection too
    (3, 2, 5): (MANY, None, ""),
    (2, 3, 5): (MANY, None, ""),
    (5, 4, 4): (MANY, None, "border == height"),
    (5, 4, 5): (MANY, None, "border == width"),
    (4, 7, 9): (MANY, None, "left twice"),
    # the largest border; 65x65 is the smallest frame that it reflects once only
    (33, 32, 64): (MANY, None, ""),
    (64, 64, 64): (MANY, None, "border == width"),
    (65, 65, 64): (ONE, None, "smallest with one"),
    # padded widths 255, 256, 257 and unpadded 256, 257: the edges of the 256-lane row blocks
    (245, 3, 5): (MANY, -1, ""),
    (246, 3, 5): (MANY, 0, ""),
    (247, 3, 5): (MANY, 1, ""),
    (256, 2, 0): (NONE, 0, ""),
    (257, 2, 0): (NONE, 1, ""),
    # the API's largest dimension, either way round
    (16384, 2, 0): (NONE, None, "largest"),
    (16384, 2, 64): (MANY, None, "largest"),
    (2, 16384, 1): (ONE, None, "largest"),
}
MAX_DIM, MAX_BORDER = 16384, 64  # flame_stereo_set_camera's limits
IMAGES = ("random", "ramp")


def case_id(case):
    return "%dx%d_b%d" % case


def reflections_class(n):
    return NONE if n == 0 else ONE if n == 1 else MANY


def single_reflection(p, length):
    """What ONE round of the rule leaves of coordinate p (the arithmetic k_frame_pad_gradient had before it reflected
    repeatedly): inside [0, length) iff one reflection is enough."""
    if p < 0:
        p = -p
    if p >= length:
        p = 2 * (length - 1) - p
    return p


def check_reaches(case):
    """Asserts that the case reaches what FRAME_CASES says of it.  Returns (xs, ys): the checker's source index of every padded
    column and row."""
    w, h, b = case
    want, pw_edge, note = FRAME_CASES[case]
    assert 2 <= w <= MAX_DIM and 2 <= h <= MAX_DIM and 0 <= b <= MAX_BORDER
    (xs, nx), (ys, ny) = fr.index_map(w, b), fr.index_map(h, b)
    assert xs.min() >= 0 and xs.max() < w and ys.min() >= 0 and ys.max() < h
    farthest = int(max(nx.max(), ny.max()))
    assert reflections_class(farthest) == want, (case, farthest)
    # the interior is where no reflection happens; it holds the first and the last column and row, the one-sided gradients
    for src, n, length in ((xs, nx, w), (ys, ny, h)):
        inner = src[n == 0]
        assert inner.tolist() == list(range(length)) and (n[b:b + length] == 0).all()
        assert inner[0] == 0 and inner[-1] == length - 1 and length >= 2
    if pw_edge is not None:
        pw = w + 2 * b
        assert pw - 256 * round(pw / 256) == pw_edge and pw >= 255, (case, pw)
    if note == "dozens":
        assert farthest >= 24
    if note == "border == height":
        assert b == h and ny[-1] >= 2 and nx.max() == 1
    if note == "border == width":
        assert b == w and nx[-1] >= 2
    if note == "left twice":
        assert b > 2 * (w - 1) and nx[0] >= 2
    if note == "smallest with one":
        assert b == MAX_BORDER and w == h and farthest == 1 and max(fr.index_map(w - 1, b)[1]) >= 2
    if note == "largest":
        assert max(w, h) == MAX_DIM
    # one round of the rule is enough exactly where the case says so
    once_ok = all(0 <= single_reflection(q - b, length) < length for length in (w, h) for q in (0, length + 2 * b - 1))
    assert once_ok == (want != MANY), case
    return xs, ys


def random_image(w, h, seed=0, high=256):
    rng = np.random.RandomState(1000 + 31 * w + 17 * h + seed)
    return rng.randint(0, high, size=(h, w)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def frame_expected(case, image):
    """(img, planes) of a case on the seeded random bytes or on the ramp, computed once; callers leave the arrays unchanged."""
    w, h, b = case
    img = random_image(w, h, b) if image == "random" else fr.ramp(w, h)
    planes = fr.make_frame(img, b)
    for a in (img,) + planes:
        a.setflags(write=False)
    return img, planes


# ---- the oracle-versus-checker sweep (CPU) ----
SWEEP_DIMS = (2, 3, 4, 5, 7, 8, 33)
SWEEP_BORDERS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 32, 33, 63, 64)

# ---- strides through the C entry ----
STRIDE_CASES = ((37, 23, 3), (2, 2, 2))
STRIDE_EXTRA = (0, 1, 13)


def strided_image(w, h, extra):
    """(buffer (h, w + extra) uint8, img): the pixels are below 200 and the bytes behind each row's pixels are 255, so a padding
    byte read as a pixel shows."""
    img = random_image(w, h, 7 + extra, high=200)
    buf = np.full((h, w + extra), 255, np.uint8)
    buf[:, :w] = img
    return buf, img


# ---- the rectifier at widths and tails it has never run ----
# output (w, h): pixel counts 4, 6, 6, 9, 15, 14 -> k_input_rectify's store tails 0, 2, 2, 1, 3, 2 behind 1, 1, 1, 2, 3, 3 dwords
RAW_SIZES = ((2, 2), (3, 2), (2, 3), (3, 3), (5, 3), (7, 2))
RAW_TAILS = (0, 2, 2, 1, 3, 2)
RAW_SOURCES = ((2, 2), (4, 3))  # the raw frames of the remapped cases


def raw_borders(w, h):
    """0 and a border of at least the width, so that the stage runs the repeated reflection as well."""
    return (0, w + 1)


def raw_bytes(rw, rh, fmt, pad, seed=0):
    rng = np.random.RandomState(77 + 131 * rw + 7 * rh + ir.BYTES[fmt] + seed)
    return rng.randint(0, 256, size=(rh, rw * ir.BYTES[fmt] + pad)).astype(np.uint8)


def raw_setup(w, h, source=None):
    """(K, Kinv, params) for an output of w x h: remap 0 when `source` is None, else a raw frame of `source` = (rw, rh) seen
    through a camera with a small radial distortion, placed so that some output pixels map inside the raw frame and some
    outside (asserted by `raw_expected`).  The working camera looks at the output's centre with a focal length of its width.
    The inside range of a raw frame is [0, rw - 1) x [0, rh - 1), for a 2x2 one the single cell x0 = y0 = 0.  Without
    distortion the raw camera would spread the output's columns over [0.3, rw - 1.3], all inside and through every x0, and its
    rows over [0.3, rh - 0.75]: the first row inside, the last one outside."""
    K, Kinv = ir.cam(float(w), float(w), 0.5 * (w - 1), 0.5 * (h - 1))
    if source is None:
        return K, Kinv, dict(remap=0, raw_width=w, raw_height=h)
    rw, rh = source
    x0, y0 = -0.5 * (w - 1) / w, -0.5 * (h - 1) / w  # the normalised coordinates of output pixel (0, 0)
    fx, fy = (rw - 1.6) / (-2 * x0), (rh - 1.05) / (-2 * y0)
    Kraw, _ = ir.cam(fx, fy, 0.3 - fx * x0, 0.3 - fy * y0)
    return K, Kinv, dict(remap=1, raw_width=rw, raw_height=rh, K_raw=Kraw, dist=np.float32([-0.05, 0.01, 1e-3, -1e-3]))


@functools.lru_cache(maxsize=None)
def raw_expected(w, h, fmt, pad, source=None):
    """(raw, grey, n_outside, K, Kinv, params) of one rectifier case by tests/input_ref.rectify, computed once.  A remapped case
    has both inside and outside pixels."""
    K, Kinv, p = raw_setup(w, h, source)
    raw = raw_bytes(p["raw_width"], p["raw_height"], fmt, pad)
    grey, n_outside = ir.rectify(raw, fmt, p, K, Kinv, w, h)
    assert grey.shape == (h, w) and grey.dtype == np.uint8
    if source is not None:
        _, _, inside = ir.source_map(p["K_raw"], p["dist"], Kinv, w, h, *source)
        assert 0 < n_outside < w * h and n_outside == int((~inside).sum()), (w, h, source, n_outside)
        assert inside.any() and (~inside).any()
    else:
        assert n_outside == 0
    raw.setflags(write=False), grey.setflags(write=False)
    return raw, grey, n_outside, K, Kinv, p
