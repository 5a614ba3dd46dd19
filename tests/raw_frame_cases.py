"""The cases of the raw-frame input stage that tests/test_raw_frame.py (CPU) and tests/test_gpu_raw_frame.py (GPU) share:
the working camera, the raw camera, the distortion, and a seeded random raw frame.  Random bytes make every tap and every
weight matter.  Every case but the last two has a 61x37 output: 2257 pixels, an odd tail for any wide store."""
import functools

import numpy as np

from tests import input_ref as ir

SMALL = (61, 37)
CAM_A = (48, 47, 30.2, 18.1)
CAM_B = (64, 64, 30, 18)

# name: (output (w, h), working camera, raw (w, h), raw camera, dist, expected inside count or None = all)
CASES = {
    "pincushion": (SMALL, CAM_A, (61, 37), CAM_A, (0.3, 0.05, 2e-3, -1e-3), 1824),
    "barrel_resize": (SMALL, CAM_A, (97, 53), (70, 69, 47.7, 26.4), (-0.28, 0.07, 2e-4, -1e-4), None),
    "denominator_zero": (SMALL, CAM_B, (67, 41), (64, 64, 33, 20), (0, 0, 0, 0, 0, -16.0), 1425),
    "overflow": (SMALL, CAM_B, (67, 41), (50, 49, 33.5, 20.25), (3e38,), 1),
    "rational": ((160, 96), (120, 118, 79.5, 47.5), (160, 96), (120, 118, 79.5, 47.5),
                 (0.4, -0.1, 1e-3, 5e-4, 0.02, 0.2, -0.05, 0.01), 13453),
    "default_size": ((640, 480), (525, 525, 319.5, 239.5), (752, 480), (458.654, 457.296, 367.215, 248.375),
                     (-0.2834, 0.0740, 1.9e-4, 1.8e-5), None),
}
EXACT_SHIFT = ((61, 37), (64, 32, 30.5, 18), (67, 41), (64, 32, 33.5, 20), ())


def raw_bytes(raw_w, raw_h, fmt, pad=0, seed=11):
    """(raw_h, raw_w * bytes + pad) seeded random bytes: the pixels and, behind them, `pad` bytes the stage must not read
    as pixels."""
    rng = np.random.RandomState(seed + 131 * raw_w + 7 * raw_h + ir.BYTES[fmt])
    return rng.randint(0, 256, size=(raw_h, raw_w * ir.BYTES[fmt] + pad)).astype(np.uint8)


def setup(case):
    """(w, h, K, Kinv, params dict) of a case given by name or as a tuple of CASES' form without the count."""
    (w, h), c, (rw, rh), craw, dist = (CASES[case][:5] if isinstance(case, str) else case)
    K, Kinv = ir.cam(*c)
    Kraw, _ = ir.cam(*craw)
    d = np.zeros(8, np.float32)
    d[:len(dist)] = dist
    return w, h, K, Kinv, dict(remap=1, raw_width=rw, raw_height=rh, K_raw=Kraw, dist=d)


@functools.lru_cache(maxsize=None)
def expected(case, fmt=ir.GREY8, pad=0):
    """(raw, (grey, n_outside)) of a named case, computed once; callers leave the arrays unchanged."""
    w, h, K, Kinv, p = setup(case)
    raw = raw_bytes(p["raw_width"], p["raw_height"], fmt, pad)
    raw.setflags(write=False)
    return raw, ir.rectify(raw, fmt, p, K, Kinv, w, h)
