"""Cameras and poses in which no entry is 0 or 1 by construction, and the probe that says whether a checker's output depends on every
entry of a matrix it reads.  The stages state their rules as full products (q = Kinv (col, row, 1), P' = R P + t, h = K_dst P',
xs = (K_raw[0] xd + K_raw[1] yd) + K_raw[2]); a pinhole matrix and a rotation about one axis leave entries at 0 that a kernel, a host
copy or a binding could then drop or read from the wrong index unnoticed.  Nothing here touches the GPU: the tests of the device
(tests/test_gpu_general_cameras.py) compare it bit for bit with the same float32 checkers on the same matrices.

    general_K64, general_kinv, rotation, pose      the matrices, float64 (round them once, where the stage takes float32)
    blind_entries                                  the probe: the swaps and zeroings of entries that change no bit of fn's output
    affine, quotient, product                      float64 values with forward bounds, the rules of tests/volume_ref64.py
"""
import itertools

import numpy as np

from tests.volume_ref64 import EPS, _affine as affine, _quotient as quotient  # noqa: F401  (one statement of the bounds)

F = np.float32


def general_K64(fx, fy, cx, cy, skew=None, shear=None, bottom=None):
    """[[fx, skew, cx], [shear, fy, cy], [b0, b1, 1]] in float64, the pattern of GENERAL_K64 in tests/test_volume_edges_ref.py scaled to
    the camera: skew = 0.035 fx, shear = 0.015 fx, bottom row (0.16 / cx, -0.24 / cy) -- (20, 19, 16, 12) gives that constant's
    0.7, 0.3, 0.01, -0.02 -- so that the third coordinate stays within 1 +- 0.5 over an image of twice the principal point."""
    skew = fx * 7.0 / 200.0 if skew is None else skew
    shear = fx * 3.0 / 200.0 if shear is None else shear
    b0, b1 = (0.16 / cx, -0.24 / cy) if bottom is None else bottom
    return np.array([[fx, skew, cx], [shear, fy, cy], [b0, b1, 1.0]], np.float64)


def general_kinv(K64):
    """The float64 inverse rounded once, (3, 3) float32: every entry non-zero for a general K."""
    return np.linalg.inv(np.asarray(K64, np.float64)).astype(F)


def rotation(deg, axis=(1, 2, 3)):
    """Rodrigues' formula in float64: about (1, 2, 3) no entry of R is 0 or +-1 and no two are equal."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(np.asarray(axis, np.float64))
    A = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * A + (1 - np.cos(th)) * (A @ A)


def pose(deg, t, axis=(1, 2, 3)):
    """(3, 4) float32 [R | t], rounded once from float64."""
    return np.hstack([rotation(deg, axis), np.asarray(t, np.float64)[:, None]]).astype(F)


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def blind_entries(fn, M, read):
    """The mutations of M, among its entries `read` (indices into M.reshape(-1)), after which fn's output is bit-identical to fn(M):
    ("swap", i, j) for every pair, and ("zero", i) for every entry set to 0 -- to 0.5 if it is exactly 1, so that a third coordinate
    that is 1 is changed too; a swap alone cannot see an entry that is 0 and ignored, nor two that are equal.  fn takes an array of
    M's shape and dtype and returns arrays, or tuples, lists or dicts of them."""
    M = np.asarray(M)
    base = fn(M.copy())
    read = list(read)
    flat = M.reshape(-1)
    blind = []
    for i, j in itertools.combinations(read, 2):
        m = flat.copy()
        m[i], m[j] = flat[j], flat[i]
        if _same(fn(m.reshape(M.shape)), base):
            blind.append(("swap", i, j))
    for i in read:
        m = flat.copy()
        m[i] = 0.5 if flat[i] == 1 else 0
        if _same(fn(m.reshape(M.shape)), base):
            blind.append(("zero", i))
    return blind


def product(x, ex, y, ey):
    """x * y -> value, bound: |x| ey + |y| ex + ex ey + EPS |x y|."""
    v = x * y
    return v, np.abs(x) * ey + np.abs(y) * ex + ex * ey + EPS * np.abs(v)


def homogeneous(M64, x, y):
    """M (x, y, 1) for float32 data x, y as three float64 arrays with the bounds of the float32 evaluation: three products, two sums."""
    one = np.ones_like(x)
    zero = np.zeros_like(x)
    return affine(np.asarray(M64, np.float64).reshape(3, 3), None, [x, y, one], [zero, zero, zero])
