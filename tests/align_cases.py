"""The generated scenes the alignment tests share (tests/test_align.py on the CPU, tests/test_gpu_align*.py on the device): nothing is
read from disk.  Each function is deterministic."""
import functools

import numpy as np

from tests import align_ref as ar

DRIVER_W, DRIVER_H = 96, 72
DRIVER_K = (64.0, 64.0, 48.0, 36.0)  # fx fy cx cy
DRIVER_Q_TRUE = (0.99980001, 0.010, -0.012, 0.008)  # about 2 degrees
DRIVER_T_TRUE = (0.06, -0.04, 0.02)
DRIVER_PARAMS = dict(border=2, huber_k=10.0, coarsest_level=2, finest_level=0, max_iters_per_level=10, min_pixels=100,
                     min_step=1e-5, lm_lambda=0.0)


def K_matrices(K):
    fx, fy, cx, cy = K
    Km = np.array([fx, 0, cx, 0, fy, cy, 0, 0, 1], np.float32)
    Ki = np.array([1 / fx, 0, -cx / fx, 0, 1 / fy, -cy / fy, 0, 0, 1], np.float32)
    return Km, Ki


@functools.lru_cache(maxsize=None)
def driver_scene():
    """-> (ref u8, new u8, idepth f32, q_true, t_true): 96 x 72, a smooth texture, a smooth known inverse depth around 0.5."""
    q = np.asarray(DRIVER_Q_TRUE, np.float64)
    q = q / np.linalg.norm(q)
    t = np.asarray(DRIVER_T_TRUE, np.float64)
    ref, new, d = ar.make_scene(DRIVER_W, DRIVER_H, DRIVER_K, q, t, seed=3)
    return ref, new, d, q, t


@functools.lru_cache(maxsize=None)
def driver_reference():
    """The checker's own loop on driver_scene from the identity: computed once, shared, not changed by anyone."""
    ref, new, d, _, _ = driver_scene()
    rp, npyr = ar.build_pyramid(ref, 3), ar.build_pyramid(new, 3)
    return ar.align_frame(rp, npyr, d, DRIVER_K, (1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0), **DRIVER_PARAMS)


def random_image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def small_pose():
    q = np.array([0.9998, 0.01, -0.012, 0.008], np.float64)
    return q / np.linalg.norm(q), np.array([0.05, -0.03, 0.02], np.float64)
