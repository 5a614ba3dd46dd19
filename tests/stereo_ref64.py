"""A plain float64 restatement of the epipolar walk (line_stereo::match without the sub-pixel step), for
tests/test_stereo_walk_edges.py.  It shares no code and no evaluation order with oracle/stereo_oracle.c: positions are
start + t * inc (no accumulation), every step samples its own five positions, the best step is numpy's argmin.
"""
from __future__ import annotations

import numpy as np


def bilinear64(img: np.ndarray, x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    dx, dy = x - x0, y - y0
    f = img.astype(np.float64)
    return ((1 - dx) * (1 - dy) * f[y0, x0] + dx * (1 - dy) * f[y0, x0 + 1] + (1 - dx) * dy * f[y0 + 1, x0]
            + dx * dy * f[y0 + 1, x0 + 1])


def walk64(patch, img_pad, start, end, sample_dist, max_steps=4096):
    """patch: the five reference samples (m2, m1, centre, p1, p2); start, end: the segment in padded coordinates.
    -> dict(costs [n], c_best, x, y, inc (2,)) or None when a sample leaves the image."""
    s, e = np.asarray(start, np.float64), np.asarray(end, np.float64)
    d = e - s
    inc = d * (float(sample_dist) / np.hypot(d[0], d[1]))
    n = 1
    while n < max_steps:
        cp = s + n * inc
        if not (((inc[0] < 0) == (cp[0] > e[0])) and ((inc[1] < 0) == (cp[1] > e[1]))):
            break
        n += 1
    t = np.arange(n, dtype=np.float64)[:, None] + np.arange(-2, 3, dtype=np.float64)[None, :]   # [n, 5]
    xs, ys = s[0] + t * inc[0], s[1] + t * inc[1]
    rows, cols = img_pad.shape
    if xs.min() < 0 or ys.min() < 0 or xs.max() >= cols - 1 or ys.max() >= rows - 1:
        return None
    v = bilinear64(img_pad, xs, ys)
    costs = ((v - np.asarray(patch, np.float64)[None, :]) ** 2).sum(axis=1)
    c = int(np.argmin(costs))
    return dict(costs=costs, c_best=c, x=s[0] + c * inc[0], y=s[1] + c * inc[1], inc=inc)
