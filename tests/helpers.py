"""Shared helpers of the test-suite (tests may use oracle/)."""
from __future__ import annotations

import os

import numpy as np

from flame_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INPUT_KEYS = ("pos", "data_term", "data_weight", "src", "dst", "alpha", "beta")
OUT_KEYS = ("x", "w1", "w2", "x_bar", "w1_bar", "w2_bar", "q1", "q2", "q3")


def load_golden(name: str):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    edges = np.stack([z["src"], z["dst"]], axis=1)
    g = synth.assemble_graph(z["pos"], z["data_term"], edges, weight=z["data_weight"])
    g["alpha"] = z["alpha"].copy()
    g["beta"] = z["beta"].copy()
    return g, z


def assert_state_equal(a: dict, b: dict, keys=OUT_KEYS, what=""):
    for k in keys:
        if not np.array_equal(a[k], b[k]):
            d = np.abs(a[k].astype(np.float64) - b[k].astype(np.float64))
            raise AssertionError(f"{what}: {k} differs: max {d.max():.3e} at {int(d.argmax())}, "
                                 f"{int((d > 0).sum())}/{d.size} elements")


ALL_STATE_KEYS = OUT_KEYS + ("x_prev", "w1_prev", "w2_prev")
CANONICAL_NAN = 0x7FC00000


def float_bits(a):
    """The float32 bit patterns of `a`, every NaN mapped to one pattern: IEEE 754 leaves the sign and payload of a NaN that an
    operation GENERATES to the implementation (x86 SSE makes 0xFFC00000, gfx950 0x7FC00000) and the reference never reads
    them; tests/test_mesh_outputs.py::bits does the same for the mesh outputs.  Where a NaN stands is compared, and every
    bit of every other value: signed zeros, subnormals and infinities included."""
    f = np.ascontiguousarray(a, np.float32)
    u = f.view(np.uint32).copy()
    u[np.isnan(f)] = CANONICAL_NAN
    return u


def assert_state_bits_equal(a: dict, b: dict, keys=ALL_STATE_KEYS, what=""):
    """assert_state_equal on the bit patterns: -0.0 is not +0.0 here, and a NaN equals any other NaN."""
    for k in keys:
        ua, ub = float_bits(a[k]), float_bits(b[k])
        if ua.shape != ub.shape:
            raise AssertionError(f"{what}: {k} has shape {ua.shape} against {ub.shape}")
        diff = np.flatnonzero(ua != ub)
        if diff.size:
            i = int(diff[0])
            raise AssertionError(f"{what}: {k} differs in its bits, first at [{i}]: 0x{int(ua[i]):08X} against 0x{int(ub[i]):08X}, "
                                 f"{diff.size}/{ua.size} elements")


def rms(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt(np.mean(d * d))) if d.size else 0.0


def random_graph(V: int, E: int, seed: int, width=100.0):
    """Random simple graph (no self loops / duplicates) with random orientation and weights."""
    rng = np.random.default_rng(seed)
    pos = (rng.random((V, 2)) * width).astype(np.float32)
    data = (0.5 + rng.random(V)).astype(np.float32)
    seen, edges = set(), []
    tries = 0
    while len(edges) < E and tries < 50 * E + 100:
        tries += 1
        i, j = int(rng.integers(V)), int(rng.integers(V))
        if i == j or (min(i, j), max(i, j)) in seen:
            continue
        if np.all(pos[i] == pos[j]):
            continue
        seen.add((min(i, j), max(i, j)))
        edges.append((i, j))
    edges = np.array(edges, dtype=np.int32).reshape(-1, 2)
    g = synth.assemble_graph(pos, data, edges, weight=(0.5 + rng.random(V)).astype(np.float32))
    if len(edges):
        g["beta"] = (0.5 + rng.random(len(edges))).astype(np.float32)
    return g
