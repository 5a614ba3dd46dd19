"""Time of the mesh-outputs stage (flame_nltgv2_mesh_outputs: vtx_idepths, vertex normals, triangle filters, filtered map) and
of the same outputs made the way a host had to before the stage existed.

    python tools/mesh_outputs_bench.py [--reps 30] [--out profiles/mesh_outputs.txt] [--commit HASH]

device   HIP events around the stage on the context's side stream (kernels and the copies out; flame_nltgv2_mesh_outputs_view
         .device_ms), median over --reps calls after warm-up, without and with the filtered map; `call` is the host's wall time of
         begin + end for the same calls.
host     download_state + the numpy checker (tests/mesh_ref.py: filters and the running-mean normals on the CPU) +
         interpolate_mesh with the uploaded tri_valid: wall time, median of 3.  The checker is numpy, not the reference's C++; it
         is the only implementation of these loops the tree had, and its time is context, not a target.
Sizes: 640x480 and 1920x1080 (flame_amd.synth graphs, scipy Delaunay triangles), 200 solver iterations first.
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()

    import torch  # noqa: F401  (one HIP runtime per process: torch's)

    import flame_amd
    from flame_amd import synth
    from tests import mesh_ref as mr

    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:  # noqa: BLE001
            commit = "unknown"
    lines = [f"mesh outputs stage: tools/mesh_outputs_bench.py --reps {a.reps}; tree at commit {commit} + this change",
             "device_us: HIP events on the side stream (kernels + copies out), median; call_us: wall time of begin + end; "
             "host_ms: download_state + numpy checker + interpolate_mesh(tri_valid), wall, median of 3"]
    for config in ("640x480", "1920x1080"):
        w, h, _ = synth.CONFIGS[config]
        g = synth.make_graph(config, seed=31)
        tris = synth.delaunay_triangles_scipy(g["pos"])
        Kinv = np.array([[1 / (0.82 * w), 0, -0.5], [0, 1 / (0.82 * w), -0.5 * h / w], [0, 0, 1]], np.float32)
        with flame_amd.Regularizer(0) as reg:
            reg.upload_graph(g)
            reg.run(flame_amd.Params(), 200)
            res = {}
            for want_map in (False, True):
                dev, call = [], []
                for r in range(a.reps + 5):
                    t0 = time.perf_counter()
                    reg.mesh_outputs_begin(tris, Kinv, h, w, graph_scale=1.1, want_filtered_map=want_map)
                    out = reg.mesh_outputs_end(copy=False)
                    t1 = time.perf_counter()
                    if r >= 5:
                        dev.append(out["device_ms"] * 1e3), call.append((t1 - t0) * 1e6)
                res[want_map] = (float(np.median(dev)), float(np.min(dev)), float(np.median(call)), out["n_valid"])
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                x = reg.download_state(("x",))["x"]
                ref = mr.mesh_outputs(g["pos"], x, tris, Kinv, h, w, graph_scale=1.1)
                reg.interpolate_mesh(tris, h, w, graph_scale=1.1, tri_valid=ref["tri_valid"])
                host.append((time.perf_counter() - t0) * 1e3)
            host_ms = float(np.median(host))
        for want_map in (False, True):
            d, dmin, c, nv = res[want_map]
            lines.append(f"{config} V={g['V']} T={len(tris)} valid={nv} filtered_map={'yes' if want_map else 'no '}: "
                         f"device_us {d:.1f} (min {dmin:.1f}) call_us {c:.1f}")
        lines.append(f"{config} host path (with filtered map): host_ms {host_ms:.1f}; ratio host / device call (with map) "
                     f"{host_ms * 1e3 / res[True][2]:.0f}x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
