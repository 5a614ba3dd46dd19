"""Time of the metric-outputs stage (flame_nltgv2_metric_outputs: depth image, millimetre image, organised and dense cloud, posed mesh)
and of the same outputs made the way a consumer had to before the stage existed.

    python tools/metric_outputs_bench.py [--reps 30] [--out profiles/metric_outputs.txt] [--commit HASH]
    python tools/metric_outputs_bench.py --workload 20      (no timing: 20 rounds of every stage, for rocprofv3 --kernel-trace --stats)

device   HIP events around what begin enqueues on the context's side stream (flame_nltgv2_metric_outputs_view.device_ms), median
         over --reps calls after warm-up; `call` is the host's wall time of begin + end (which also brings the dense cloud over).
         Rows: every output with the copies out; every output with copy_out = 0; the pixel pass alone (depth + depth_mm + organized,
         copy_out = 0) and the dense cloud alone (copy_out = 0).
host     interpolate_mesh_end + mesh_outputs_end + the numpy checker (tests/metric_ref.py): wall time, median of 3.  The checker is
         vectorised numpy, not a C++ loop; it is the only other implementation the tree has, and its time is context, not a target.
solver   iterations per second of run_async(N) with ten calls of the stage issued beside it, against ten calls of mesh_outputs
         beside it and against the run alone, taken in turn, best of 3.
Scene: the 8480 vertices of the 640x480 synth graph, placed so that their mesh covers about half of a 640x480 and of a 1920x1080 map.
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

HBM_PEAK = 8.0e12      # bytes / s, the data sheet's
PIXEL_BYTES = 4 + 18   # the pixel pass: a float in; a float, a uint16 and three floats out
POSE = np.array([[0.8660254, -0.5, 0, 0.25], [0.5, 0.8660254, 0, -1.5], [0, 0, 1, 3.0]], np.float32)
SCALE = 1.1


def scene(synth, w, h):
    """The 640x480 point set squeezed into half of a w x h map, with its data term and Delaunay graph."""
    g0 = synth.make_graph("640x480", seed=31)
    pos = g0["pos"].astype(np.float64) * [0.5 * w / 640.0, h / 480.0]
    pos = pos.astype(np.float32)
    edges = synth.delaunay_edges_native(pos)
    g = synth.assemble_graph(pos, g0["data_term"], edges)
    return g, synth.delaunay_triangles_scipy(pos)


def prepare(flame_amd, reg, g, tris, Kinv, h, w):
    reg.upload_graph(g)
    reg.run(flame_amd.Params(), 200)
    reg.interpolate_mesh_begin(tris, h, w, graph_scale=SCALE)
    reg.mesh_outputs_begin(None, Kinv, h, w, graph_scale=SCALE, want_filtered_map=True)
    dense, cov = reg.interpolate_mesh_end()
    return dense, cov, reg.mesh_outputs_end()


def timed(reg, Kinv, h, w, params, reps):
    dev, call = [], []
    out = None
    for r in range(reps + 5):
        t0 = time.perf_counter()
        reg.metric_outputs_begin(Kinv, h, w, pose=POSE, params=params)
        out = reg.metric_outputs_end(copy=False)
        t1 = time.perf_counter()
        if r >= 5:
            dev.append(out["device_ms"] * 1e3), call.append((t1 - t0) * 1e6)
    return float(np.median(dev)), float(np.min(dev)), float(np.median(call)), out


def solver_rate(flame_amd, reg, n_iters, beside):
    p = flame_amd.Params()
    best = 0.0
    for _ in range(3):
        reg.sync()
        t0 = time.perf_counter()
        reg.run_async(p, n_iters)
        for _ in range(10):
            beside()
        reg.sync()
        best = max(best, n_iters / (time.perf_counter() - t0))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--workload", type=int, default=0)
    a = ap.parse_args()

    import torch  # noqa: F401  (one HIP runtime per process: torch's)

    import flame_amd
    from flame_amd import synth
    from flame_amd.regularizer import OPT_MESH_STATE
    from tests import metric_ref as xr

    MP = flame_amd.MetricParams
    if a.workload:
        for w, h in ((640, 480), (1920, 1080)):
            g, tris = scene(synth, w, h)
            Kinv = np.array([[1 / (0.82 * w), 0, -0.5], [0, 1 / (0.82 * w), -0.5 * h / w], [0, 0, 1]], np.float32)
            K = np.linalg.inv(Kinv.astype(np.float64)).astype(np.float32)
            gray = np.full((h, w), 100, np.uint8)
            with flame_amd.Regularizer(0) as reg:
                reg.upload_graph(g)
                for _ in range(a.workload):
                    reg.interpolate_mesh_begin(tris, h, w, graph_scale=SCALE)
                    reg.mesh_outputs_begin(None, Kinv, h, w, graph_scale=SCALE, want_filtered_map=True)
                    reg.debug_images_begin(gray, K, h, w)
                    reg.metric_outputs_begin(Kinv, h, w, pose=POSE, params=MP(want_mesh=True))
                    reg.interpolate_mesh_end(copy=False), reg.mesh_outputs_end(copy=False), reg.debug_images_end(copy=False)
                    reg.metric_outputs_end(copy=False)
        return

    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:  # noqa: BLE001
            commit = "unknown"
    lines = [f"metric outputs stage: tools/metric_outputs_bench.py --reps {a.reps}; tree at commit {commit} + this change",
             "device_us: HIP events on the side stream around what begin enqueues, median; call_us: wall time of begin + end; host_ms: "
             "interpolate_mesh_end + mesh_outputs_end + numpy checker, wall, median of 3"]
    for w, h in ((640, 480), (1920, 1080)):
        n = w * h
        g, tris = scene(synth, w, h)
        Kinv = np.array([[1 / (0.82 * w), 0, -0.5], [0, 1 / (0.82 * w), -0.5 * h / w], [0, 0, 1]], np.float32)
        with flame_amd.Regularizer(0) as reg:
            dense, cov, mo = prepare(flame_amd, reg, g, tris, Kinv, h, w)
            x = reg.download_state(("x",))["x"]
            rows = {}
            rows["all outputs, copied out"] = timed(reg, Kinv, h, w, MP(want_mesh=True), a.reps)
            rows["all outputs, copy_out = 0"] = timed(reg, Kinv, h, w, MP(want_mesh=True, copy_out=False), a.reps)
            pixel = MP(want_cloud=False, copy_out=False)
            rows["pixel pass alone"] = timed(reg, Kinv, h, w, pixel, a.reps)
            rows["cloud alone"] = timed(reg, Kinv, h, w, MP(want_depth=False, want_depth_mm=False, want_organized=False, copy_out=False), a.reps)
            out = rows["all outputs, copied out"][3]
            # the result is the checker's (the tests say so bit for bit; here: the counters)
            ref = xr.metric_points(dense, Kinv, POSE)
            assert ref["n_points"] == out["n_points"] and out["n_valid"] == mo["n_valid"], (ref["n_points"], out["n_points"])
            host = []
            for _ in range(3):
                reg.interpolate_mesh_begin(tris, h, w, graph_scale=SCALE)
                reg.mesh_outputs_begin(None, Kinv, h, w, graph_scale=SCALE, want_filtered_map=True)
                t0 = time.perf_counter()
                d2, _ = reg.interpolate_mesh_end(copy=False)
                m2 = reg.mesh_outputs_end(copy=False)
                xr.metric_points(d2, Kinv, POSE)
                xr.metric_mesh(g["pos"], x, SCALE, Kinv, m2["normals"], tris, m2["tri_valid"], POSE)
                host.append((time.perf_counter() - t0) * 1e3)
            host_ms = float(np.median(host))
            # the solver beside the stage
            reg.set_option(OPT_MESH_STATE, 1)
            n_iters = 20000
            full = MP(want_mesh=True)

            def beside_metric():
                reg.metric_outputs_begin(Kinv, h, w, pose=POSE, params=full)
                reg.metric_outputs_end(copy=False)

            def beside_mesh():
                reg.mesh_outputs_begin(None, Kinv, h, w, graph_scale=SCALE, want_filtered_map=True)
                reg.mesh_outputs_end(copy=False)

            rates = {}
            for name, fn in (("alone", lambda: None), ("beside 10 metric_outputs", beside_metric), ("beside 10 mesh_outputs", beside_mesh),
                             ("alone again", lambda: None)):
                rates[name] = solver_rate(flame_amd, reg, n_iters, fn)
        lines.append(f"{w}x{h} V={g['V']} T={len(tris)} coverage={cov / n:.2f} n_points={out['n_points']} n_valid={out['n_valid']}")
        for name, (d, dmin, c, _) in rows.items():
            extra = ""
            if name.startswith("pixel pass"):
                extra = f"  {PIXEL_BYTES * n / 1e6:.1f} MB -> {PIXEL_BYTES * n / (dmin * 1e-6) / 1e12:.2f} TB/s over the event time (min), " \
                        f"{100 * PIXEL_BYTES * n / (dmin * 1e-6) / HBM_PEAK:.0f} % of {HBM_PEAK / 1e12:.0f} TB/s"
            lines.append(f"  {name}: device_us {d:.1f} (min {dmin:.1f}) call_us {c:.1f}{extra}")
        lines.append(f"  host path: host_ms {host_ms:.1f}; ratio host / call (all outputs, copied out) {host_ms * 1e3 / rows['all outputs, copied out'][2]:.0f}x")
        lines.append("  solver, run_async(%d): " % n_iters + "; ".join(f"{k} {v / 1e3:.0f} k it/s" for k, v in rates.items()))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
