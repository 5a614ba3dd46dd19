"""Time of the view renderer (flame_nltgv2_render_view: the resident mesh seen from another camera, the nearest surface kept) and of
its yardsticks.

    python tools/render_view_bench.py [--reps 30] [--out profiles/render_view.txt] [--commit HASH]
    python tools/render_view_bench.py --workload 20        (no timing: 20 rounds of the stage and of interpolate_mesh_begin per size,
                                                            for rocprofv3 --kernel-trace --stats, no counters in that run)
    python tools/render_view_bench.py --trace-db DIR/NAME_results.db   (per kernel, grid and size: calls, median / least duration; host only)

device   HIP events around what begin enqueues on the context's side stream (flame_nltgv2_view_outputs_view.device_ms), median (min)
         over --reps calls after 5 warm-up calls; `call` is the host's wall time of begin + end.  Rows: map and owner indices copied
         out; the same with copy_out = 0 (only the 16 bytes of counters travel); the map alone with copy_out = 0.
yardstick  the rasteriser of interpolate_mesh on the same triangles -- k_raster_triangles + k_raster_resolve in the kernel trace of
         --workload: the same triangles and atomics without the transform and the int64 edges.
host     download_state (pos is the caller's, x comes down) + the numpy checker (tests/view_ref.py): wall time, median of 3.  The
         checker is the only other implementation the tree has; its time is context, not a target.
solver   iterations per second of run_async(N) with ten calls of the stage issued beside it, against ten calls of metric_outputs
         beside it and against the run alone, taken in turn, best of 3.
Scene: the 8480 vertices of the 640x480 synth graph, placed so that their mesh covers about half of a 640x480 and of a 1920x1080 map,
after 200 iterations; the target camera has the source's intrinsics and size, turned by 3 degrees and moved sideways.
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

KERNELS = ("k_view_clear", "k_view_vertices", "k_view_count", "k_view_raster_big", "k_view_raster", "k_view_resolve", "k_raster_triangles",
           "k_raster_resolve")
ANGLE = np.deg2rad(3.0)
R = np.array([[np.cos(ANGLE), 0, np.sin(ANGLE)], [0, 1, 0], [-np.sin(ANGLE), 0, np.cos(ANGLE)]], np.float32)
T = np.array([-0.08, 0.01, 0.02], np.float32)


def scene(synth, w, h):
    """The 640x480 point set squeezed into half of a w x h map, with its data term and Delaunay graph."""
    g0 = synth.make_graph("640x480", seed=31)
    pos = g0["pos"].astype(np.float64) * [0.5 * w / 640.0, h / 480.0]
    pos = pos.astype(np.float32)
    edges = synth.delaunay_edges_native(pos)
    g = synth.assemble_graph(pos, g0["data_term"], edges)
    return g, synth.delaunay_triangles_scipy(pos)


def cameras(w, h):
    Kinv = np.array([[1 / (0.82 * w), 0, -0.5], [0, 1 / (0.82 * w), -0.5 * h / w], [0, 0, 1]], np.float32)
    return Kinv, np.linalg.inv(Kinv.astype(np.float64)).astype(np.float32)


def trace_stats(db_path):
    import collections
    import sqlite3

    db = sqlite3.connect(db_path)
    rows = collections.defaultdict(list)
    for name, gx, start, end in db.execute("select name, grid_x, start, end from kernels order by start"):
        short = next((k for k in KERNELS if k in name), None)
        if short is not None:
            rows[(short, int(gx))].append((end - start) / 1e3)
    lines = []
    for (k, grid), v in sorted(rows.items()):
        # a grid that follows the mesh, not the map, is the same at both sizes: --workload runs 640x480 first, then 1920x1080
        sized = k in ("k_view_clear", "k_view_resolve", "k_raster_resolve")
        for what, part in ((("", v),) if sized else (("640x480", v[:len(v) // 2]), ("1920x1080", v[len(v) // 2:]))):
            lines.append("  %-20s grid %9d %-9s calls %4d  median %8.2f  min %8.2f us" % (k, grid, what, len(part), float(np.median(part)), min(part)))
    return "\n".join(lines)


def timed(reg, params, h, w, reps):
    dev, call = [], []
    out = None
    for r in range(reps + 5):
        t0 = time.perf_counter()
        reg.render_view_begin(params, h, w)
        out = reg.render_view_end(copy=False)
        t1 = time.perf_counter()
        if r >= 5:
            dev.append(out["device_ms"] * 1e3), call.append((t1 - t0) * 1e6)
    return float(np.median(dev)), float(np.min(dev)), float(np.median(call)), float(np.min(call)), out


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
    ap.add_argument("--trace-db", default=None)
    a = ap.parse_args()
    if a.trace_db:  # (host only: reads what an earlier traced run left)
        print(trace_stats(a.trace_db))
        return

    import torch  # noqa: F401  (one HIP runtime per process: torch's)

    assert torch.cuda.is_available(), "render_view_bench.py measures on a GPU; there is no other path"
    import flame_amd
    from flame_amd import synth
    from flame_amd.regularizer import OPT_MESH_STATE
    from tests import view_ref as vr

    VP, MP = flame_amd.ViewParams, flame_amd.MetricParams

    if a.workload:
        for w, h in ((640, 480), (1920, 1080)):
            g, tris = scene(synth, w, h)
            Kinv, K = cameras(w, h)
            with flame_amd.Regularizer(0) as reg:
                reg.upload_graph(g)
                reg.run(flame_amd.Params(), 200)
                for _ in range(a.workload):
                    reg.interpolate_mesh_begin(tris, h, w)
                    reg.render_view_begin(VP(Kinv_src=Kinv, K_dst=K, R=R, t=T, copy_out=False), h, w)
                    reg.interpolate_mesh_end(copy=False), reg.render_view_end(copy=False)
        return

    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:  # noqa: BLE001
            commit = "unknown"
    lines = [f"view renderer: tools/render_view_bench.py --reps {a.reps}; tree at commit {commit} + this change",
             "device_us: HIP events on the side stream around what begin enqueues, median (min); call_us: wall time of begin + end, median (min); "
             "host_ms: download_state + numpy checker, wall, median of 3"]
    for w, h in ((640, 480), (1920, 1080)):
        g, tris = scene(synth, w, h)
        Kinv, K = cameras(w, h)
        cam = dict(Kinv_src=Kinv, K_dst=K, R=R, t=T)
        with flame_amd.Regularizer(0) as reg:
            reg.upload_graph(g)
            reg.run(flame_amd.Params(), 200)
            reg.interpolate_mesh(tris, h, w)
            rows = {}
            rows["map + owner indices, copied out"] = timed(reg, VP(**cam), h, w, a.reps)
            rows["map + owner indices, copy_out = 0"] = timed(reg, VP(copy_out=False, **cam), h, w, a.reps)
            rows["map alone, copy_out = 0"] = timed(reg, VP(copy_out=False, want_tri_index=False, **cam), h, w, a.reps)
            got = rows["map + owner indices, copied out"][4]
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                x = reg.download_state(("x",))["x"]
                want = vr.render_view(tris, g["pos"], x, Kinv, K, R, T, h, w)
                host.append((time.perf_counter() - t0) * 1e3)
            vr.assert_same(got, want, f"{w}x{h}")  # the result is the checker's, bit for bit
            reg.set_option(OPT_MESH_STATE, 1)
            n_iters = 20000
            stage, metric = VP(copy_out=False, **cam), MP(copy_out=False)

            def beside_view():
                reg.render_view_begin(stage, h, w)
                reg.render_view_end(copy=False)

            def beside_metric():
                reg.metric_outputs_begin(Kinv, h, w, params=metric)
                reg.metric_outputs_end(copy=False)

            rates = {}
            for name, fn in (("alone", lambda: None), ("beside 10 render_view", beside_view), ("beside 10 metric_outputs", beside_metric),
                             ("alone again", lambda: None), ("beside 10 render_view again", beside_view)):
                rates[name] = solver_rate(flame_amd, reg, n_iters, fn)
        lines.append(f"{w}x{h} V={g['V']} T={len(tris)} coverage={got['coverage'] / (w * h):.2f} drawn={got['tris_drawn']} "
                     f"culled_vertex={got['tris_culled_vertex']} culled_facing={got['tris_culled_facing']}")
        for name, (d, dmin, c, cmin, _) in rows.items():
            lines.append(f"  {name}: device_us {d:.1f} (min {dmin:.1f}) call_us {c:.1f} (min {cmin:.1f})")
        ms = float(np.median(host))
        lines.append(f"  host path: host_ms {ms:.1f}; ratio host / call (copied out) {ms * 1e3 / rows['map + owner indices, copied out'][2]:.0f}x")
        lines.append("  solver, run_async(%d): " % n_iters + "; ".join(f"{k} {v / 1e3:.0f} k it/s" for k, v in rates.items()))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
