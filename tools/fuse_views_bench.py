"""Time of the fusion stage (flame_nltgv2_fuse_views: up to eight kept meshes rendered into one camera in one batch, a vote per pixel)
and of its yardsticks.

    python tools/fuse_views_bench.py [--reps 30] [--out profiles/fuse_views.txt] [--commit HASH]
    python tools/fuse_views_bench.py --workload 20        (no timing: per size and N = 1, 4, 8, 20 rounds of the stage, of N render_view
                                                           calls and of metric_outputs, for rocprofv3 --kernel-trace --stats, no counters
                                                           in that run)
    python tools/fuse_views_bench.py --trace-db DIR/NAME_results.db   (per kernel, grid and N: calls, median / least duration, and for the
                                                           vote its bytes over its time; host only)

device   HIP events around what begin enqueues on the context's side stream (flame_nltgv2_fuse_outputs_view.device_ms), median (min)
         over --reps calls after 5 warm-up calls, fused + masks + spread with copy_out = 0; `call` is the host's wall time of begin + end.
yardstick  what the tree had before this stage: N calls of render_view_begin / _end with copy_out = 0 on the same meshes and cameras,
         the sum of their device times (median per call).  The batch launches less and has no resolve pass.
host     the path this replaces: N x render_view_arrays with the meshes in host memory, the maps brought down, the vote in numpy
         (tests/fuse_ref.py): wall time, once.  Its result must equal the stage's, bit for bit.
solver   iterations per second of run_async(N) with ten calls of the stage (N = 4) issued beside it, against the run alone, taken in
         turn, best of 3.
Scene: tools/render_view_bench.py's -- the 8480 vertices of the 640x480 synth graph over half of a 640x480 and of a 1920x1080 map, after
200 iterations --, kept N times and seen from N poses turned by up to 5 degrees and moved sideways.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from render_view_bench import cameras, scene, solver_rate  # noqa: E402

KERNELS = ("k_keep_vertices", "k_fuse_clear", "k_fuse_vertices", "k_fuse_count", "k_fuse_raster_big", "k_fuse_raster", "k_fuse_vote",
           "k_view_clear", "k_view_vertices", "k_view_count", "k_view_raster_big", "k_view_raster", "k_view_resolve", "k_metric_")
SIZES = ((640, 480), (1920, 1080))
COUNTS = (1, 4, 8)


def pose(s):
    a = np.deg2rad(1.4 * (s - 3.5))
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
    return R, np.array([0.03 * (s - 3.5), 0.01 * (s % 3 - 1), 0.005 * s], np.float32)


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
        lines.append("  %-18s grid %9d calls %5d  median %8.2f  min %8.2f us" % (k, grid, len(v), float(np.median(v)), min(v)))
        if k == "k_fuse_vote":  # --workload runs N = 1, 4, 8 in turn at each size: thirds of the calls; 256 threads x 8 pixels per workgroup
            pixels = {w * h for w, h in SIZES if (w * h + 2047) // 2048 * 256 == grid or (w * h + 2047) // 2048 == grid}
            for i, n in enumerate(COUNTS):
                part = v[i * len(v) // 3:(i + 1) * len(v) // 3]
                for px in pixels:
                    nbytes = px * (8 * n + 4 + 1 + 1 + 4)
                    lines.append("      N = %d: median %8.2f us, %d bytes (N * 8 read + fused, masks, spread written per pixel): %.0f GB/s" % (
                        n, float(np.median(part)), nbytes, nbytes / float(np.median(part)) / 1e3))
    return "\n".join(lines)


def timed(begin, end, reps):
    dev, call = [], []
    out = None
    for r in range(reps + 5):
        t0 = time.perf_counter()
        begin()
        out = end()
        t1 = time.perf_counter()
        if r >= 5:
            dev.append(out["device_ms"] * 1e3), call.append((t1 - t0) * 1e6)
    return float(np.median(dev)), float(np.min(dev)), float(np.median(call)), float(np.min(call)), out


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

    assert torch.cuda.is_available(), "fuse_views_bench.py measures on a GPU; there is no other path"
    import flame_amd
    from flame_amd import synth
    from flame_amd.regularizer import OPT_MESH_STATE
    from tests import fuse_ref as fr

    FP, FS, VP, MP = flame_amd.FuseParams, flame_amd.FuseSource, flame_amd.ViewParams, flame_amd.MetricParams

    def fuse_params(n, Kinv, K, **kw):
        return FP(sources=[FS(slot=s, Kinv_src=Kinv, R=pose(s)[0], t=pose(s)[1], weight=1.0 + 0.1 * s) for s in range(n)], K_dst=K, rel_tol=0.05,
                  min_support=min(2, n), **kw)

    def prepared(reg, g, tris, h, w):
        reg.upload_graph(g)
        reg.run(flame_amd.Params(), 200)
        reg.interpolate_mesh(tris, h, w)
        for s in range(max(COUNTS)):
            reg.keep_mesh(s)

    if a.workload:
        for w, h in SIZES:
            g, tris = scene(synth, w, h)
            Kinv, K = cameras(w, h)
            with flame_amd.Regularizer(0) as reg:
                prepared(reg, g, tris, h, w)
                for n in COUNTS:
                    p = fuse_params(n, Kinv, K, copy_out=False)
                    for _ in range(a.workload):
                        reg.fuse_views_begin(p, h, w)
                        reg.fuse_views_end(copy=False)
                        for s in range(n):
                            reg.render_view_begin(VP(Kinv_src=Kinv, K_dst=K, R=pose(s)[0], t=pose(s)[1], copy_out=False, want_tri_index=False), h, w)
                            reg.render_view_end(copy=False)
                        reg.metric_outputs_begin(Kinv, h, w, params=MP(copy_out=False))
                        reg.metric_outputs_end(copy=False)
        return

    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:  # noqa: BLE001
            commit = "unknown"
    lines = [f"fusion of views: tools/fuse_views_bench.py --reps {a.reps}; tree at commit {commit} + this change",
             "device_us: HIP events on the side stream around what begin enqueues, median (min); call_us: wall time of begin + end, median (min); "
             "yardstick: the sum over N render_view calls (map alone, copy_out = 0) of their median device_us; host_ms: N x render_view_arrays + "
             "the numpy vote, wall, once"]
    for w, h in SIZES:
        g, tris = scene(synth, w, h)
        Kinv, K = cameras(w, h)
        with flame_amd.Regularizer(0) as reg:
            prepared(reg, g, tris, h, w)
            mesh = reg.get_kept_mesh(0)
            lines.append(f"{w}x{h} V={g['V']} T={len(tris)} per source")
            per_view = []
            for s in range(max(COUNTS)):
                vp = VP(Kinv_src=Kinv, K_dst=K, R=pose(s)[0], t=pose(s)[1], copy_out=False, want_tri_index=False)
                per_view.append(timed(lambda: reg.render_view_begin(vp, h, w), lambda: reg.render_view_end(copy=False), a.reps))
            for n in COUNTS:
                p = fuse_params(n, Kinv, K, copy_out=False)
                d, dmin, c, cmin, out = timed(lambda: reg.fuse_views_begin(p, h, w), lambda: reg.fuse_views_end(copy=False), a.reps)
                yard, yard_call = sum(v[0] for v in per_view[:n]), sum(v[2] for v in per_view[:n])
                full = reg.fuse_views(fuse_params(n, Kinv, K, want_layers=True), h, w)
                t0 = time.perf_counter()
                maps = [reg.render_view_arrays(VP(Kinv_src=Kinv, K_dst=K, R=pose(s)[0], t=pose(s)[1], want_tri_index=False), mesh["triangles"],
                                               mesh["vertices"], mesh["idepths"], h, w) for s in range(n)]
                voted = fr.fuse_views(np.stack([m["map"] for m in maps]), [1.0 + 0.1 * s for s in range(n)], 0.05, min(2, n),
                                      sum(m["tris_drawn"] for m in maps))
                host_ms = (time.perf_counter() - t0) * 1e3
                voted["layers"] = np.stack([m["map"] for m in maps])
                fr.assert_same(full, voted, f"{w}x{h} N={n}")  # the stage gives what the host path gives, bit for bit
                assert out["counts"].tolist() == voted["counts"].tolist()
                lines.append(f"  N = {n}: device_us {d:.1f} (min {dmin:.1f}) call_us {c:.1f} (min {cmin:.1f}); yardstick device_us {yard:.1f} call_us "
                             f"{yard_call:.1f}: ratio {d / yard:.2f}; host_ms {host_ms:.1f}; coverage {out['coverage'] / (w * h):.2f} support "
                             f"{out['support_hist'][:n + 1]}")
            reg.set_option(OPT_MESH_STATE, 1)
            n_iters = 20000
            stage = fuse_params(4, Kinv, K, copy_out=False)

            def beside_fuse():
                reg.fuse_views_begin(stage, h, w)
                reg.fuse_views_end(copy=False)

            rates = {}
            for name, fn in (("alone", lambda: None), ("beside 10 fuse_views (N = 4)", beside_fuse), ("alone again", lambda: None),
                             ("beside 10 fuse_views again", beside_fuse)):
                rates[name] = solver_rate(flame_amd, reg, n_iters, fn)
        lines.append("  solver, run_async(%d): " % n_iters + "; ".join(f"{k} {v / 1e3:.0f} k it/s" for k, v in rates.items()))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
