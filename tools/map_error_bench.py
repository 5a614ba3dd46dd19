"""Time of the map-error stage (flame_nltgv2_map_error: photometric error or error against a true map, box mean, histogram, ranks, sum)
and of the same measurement made the way the tests had to before the stage existed.

    python tools/map_error_bench.py [--reps 30] [--out profiles/map_error.txt] [--commit HASH]
    python tools/map_error_bench.py --workload 20          (no timing: 20 rounds of the stage and its yardsticks per size, for
                                                            rocprofv3 --kernel-trace --stats, no counters in that run)
    python tools/map_error_bench.py --trace-db DIR/NAME_results.db   (per kernel and grid: calls, median / least duration, the bytes
                                                            the kernel must move over the median; host only)

device   HIP events around what begin enqueues on the context's side stream (flame_nltgv2_map_error_view.device_ms), median (min) over
         --reps calls after 5 warm-up calls; `call` is the host's wall time of begin + end.  Rows per source: error map + statistics
         copied out; the same with copy_out = 0 (only the 1048 bytes of statistics travel); PHOTO also with the picture.
host     interpolate_mesh_end (the map's download) + the numpy checker (tests/map_error_ref.py): wall time, median of 3.  The checker
         is vectorised numpy over the oracle's C loop, not a consumer's C++; it is the only other implementation the tree has, and its
         time is context, not a target.
solver   iterations per second of run_async(N) with ten calls of the stage issued beside it, against ten calls of metric_outputs
         beside it and against the run alone, taken in turn, best of 3.
Scene: the 8480 vertices of the 640x480 synth graph, placed so that their mesh covers about half of a 640x480 and of a 1920x1080 map;
two random grey images; a parallax of a few pixels; PHOTO with win_size 11 and border 3, TRUTH relative with win_size 11.
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

HBM_PEAK = 8.0e12  # bytes / s, the data sheet's
KRKINV = np.array([[1, 0, 1.5], [0, 1, -0.75], [0, 0, 1]], np.float32)
KT = np.array([2.0, 1.0, 0.0], np.float32)
WIN, BORDER = 11, 3
POSE = np.array([[0.8660254, -0.5, 0, 0.25], [0.5, 0.8660254, 0, -1.5], [0, 0, 1, 3.0]], np.float32)
# bytes per pixel a kernel must move (in + out), by a substring of its name; 1080p and 640x480 are told apart by the grid
KERNEL_BYTES = {"k_map_error_photo": 4 + 2 + 4, "k_map_error_truth": 8 + 4, "k_map_error_box": 4 + 4, "k_map_error_hist": 4,
                "k_map_error_picture": 5 + 3, "k_map_error_finish": 0, "k_metric_pixels": 4 + 18, "k_debug_images": 13 + 6}


def scene(synth, w, h):
    """The 640x480 point set squeezed into half of a w x h map, with its data term and Delaunay graph."""
    g0 = synth.make_graph("640x480", seed=31)
    pos = g0["pos"].astype(np.float64) * [0.5 * w / 640.0, h / 480.0]
    pos = pos.astype(np.float32)
    edges = synth.delaunay_edges_native(pos)
    g = synth.assemble_graph(pos, g0["data_term"], edges)
    return g, synth.delaunay_triangles_scipy(pos)


def inputs(w, h):
    rng = np.random.default_rng(w)
    ref, cmp = (rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(2))
    truth = rng.uniform(0.2, 2.0, (h, w)).astype(np.float32)
    return ref, cmp, truth


def trace_stats(db_path):
    import collections
    import sqlite3

    db = sqlite3.connect(db_path)
    rows = collections.defaultdict(list)
    try:
        cur = db.execute("select name, grid_x, grid_y, start, end from kernels")
    except sqlite3.OperationalError:  # (a view without grid_y)
        cur = db.execute("select name, grid_x, 1, start, end from kernels")
    for name, gx, gy, start, end in cur:
        short = next((k for k in KERNEL_BYTES if k in name), None)
        if short is None:
            continue
        if "<" in name:
            short += name[name.index("<"):name.index(">") + 1]
        rows[(short, int(gx) * int(gy))].append((end - start) / 1e3)
    lines = []
    for (k, grid), v in sorted(rows.items()):
        lines.append("  %-36s grid %9d  calls %4d  median %7.2f  min %7.2f us" % (k, grid, len(v), float(np.median(v)), min(v)))
    return "\n".join(lines)


def timed(reg, params, h, w, reps):
    dev, call = [], []
    out = None
    for r in range(reps + 5):
        t0 = time.perf_counter()
        reg.map_error_begin(params, h, w)
        out = reg.map_error_end(copy=False)
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

    assert torch.cuda.is_available(), "map_error_bench.py measures on a GPU; there is no other path"
    import flame_amd
    from flame_amd import synth
    from flame_amd.regularizer import OPT_MESH_STATE
    from tests import map_error_ref as er

    MP, EP = flame_amd.MetricParams, flame_amd.MapErrorParams
    photo_kw = dict(KRKinv=KRKINV, Kt=KT, border=BORDER, win_size=WIN)

    def truth_kw(truth):
        return dict(source=flame_amd.MAP_ERROR_TRUTH, truth=truth, relative=True, win_size=WIN)

    if a.workload:
        for w, h in ((640, 480), (1920, 1080)):
            g, tris = scene(synth, w, h)
            ref, cmp, truth = inputs(w, h)
            Kinv = np.array([[1 / (0.82 * w), 0, -0.5], [0, 1 / (0.82 * w), -0.5 * h / w], [0, 0, 1]], np.float32)
            K = np.linalg.inv(Kinv.astype(np.float64)).astype(np.float32)
            with flame_amd.Regularizer(0) as reg:
                reg.upload_graph(g)
                reg.photo_set_images(ref, cmp)
                for _ in range(a.workload):
                    reg.interpolate_mesh_begin(tris, h, w)
                    reg.debug_images_begin(ref, K, h, w)
                    reg.metric_outputs_begin(Kinv, h, w, pose=POSE, params=MP(copy_out=False))
                    reg.map_error_begin(EP(want_image=True, copy_out=False, **photo_kw), h, w)
                    reg.map_error_end(copy=False)
                    reg.map_error_begin(EP(copy_out=False, **truth_kw(truth)), h, w)
                    reg.interpolate_mesh_end(copy=False), reg.debug_images_end(copy=False), reg.metric_outputs_end(copy=False)
                    reg.map_error_end(copy=False)
        return

    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:  # noqa: BLE001
            commit = "unknown"
    lines = [f"map error stage: tools/map_error_bench.py --reps {a.reps}; tree at commit {commit} + this change",
             "device_us: HIP events on the side stream around what begin enqueues, median (min); call_us: wall time of begin + end, median (min); "
             "host_ms: interpolate_mesh_end + numpy checker, wall, median of 3"]
    for w, h in ((640, 480), (1920, 1080)):
        n = w * h
        g, tris = scene(synth, w, h)
        ref, cmp, truth = inputs(w, h)
        Kinv = np.array([[1 / (0.82 * w), 0, -0.5], [0, 1 / (0.82 * w), -0.5 * h / w], [0, 0, 1]], np.float32)
        with flame_amd.Regularizer(0) as reg:
            reg.upload_graph(g)
            reg.run(flame_amd.Params(), 200)
            dense, cov = reg.interpolate_mesh(tris, h, w)
            reg.photo_set_images(ref, cmp)
            rows = {}
            rows["PHOTO win 11, error map + statistics, copied out"] = timed(reg, EP(**photo_kw), h, w, a.reps)
            rows["PHOTO win 11, + picture, copied out"] = timed(reg, EP(want_image=True, **photo_kw), h, w, a.reps)
            rows["PHOTO win 11, copy_out = 0"] = timed(reg, EP(copy_out=False, **photo_kw), h, w, a.reps)
            rows["TRUTH win 11, error map + statistics, copied out"] = timed(reg, EP(**truth_kw(truth)), h, w, a.reps)
            rows["TRUTH win 11, copy_out = 0 (host truth staged)"] = timed(reg, EP(copy_out=False, **truth_kw(truth)), h, w, a.reps)
            tdev = torch.from_numpy(truth).cuda()
            torch.cuda.synchronize()
            rows["TRUTH win 11, copy_out = 0, truth on the device"] = timed(
                reg, EP(source=flame_amd.MAP_ERROR_TRUTH, truth_device=tdev.data_ptr(), win_size=WIN, copy_out=False), h, w, a.reps)
            # the result is the checker's (the tests say so bit for bit; here: the statistics)
            got = rows["PHOTO win 11, copy_out = 0"][4]
            want = er.map_error(dense, er.PHOTO, KRKINV, KT, ref, cmp, BORDER, win_size=WIN)
            assert (got["n_valid"], got["median_bin"], got["ptile_bin"], got["sum"]) == (want["n_valid"], want["median_bin"], want["ptile_bin"], want["sum"])
            host = {}
            for name in ("PHOTO", "TRUTH"):
                ts = []
                for _ in range(3):
                    reg.interpolate_mesh_begin(tris, h, w)
                    t0 = time.perf_counter()
                    d2, _ = reg.interpolate_mesh_end(copy=False)
                    if name == "PHOTO":
                        er.map_error(d2, er.PHOTO, KRKINV, KT, ref, cmp, BORDER, win_size=WIN)
                    else:
                        er.map_error(d2, er.TRUTH, truth=truth, relative=True, win_size=WIN)
                    ts.append((time.perf_counter() - t0) * 1e3)
                host[name] = float(np.median(ts))
            # the solver beside the stage
            reg.set_option(OPT_MESH_STATE, 1)
            reg.mesh_outputs(None, Kinv, h, w, want_filtered_map=True)
            n_iters = 20000
            stage, metric = EP(copy_out=False, **photo_kw), MP(want_mesh=True)

            def beside_map_error():
                reg.map_error_begin(stage, h, w)
                reg.map_error_end(copy=False)

            def beside_metric():
                reg.metric_outputs_begin(Kinv, h, w, pose=POSE, params=metric)
                reg.metric_outputs_end(copy=False)

            rates = {}
            for name, fn in (("alone", lambda: None), ("beside 10 map_error", beside_map_error), ("beside 10 metric_outputs", beside_metric),
                             ("alone again", lambda: None), ("beside 10 map_error again", beside_map_error)):
                rates[name] = solver_rate(flame_amd, reg, n_iters, fn)
        lines.append(f"{w}x{h} V={g['V']} T={len(tris)} coverage={cov / n:.2f} photo n_valid={got['n_valid']} median_bin={got['median_bin']} ptile_bin={got['ptile_bin']}")
        for name, (d, dmin, c, cmin, _) in rows.items():
            lines.append(f"  {name}: device_us {d:.1f} (min {dmin:.1f}) call_us {c:.1f} (min {cmin:.1f})")
        for name, ms in host.items():
            call = rows[f"{name} win 11, error map + statistics, copied out"][2]
            lines.append(f"  host path {name}: host_ms {ms:.1f}; ratio host / call (error map + statistics, copied out) {ms * 1e3 / call:.0f}x")
        lines.append("  solver, run_async(%d): " % n_iters + "; ".join(f"{k} {v / 1e3:.0f} k it/s" for k, v in rates.items()))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
