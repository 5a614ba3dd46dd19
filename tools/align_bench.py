"""Time of the direct alignment (flame_stereo_build_pyramid, flame_stereo_align_linearize, flame_stereo_align_frame) and of the same
linearisation made the way a caller had to before the stage existed.

    python tools/align_bench.py [--reps 30] [--out profiles/align.txt] [--commit HASH]
    python tools/align_bench.py --workload 20          (no timing: 20 rounds of the stage per size, for rocprofv3 --kernel-trace
                                                        --stats, no counters in that run)
    python tools/align_bench.py --trace-db DIR/NAME_results.db   (per kernel and grid: calls, median / least duration; host only)

pyramid  HIP events around the kernels of build_pyramid(5 levels) (flame_stereo_last_kernel_ms), median (min) over --reps builds of a
         frame added anew each time, after 5 warm-up rounds; `call` is the host's wall time of the call, which only enqueues.
linearise  per level: device = HIP events around the memset and the two kernels; call = wall time of the call, which enqueues, waits
         once and copies 248 bytes through pinned memory.  The map lies in device memory.  call - device is the host round trip.
align    a full align_frame (levels 4 -> 0 at 1080p, 3 -> 0 at 640x480) from a start a few pixels off: wall time, evaluations made.
host     download_frame of both frames + the numpy checker's linearisation at level 0 (tests/align_ref.py): wall time, median of 3.
         The checker is vectorised numpy, not a consumer's C++; it is the only other implementation the tree has: context, not a target.
solver   iterations per second of run_async(N) on a 640x480 graph with ten linearisations at level 0 issued beside it on the tracker's
         stream, against the run alone, taken in turn, best of 3.
Scene: tests/align_ref.make_scene -- a smooth texture, a smooth inverse depth around 0.5, a true pose of about 2 degrees; K = (0.8 w, 0.8
w, w / 2, h / 2).
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

KERNELS = ("k_pyr_down", "k_align_linearize", "k_align_finish")
SIZES = ((640, 480, 4), (1920, 1080, 5))  # (w, h, n_levels)


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
        short = next((k for k in KERNELS if k in name), None)
        if short is not None:
            rows[(short, int(gx) * int(gy))].append((end - start) / 1e3)
    return "\n".join("  %-20s grid %9d  calls %4d  median %7.2f  min %7.2f us" % (k, grid, len(v), float(np.median(v)), min(v))
                     for (k, grid), v in sorted(rows.items()))


def scene(w, h):
    from tests import align_ref as ar

    K = (0.8 * w, 0.8 * w, w / 2.0, h / 2.0)
    q = np.array([0.9998, 0.01, -0.012, 0.008])
    q /= np.linalg.norm(q)
    t = np.array([0.02, -0.015, 0.01])
    ref, new, d = ar.make_scene(w, h, K, q, t, seed=3, scale=w / 96.0)
    Km = np.array([K[0], 0, K[2], 0, K[1], K[3], 0, 0, 1], np.float32)
    Ki = np.array([1 / K[0], 0, -K[2] / K[0], 0, 1 / K[1], -K[3] / K[1], 0, 0, 1], np.float32)
    return K, Km, Ki, ref, new, d, q, t


def med(v):
    return float(np.median(v)), float(np.min(v))


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

    assert torch.cuda.is_available(), "align_bench.py measures on a GPU; there is no other path"
    import flame_amd
    from flame_amd import synth
    from flame_amd.stereo import AlignParams, FeatureTracker
    from tests import align_ref as ar

    ident = (np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3))
    if a.workload:
        for w, h, n_levels in SIZES:
            K, Km, Ki, ref, new, d, q, t = scene(w, h)
            dev = torch.from_numpy(d).cuda()
            torch.cuda.synchronize()
            with FeatureTracker(Km, Ki, w, h, border=5) as tr:
                for _ in range(a.workload):
                    tr.add_frame(1, ref)
                    tr.add_frame(2, new)
                    tr.build_pyramid(1, n_levels)
                    tr.build_pyramid(2, n_levels)
                    for level in range(n_levels):
                        tr.align_linearize(AlignParams(), 1, 2, level, int(dev.data_ptr()), q, t)
        return

    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:  # noqa: BLE001
            commit = "unknown"
    lines = [f"direct alignment: tools/align_bench.py --reps {a.reps}; tree at commit {commit} + this change",
             "device_us: HIP events on the tracker's stream around the call's kernels, median (min); call_us: wall time of the call, median (min); "
             "host_ms: 2 x download_frame + numpy checker at level 0, wall, median of 3"]
    for w, h, n_levels in SIZES:
        K, Km, Ki, ref, new, d, q, t = scene(w, h)
        dev = torch.from_numpy(d).cuda()
        torch.cuda.synchronize()
        ptr = int(dev.data_ptr())
        P = AlignParams()
        with FeatureTracker(Km, Ki, w, h, border=5) as tr:
            tr.add_frame(1, ref)
            pd, pc = [], []
            for r in range(a.reps + 5):
                tr.add_frame(2, new)  # (a frame added anew has no levels)
                t0 = time.perf_counter()
                tr.build_pyramid(2, n_levels)
                t1 = time.perf_counter()
                if r >= 5:
                    pd.append(tr.last_kernel_ms() * 1e3), pc.append((t1 - t0) * 1e6)
            tr.build_pyramid(1, n_levels)
            lines.append(f"{w}x{h}, {n_levels} levels")
            lines.append("  build_pyramid (levels 1 .. %d): device_us %.1f (min %.1f) call_us %.1f (min %.1f)" % ((n_levels - 1,) + med(pd) + med(pc)))
            for level in range(n_levels):
                ld, lc = [], []
                got = None
                for r in range(a.reps + 5):
                    t0 = time.perf_counter()
                    got = tr.align_linearize(P, 1, 2, level, ptr, q, t)
                    t1 = time.perf_counter()
                    if r >= 5:
                        ld.append(tr.last_kernel_ms() * 1e3), lc.append((t1 - t0) * 1e6)
                wl, hl = tr.level_size(level)
                lines.append("  linearise level %d (%dx%d, %d used): device_us %.1f (min %.1f) call_us %.1f (min %.1f)"
                             % ((level, wl, hl, got["n_used"]) + med(ld) + med(lc)))
            fa = []
            res = None
            PA = AlignParams(coarsest_level=n_levels - 1)
            for r in range(8):
                t0 = time.perf_counter()
                res = tr.align_frame(PA, 1, 2, ptr, *ident)
                if r >= 3:
                    fa.append((time.perf_counter() - t0) * 1e3)
            r0, t0_ = ar.pose_error(*ident, q, t)
            r1, t1_ = ar.pose_error(res["q"], res["t"], q, t)
            lines.append("  align_frame levels %d -> 0 from the identity: call_ms %.2f (min %.2f), %d evaluations, iters %s, status %d flags %d; "
                         "rotation error %.2e -> %.2e rad, translation error %.2e -> %.2e"
                         % ((n_levels - 1,) + med(fa) + (res["n_evals"], res["iters"][:n_levels], res["status"], res["flags"], r0, r1, t0_, t1_)))
            hs = []
            want = None
            for _ in range(3):
                t0 = time.perf_counter()
                a0, _, _ = tr.download_frame(1)
                b0, bx, by = tr.download_frame(2)
                s = slice(5, -5)
                want = ar.linearize(a0[s, s], (b0[s, s], bx[s, s], by[s, s]), d, 0, K, P.border, P.huber_k, q, t)
                hs.append((time.perf_counter() - t0) * 1e3)
            got = tr.align_linearize(P, 1, 2, 0, ptr, q, t)
            ar.assert_same_system(got, want, "the bench's own check")  # the result is the checker's
            lines.append("  host path, level 0: host_ms %.1f" % float(np.median(hs)))
            if w == 640:
                g = synth.make_graph("640x480", seed=31)
                with flame_amd.Regularizer(0) as reg:
                    reg.upload_graph(g)
                    n_iters = 20000
                    rates = {}

                    def beside():
                        tr.align_linearize(P, 1, 2, 0, ptr, q, t)

                    for name, fn in (("alone", lambda: None), ("beside 10 linearisations", beside), ("alone again", lambda: None),
                                     ("beside 10 linearisations again", beside)):
                        best = 0.0
                        for _ in range(3):
                            reg.sync()
                            t0 = time.perf_counter()
                            reg.run_async(flame_amd.Params(), n_iters)
                            for _ in range(10):
                                fn()
                            reg.sync()
                            best = max(best, n_iters / (time.perf_counter() - t0))
                        rates[name] = best
                lines.append("  solver, run_async(%d), V=%d: " % (n_iters, g["V"]) + "; ".join(f"{k} {v / 1e3:.0f} k it/s" for k, v in rates.items()))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
