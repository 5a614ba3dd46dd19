"""Time of the volumetric map's two stages (flame_nltgv2_volume_integrate: one inverse-depth map folded into the truncated-signed-distance
volume; flame_nltgv2_volume_raycast: the volume seen from a camera) and of their yardsticks.

    python tools/volume_bench.py [--reps 20] [--out profiles/volume.txt] [--commit HASH]
    python tools/volume_bench.py --workload 10          (no timing: per map size and volume, 10 rounds of integrate, raycast and
                                                         metric_outputs, for rocprofv3 --kernel-trace --stats, no counters in that run)
    python tools/volume_bench.py --trace-db DIR/NAME_results.db   (per kernel and grid: calls, median / least duration, the integration per
                                                         map size and volume; host only)

device   HIP events around what begin enqueues on the context's side stream (device_ms of the two views), median (min) over --reps calls
         after 3 warm-up calls; the raycast with copy_out = 0; `call` is the host's wall time of begin + end.
bytes    an integration loads and stores 8 bytes of every voxel it updates and nothing of the others: 16 B per updated voxel, with the
         share of the voxels updated beside it, over the device time, against 6.3 TB/s.  The map's pixels (4 B per voxel in the image, mostly
         from cache) are not counted.
yardstick  the metric outputs' pixel kernel (depth alone, copy_out = 0) over the same map: the project's streaming kernel of that size.
host     the path the integration replaces: metric_outputs with the depth image brought down + the numpy integration
         (tests/volume_ref.py): wall time, once, at 128^3.  The stage's volume must equal the checker's on the resident map, bit for bit.
solver   iterations per second of run_async(N) with ten calls of each stage issued beside it, against the run alone, taken in turn,
         best of 3.
Scene: tools/render_view_bench.py's -- the 8480 vertices of the 640x480 synth graph over half of a 640x480 and of a 1920x1080 map, after
200 iterations --, in a cube of 1.6 m that holds it, 128^3 and 256^3 voxels; the raycast marches one voxel per step through the cube.
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

KERNELS = ("k_volume_fill", "k_volume_integrate", "k_volume_raycast", "k_metric_pixels")
SIZES = ((640, 480), (1920, 1080))
VOXELS = (128, 256)
EXTENT, ORIGIN = 1.6, (-1.4, -0.8, 0.5)
ACHIEVABLE = 6.3e12  # bytes per second a streaming kernel reaches on this part


def volume_of(n):
    return dict(nx=n, ny=n, nz=n, voxel_size=EXTENT / n, origin=ORIGIN, trunc=0.1, max_weight=1e6)


def raycast_of(n):
    return dict(z_near=0.4, dz=EXTENT / n, n_steps=int(np.ceil(1.8 * n / 1.6)))


POSE = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)


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
        lines.append("  %-20s grid %9d calls %5d  median %9.2f  min %9.2f us" % (k, grid, len(v), float(np.median(v)), min(v)))
        if k == "k_volume_integrate" and len(v) % (len(SIZES) * len(VOXELS)) == 0:
            # its grid is kIntegrateGrid workgroups whatever the volume: --workload runs, per map size, the volumes in turn
            part = len(v) // (len(SIZES) * len(VOXELS))
            for i, (size, n) in enumerate((size, n) for size in SIZES for n in VOXELS):
                q = v[i * part:(i + 1) * part]
                lines.append("      %dx%d map into %d^3: median %9.2f  min %9.2f us, %.4f ns per voxel visited" % (
                    size[0], size[1], n, float(np.median(q)), min(q), float(np.median(q)) * 1e3 / float(n) ** 3))
    return "\n".join(lines)


def timed(begin, end, reps):
    dev, call = [], []
    out = None
    for r in range(reps + 3):
        t0 = time.perf_counter()
        begin()
        out = end()
        t1 = time.perf_counter()
        if r >= 3:
            dev.append(out["device_ms"] * 1e3), call.append((t1 - t0) * 1e6)
    return float(np.median(dev)), float(np.min(dev)), float(np.median(call)), float(np.min(call)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--workload", type=int, default=0)
    ap.add_argument("--trace-db", default=None)
    a = ap.parse_args()
    if a.trace_db:  # (host only: reads what an earlier traced run left)
        print(trace_stats(a.trace_db))
        return

    import torch  # noqa: F401  (one HIP runtime per process: torch's)

    assert torch.cuda.is_available(), "volume_bench.py measures on a GPU; there is no other path"
    import flame_amd
    from flame_amd import synth
    from flame_amd.regularizer import OPT_MESH_STATE
    from tests import volume_ref as vr

    VP, RP, MP = flame_amd.VolumeParams, flame_amd.RaycastParams, flame_amd.MetricParams

    def prepared(reg, g, tris, h, w):
        reg.upload_graph(g)
        reg.run(flame_amd.Params(), 200)
        return reg.interpolate_mesh(tris, h, w)[0]

    depth_only = MP(want_depth=True, want_depth_mm=False, want_organized=False, want_cloud=False, copy_out=False)

    if a.workload:
        for w, h in SIZES:
            g, tris = scene(synth, w, h)
            Kinv, K = cameras(w, h)
            with flame_amd.Regularizer(0) as reg:
                prepared(reg, g, tris, h, w)
                for n in VOXELS:
                    reg.volume_create(VP(**volume_of(n)))
                    rp = RP(copy_out=False, **raycast_of(n))
                    for _ in range(a.workload):
                        reg.volume_integrate(K, POSE, h, w)
                        reg.volume_raycast_begin(Kinv, POSE, h, w, rp)
                        reg.volume_raycast_end(copy=False)
                        reg.metric_outputs_begin(Kinv, h, w, params=depth_only)
                        reg.metric_outputs_end(copy=False)
        return

    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:  # noqa: BLE001
            commit = "unknown"
    info = None
    lines = []
    for w, h in SIZES:
        g, tris = scene(synth, w, h)
        Kinv, K = cameras(w, h)
        with flame_amd.Regularizer(0) as reg:
            info = info or reg.info()
            dense = prepared(reg, g, tris, h, w)
            yd, ydmin, _, _, _ = timed(lambda: reg.metric_outputs_begin(Kinv, h, w, params=depth_only), lambda: reg.metric_outputs_end(copy=False), a.reps)
            px_bytes = 8 * w * h
            lines.append(f"{w}x{h} map, V={g['V']} T={len(tris)}; yardstick k_metric_pixels stage (depth alone, copy_out = 0): device_us {yd:.1f} (min {ydmin:.1f}), "
                         f"{px_bytes} bytes read + written: {px_bytes / yd / 1e3:.0f} GB/s")
            for n in VOXELS:
                vol = volume_of(n)
                reg.volume_create(VP(**vol))
                d, dmin, c, cmin, out = timed(lambda: reg.volume_integrate_begin(K, POSE, h, w), reg.volume_integrate_end, a.reps)
                share = out["updated"] / float(n) ** 3
                nbytes = 16 * out["updated"]
                lines.append(f"  {n}^3 integrate: device_us {d:.1f} (min {dmin:.1f}) call_us {c:.1f} (min {cmin:.1f}); counters {out['counts'][:6].tolist()}; "
                             f"updated {share:.3f} of the voxels, {nbytes} bytes: {nbytes / d / 1e3:.0f} GB/s = {nbytes / (d * 1e-6) / ACHIEVABLE:.3f} of 6.3 TB/s; "
                             f"{d * 1e3 / float(n) ** 3:.4f} ns per voxel visited")
                rp = RP(copy_out=False, **raycast_of(n))
                d, dmin, c, cmin, out = timed(lambda: reg.volume_raycast_begin(Kinv, POSE, h, w, rp), lambda: reg.volume_raycast_end(copy=False), a.reps)
                lines.append(f"  {n}^3 raycast ({rp.n_steps} steps of {rp.dz:.5f}): device_us {d:.1f} (min {dmin:.1f}) call_us {c:.1f} (min {cmin:.1f}); "
                             f"hits {out['hits']} back {out['back']} empty {out['empty']} of {w * h}")
                if n == VOXELS[0]:
                    reg.volume_reset()
                    reg.volume_integrate(K, POSE, h, w)
                    t0 = time.perf_counter()
                    m = reg.metric_outputs(Kinv, h, w, params=MP(want_depth_mm=False, want_organized=False, want_cloud=False))["depth"]
                    t1 = time.perf_counter()
                    host = vr.Volume(**vol)
                    with np.errstate(all="ignore"):
                        host.integrate((np.float32(1.0) / m).astype(np.float32), K, POSE)
                    t2 = time.perf_counter()
                    ref = vr.Volume(**vol)
                    ref.integrate(dense, K, POSE)
                    vr.assert_same_volume(reg.volume_download(), ref, f"{w}x{h} {n}^3")  # the stage gives what the checker gives, bit for bit
                    lines.append(f"  {n}^3 host path: metric_outputs with the depth image brought down {1e3 * (t1 - t0):.2f} ms + numpy integration "
                                 f"{1e3 * (t2 - t1):.1f} ms (the stage's volume equals the checker's on the resident map, bit for bit)")
            reg.set_option(OPT_MESH_STATE, 1)
            n_iters = 20000
            rp = RP(copy_out=False, **raycast_of(VOXELS[0]))
            reg.volume_create(VP(**volume_of(VOXELS[0])))

            def beside_integrate():
                reg.volume_integrate_begin(K, POSE, h, w)
                reg.volume_integrate_end()

            def beside_raycast():
                reg.volume_raycast_begin(Kinv, POSE, h, w, rp)
                reg.volume_raycast_end(copy=False)

            rates = {}
            for name, fn in (("alone", lambda: None), ("beside 10 integrations (128^3)", beside_integrate), ("beside 10 raycasts (128^3)", beside_raycast),
                             ("alone again", lambda: None)):
                rates[name] = solver_rate(flame_amd, reg, n_iters, fn)
        lines.append("  solver, run_async(%d): " % n_iters + "; ".join(f"{k} {v / 1e3:.0f} k it/s" for k, v in rates.items()))
    head = [f"volumetric map: tools/volume_bench.py --reps {a.reps}; tree at commit {commit} + this change; {info['device_name']} {info['gcn_arch']}",
            "device_us: HIP events on the side stream around what begin enqueues, median (min); call_us: wall time of begin + end, median (min); "
            "bytes: 16 per updated voxel"]
    text = "\n".join(head + lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
