"""Time of the volume's surface extraction (flame_nltgv2_volume_mesh: marching tetrahedra over the truncated-signed-distance volume) and of
its yardsticks.

    python tools/volume_mesh_bench.py [--reps 20] [--out profiles/volume_mesh.txt] [--commit HASH]

device   HIP events around what begin enqueues on the context's side stream (device_ms and pass_ms of the view), median (min .. max) over
         --reps calls after 3 warm-up calls, with copy_out = 0 and exactly the capacities a count query gave; `call` is the host's wall
         time of begin + end.
bytes    what each pass must move at least, over its device time, against 6.3 TB/s:
           classify  8 B read + 1 B written per voxel (the seven neighbours' records are the next rows', met again in cache)
           count     1 B read + 5 B written per voxel (14 neighbours' bytes from cache), 8 B per workgroup
           scan      8 B read + 8 B written per workgroup
           emit      2 B read per voxel; per vertex 24 B written (position, normal) and the records of the gradients' taps; per triangle
                     12 B written
yardstick  the integration of the same map into the same volume, from the same run: a pass that only classifies should not cost several
         integrations.
host     the path it replaces: volume_download + the numpy checker (tests/volume_mesh_ref.py): wall time, once, at 128^3, where the
         stage's mesh must equal the checker's bit for bit.
solver   iterations per second of run_async(N) with ten extractions (128^3) issued beside it, against the run alone, taken in turn,
         best of 3.
Scene: tools/volume_bench.py's -- the 640x480 synth graph after 200 iterations, integrated once into a cube of 1.6 m of 128^3 and 256^3
voxels.
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
from volume_bench import ACHIEVABLE, POSE, VOXELS, timed, volume_of  # noqa: E402

PASSES = ("classify", "count", "scan", "emit")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()

    import torch  # noqa: F401  (one HIP runtime per process: torch's)

    assert torch.cuda.is_available(), "volume_mesh_bench.py measures on a GPU; there is no other path"
    import flame_amd
    from flame_amd import synth
    from flame_amd.regularizer import OPT_MESH_STATE
    from tests import volume_mesh_ref as mr
    from tests import volume_ref as vr

    VP, MP = flame_amd.VolumeParams, flame_amd.VolumeMeshParams
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:  # noqa: BLE001
            commit = "unknown"
    w, h = 640, 480
    g, tris = scene(synth, w, h)
    Kinv, K = cameras(w, h)
    lines = []
    with flame_amd.Regularizer(0) as reg:
        info = reg.info()
        reg.upload_graph(g)
        reg.run(flame_amd.Params(), 200)
        dense = reg.interpolate_mesh(tris, h, w)[0]
        lines.append(f"{w}x{h} map, V={g['V']} T={len(tris)}")
        for n in VOXELS:
            vol = volume_of(n)
            reg.volume_create(VP(**vol))
            d, dmin, c, cmin, out = timed(lambda: reg.volume_integrate_begin(K, POSE, h, w), reg.volume_integrate_end, a.reps)
            lines.append(f"  {n}^3 integrate (the yardstick): device_us {d:.1f} (min {dmin:.1f}) call_us {c:.1f} (min {cmin:.1f}); updated {out['updated']}")
            integrate_us = d
            q = reg.volume_mesh(MP(copy_out=False))
            nv, nt = q["n_vertices"], q["n_triangles"]
            p = MP(max_vertices=nv, max_triangles=nt, copy_out=False)
            dev, call, passes = [], [], []
            for r in range(a.reps + 3):
                t0 = time.perf_counter()
                reg.volume_mesh_begin(p)
                m = reg.volume_mesh_end()
                t1 = time.perf_counter()
                if r >= 3:
                    dev.append(m["device_ms"] * 1e3), call.append((t1 - t0) * 1e6), passes.append(m["pass_ms"] * 1e3)
            passes = np.array(passes)
            nvox, nblk = n ** 3, (n ** 3 + 255) // 256
            least = dict(classify=9 * nvox, count=6 * nvox + 8 * nblk, scan=16 * nblk, emit=2 * nvox + 24 * nv + 12 * nt)
            lines.append(f"  {n}^3 mesh: device_us {np.median(dev):.1f} (min {np.min(dev):.1f} .. max {np.max(dev):.1f}) call_us {np.median(call):.1f} "
                         f"(min {np.min(call):.1f}); counters {m['counts'][:5].tolist()}; {np.median(dev) / integrate_us:.2f} integrations")
            for i, name in enumerate(PASSES):
                us = float(np.median(passes[:, i]))
                lines.append(f"      {name:9s} {us:8.1f} us (min {passes[:, i].min():.1f} .. max {passes[:, i].max():.1f}); at least {least[name]} bytes: "
                             f"{least[name] / us / 1e3:.0f} GB/s = {least[name] / (us * 1e-6) / ACHIEVABLE:.3f} of 6.3 TB/s; {us / integrate_us:.2f} integrations")
            t0 = time.perf_counter()
            full = reg.volume_mesh()
            t1 = time.perf_counter()
            lines.append(f"      to the host (a count query, then the call with copy_out = 1): {1e3 * (t1 - t0):.2f} ms wall, "
                         f"{24 * nv + 12 * nt} bytes of mesh")
            if n == VOXELS[0]:
                t0 = time.perf_counter()
                down = reg.volume_download()
                t1 = time.perf_counter()
                ref = vr.Volume(**vol)
                ref.tsdf, ref.weight = down["tsdf"], down["weight"]
                want = mr.extract(ref)
                t2 = time.perf_counter()
                mr.assert_same_mesh(full, want, f"{n}^3")  # the stage gives what the checker gives, bit for bit
                lines.append(f"      host path: volume_download {1e3 * (t1 - t0):.1f} ms + numpy marching tetrahedra {1e3 * (t2 - t1):.0f} ms "
                             f"(the stage's mesh equals the checker's, bit for bit)")
        reg.set_option(OPT_MESH_STATE, 1)
        n_iters = 20000
        reg.volume_create(VP(**volume_of(VOXELS[0])))
        reg.volume_integrate(K, POSE, h, w)
        q = reg.volume_mesh(MP(copy_out=False))
        p = MP(max_vertices=q["n_vertices"], max_triangles=q["n_triangles"], copy_out=False)

        def beside_mesh():
            reg.volume_mesh_begin(p)
            reg.volume_mesh_end()

        rates = {}
        for name, fn in (("alone", lambda: None), ("beside 10 extractions (128^3)", beside_mesh), ("alone again", lambda: None)):
            rates[name] = solver_rate(flame_amd, reg, n_iters, fn)
        lines.append("  solver, run_async(%d): " % n_iters + "; ".join(f"{k} {v / 1e3:.0f} k it/s" for k, v in rates.items()))
    del dense
    head = [f"volume mesh: tools/volume_mesh_bench.py --reps {a.reps}; tree at commit {commit} + this change; {info['device_name']} {info['gcn_arch']}",
            "device_us: HIP events on the side stream around what begin enqueues, median (min .. max); call_us: wall time of begin + end; "
            "one form was built: neighbour taps through the caches, no brick staged in LDS"]
    text = "\n".join(head + lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
