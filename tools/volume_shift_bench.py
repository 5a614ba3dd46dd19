"""Time of the volume's shift (flame_nltgv2_volume_shift_begin: the window moved over the grid, out of place) and of its yardsticks.

    python tools/volume_shift_bench.py [--reps 30] [--out profiles/volume_shift.txt] [--commit HASH]
    python tools/volume_shift_bench.py --workload 20        (no timing: per volume, 20 shifts of each path there and back, for a
                                                             kernel trace in a run of its own)
    python tools/volume_shift_bench.py --trace-csv DIR/NAME_kernel_trace.csv   (per kernel and volume: calls, median / least duration;
                                                             host only)

(a) device  a shift by (8, 0, 0) -- the 16-byte path -- by the HIP events around what begin enqueues on the side stream (device_ms of
            the view), median (min) over --reps calls after 3 warm-up calls; `call` is the host's wall time of begin + end.
    copy    a hipMemcpyDtoDAsync of the volume's bytes between two buffers of that size on a stream of this tool's, between two HIP
            events, the same number of calls with the same warm-up, in the same run, taken in turn with the shift: the copy reads
            and writes exactly the bytes the shift must move.  The shift is given a quarter over the copy's time (one range test and one
            weight compare per record, the fresh records, the counters and their way down); the line says whether it made it.
(b)         a shift by (3, -2, 1) -- the 8-byte path --, as a ratio to (a).
(c)         one integration of a 640x480 map into the same volume beside it, as a ratio to (a).
(d) host    the path the shift replaces: volume_download + a numpy roll and fill + volume_upload, wall time, median of 3.  The shift's
            volume must equal what that path gives, bit for bit.
(e) solver  iterations per second of run_async(N) with ten shifts issued beside it, against the run alone, taken in turn, best of 3.
Volumes: tools/volume_bench.py's cube, 128^3 and 256^3 voxels, holding its 640x480 scene after one integration.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from render_view_bench import cameras, scene, solver_rate  # noqa: E402
from volume_bench import POSE, VOXELS, volume_of  # noqa: E402

WIDE, NARROW = (8, 0, 0), (3, -2, 1)
ALLOWED = 1.25


def back(s):
    return tuple(-v for v in s)


class DeviceCopy:
    """hipMemcpyDtoDAsync of `nbytes` between two device buffers on a stream of its own, timed by HIP events."""

    def __init__(self, torch, nbytes):
        from tests.metric_helpers import hip_runtime

        self.hip = hip_runtime()
        self.nbytes = nbytes
        self.src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        self.dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.stream, self.ev0, self.ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.chk(self.hip.hipStreamCreateWithFlags(C.byref(self.stream), 1))  # hipStreamNonBlocking, as the side stream is
        self.chk(self.hip.hipEventCreate(C.byref(self.ev0)))
        self.chk(self.hip.hipEventCreate(C.byref(self.ev1)))

    @staticmethod
    def chk(rc):
        assert rc == 0, f"a HIP call failed with {rc}"

    def once(self):
        h = self.hip
        self.chk(h.hipEventRecord(self.ev0, self.stream))
        self.chk(h.hipMemcpyDtoDAsync(C.c_void_p(self.dst.data_ptr()), C.c_void_p(self.src.data_ptr()), C.c_size_t(self.nbytes), self.stream))
        self.chk(h.hipEventRecord(self.ev1, self.stream))
        self.chk(h.hipStreamSynchronize(self.stream))
        ms = C.c_float()
        self.chk(h.hipEventElapsedTime(C.byref(ms), self.ev0, self.ev1))
        return ms.value * 1e3

    def close(self):
        self.hip.hipEventDestroy(self.ev0), self.hip.hipEventDestroy(self.ev1), self.hip.hipStreamDestroy(self.stream)


def trace_stats(csv_path):
    """The shift's kernels in a kernel trace of --workload: it runs the volumes in turn, so a kernel's calls split evenly among them."""
    import collections
    import csv

    rows = collections.defaultdict(list)
    with open(csv_path, newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            if "k_volume_shift" in name or "k_volume_integrate" in name:
                name = name[name.index("k_volume"):].split("(")[0]
                rows[name].append(((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3, int(r["Start_Timestamp"])))
    lines = []
    for name, v in sorted(rows.items()):
        v = [d for d, _ in sorted(v, key=lambda q: q[1])]
        part = len(v) // len(VOXELS)
        for i, n in enumerate(VOXELS):
            q = v[i * part:(i + 1) * part]
            lines.append("  %-60s %d^3 calls %4d  median %8.2f  min %8.2f us: %5.0f GB/s read + written at the median" % (
                name[-60:], n, len(q), float(np.median(q)), min(q), 16.0 * n ** 3 / float(np.median(q)) / 1e3))
    return "\n".join(lines)


def shift_once(reg, s):
    t0 = time.perf_counter()
    reg.volume_shift_begin(s)
    out = reg.volume_shift_end()
    return out["device_ms"] * 1e3, (time.perf_counter() - t0) * 1e6, out


def stats(v):
    return float(np.median(v)), float(np.min(v))


def host_path(reg, s, n):
    """download + numpy + upload: destination (i, j, k) = source (i, j, k) + s, fresh elsewhere."""
    t0 = time.perf_counter()
    d = reg.volume_download()
    out = {"tsdf": np.ones_like(d["tsdf"]), "weight": np.zeros_like(d["weight"])}
    dst = [slice(max(0, -s[a]), min(n, n - s[a])) for a in range(3)]
    src = [slice(q.start + s[a], q.stop + s[a]) for a, q in enumerate(dst)]
    for k in out:
        out[k][dst[2], dst[1], dst[0]] = d[k][src[2], src[1], src[0]]
    reg.volume_upload(out["tsdf"], out["weight"])
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--workload", type=int, default=0)
    ap.add_argument("--trace-csv", default=None)
    a = ap.parse_args()
    if a.trace_csv:  # (host only: reads what an earlier traced run left)
        print(trace_stats(a.trace_csv))
        return

    import torch  # noqa: F401  (one HIP runtime per process: torch's)

    assert torch.cuda.is_available(), "volume_shift_bench.py measures on a GPU; there is no other path"
    import flame_amd
    from flame_amd import synth
    from flame_amd.regularizer import OPT_MESH_STATE

    w, h = 640, 480
    g, tris = scene(synth, w, h)
    _, K = cameras(w, h)
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:  # noqa: BLE001
            commit = "unknown"
    lines = []
    with flame_amd.Regularizer(0) as reg:
        info = reg.info()
        reg.upload_graph(g)
        reg.run(flame_amd.Params(), 200)
        reg.interpolate_mesh(tris, h, w)
        for n in VOXELS:
            reg.volume_create(flame_amd.VolumeParams(**volume_of(n)))
            seen = reg.volume_integrate(K, POSE, h, w)["updated"]
            if a.workload:
                for _ in range(a.workload):
                    for s in (WIDE, back(WIDE), NARROW, back(NARROW)):
                        reg.volume_shift(s)
                continue
            nbytes = 8 * n ** 3
            copy = DeviceCopy(torch, nbytes)
            wide, wide_call, narrow, copies, integ = [], [], [], [], []
            paths = set()
            for r in range(a.reps + 3):  # in turn, so that all of them meet the same clocks
                c = copy.once()
                s1, call, o1 = shift_once(reg, WIDE if r % 2 == 0 else back(WIDE))
                s2, _, o2 = shift_once(reg, NARROW if r % 2 == 0 else back(NARROW))
                reg.volume_integrate_begin(K, POSE, h, w)
                i = reg.volume_integrate_end()["device_ms"] * 1e3
                if r >= 3:
                    copies.append(c), wide.append(s1), wide_call.append(call), narrow.append(s2), integ.append(i)
                    paths.add((o1["record_bytes"], o2["record_bytes"]))
            copy.close()
            assert paths == {(16, 8)}, paths
            (cm, cmin), (wm, wmin), (nm, nmin), (im, imin) = stats(copies), stats(wide), stats(narrow), stats(integ)
            verdict = "within" if wm <= ALLOWED * cm else "OVER"
            lines.append(f"{n}^3 ({nbytes} bytes, {seen} voxels seen by the first integration)")
            lines.append(f"  (a) shift {WIDE}, 16-byte path: device_us {wm:.1f} (min {wmin:.1f}) call_us {stats(wide_call)[0]:.1f}; "
                         f"{2 * nbytes / wm / 1e3:.0f} GB/s read + written")
            lines.append(f"      hipMemcpyDtoDAsync of the same bytes: device_us {cm:.1f} (min {cmin:.1f}); shift / copy = {wm / cm:.3f} "
                         f"(min / min {wmin / cmin:.3f}): {verdict} the {ALLOWED:.2f} allowed")
            lines.append(f"  (b) shift {NARROW}, 8-byte path: device_us {nm:.1f} (min {nmin:.1f}); (b) / (a) = {nm / wm:.3f}")
            lines.append(f"  (c) one integration of the {w}x{h} map beside it: device_us {im:.1f} (min {imin:.1f}); (a) / integration = {wm / im:.3f}")
            # (d) the host path, and the shift against it bit for bit
            reg.volume_reset()
            reg.volume_integrate(K, POSE, h, w)
            start = reg.volume_download()
            host_ms = []
            for _ in range(3):
                reg.volume_upload(start["tsdf"], start["weight"])
                ms, want = host_path(reg, NARROW, n)
                host_ms.append(ms)
            reg.volume_upload(start["tsdf"], start["weight"])
            reg.volume_shift(NARROW)
            got = reg.volume_download()
            for k in want:
                assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
            lines.append(f"  (d) host path, volume_download + numpy + volume_upload: {float(np.median(host_ms)):.1f} ms "
                         f"(the shift's volume equals it bit for bit): {float(np.median(host_ms)) * 1e3 / nm:.0f} x the shift")
        if not a.workload:
            # (e) the solver beside ten shifts
            reg.set_option(OPT_MESH_STATE, 1)
            reg.volume_create(flame_amd.VolumeParams(**volume_of(VOXELS[0])))
            reg.volume_integrate(K, POSE, h, w)
            turn = [0]

            def beside():
                turn[0] += 1
                reg.volume_shift_begin(WIDE if turn[0] % 2 else back(WIDE))
                reg.volume_shift_end()

            n_iters = 20000
            rates = {name: solver_rate(flame_amd, reg, n_iters, fn) for name, fn in
                     (("alone", lambda: None), (f"beside 10 shifts ({VOXELS[0]}^3)", beside), ("alone again", lambda: None))}
            lines.append("(e) solver, run_async(%d): " % n_iters + "; ".join(f"{k} {v / 1e3:.0f} k it/s" for k, v in rates.items()))
    if a.workload:
        return
    head = [f"volume shift: tools/volume_shift_bench.py --reps {a.reps}; tree at commit {commit} + this change; {info['device_name']} {info['gcn_arch']}",
            "device_us: HIP events around what is enqueued, median (min); the copy and the shifts taken in turn in one run"]
    text = "\n".join(head + lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
