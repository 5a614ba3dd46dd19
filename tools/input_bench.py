"""Time of the raw-frame input stage (flame_stereo_add_raw_frame) and of the entry point it stands beside (flame_stereo_add_frame).

    python tools/input_bench.py [--reps 300] [--out profiles/input_stage.txt]
    python tools/input_bench.py --add-frame-only [--reps 300]      (flame_stereo_add_frame alone, through plain ctypes: works with
                                                                     FLAME_AMD_LIBRARY on a build that has no raw-frame symbols)
    python tools/input_bench.py --workload 40                      (no timing: the stage's launches and the metric pixel pass, for
                                                                     rocprofv3 --kernel-trace --stats)
    python tools/input_bench.py --trace-db DIR/NAME_results.db     (per kernel and grid: calls, median and least duration of that trace)

host     per-call wall time of add_frame and of add_raw_frame(GREY8, remap 0, host source): both upload pageable memory and wait
         for the stream; median over --reps calls after 20 warm-up calls.
device   add_raw_frame from a device buffer, enqueue-only (stats NULL): host_us is the wall time of the call alone (the stream is
         drained, untimed, after every call), device_us the HIP events around its two kernels (flame_stereo_last_kernel_ms).
checker  the host path the stage replaces, as far as this tree has one: the numpy checker (tests/input_ref.py) + add_frame.  A real
         host path (cv::cvtColor + cv::undistort) is compiled code and faster than numpy; no OpenCV is here to time.
solver   iterations per second of run_async(N) with ten add_raw_frame calls (device source, enqueue-only) issued beside it, against
         ten add_frame calls beside it and against the run alone, taken in turn, best of 3.
Sizes: 640x480 (from a 752x480 raw frame where the map runs) and 1920x1080 (from 1920x1080).
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # bytes / s, the data sheet's
WARM = 20
RATIONAL = (0.4, -0.1, 1e-3, 5e-4, 0.02, 0.2, -0.05, 0.01)
SIZES = {(640, 480): ((752, 480), (458.654, 457.296, 367.215, 248.375), (525.0, 525.0, 319.5, 239.5), (-0.2834, 0.0740, 1.9e-4, 1.8e-5)),
         (1920, 1080): ((1920, 1080), (1400.0, 1398.0, 959.5, 539.5), (1400.0, 1398.0, 959.5, 539.5), (-0.2834, 0.0740, 1.9e-4, 1.8e-5))}
# per output size: the raw size, the raw camera, the working camera, the raw camera's radial-tangential coefficients; the rational
# model's eight coefficients (tests/test_gpu_raw_frame.py's `rational` case) are the same at both sizes


def cam(fx, fy, cx, cy):
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
    Kinv = np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]], np.float64)
    return K.astype(np.float32), Kinv.astype(np.float32)


def median_us(ts):
    return float(np.median(ts)) * 1e6, float(np.min(ts)) * 1e6


def add_frame_only(reps):
    """flame_stereo_add_frame through plain ctypes, so that the same code times any build of the library."""
    import flame_amd

    L = C.CDLL(flame_amd.library_path())
    FP = C.POINTER(C.c_float)
    L.flame_stereo_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    L.flame_stereo_set_camera.argtypes = [C.c_void_p, FP, FP, C.c_int, C.c_int, C.c_int]
    L.flame_stereo_add_frame.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int]
    L.flame_stereo_destroy.argtypes = [C.c_void_p]
    out = []
    for (w, h), (_, _, c, _) in SIZES.items():
        K, Kinv = cam(*c)
        ctx = C.c_void_p()
        assert L.flame_stereo_create(C.byref(ctx), 0) == 0
        assert L.flame_stereo_set_camera(ctx, K.ctypes.data_as(FP), Kinv.ctypes.data_as(FP), w, h, 5) == 0
        img = np.random.RandomState(3).randint(0, 256, size=(h, w)).astype(np.uint8)
        ts = []
        for r in range(reps + WARM):
            t0 = time.perf_counter()
            rc = L.flame_stereo_add_frame(ctx, r & 1, img.ctypes.data, w)
            t1 = time.perf_counter()
            assert rc == 0
            if r >= WARM:
                ts.append(t1 - t0)
        L.flame_stereo_destroy(ctx)
        med, mn = median_us(ts)
        out.append(f"{w}x{h} add_frame: call_us {med:.1f} (min {mn:.1f})")
    return os.path.basename(flame_amd.library_path()) + ": " + "; ".join(out)


def trace_stats(db_path):
    """Per kernel of interest and grid size: calls, median / min duration in us, from the database rocprofv3 --kernel-trace writes."""
    import collections
    import sqlite3

    db = sqlite3.connect(db_path)
    rows = collections.defaultdict(list)
    for name, grid, start, end in db.execute("select name, grid_x, start, end from kernels"):
        short = next((k for k in ("k_input_rectify", "k_frame_pad_gradient", "k_metric_pixels") if k in name), None)
        if short is None:
            continue
        if "<" in name:
            short += name[name.index("<"):name.index(">") + 1]
        rows[(short, int(grid))].append((end - start) / 1e3)
    return "\n".join("  %-48s grid %8d  calls %4d  median %6.2f  min %6.2f us" % (k[0], k[1], len(v), float(np.median(v)), min(v))
                     for k, v in sorted(rows.items()))


def raw_frame(rng, rw, rh, bpp, pad=0):
    return rng.randint(0, 256, size=(rh, rw * bpp + pad)).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--add-frame-only", action="store_true")
    ap.add_argument("--workload", type=int, default=0)
    ap.add_argument("--trace-db", default=None)
    a = ap.parse_args()
    if a.trace_db:  # (host only: reads what an earlier traced run left)
        print(trace_stats(a.trace_db))
        return

    import torch  # (one HIP runtime per process: torch's)

    assert torch.cuda.is_available(), "input_bench.py measures on a GPU; there is no other path"
    if a.add_frame_only:
        print(add_frame_only(a.reps), flush=True)
        return

    import flame_amd
    from flame_amd import stereo as st
    from flame_amd import synth
    from tests import input_ref as ir

    rng = np.random.RandomState(5)

    def device_frame(raw):
        d = torch.from_numpy(raw).cuda()
        torch.cuda.synchronize()
        return d

    if a.workload:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import metric_outputs_bench as mb

        for (w, h), ((rw, rh), craw, c, dist) in SIZES.items():
            K, Kinv = cam(*c)
            Kraw, _ = cam(*craw)
            with st.FeatureTracker(K, Kinv, w, h) as tr:
                for fmt, remap, dd in ((st.FMT_BGRA8, 1, RATIONAL), (st.FMT_BGR8, 1, dist), (st.FMT_GREY8, 0, ())):
                    size = (rw, rh) if remap else (w, h)
                    dev = device_frame(raw_frame(rng, size[0], size[1], st.FORMAT_BYTES[fmt]))
                    tr.set_input(format=fmt, remap=remap, raw_width=size[0], raw_height=size[1], K_raw=Kraw, dist=dd)
                    for r in range(a.workload):
                        tr.add_raw_frame(r & 1, None, device_ptr=dev.data_ptr(), want_stats=False)
                    tr.download_frame(0)
                    del dev
            g, tris = mb.scene(synth, w, h)
            Kinv_m = np.array([[1 / (0.82 * w), 0, -0.5], [0, 1 / (0.82 * w), -0.5 * h / w], [0, 0, 1]], np.float32)
            with flame_amd.Regularizer(0) as reg:
                mb.prepare(flame_amd, reg, g, tris, Kinv_m, h, w)
                for _ in range(a.workload):
                    reg.metric_outputs_begin(Kinv_m, h, w, pose=mb.POSE, params=flame_amd.MetricParams(want_cloud=False, copy_out=False))
                    reg.metric_outputs_end(copy=False)
        return

    lines = [f"raw-frame input stage: tools/input_bench.py --reps {a.reps}",
             "call_us: wall time of the call (host sources wait for the stream); host_us: wall time of an enqueue-only call; device_us: "
             "HIP events around k_input_rectify + k_frame_pad_gradient; medians (min)"]
    for (w, h), ((rw, rh), craw, c, dist) in SIZES.items():
        K, Kinv = cam(*c)
        Kraw, _ = cam(*craw)
        n = w * h
        lines.append(f"{w}x{h}")
        with st.FeatureTracker(K, Kinv, w, h) as tr:
            img = raw_frame(rng, w, h, 1)
            # 1. host sources
            ts = {"add_frame": [], "add_raw_frame GREY8 remap 0, host": []}
            tr.set_input(format=st.FMT_GREY8, remap=0, raw_width=w, raw_height=h)
            for r in range(a.reps + WARM):
                for name in ts:  # in turn, call by call
                    t0 = time.perf_counter()
                    if name == "add_frame":
                        tr.add_frame(r & 1, img)
                    else:
                        tr.add_raw_frame(r & 1, img, want_stats=False)
                    t1 = time.perf_counter()
                    if r >= WARM:
                        ts[name].append(t1 - t0)
            for name, v in ts.items():
                lines.append("  %s: call_us %.1f (min %.1f)" % ((name,) + median_us(v)))
            add_frame_us = median_us(ts["add_frame"])[0]
            # 2. device sources, enqueue-only; 3. the kernel's bytes
            for label, fmt, remap, dd in (("GREY8 remap 0", st.FMT_GREY8, 0, ()), ("BGRA8 remap 0", st.FMT_BGRA8, 0, ()),
                                          ("BGR8 radial-tangential %dx%d" % (rw, rh), st.FMT_BGR8, 1, dist),
                                          ("BGRA8 rational %dx%d" % (rw, rh), st.FMT_BGRA8, 1, RATIONAL)):
                size = (rw, rh) if remap else (w, h)
                bpp = st.FORMAT_BYTES[fmt]
                raw = raw_frame(rng, size[0], size[1], bpp)
                dev = device_frame(raw)
                tr.set_input(format=fmt, remap=remap, raw_width=size[0], raw_height=size[1], K_raw=Kraw, dist=dd)
                host, devt = [], []
                for r in range(a.reps + WARM):
                    t0 = time.perf_counter()
                    tr.add_raw_frame(r & 1, None, device_ptr=dev.data_ptr(), want_stats=False)
                    t1 = time.perf_counter()
                    ms = tr.last_kernel_ms()  # (waits for the second event: the stream is drained, untimed)
                    if r >= WARM:
                        host.append(t1 - t0), devt.append(ms * 1e-3)
                n_outside = tr.add_raw_frame(0, None, device_ptr=dev.data_ptr(), want_stats=True)["n_outside"]
                hm, dm = median_us(host), median_us(devt)
                rect_bytes = size[0] * size[1] * bpp + n            # raw read once, one byte written per pixel
                stage_bytes = rect_bytes + 10 * n                   # + k_frame_pad_gradient: 1 read, 1 + 4 + 4 written per pixel
                lines.append(f"  add_raw_frame {label}, device source: host_us {hm[0]:.1f} (min {hm[1]:.1f}) device_us {dm[0]:.1f} "
                             f"(min {dm[1]:.1f}); {n_outside} outside; the two kernels must move {stage_bytes / 1e6:.1f} MB "
                             f"({rect_bytes / 1e6:.1f} of them the rectification) -> {stage_bytes / (dm[0] * 1e-6) / 1e12:.2f} TB/s over "
                             f"the event time; add_frame's call is {add_frame_us / hm[0]:.0f}x the enqueue, {add_frame_us / dm[0]:.1f}x the device time")
                del dev
            # 4. the host path it replaces: numpy checker + add_frame (BGR8, the camera's own distortion)
            p = dict(remap=1, raw_width=rw, raw_height=rh, K_raw=Kraw, dist=np.float32(dist))
            raw = raw_frame(rng, rw, rh, 3)
            tsc = []
            for _ in range(3):
                t0 = time.perf_counter()
                grey, _ = ir.rectify(raw, ir.BGR8, p, K, Kinv, w, h)
                tr.add_frame(0, grey)
                tsc.append(time.perf_counter() - t0)
            tr.set_input(format=st.FMT_BGR8, **p)
            tsr = []
            for r in range(20):
                t0 = time.perf_counter()
                tr.add_raw_frame(1, raw, want_stats=False)
                tsr.append(time.perf_counter() - t0)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(tr.download_frame(0), tr.download_frame(1)))
            lines.append(f"  host path (numpy checker + add_frame), BGR8 {rw}x{rh}: {np.median(tsc) * 1e3:.1f} ms; add_raw_frame of the same "
                         f"frame from the host: call_us {np.median(tsr[5:]) * 1e6:.1f}; same bytes")
            # 5. the solver beside it
            g = synth.make_graph("640x480", seed=31)
            dev = device_frame(raw_frame(rng, rw, rh, 4))
            tr.set_input(format=st.FMT_BGRA8, remap=1, raw_width=rw, raw_height=rh, K_raw=Kraw, dist=RATIONAL)
            with flame_amd.Regularizer(0) as reg:
                reg.upload_graph(g)
                reg.run(flame_amd.Params(), 200)
                n_iters = 20000

                def rate(beside):
                    best = 0.0
                    for _ in range(3):
                        reg.sync()
                        t0 = time.perf_counter()
                        reg.run_async(flame_amd.Params(), n_iters)
                        for k in range(10):
                            beside(k)
                        reg.sync()
                        best = max(best, n_iters / (time.perf_counter() - t0))
                    tr.last_kernel_ms()  # (drains the tracker's stream)
                    return best

                tr.add_frame(0, img), tr.add_frame(1, img)
                rates = {}
                for name, fn in (("alone", lambda k: None),
                                 ("beside 10 add_raw_frame", lambda k: tr.add_raw_frame(k & 1, None, device_ptr=dev.data_ptr(), want_stats=False)),
                                 ("beside 10 add_frame", lambda k: tr.add_frame(k & 1, img)), ("alone again", lambda k: None)):
                    rates[name] = rate(fn)
            del dev
            lines.append("  solver, run_async(%d) on the 640x480 graph: " % n_iters + "; ".join(f"{k} {v / 1e3:.0f} k it/s" for k, v in rates.items()))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
