"""Time of the detections picture (flame_stereo_draw_detections, getDebugImageDetections) and of the host path it replaces.

    python tools/detections_bench.py [--reps 30] [--out profiles/detections.txt] [--commit HASH]

kernel   flame_stereo_last_kernel_ms (HIP events on the context's stream around the stats memset and k_draw_detections), median
         and minimum over --reps calls after warm-up; beside it the bytes the kernel must move, width * height * (8 + 1 + 3) (two
         gradient floats and the grey byte in, three bytes out), and the rate that makes of the median.
call     the host's wall time of the whole call (validation, enqueue, the picture's copy to pageable host memory, one wait).
draw_features  flame_stereo_draw_features at the same size on the same box (memsets + claim + paint; its picture moves
         width * height * (4 + 4 + 1 + 3) bytes plus the claims), as the nearest existing stage.
host     what the call replaces, in the same run: download_frame (both padded gradients and the padded image come down) + the
         numpy checker tests/detections_ref.py (score + colours + blend): wall time, median of 3.  numpy, not the reference's C++:
         context, not a target.  The picture it makes must equal the device's.
Sizes: 640x480 and 1920x1080, a textured plane (flame_amd.synth_stereo), reference parameters, max_score 0.005 and 64.
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

    from flame_amd import synth_stereo as ss
    from flame_amd.stereo import FEATURE_DTYPE, DetectParams, FeatureTracker, StereoParams
    from oracle import stereo_capi as so
    from tests import detections_ref as dt

    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:  # noqa: BLE001
            commit = "unknown"
    lines = [f"detections picture: tools/detections_bench.py --reps {a.reps}; tree at commit {commit} + this change",
             "kernel_us: HIP events around the stats memset and k_draw_detections, median (min); bytes: width * height * (8 + 1 + 3); call_us: "
             "wall time of flame_stereo_draw_detections; host_ms: download_frame + numpy checker, wall, median of 3"]
    pad = 5
    for w, h in ((640, 480), (1920, 1080)):
        sc = ss.PlaneScene(w, h, seed=5, normal=(0.2, -0.1, 1.0), distance=2.2)
        sc.add_camera(9, ss.rot([0, 1, 0], -0.004), [0.03, -0.002, 0.01])
        sc.add_camera(10, np.eye(3), [0, 0, 0])
        img = sc.render(10)
        q, t = sc.relative(10, 9)
        geo = so.load_geometry(sc.K32, sc.Kinv32, q, t)
        sp, dp = StereoParams(), DetectParams()
        bytes_moved = w * h * 12
        with FeatureTracker(sc.K32, sc.Kinv32, w, h, border=pad) as tr:
            tr.add_frame(10, img)
            for max_score in (0.005, 64.0):
                ker, call = [], []
                for r in range(a.reps + 5):
                    t0 = time.perf_counter()
                    got, st = tr.draw_detections(sp, dp, 10, q, t, max_score=max_score)
                    t1 = time.perf_counter()
                    if r >= 5:
                        ker.append(tr.last_kernel_ms() * 1e3), call.append((t1 - t0) * 1e6)
                k_med = float(np.median(ker))
                lines.append(f"{w}x{h} draw_detections max_score {max_score:g}, {st['num_scored']} of {st['num_examined']} pixels scored: "
                             f"kernel_us {k_med:.1f} (min {np.min(ker):.1f}) for {bytes_moved / 1e6:.2f} MB = {bytes_moved / k_med / 1e6:.2f} TB/s; "
                             f"call_us {np.median(call):.1f}")
            # the nearest existing stage at the same size: draw_features over a projected set of one feature per 16 x 16 cell
            ys, xs = np.mgrid[8:h - 8:16, 8:w - 8:16]
            feats = np.zeros(xs.size, FEATURE_DTYPE)
            feats["id"], feats["frame_id"], feats["valid"] = np.arange(xs.size), 10, 1
            feats["x"], feats["y"] = xs.ravel(), ys.ravel()
            feats["idepth_mu"], feats["idepth_var"] = 0.45, 0.001
            tr.set_features(feats)
            n_proj = tr.project_features(sp, 10, [dict(id=10, q_to_new=[1, 0, 0, 0], t_to_new=[0, 0, 0])])
            fk, fc = [], []
            for r in range(a.reps + 5):
                t0 = time.perf_counter()
                tr.draw_features(10, 0.01)
                t1 = time.perf_counter()
                if r >= 5:
                    fk.append(tr.last_kernel_ms() * 1e3), fc.append((t1 - t0) * 1e6)
            lines.append(f"{w}x{h} draw_features, {n_proj} projected features: kernels_us {np.median(fk):.1f} (min {np.min(fk):.1f}) "
                         f"call_us {np.median(fc):.1f}")
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                img_pad, gx, gy = tr.download_frame(10)
                rc, _, score = dt.detection_score(gx, gy, pad, w, h, geo)
                want = dt.draw_detections(img_pad[pad:pad + h, pad:pad + w], score, 64.0)
                host.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0 and np.array_equal(want, got), "the picture differs from the checker"
            lines.append(f"{w}x{h} host path (download_frame + numpy checker, same bytes): host_ms {np.median(host):.1f}; ratio host / device "
                         f"call {np.median(host) * 1e3 / np.median(call):.0f}x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
