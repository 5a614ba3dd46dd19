"""Device time of projectFeatures and detectFeatures on the resident set (flame_stereo_project_features /
flame_stereo_detect_features), with the same-box CPU checker time (tests/frontend_ref.py) as context.

    python tools/frontend_bench.py [--reps 50] [--json out.json]

Device time = HIP events around the stage's kernels on the context's stream (flame_stereo_last_kernel_ms), after warm-up;
the median over --reps calls is reported.  Cases: detect at 640x480 and 1920x1080 (PlaneScene, win 16), project for 4 k
and 16 k features.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()

    import torch  # noqa: F401  (one HIP runtime per process: torch's)

    from flame_amd import synth_stereo as ss
    from flame_amd.stereo import FEATURE_DTYPE, DetectParams, FeatureTracker, StereoParams
    from oracle import stereo_capi as so
    from tests import frontend_ref as fr

    rows = []
    for w, h in ((640, 480), (1920, 1080)):
        sc = ss.PlaneScene(w, h, seed=5)
        sc.add_camera(9, ss.rot([0, 1, 0], -0.004), [0.03, -0.002, 0.01])
        sc.add_camera(10, np.eye(3), [0, 0, 0])
        img = sc.render(10)
        q, t = sc.relative(10, 9)
        with FeatureTracker(sc.K32, sc.Kinv32, w, h, border=5) as tr:
            tr.add_frame(10, img)
            ms = []
            for r in range(a.reps + 5):
                tr.set_features(np.zeros(0, FEATURE_DTYPE))
                n = tr.detect_features(StereoParams(), DetectParams(), 10, q, t)
                if r >= 5:
                    ms.append(tr.last_kernel_ms())
            t0 = time.perf_counter()
            for _ in range(10):
                tr.set_features(np.zeros(0, FEATURE_DTYPE))
                tr.detect_features(StereoParams(), DetectParams(), 10, q, t)
            call_us = (time.perf_counter() - t0) / 10 * 1e6
        _, gx, gy = so.make_frame(img, 5)
        geo = so.load_geometry(sc.K32, sc.Kinv32, q, t)
        t0 = time.perf_counter()
        for _ in range(3):
            fr.detect_features(gx, gy, 5, w, h, geo, 10, dtype=so.FEATURE_DTYPE)
        cpu_ms = (time.perf_counter() - t0) / 3 * 1e3
        rows.append(dict(stage="detect", size="%dx%d" % (w, h), new_features=n, device_us=float(np.median(ms)) * 1e3,
                         device_us_min=float(np.min(ms)) * 1e3, call_us=call_us, cpu_checker_ms=cpu_ms,
                         bytes_floor_mb=8.0 * w * h / 1e6))

    sc = ss.standard_scene(1920, 1080)
    poses = [dict(id=a_, q_to_new=sc.relative(a_, 12)[0], t_to_new=sc.relative(a_, 12)[1]) for a_ in (10, 11)]
    for n_target in (4096, 16384):
        feats = ss.make_features(sc, FEATURE_DTYPE, [10, 11], n_target // 2, 3)
        with FeatureTracker(sc.K32, sc.Kinv32, 1920, 1080, border=5) as tr:
            ms = []
            for r in range(a.reps + 5):
                tr.set_features(feats)
                kept = tr.project_features(StereoParams(), 12, poses)
                if r >= 5:
                    ms.append(tr.last_kernel_ms())
        geos = {a_: so.load_geometry(sc.K32, sc.Kinv32, *sc.relative(a_, 12)) for a_ in (10, 11)}
        ofeats = feats.view(so.FEATURE_DTYPE)
        t0 = time.perf_counter()
        for _ in range(3):
            fr.project_features(ofeats, geos, 12, 1920, 1080)
        cpu_ms = (time.perf_counter() - t0) / 3 * 1e3
        rows.append(dict(stage="project", features=int(feats.shape[0]), kept=kept, device_us=float(np.median(ms)) * 1e3,
                         device_us_min=float(np.min(ms)) * 1e3, cpu_checker_ms=cpu_ms))
    for r in rows:
        print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
