"""Time of letting pose-frames go: flame_stereo_prune_pose_frames on the resident set against what a caller had to do
without it for the same effect (get_features, the loop on the host, set_features, drop_frame per pose-frame).

    python tools/prune_bench.py [--reps 30] [--warmup 5] [--out profiles/prune_pose_frames.txt] [--commit ID]

Cases: 8.4 k, 16 k and 57 k features at 640x480 (tests/prune_cases.py), half of them anchored in the two pose-frames
that go away.  Per case and repetition the two sides run alternately in one process on one context, after --warmup
unmeasured rounds; every figure is the median over --reps with the 10th and 90th percentile.

  prune kernels   HIP events around k_prune_move + k_prune_commit (flame_stereo_last_kernel_ms), for first_new = n (the
                  move is in place) and first_new = n / 2 (records are removed: the compaction runs)
  project kernels the same for flame_stereo_project_features on the same set -- the expectation to check is that the
                  prune costs about what projectFeatures costs for the same count
  prune call      wall clock of prune_pose_frames (tables up, kernels, one wait, frames released), first_new = n
  host way        wall clock of get_features + tests/prune_ref.prune_vectorised (whole-array numpy float32, NOT the
                  per-feature checker, which is far slower; a C++ loop would be faster than numpy) + set_features +
                  drop_frame x 2
The set is restored (set_features, add_frame of blank images) outside the timed regions.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pct(v):
    v = np.asarray(v, np.float64)
    return "%9.1f  [%8.1f .. %8.1f]" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="(not given)")
    a = ap.parse_args()

    import torch  # noqa: F401  (one HIP runtime per process: torch's)

    from flame_amd.stereo import FEATURE_DTYPE, FeatureTracker, StereoParams
    from tests import prune_cases as pc
    from tests import prune_ref as pr

    sc = pc.scene("640x480")
    keep, dropped, target = pc.split(2)
    poses = pc.dropped_poses(sc, dropped, target)
    geos = pc.dropped_geos(sc, dropped, target)
    all_poses = [dict(id=k, q_to_new=sc.relative(k, target)[0], t_to_new=sc.relative(k, target)[1]) for k in pc.PF_IDS]
    blank = np.zeros((sc.height, sc.width), np.uint8)
    sp = StereoParams()
    lines = ["prune_pose_frames vs the host way, %s, commit %s" % (torch.cuda.get_device_name(0), a.commit),
             "640x480, pose-frames %s kept, %s dropped, half of the features orphaned; %d reps after %d warm-up rounds, sides "
             "alternated; median [p10 .. p90] in microseconds" % (keep, dropped, a.reps, a.warmup), ""]
    for n in (8400, 16000, 57000):
        rng = np.random.default_rng(n)
        feats = pc.features(sc, n, seed=n, anchors=pc.PF_IDS)
        feats["frame_id"] = np.where(rng.random(n) < 0.5, rng.choice(dropped, n), rng.choice(keep, n)).astype(np.uint32)
        feats = np.ascontiguousarray(feats).view(FEATURE_DTYPE)
        orphaned = int(np.isin(feats["frame_id"], dropped).sum())
        t = dict(kernel_inplace=[], kernel_compact=[], kernel_project=[], call=[], host=[], host_get=[], host_loop=[],
                 host_set=[], host_drop=[])
        with FeatureTracker(sc.K32, sc.Kinv32, sc.width, sc.height, border=5) as tr:
            for k in pc.PF_IDS:
                tr.add_frame(k, blank)
            ref = None
            for r in range(a.warmup + a.reps):
                rec = r >= a.warmup
                # -- the device way
                tr.set_features(feats)
                t0 = time.perf_counter()
                st = tr.prune_pose_frames(sp, target, keep, poses, n)
                t1 = time.perf_counter()
                ms = tr.last_kernel_ms()
                out_dev = tr.get_features()
                for k in dropped:
                    tr.add_frame(k, blank)
                # -- the host way
                tr.set_features(feats)
                h0 = time.perf_counter()
                host = tr.get_features()
                h1 = time.perf_counter()
                out_host = pr.prune_vectorised(host, keep, geos, target, sc.width, sc.height, first_new=n)
                h2 = time.perf_counter()
                tr.set_features(np.ascontiguousarray(out_host))
                h3 = time.perf_counter()
                for k in dropped:
                    tr.drop_frame(k)
                h4 = time.perf_counter()
                for k in dropped:
                    tr.add_frame(k, blank)
                if ref is None:
                    assert out_dev.tobytes() == np.ascontiguousarray(out_host).tobytes(), "the two ways disagree"
                    ref = st
                # -- the compaction path and projectFeatures, device time only
                tr.set_features(feats)
                st2 = tr.prune_pose_frames(sp, target, keep, poses, n // 2)
                ms2 = tr.last_kernel_ms()
                for k in dropped:
                    tr.add_frame(k, blank)
                tr.set_features(feats)
                tr.project_features(sp, target, all_poses)
                ms3 = tr.last_kernel_ms()
                if rec:
                    t["kernel_inplace"].append(ms * 1e3)
                    t["kernel_compact"].append(ms2 * 1e3)
                    t["kernel_project"].append(ms3 * 1e3)
                    t["call"].append((t1 - t0) * 1e6)
                    t["host"].append((h4 - h0) * 1e6)
                    t["host_get"].append((h1 - h0) * 1e6)
                    t["host_loop"].append((h2 - h1) * 1e6)
                    t["host_set"].append((h3 - h2) * 1e6)
                    t["host_drop"].append((h4 - h3) * 1e6)
        lines += ["n = %d features, %d orphaned: %d moved, %d invalidated (first_new = n); %d removed with first_new = n / 2"
                  % (n, orphaned, ref["num_moved"], ref["num_invalidated"], st2["num_removed"]),
                  "  prune kernels, in place        %s" % pct(t["kernel_inplace"]),
                  "  prune kernels, with compaction %s" % pct(t["kernel_compact"]),
                  "  project kernels, same set      %s" % pct(t["kernel_project"]),
                  "  prune call (wall clock)        %s" % pct(t["call"]),
                  "  host way (wall clock)          %s" % pct(t["host"]),
                  "    get_features                 %s" % pct(t["host_get"]),
                  "    numpy loop                   %s" % pct(t["host_loop"]),
                  "    set_features                 %s" % pct(t["host_set"]),
                  "    drop_frame x %d               %s" % (len(dropped), pct(t["host_drop"])),
                  "  host way / prune call          %9.1f" % (np.median(t["host"]) / np.median(t["call"])), ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
