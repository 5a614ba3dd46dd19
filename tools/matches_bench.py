"""Time of the matches picture (flame_stereo_draw_matches, getDebugImageMatches), of the update with recording on against off, and of
the host path the stage replaces.

    python tools/matches_bench.py [--reps 30] [--out profiles/matches.txt] [--commit HASH] [--no-host] [--kernel-stats DIR ...]
    rocprofv3 --kernel-trace --stats -d DIR -o kt --output-format csv -- python tools/matches_bench.py --draw-only 640x480

draw     flame_stereo_last_kernel_ms (HIP events on the context's stream: two memsets, count, offsets, the counters' copy, fill,
         fold) and the call's wall time, over --reps calls after warm-up: median, minimum, maximum.
update   update_resident on the same resident set with FLAME_STEREO_OPT_RECORD_MATCHES off and on, alternating in one process (the set
         is restored before every call): device time of the update kernel (the records' memset is outside the events) and the call.
host     what the stage replaces, once: get_features + the sequential Python walk tests/matches_ref.py on the frame's input (it calls
         the oracle's C routines per feature).  Context, not a target; the same run checks that both give the same bytes.
kernels  with --kernel-stats DIR (one per size, from the rocprofv3 command above): average time per kernel.
Sizes: 640x480 with about 8.4 k features and 1920x1080 with about 57 k, on flame_amd.synth_stereo.standard_scene.
"""
from __future__ import annotations

import argparse
import csv
import glob
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = {"640x480": (640, 480, 4200), "1920x1080": (1920, 1080, 28500)}


def make_case(name):
    from flame_amd import synth_stereo as ss
    from flame_amd.stereo import FEATURE_DTYPE

    w, h, n_per_anchor = SIZES[name]
    sc = ss.standard_scene(w, h)
    imgs = {c: sc.render(c) for c in (10, 11, 12)}
    feats = ss.make_features(sc, FEATURE_DTYPE, [10, 11], n_per_anchor, 7)
    return sc, imgs, feats, ss.poses_for(sc, [10, 11], 12, 11)


def stats3(v):
    return "median %.1f (min %.1f, max %.1f)" % (float(np.median(v)), float(np.min(v)), float(np.max(v)))


def kernel_lines(name, d):
    f = sorted(glob.glob(d + "/**/*kernel_stats.csv", recursive=True))
    if not f:
        return ["%s kernels: no kernel_stats.csv under %s" % (name, d)]
    rows = [r for r in csv.DictReader(open(f[0])) if any(k in r["Name"] for k in ("k_match_", "k_draw_offsets", "k_update_feature"))]
    out = []
    for r in sorted(rows, key=lambda r: r["Name"]):
        n = r["Name"].replace("flame_hip::(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        out.append("%s (calls %d) %.1f" % (n, int(r["Calls"]), float(r["AverageNs"]) / 1e3))
    return ["%s kernels, rocprofv3 --kernel-trace --stats over --draw-only, average us: " % name + ", ".join(out)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--no-host", action="store_true", help="skip the sequential Python walk (tens of seconds at 1080p)")
    ap.add_argument("--draw-only", default=None, metavar="SIZE", help="one update and 12 draw_matches calls at SIZE, nothing else")
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="SIZE=DIR")
    a = ap.parse_args()

    import torch  # noqa: F401  (one HIP runtime per process: torch's)

    from flame_amd.stereo import FeatureTracker, StereoParams

    P = StereoParams()
    if a.draw_only:
        sc, imgs, feats, poses = make_case(a.draw_only)
        with FeatureTracker(sc.K32, sc.Kinv32, sc.width, sc.height) as tr:
            for fid, img in imgs.items():
                tr.add_frame(fid, img)
            tr.set_record_matches(True)
            tr.set_features(feats)
            tr.update_resident(P, 12, 11, poses)
            for _ in range(12):
                pic = tr.draw_matches()
        print("draw-only", a.draw_only, pic["kind_count"], pic["entries"])
        return

    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:  # noqa: BLE001
            commit = "unknown"
    lines = ["matches picture: tools/matches_bench.py --reps %d; tree at commit %s + this change" % (a.reps, commit),
             "device_us: HIP events on the context's stream; call_us: wall time of the call; host_ms: get_features + the sequential "
             "Python walk, once; every figure over %d calls after 5 warm-up calls" % a.reps]
    for name in SIZES:
        sc, imgs, feats, poses = make_case(name)
        n = feats.shape[0]
        with FeatureTracker(sc.K32, sc.Kinv32, sc.width, sc.height) as tr:
            for fid, img in imgs.items():
                tr.add_frame(fid, img)
            dev = {0: [], 1: []}
            call = {0: [], 1: []}
            for r in range(a.reps + 5):
                for on in (0, 1):
                    tr.set_record_matches(on)
                    tr.set_features(feats)
                    t0 = time.perf_counter()
                    _, st = tr.update_resident(P, 12, 11, poses)
                    t1 = time.perf_counter()
                    if r >= 5:
                        dev[on].append(tr.last_kernel_ms() * 1e3), call[on].append((t1 - t0) * 1e6)
            after = tr.get_features()
            ddev, dcall, refills = [], [], 0
            for r in range(a.reps + 5):
                t0 = time.perf_counter()
                pic = tr.draw_matches()
                t1 = time.perf_counter()
                refills += pic["refilled"]
                if r >= 5:
                    ddev.append(tr.last_kernel_ms() * 1e3), dcall.append((t1 - t0) * 1e6)
            host_ms = None
            if not a.no_host:
                from oracle import stereo_capi as so
                from tests import matches_ref as mr

                t0 = time.perf_counter()
                tr.get_features()
                frames = [dict(p, img_pad=so.make_frame(imgs[p["id"]], 5)[0]) for p in poses]
                walk = feats.copy().view(so.FEATURE_DTYPE)
                ref = mr.update_and_draw(so.Params(), sc.K32, sc.Kinv32, sc.width, sc.height, 5, frames, so.make_frame(imgs[12], 5),
                                         imgs[12], 11, walk)
                host_ms = (time.perf_counter() - t0) * 1e3
                assert ref["rc"] == 0 and walk.tobytes() == after.tobytes(), "the walk's records differ from the update's"
                assert np.array_equal(ref["img"], pic["img"]) and ref["kind_count"] == pic["kind_count"], "the picture differs from the checker"
        failing = n - st["num_idepth_updates"]
        lines.append("%s %d features, %d (%.1f %%) not updated this frame; draws by kind %s, %d segments, %d entries (%.3f per pixel)"
                     % (name, n, failing, 100.0 * failing / n, pic["kind_count"], pic["lines_drawn"], pic["entries"],
                        pic["entries"] / (sc.width * sc.height)))
        lines.append("%s draw_matches: device_us %s call_us %s; calls that refilled: %d of %d" % (name, stats3(ddev), stats3(dcall), refills,
                                                                                               a.reps + 5))
        for on in (0, 1):
            lines.append("%s update_resident, recording %s: device_us %s call_us %s" % (name, "on" if on else "off", stats3(dev[on]),
                                                                                       stats3(call[on])))
        lines.append("%s update, recording on / off: device %.3f, call %.3f (medians)" % (name, np.median(dev[1]) / np.median(dev[0]),
                                                                                       np.median(call[1]) / np.median(call[0])))
        if host_ms is not None:
            lines.append("%s host path (get_features + sequential Python walk): host_ms %.0f, same bytes; draw_matches call is %.0fx shorter"
                         % (name, host_ms, host_ms * 1e3 / float(np.median(dcall))))
    for spec in a.kernel_stats:
        size, d = spec.split("=", 1)
        lines += kernel_lines(size, d)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
