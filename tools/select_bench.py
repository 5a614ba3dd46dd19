"""Time of selecting the graph's vertices: flame_stereo_select_graph_features on the resident and the projected set
against what a caller had to do without it (get_features + get_projected + the selection in numpy + building the four
arrays of flame_nltgv2_sync_input).

    python tools/select_bench.py [--reps 30] [--warmup 5] [--out profiles/graph_inputs.txt] [--commit ID]

Cases: 8.4 k, 16 k and 61 k features (tests/select_cases.py: 10 % invalid, half above the variance threshold, half below
the height band, 3 % above it or not finite, 17 % selected), brought into the resident set by set_features +
project_features, which keeps about three quarters of them (all valid).  After a warm-up of every size the sides run
alternately, repetition by repetition, in one process on one context; every figure is the median over --reps with the
10th and 90th percentile, in microseconds.

  select kernels    HIP events around k_select_flag + k_select_scatter (flame_stereo_last_kernel_ms)
  select call       host clock around the resident C-ABI call, which ends in its own wait; for both ways of copying out
                    (FLAME_STEREO_OPT_GRAPH_COPY 0: one block, sections n apart, one wait; 1: counters, then 24 V bytes)
  arrays call       the same on two host arrays of the ORIGINAL n records (two uploads of 40 n bytes on top)
  project call      flame_stereo_project_features on the same context, kernels and host clock: the expectation to check
                    is that the selection costs about what projectFeatures costs
  host way          get_features + get_projected + tests/select_ref.select (whole-array numpy float32 on one core; a
                    C++ loop would be faster than numpy, so the numpy line is context and the round trip is the part
                    no loop can avoid)
Kernel times by name come from a run of their own:  rocprofv3 --kernel-trace --stats -- python tools/select_bench.py
--reps 10 (no counter collection in that run).
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

    import ctypes as C

    from flame_amd.stereo import FEATURE_DTYPE, FeatureTracker, GraphParams, StereoParams, _FeatureStats, _GraphInputs, _lib
    from tests import select_cases as sc_
    from tests import select_ref as sr

    sp, gp, L = StereoParams(), GraphParams(), _lib()
    sizes = (8400, 16000, 61000)
    lines = ["select_graph_features vs the host way, %s, commit %s" % (torch.cuda.get_device_name(0), a.commit),
             "default graph parameters, graph_scale 1; %d reps after %d warm-up rounds of every size, sides alternated; "
             "median [p10 .. p90] in microseconds" % (a.reps, a.warmup), ""]
    trackers = {}
    for n in sizes:
        case = sc_.make(n)
        sc = case["sc"]
        key = (sc.width, sc.height)
        if key not in trackers:
            trackers[key] = FeatureTracker(sc.K32, sc.Kinv32, sc.width, sc.height, border=5)
    results = {n: dict(kernel=[], call0=[], call1=[], arrays0=[], arrays1=[], proj_kernel=[], proj_call=[], host=[], host_get=[],
                       host_numpy=[]) for n in sizes}
    info = {}
    for phase, rounds in (("warmup", a.warmup), ("timed", a.reps)):
        for r in range(rounds):
            for n in sizes:
                case = sc_.make(n)
                sc, world = case["sc"], case["world"]
                tr = trackers[(sc.width, sc.height)]
                feats, proj = np.ascontiguousarray(case["feats"]).view(FEATURE_DTYPE), np.ascontiguousarray(case["proj"]).view(FEATURE_DTYPE)
                poses = sc_.project_poses(sc)
                t = results[n]
                # (the raw C-ABI calls are timed, with their arguments built beforehand: the mirror's packing of the pose
                # lists and its numpy copies of the result are Python's cost, not the call's)
                pose_arr, world_arr = tr._poses(poses), tr._world_poses(world)
                fst, gout = _FeatureStats(), _GraphInputs()
                tr.set_features(feats)
                p0 = time.perf_counter()
                rc = L.flame_stereo_project_features(tr._ctx, C.byref(sp), sc_.CUR, len(poses), pose_arr, C.byref(fst))
                p1 = time.perf_counter()
                assert rc == 0
                m = fst.num_features
                pk = tr.last_kernel_ms()
                call, res = {}, {}
                for mode in (0, 1):
                    tr.set_graph_copy(mode)
                    c0 = time.perf_counter()
                    rc = L.flame_stereo_select_graph_features(tr._ctx, C.byref(gp), 1.0, len(world), world_arr, C.byref(gout))
                    c1 = time.perf_counter()
                    assert rc == 0
                    call[mode] = (c1 - c0) * 1e6
                    if mode == 0:
                        sk = tr.last_kernel_ms()
                    res[mode] = tr.select_graph_features(gp, 1.0, world)  # (untimed: the copies, for the comparison below)
                    # -- the host way, alternated
                    if mode == 0:
                        h0 = time.perf_counter()
                        hf = tr.get_features()
                        hp = tr.get_projected()
                        h1 = time.perf_counter()
                        rc, ref = sr.select(hf, hp, sc.Kinv32, world, 1.0)
                        h2 = time.perf_counter()
                arr = {}
                for mode in (0, 1):
                    tr.set_graph_copy(mode)
                    c0 = time.perf_counter()
                    rc = L.flame_stereo_select_graph_features_arrays(tr._ctx, C.byref(gp), 1.0, len(world), world_arr, n,
                                                                     feats.ctypes.data, proj.ctypes.data, C.byref(gout))
                    arr[mode] = (time.perf_counter() - c0) * 1e6
                    assert rc == 0
                out_a = dict(V=int(gout.V), num_invalid=int(gout.num_invalid))
                tr.set_graph_copy(0)
                if n not in info:
                    for mode in (0, 1):
                        for k in sr.ARRAYS:
                            assert res[mode][k].tobytes() == ref[k].tobytes(), "the two ways disagree: %s" % k
                    info[n] = "n = %d features, %d resident after the projection: %d selected, %d variance, %d height; arrays form on " \
                              "all %d: %d selected, %d invalid" % (n, m, ref["V"], ref["num_fail_var"], ref["num_fail_height"], n,
                                                                   out_a["V"], out_a["num_invalid"])
                if phase == "timed":
                    t["kernel"].append(sk * 1e3)
                    t["call0"].append(call[0])
                    t["call1"].append(call[1])
                    t["arrays0"].append(arr[0])
                    t["arrays1"].append(arr[1])
                    t["proj_kernel"].append(pk * 1e3)
                    t["proj_call"].append((p1 - p0) * 1e6)
                    t["host"].append((h2 - h0) * 1e6)
                    t["host_get"].append((h1 - h0) * 1e6)
                    t["host_numpy"].append((h2 - h1) * 1e6)
    for tr in trackers.values():
        tr.close()
    for n in sizes:
        t = results[n]
        best = min(np.median(t["call0"]), np.median(t["call1"]))
        lines += [info[n],
                  "  select kernels                      %s" % pct(t["kernel"]),
                  "  select call, one block (copy 0)     %s" % pct(t["call0"]),
                  "  select call, count first (copy 1)   %s" % pct(t["call1"]),
                  "  arrays call, one block (copy 0)     %s" % pct(t["arrays0"]),
                  "  arrays call, count first (copy 1)   %s" % pct(t["arrays1"]),
                  "  project kernels                     %s" % pct(t["proj_kernel"]),
                  "  project call                        %s" % pct(t["proj_call"]),
                  "  host way                            %s" % pct(t["host"]),
                  "    get_features + get_projected      %s" % pct(t["host_get"]),
                  "    numpy selection + the four arrays %s" % pct(t["host_numpy"]),
                  "  select call (copy 0) / project call %9.2f" % (np.median(t["call0"]) / np.median(t["proj_call"])),
                  "  select call (copy 1) / project call %9.2f" % (np.median(t["call1"]) / np.median(t["proj_call"])),
                  "  select kernels / project kernels    %9.2f" % (np.median(t["kernel"]) / np.median(t["proj_kernel"])),
                  "  host way / faster select call       %9.1f" % (np.median(t["host"]) / best),
                  "  round trip alone / faster select    %9.1f" % (np.median(t["host_get"]) / best), ""]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
