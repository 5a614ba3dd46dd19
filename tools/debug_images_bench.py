"""Time of the debug-image stages (flame_nltgv2_debug_images: idepth colours, w1 / w2 maps, normals; flame_stereo_draw_features;
flame_nltgv2_debug_wireframe) and of the same pictures made the way a host had to before the stages existed.

    python tools/debug_images_bench.py [--reps 30] [--out profiles/debug_images.txt] [--commit HASH] [--no-host-wireframe]

device   HIP events around the stage on the context's side stream (kernels and the copies out; flame_nltgv2_debug_images_view
         .device_ms), median over --reps calls after warm-up, with the frame's image in device memory and in host memory; `call` is
         the host's wall time of begin + end for the same calls.  draw_features: the kernels' HIP-event time and the call.
host     what the stage replaces, in the same run: interpolate_mesh (rasteriser + the map's way down) + download_state(x, w1, w2) +
         get_projected + two host rasterisations (the raster checker, C) + numpy colouring of the three pictures
         (tests/debug_ref.py): wall time, median of 3.  The colouring is numpy, not the reference's C++: context, not a target.
wireframe  flame_nltgv2_debug_wireframe with the validity mesh_outputs left on the device and the image in device memory: device and
         call as above, the entries (pixel visits of all lines) and whether a call had to refill.  Its host path: download_state(x) +
         mesh_outputs (validity) + the sequential Python restatement tests/wireframe_ref.py, once: context, not a target.
solver   iterations per microsecond of run_async beside nothing, beside ten mesh_outputs calls, beside ten debug_images calls and
         beside ten debug_wireframe calls (FLAME_NLTGV2_OPT_MESH_STATE = 1, so that no stage waits for the run).
Sizes: 640x480 and 1920x1080 (flame_amd.synth graphs, scipy Delaunay triangles), 200 solver iterations first.
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
    ap.add_argument("--no-host-wireframe", action="store_true", help="skip the sequential Python wireframe (tens of seconds at 1080p)")
    a = ap.parse_args()

    import torch  # noqa: F401  (one HIP runtime per process: torch's)

    import flame_amd
    from flame_amd import synth
    from flame_amd.regularizer import OPT_MESH_STATE
    from flame_amd.stereo import FEATURE_DTYPE, FeatureTracker, StereoParams
    from oracle import capi as oracle
    from tests import debug_ref as dr
    from tests import wireframe_ref as wr

    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:  # noqa: BLE001
            commit = "unknown"
    lines = [f"debug image stage: tools/debug_images_bench.py --reps {a.reps}; tree at commit {commit} + this change",
             "device_us: HIP events on the side stream (kernels + copies out), median; call_us: wall time of begin + end; host_ms: "
             "interpolate_mesh + download_state + get_projected + 2 host rasterisations + numpy colouring, wall, median of 3"]
    rng = np.random.default_rng(3)
    for config in ("640x480", "1920x1080"):
        w, h, _ = synth.CONFIGS[config]
        g = synth.make_graph(config, seed=31)
        tris = synth.delaunay_triangles_scipy(g["pos"])
        K = np.array([[0.82 * w, 0, 0.5 * w], [0, 0.82 * w, 0.5 * h], [0, 0, 1]], np.float32)
        Kinv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        n_feats = g["V"]
        feats = np.zeros(n_feats, FEATURE_DTYPE)
        feats["id"], feats["frame_id"], feats["valid"] = np.arange(n_feats), 10, 1
        feats["x"], feats["y"] = g["pos"][:, 0], g["pos"][:, 1]
        feats["idepth_mu"] = np.maximum(g["data_term"], 0.01)
        feats["idepth_var"] = rng.random(n_feats).astype(np.float32) * 0.02
        params = flame_amd.Params()
        p = flame_amd.DebugImageParams()
        with flame_amd.Regularizer(0) as reg, FeatureTracker(K, Kinv, w, h) as tr:
            tr.add_frame(11, img)
            tr.set_features(feats)
            n_proj = tr.project_features(StereoParams(), 11, [dict(id=10, q_to_new=[1, 0, 0, 0], t_to_new=[0, 0, 0])])
            ptr, step = tr.frame_image_device(11)
            reg.upload_graph(g)
            reg.run(params, 200)
            reg.interpolate_mesh(tris, h, w, graph_scale=1.1)
            res = {}
            for where in ("device", "host"):
                dev, call = [], []
                for r in range(a.reps + 5):
                    t0 = time.perf_counter()
                    if where == "device":
                        reg.debug_images_begin(None, K, h, w, p, img_device=ptr, step_bytes=step)
                    else:
                        reg.debug_images_begin(img, K, h, w, p)
                    out = reg.debug_images_end(copy=False)
                    t1 = time.perf_counter()
                    if r >= 5:
                        dev.append(out["device_ms"] * 1e3), call.append((t1 - t0) * 1e6)
                res[where] = (float(np.median(dev)), float(np.min(dev)), float(np.median(call)))
            fk, fc = [], []
            for r in range(a.reps + 5):
                t0 = time.perf_counter()
                _, nc, nu = tr.draw_features(11, 0.01)
                t1 = time.perf_counter()
                if r >= 5:
                    fk.append(tr.last_kernel_ms() * 1e3), fc.append((t1 - t0) * 1e6)
            # the wireframe, with the validity the filters leave on the device
            wp = flame_amd.WireframeParams(validity=2)
            n_valid = reg.mesh_outputs(None, Kinv, h, w, graph_scale=1.1)["n_valid"]
            wdev, wcall, wrefills = [], [], 0
            for r in range(a.reps + 5):
                t0 = time.perf_counter()
                reg.debug_wireframe_begin(None, h, w, 1.1, wp, img_device=ptr, step_bytes=step)
                wout = reg.debug_wireframe_end(copy=False)
                t1 = time.perf_counter()
                wrefills += wout["refilled"]
                if r >= 5:
                    wdev.append(wout["device_ms"] * 1e3), wcall.append((t1 - t0) * 1e6)
            whost_ms = None
            if not a.no_host_wireframe:
                t0 = time.perf_counter()
                st = reg.download_state(("x",))
                mo = reg.mesh_outputs(None, Kinv, h, w, graph_scale=1.1)
                wref, _, _ = wr.draw_wireframe(img, tris, g["pos"], mo["vtx_idepth"], mo["tri_valid"])
                whost_ms = (time.perf_counter() - t0) * 1e3
                assert st["x"].shape == mo["vtx_idepth"].shape and np.array_equal(wref, wout["wireframe_img"]), "the wireframe differs from the checker"
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                dense, _ = reg.interpolate_mesh(tris, h, w, graph_scale=1.1)
                st = reg.download_state(("x", "w1", "w2"))
                proj = tr.get_projected()
                w1m = oracle.raster_interpolate_mesh(tris, g["pos"], st["w1"], h, w)
                w2m = oracle.raster_interpolate_mesh(tris, g["pos"], st["w2"], h, w)
                dr.draw_inverse_depth_map(img, dense, 1.0)
                dr.draw_normals(img, K, dense, w1m, w2m)
                dr.draw_features(img, proj, 0.01)
                host.append((time.perf_counter() - t0) * 1e3)
            host_ms = float(np.median(host))
            # the solver beside the stage
            reg.set_option(OPT_MESH_STATE, 1)
            n_iters = 30000
            rate = {}
            reg.mesh_outputs(None, Kinv, h, w, graph_scale=1.1)  # (interpolate_mesh above handed the triangles in again: validity for them)
            for beside in ("nothing", "mesh_outputs", "debug_images", "debug_wireframe"):
                best = 0.0
                for _ in range(3):
                    reg.sync()
                    reg.download_state(("x",))
                    t0 = time.perf_counter()
                    reg.run_async(params, n_iters)
                    for _ in range(10):
                        if beside == "mesh_outputs":
                            reg.mesh_outputs_begin(None, Kinv, h, w, graph_scale=1.1, want_filtered_map=True)
                            reg.mesh_outputs_end(copy=False)
                        elif beside == "debug_images":
                            reg.debug_images_begin(None, K, h, w, p, img_device=ptr, step_bytes=step)
                            reg.debug_images_end(copy=False)
                        elif beside == "debug_wireframe":
                            reg.debug_wireframe_begin(None, h, w, 1.1, wp, img_device=ptr, step_bytes=step)
                            reg.debug_wireframe_end(copy=False)
                    t_stage = time.perf_counter()
                    reg.sync()
                    t1 = time.perf_counter()
                    best = max(best, n_iters / ((t1 - t0) * 1e6))
                rate[beside] = (best, (t_stage - t0) * 1e3, (t1 - t0) * 1e3)
        for where in ("device", "host"):
            d, dmin, c = res[where]
            lines.append(f"{config} V={g['V']} T={len(tris)} idepth + normals + w maps, image in {where} memory: device_us {d:.1f} (min {dmin:.1f}) "
                         f"call_us {c:.1f}")
        lines.append(f"{config} draw_features, {n_proj} projected features ({nc} drawn): kernels_us {np.median(fk):.1f} call_us {np.median(fc):.1f}")
        lines.append(f"{config} wireframe, {n_valid} of {len(tris)} triangles valid, {wout['lines_drawn']} lines, {wout['entries']} entries "
                     f"({wout['entries'] / (h * w):.2f} per pixel), image in device memory: device_us {np.median(wdev):.1f} (min {np.min(wdev):.1f}) "
                     f"call_us {np.median(wcall):.1f}; calls that refilled: {wrefills} of {a.reps + 5}"
                     + (f"; host path (download_state + mesh_outputs + sequential Python): host_ms {whost_ms:.0f}, same bytes" if whost_ms is not None else ""))
        total_call = res["device"][2] + float(np.median(fc))
        lines.append(f"{config} host path (three pictures): host_ms {host_ms:.1f}; ratio host / device calls {host_ms * 1e3 / total_call:.0f}x")
        lines.append(f"{config} solver, {n_iters} iterations of run_async, iterations per us (best of 3): " + ", ".join(
            f"beside {k}: {v[0]:.3f} (stages done after {v[1]:.1f} ms of {v[2]:.1f} ms)" for k, v in rate.items()))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
