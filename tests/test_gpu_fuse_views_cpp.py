"""DeviceGraph::keepMesh / dropMesh / fuseViewsBegin / End (include/flame_hip/nltgv2_l1_graph_regularizer.hpp): the program
tests/cpp/fuse_views_test.cc compiles as C++11 against include/ and, on a GPU, reproduces byte for byte what the Python mirror obtained
for the same graph, triangles, cameras and vote (dumped to a temporary file)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import fuse_ref as fr
from tests import test_fuse_views_ref as ref
from tests import test_gpu_render_view as tg
from tests.conftest import HAS_GPU, ROOT

F = np.float32


def build_program(tmp_path):
    exe = str(tmp_path / "fuse_views_test")
    lib_dir = os.path.join(ROOT, "flame_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "fuse_views_test.cc"), "-o", exe, "-L", lib_dir, "-lflame_nltgv2_hip",
        f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_fuse_views_facade_compiles_and_fails_loudly_without_a_device(built, tmp_path):
    exe = build_program(tmp_path)
    if not HAS_GPU:
        r = subprocess.run([exe, "/dev/null"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no usable HIP device" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_fuse_views_facade_round_trip(built, tmp_path):
    import torch  # noqa: F401

    import flame_amd

    rows, cols = 75, 100
    K_dst = ref.cases.camera(90.0, 50.0, 37.5)[0]
    mesh = ref.plane_source(2)
    tris, rel_tol, min_support = mesh["tris"], 0.05, 2
    # the same mesh as three pose-frames saw it: two kept at their own scales, one live
    R, t = ref.POSES[2]
    views = [dict(R=R, t=t, weight=0.3, scale=1.0), dict(R=R, t=t, weight=1.7, scale=1.04),
             dict(R=R, t=t + np.array([0.1, 0, 0], F), weight=0.9, scale=0.93)]  # (0.93: beyond the tolerance of 0.05)
    g = tg.graph_of(mesh["pos"], mesh["idepth"], tris)
    with flame_amd.Regularizer(0) as reg:
        reg.upload_graph(g)
        reg.interpolate_mesh(tris, *ref.SRC)
        sources = []
        for s, v in enumerate(views):
            if s < 2:
                reg.keep_mesh(s + 4, graph_scale=v["scale"])
            sources.append(flame_amd.FuseSource(slot=s + 4 if s < 2 else -1, Kinv_src=ref.KINV, R=v["R"], t=v["t"], weight=v["weight"],
                                                graph_scale=v["scale"]))
        out = reg.fuse_views(flame_amd.FuseParams(sources=sources, K_dst=K_dst, rel_tol=rel_tol, min_support=min_support, want_layers=True), rows, cols)
    want = fr.fuse_sources([dict(mesh, idepth=(mesh["idepth"] * F(v["scale"])).astype(F), R=v["R"], t=v["t"], weight=v["weight"]) for v in views],
                           K_dst, rows, cols, rel_tol, min_support)
    fr.assert_same(out, want, "three views of one mesh")
    assert want["coverage"] > 1000 and want["support_hist"][1] > 0 and want["support_hist"][2] > 1000 and (want["present_mask"] & ~want["inlier_mask"]).any()
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(b"FUS1" + struct.pack("<8i", g["V"], g["E"], len(tris), *ref.SRC, rows, cols, min_support))
        camera = np.concatenate([np.concatenate([np.asarray(ref.KINV, F).reshape(-1), np.asarray(v["R"], F).reshape(-1), np.asarray(v["t"], F).reshape(-1),
                                                 np.array([v["weight"], v["scale"]], F)]) for v in views]
                                + [np.asarray(K_dst, F).reshape(-1), np.array([rel_tol], F)])
        assert camera.size == 3 * 23 + 10
        for a, t in ((camera, "<f4"), (g["pos"], "<f4"), (g["x"], "<f4"), (g["src"], "<i4"), (g["dst"], "<i4"), (g["alpha"], "<f4"), (g["beta"], "<f4"),
                     (tris, "<i4"), (out["fused"], "<f4"), (out["present_mask"], "u1"), (out["inlier_mask"], "u1"), (out["spread"], "<f4"),
                     (out["layers"], "<f4"), (out["counts"], "<i4")):
            f.write(np.ascontiguousarray(a, t).tobytes())
    r = subprocess.run([build_program(tmp_path), path], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count(": ok") == 4 and "FAIL" not in r.stdout, r.stdout + r.stderr
