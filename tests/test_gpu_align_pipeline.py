"""The alignment behind a regulariser context on the same device, on the scene of tests/test_pipeline.py:

    upload_graph (the pose-frame's vertices) -> run -> interpolate_mesh_begin / _end -> render_view (the resident mesh into the
    pose-frame's own camera, which leaves the dense map in device memory) -> align_frame reads that map in place

interpolate_mesh_end hands out pinned host memory; the address of a dense map of that context in device memory is what render_view_end
reports, so that is the pointer the tracker reads here, the caller having waited for the regulariser (render_view_end waits).  Every
evaluation of the device's trace must equal the checker (tests/align_ref.py) fed the downloaded map, bit for bit; the checker's own loop
from the same start must end at the same pose (the two loops see the same float32 poses and the same sums; their 6 x 6 solves and sines
differ by double rounding, 1e-15, and 1e-9 is far below the 1e-7 at which a float32 pose would change)."""
import numpy as np
import pytest

from tests import align_ref as ar
from tests import test_pipeline as tp

pytestmark = pytest.mark.gpu
PF, NEW = 11, 20
PARAMS = dict(border=2, huber_k=10.0, coarsest_level=2, finest_level=0, max_iters_per_level=10, min_pixels=100, min_step=1e-5,
              lm_lambda=0.0)


def test_gpu_align_reads_the_regularisers_map_in_place(built):
    import torch  # noqa: F401

    import flame_amd
    from flame_amd import synth
    from flame_amd.stereo import ALIGN_OK, AlignParams, FeatureTracker

    sc, imgs, _ = tp.make_scene()
    W, H = tp.W, tp.H
    K = (float(sc.K32[0, 0]), float(sc.K32[1, 1]), float(sc.K32[0, 2]), float(sc.K32[1, 2]))
    rng = np.random.default_rng(4)
    ys, xs = np.mgrid[12:H - 12:14, 12:W - 12:14]
    pos = (np.stack([xs.ravel(), ys.ravel()], 1) + rng.uniform(-3, 3, (xs.size, 2))).astype(np.float32)
    idepth = (sc.true_idepth(PF, pos) * (1 + 0.03 * rng.standard_normal(pos.shape[0]))).astype(np.float32)
    tris, edges = flame_amd.delaunay(pos)  # as tests/test_pipeline.py builds its mesh
    g = synth.assemble_graph(pos, idepth, edges)
    q_true, t_true = (np.asarray(v, np.float64) for v in sc.relative(PF, NEW))
    start = (np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3))
    with flame_amd.Regularizer(0) as reg, FeatureTracker(sc.K32, sc.Kinv32, W, H, border=tp.PAD) as tr:
        reg.upload_graph(g)
        reg.run(flame_amd.Params(), 30)
        reg.interpolate_mesh_begin(tris, H, W)
        _, coverage = reg.interpolate_mesh_end()
        view = reg.render_view(flame_amd.regularizer.ViewParams(Kinv_src=sc.Kinv32, K_dst=sc.K32), H, W)  # waits for that context
        ptr, down = view["device"]["map"], view["map"]
        assert ptr and coverage > 0.5 * W * H and np.isfinite(down).sum() > 0.5 * W * H and np.isnan(down).any()
        tr.add_frame(PF, imgs[PF])
        tr.add_frame(NEW, imgs[NEW])
        tr.build_pyramid(PF, 3)
        tr.build_pyramid(NEW, 3)
        res = tr.align_frame(AlignParams(**PARAMS), PF, NEW, int(ptr), *start)
    rp, npyr = ar.build_pyramid(imgs[PF], 3), ar.build_pyramid(imgs[NEW], 3)
    assert res["status"] == ALIGN_OK and {e["level"] for e in res["trace"]} == {0, 1, 2} and sum(res["iters"]) >= 3
    for k, e in enumerate(res["trace"]):
        want = ar.linearize(rp[e["level"]][0], npyr[e["level"]], down, e["level"], K, PARAMS["border"], PARAMS["huber_k"], e["q"], e["t"])
        assert want["n_used"] > 0 and want["n_no_depth"] > 0
        ar.assert_same_system(e, want, "evaluation %d (level %d)" % (k, e["level"]))
    alone = ar.align_frame(rp, npyr, down, K, *start, **PARAMS)
    assert len(alone["trace"]) == len(res["trace"]) and alone["iters"] == res["iters"]
    assert np.abs(alone["q"] - res["q"]).max() <= 1e-9 and np.abs(alone["t"] - res["t"]).max() <= 1e-9
    r0, t0 = ar.pose_error(*start, q_true, t_true)
    r1, t1 = ar.pose_error(res["q"], res["t"], q_true, t_true)
    print("start", r0, t0, "end", r1, t1, "evaluations", len(res["trace"]), "iters", res["iters"])
    assert r1 < r0 and t1 < t0
