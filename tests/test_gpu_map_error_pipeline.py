"""The map error inside the per-frame chain of tests/test_select_pipeline.py -- its scene, its size, all its frames -- on the resident
map, with two frames resident in the stereo context read in place:

    ... -> run -> interpolate_mesh_begin -> run_async (the solver goes on) -> map_error_begin (PHOTO, then TRUTH) -> ...

On every frame with a graph both calls must equal the checker (tests/map_error_ref.py) fed the downloaded map, bit for bit; after the
last frame the TRUTH bins must say what check_run asserts on the host; and the solver's state must be the checker chain's after every
frame, so the stage only read."""
import numpy as np
import pytest

from tests import map_error_ref as er
from tests import test_select_pipeline as tsp
from tests.helpers import OUT_KEYS, assert_state_equal

F = np.float32
EXTRA = 200  # iterations enqueued between interpolate_mesh_begin and the stage behind it
BORDER = 4


class ExtraChecker(tsp.CheckerChain):
    """The checker chain with the same further iterations behind the map."""

    def interpolate(self, tris):
        dense = super().interpolate(tris)
        self.run(EXTRA)
        return dense


class MapErrorChain(tsp.HipChain):
    def __init__(self, sc, imgs):
        from flame_amd.regularizer import OPT_MESH_STATE

        super().__init__(sc, imgs)
        self.reg.set_option(OPT_MESH_STATE, 1)  # a stage behind runs in flight describes the state the last settle left
        self.cur = self.pf = None
        self.checked, self.last = 0, None
        ys, xs = np.mgrid[0:tsp.H, 0:tsp.W]
        self.grid = np.stack([xs.ravel(), ys.ravel()], 1).astype(F)

    def update(self, k, curr_pf, anchors):
        self.cur, self.pf = k, curr_pf
        return super().update(k, curr_pf, anchors)

    def interpolate(self, tris):
        fa, reg, sc, k, pf = self.flame_amd, self.reg, self.sc, self.cur, self.pf
        H, W = tsp.H, tsp.W
        reg.interpolate_mesh_begin(tris, H, W)
        reg.run_async(self.params, EXTRA)  # the solver runs beside everything below
        (ref_ptr, step), (cmp_ptr, cmp_step) = self.tr.frame_image_device(k), self.tr.frame_image_device(pf)
        assert ref_ptr and cmp_ptr and step == cmp_step == W + 2 * self.tr.border and pf != k
        _, t, KRKinv = tsp.projection_between(sc, k, pf)
        Kt = (sc.K32 @ t).astype(F)
        reg.map_error_begin(fa.MapErrorParams(KRKinv=KRKinv, Kt=Kt, border=BORDER, ref_device=ref_ptr, cmp_device=cmp_ptr, image_step_bytes=step,
                                              want_image=True), H, W)
        in_flight = reg.runs_in_flight()
        dense, _ = reg.interpolate_mesh_end()
        photo = reg.map_error_end()
        truth = sc.true_idepth(k, self.grid).reshape(H, W).astype(F)
        reg.map_error_begin(fa.MapErrorParams(source=fa.MAP_ERROR_TRUTH, truth=truth, relative=True, win_size=1, ptile_num=90, ptile_den=100), H, W)
        true = reg.map_error_end()
        er.assert_same(photo, er.map_error(dense, er.PHOTO, KRKinv, Kt, self.imgs[k], self.imgs[pf], BORDER, want_image=True),
                       "frame %d against pose-frame %d" % (k, pf))
        er.assert_same(true, er.map_error(dense, er.TRUTH, truth=truth, relative=True, win_size=1, ptile_num=90, ptile_den=100), "frame %d against the truth" % k)
        print("frame %d: photo against pf %d: n_valid %d median_bin %d p99 bin %d mean %.2f | truth: median_bin %d p90 bin %d | runs in flight behind "
              "the first begin: %d, device_ms %.3f / %.3f" % (k, pf, photo["n_valid"], photo["median_bin"], photo["ptile_bin"], photo["mean"],
                                                             true["median_bin"], true["ptile_bin"], in_flight, photo["device_ms"], true["device_ms"]))
        self.checked += 1
        self.last = (k, photo, true, dense, truth)
        reg.sync()
        return dense


@pytest.mark.gpu
def test_gpu_chain_measures_its_final_map_beside_the_running_solver(built):
    import torch  # noqa: F401

    sc = tsp.make_scene()
    imgs = {c: sc.render(c) for c in sc.cams}
    sides = [ExtraChecker(sc, imgs), MapErrorChain(sc, imgs)]
    try:
        dense, last, log = tsp.drive(sides, sc)  # (compares the two sides' solver state after every frame's run: the stage only read)
        hip = sides[1]
        assert hip.checked == log["frames_with_graph"] >= 6
        assert_state_equal(hip.graph_state(), sides[0].graph_state(), keys=OUT_KEYS, what="after the last frame's further iterations")
        k, photo, true, final, truth = hip.last
        assert k == last == tsp.LAST
        tsp.check_run(sc, final, last, log)  # median < 0.02 and p90 < 0.08 of |dense - truth| / truth, on the host
        # ... which the device's 0.1 % bins must repeat: a median below 0.02 cannot lie above bin 20, a 90th percentile below 0.08
        # not above bin 80 (the bins round to nearest; the ranks are the smallest bin whose cumulated count passes the share)
        assert true["n_valid"] == int((~np.isnan(final)).sum()) and 0 <= true["median_bin"] <= 20 and true["median_bin"] <= true["ptile_bin"] <= 80, \
            (true["median_bin"], true["ptile_bin"])
        ok = ~np.isnan(final)
        rel = np.abs(final[ok] - truth[ok]) / truth[ok]
        assert abs(true["median_bin"] - 1000 * np.median(rel)) <= 1 and abs(true["ptile_bin"] - 1000 * np.percentile(rel, 90)) <= 1.5
        assert abs(float(true["mean"]) - rel.mean()) < 1e-5
        assert 0 < photo["n_valid"] <= true["n_valid"] and photo["median_bin"] >= 0
    finally:
        for s in sides:
            s.close()
