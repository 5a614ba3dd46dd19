"""The view renderer inside the per-frame chain of tests/test_select_pipeline.py, at its size: on four frames the current mesh is
rendered into the previous frame's pose with copy_out = 0, beside runs in flight, and the map that stays on the device is handed on

    ... -> run -> interpolate_mesh_begin -> run_async -> render_view_begin -> map_error_begin (TRUTH: the map the previous frame kept,
           on the device) -> metric_outputs_begin (map_device) -> ...

Everything must equal the chained numpy checkers -- tests/view_ref.py, then tests/map_error_ref.py and tests/metric_ref.py fed the
checker's view -- bit for bit, and the solver's state must be the state of a chain that never made the calls."""
import numpy as np
import pytest

from tests import map_error_ref as er
from tests import metric_ref as xr
from tests import test_select_pipeline as tsp
from tests import view_ref as vr
from tests.helpers import assert_state_equal
from tests.metric_helpers import fetch, on_device
from tests.test_gpu_metric_outputs_pipeline import EXTRA, PlainChain

F = np.float32
RENDERED_FRAMES = 4


class ViewChain(tsp.HipChain):
    def __init__(self, sc, imgs):
        from flame_amd.regularizer import OPT_MESH_STATE

        super().__init__(sc, imgs)
        self.reg.set_option(OPT_MESH_STATE, 1)  # a stage behind runs in flight describes the state the last settle left
        self.cur = None
        self.kept = None  # (frame, its dense map on the host, the same on the device): what the previous frame kept
        self.checked = 0

    def update(self, k, curr_pf, anchors):
        self.cur = k
        return super().update(k, curr_pf, anchors)

    def first_graph(self, g, fid):
        super().first_graph(g, fid)
        self.positions = np.asarray(g["pos"], F).copy()

    def sync_graph(self, sel, edges):
        super().sync_graph(sel, edges)
        self.positions = np.asarray(sel["pos"], F).copy()

    def interpolate(self, tris):
        fa, reg, sc, k = self.flame_amd, self.reg, self.sc, self.cur
        H, W = tsp.H, tsp.W
        x = reg.download_state(("x",))["x"]  # (settled: drive has just compared this state)
        reg.interpolate_mesh_begin(tris, H, W)
        reg.run_async(self.params, EXTRA)  # the solver runs beside everything below
        if self.kept is not None:
            prev, prev_map, prev_dev = self.kept
            (Rk, tk), (Rp, tp) = sc.cams[k], sc.cams[prev]
            R = Rp @ Rk.T
            R, t = R.astype(F), (tp - R @ tk).astype(F)
            reg.render_view_begin(fa.ViewParams(Kinv_src=sc.Kinv32, K_dst=sc.K32, R=R, t=t, copy_out=False), H, W)
            in_flight = reg.runs_in_flight()
            view = reg.render_view_end()
            assert "map" not in view and "tri_index" not in view
            ptr = view["device"]["map"]
            reg.map_error_begin(fa.MapErrorParams(source=fa.MAP_ERROR_TRUTH, map_device=ptr, truth_device=prev_dev.data_ptr(), relative=True,
                                                  win_size=1), H, W)
            reg.metric_outputs_begin(sc.Kinv32, H, W, params=fa.MetricParams(map_device=ptr))
            err = reg.map_error_end()
            metric = reg.metric_outputs_end()
            want = vr.render_view(tris, self.positions, x, sc.Kinv32, sc.K32, R, t, H, W)
            view["map"], view["tri_index"] = fetch(ptr, (H, W), F), fetch(view["device"]["tri_index"], (H, W), np.int32)
            vr.assert_same(view, want, "frame %d seen from frame %d" % (k, prev))
            er.assert_same(err, er.map_error(want["map"], er.TRUTH, truth=prev_map, relative=True, win_size=1), "frame %d against frame %d's map" % (k, prev))
            xr.assert_same(metric, xr.metric_points(want["map"], sc.Kinv32), xr.POINT_KEYS, "frame %d registered to frame %d" % (k, prev))
            assert want["coverage"] > 1000 and want["tris_drawn"] > 0 and 0 < err["n_valid"] <= want["coverage"]
            print("frame %d into frame %d: coverage %d, drawn %d, culled %d + %d; against the kept map: n_valid %d median_bin %d p99 bin %d; runs in "
                  "flight behind begin: %d, device_ms %.3f" % (k, prev, want["coverage"], want["tris_drawn"], want["tris_culled_vertex"],
                                                               want["tris_culled_facing"], err["n_valid"], err["median_bin"], err["ptile_bin"], in_flight,
                                                               view["device_ms"]))
            self.checked += 1
        dense, _ = reg.interpolate_mesh_end()
        self.kept = (k, dense, on_device(dense))
        reg.sync()
        return dense


@pytest.mark.gpu
def test_gpu_four_frames_rendered_into_the_previous_pose_and_handed_on(built, monkeypatch):
    import torch  # noqa: F401

    monkeypatch.setattr(tsp, "LAST", tsp.FIRST + 2 + RENDERED_FRAMES)  # the graph starts at the second frame; the first one has no predecessor
    sc = tsp.make_scene()
    imgs = {c: sc.render(c) for c in sc.cams}
    sides = [PlainChain(sc, imgs), ViewChain(sc, imgs)]
    try:
        _, last, log = tsp.drive(sides, sc)  # (compares the two sides' solver state after every frame's run)
        assert last == tsp.LAST and log["frames_with_graph"] == RENDERED_FRAMES + 1 and sides[1].checked == RENDERED_FRAMES, log
        a, b = sides[0].reg.download_state(), sides[1].reg.download_state()
        assert_state_equal(b, a, keys=tuple(a), what="after the last frame")
    finally:
        for s in sides:
            s.close()
