"""The metric outputs inside the per-frame chain of tests/test_select_pipeline.py, at its size: three frames with a graph, on each of
them interpolate_mesh_begin + run_async + mesh_outputs_begin + metric_outputs_begin with the runs in flight.  The outputs must equal
the checker (tests/metric_ref.py) fed with the maps the other two stages hand out, bit for bit, and the solver's state must be the
state of a chain that never made the calls."""
import numpy as np
import pytest

from tests import metric_ref as xr
from tests import test_select_pipeline as tsp
from tests.helpers import assert_state_equal
from tests.metric_helpers import rot_z

EXTRA = 200      # iterations enqueued between interpolate_mesh_begin and the two stages behind it
GRAPH_FRAMES = 3


class PlainChain(tsp.HipChain):
    """The chain without the stage: the map, then the same further iterations."""

    def interpolate(self, tris):
        dense = self.reg.interpolate_mesh(tris, tsp.H, tsp.W)[0]
        self.reg.run(self.params, EXTRA)
        return dense


class MetricChain(tsp.HipChain):
    def __init__(self, sc, imgs):
        from flame_amd.regularizer import OPT_MESH_STATE

        super().__init__(sc, imgs)
        self.reg.set_option(OPT_MESH_STATE, 1)  # a stage behind runs in flight describes the state the last settle left
        self.checked = 0

    def interpolate(self, tris):
        fa, reg, Kinv = self.flame_amd, self.reg, self.sc.Kinv32
        st = reg.download_state(("x",))  # (settled: drive has just compared this state)
        pose = rot_z(10.0 + self.checked, t=(0.1 * self.checked, -0.2, 0.3))
        reg.interpolate_mesh_begin(tris, tsp.H, tsp.W)
        reg.run_async(self.params, EXTRA)
        reg.mesh_outputs_begin(None, Kinv, tsp.H, tsp.W, want_filtered_map=True)
        reg.metric_outputs_begin(Kinv, tsp.H, tsp.W, pose=pose, params=fa.MetricParams(want_mesh=True, use_filtered_map=self.checked % 2 == 1))
        dense, _ = reg.interpolate_mesh_end()
        mo = reg.mesh_outputs_end()
        got = reg.metric_outputs_end()
        which = mo["filtered_map"] if self.checked % 2 == 1 else dense
        ref = xr.metric_points(which, Kinv, pose)
        ref.update(xr.metric_mesh(self.positions, st["x"], 1.0, Kinv, mo["normals"], tris, mo["tri_valid"], pose))
        xr.assert_same(got, ref, xr.POINT_KEYS + xr.MESH_KEYS, f"graph frame {self.checked}")
        assert got["n_valid"] == mo["n_valid"] and got["n_points"] > 1000
        self.checked += 1
        reg.sync()
        return dense

    # the vertex positions of the current graph, as the chain handed them in
    def first_graph(self, g, fid):
        super().first_graph(g, fid)
        self.positions = np.asarray(g["pos"], np.float32).copy()

    def sync_graph(self, sel, edges):
        super().sync_graph(sel, edges)
        self.positions = np.asarray(sel["pos"], np.float32).copy()


@pytest.mark.gpu
def test_gpu_three_frames_with_the_stage_beside_runs_in_flight(built, monkeypatch):
    import torch  # noqa: F401

    monkeypatch.setattr(tsp, "LAST", tsp.FIRST + 1 + GRAPH_FRAMES)  # the graph starts at the second frame (V: 0, 64, 123, 157)
    sc = tsp.make_scene()
    imgs = {c: sc.render(c) for c in sc.cams}
    sides = [PlainChain(sc, imgs), MetricChain(sc, imgs)]
    try:
        _, last, log = tsp.drive(sides, sc)  # (compares the two sides' solver state after every frame's run)
        assert last == tsp.LAST and log["frames_with_graph"] == GRAPH_FRAMES == sides[1].checked, log
        a, b = sides[0].reg.download_state(), sides[1].reg.download_state()
        assert_state_equal(b, a, keys=tuple(a), what="after the last frame")
    finally:
        for s in sides:
            s.close()
