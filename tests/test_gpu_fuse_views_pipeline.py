"""The kept-mesh store and the fusion inside the per-frame chain of tests/test_select_pipeline.py, at its size.  On four frames every
frame is a pose-frame that keeps its mesh:

    ... -> run -> interpolate_mesh_begin -> run_async -> fuse_views_begin (the kept meshes + the live one, into this frame's camera)
           -> drop_mesh (the pose-frame that is pruned) -> keep_mesh (slot frame % 3) -> ...

beside runs in flight.  Everything must equal the chained numpy checkers -- tests/view_ref.py per source, tests/fuse_ref.py over them --
bit for bit, the kept slots must hold what the host remembers, and the solver's state must be the state of a chain that never made
the calls."""
import numpy as np
import pytest

from tests import fuse_ref as fr
from tests import test_select_pipeline as tsp
from tests.helpers import assert_state_equal
from tests.test_gpu_metric_outputs_pipeline import EXTRA, PlainChain

F = np.float32
FUSED_FRAMES = 4
WINDOW = 2  # kept pose-frames a fusion sees beside the live mesh; older ones are pruned
REL_TOL = 0.05


class FuseChain(tsp.HipChain):
    def __init__(self, sc, imgs):
        from flame_amd.regularizer import OPT_MESH_STATE

        super().__init__(sc, imgs)
        self.reg.set_option(OPT_MESH_STATE, 1)  # a stage behind runs in flight describes the state the last settle left
        self.cur = None
        self.kept = []  # (frame, slot, tris, positions, x) of the pose-frames in the window, oldest first
        self.checked, self.sources_seen = 0, []

    def update(self, k, curr_pf, anchors):
        self.cur = k
        return super().update(k, curr_pf, anchors)

    def first_graph(self, g, fid):
        super().first_graph(g, fid)
        self.positions = np.asarray(g["pos"], F).reshape(-1, 2).copy()

    def sync_graph(self, sel, edges):
        super().sync_graph(sel, edges)
        self.positions = np.asarray(sel["pos"], F).reshape(-1, 2).copy()

    def interpolate(self, tris):
        fa, reg, sc, k = self.flame_amd, self.reg, self.sc, self.cur
        H, W = tsp.H, tsp.W
        x = reg.download_state(("x",))["x"]  # (settled: drive has just compared this state)
        reg.interpolate_mesh_begin(tris, H, W)
        reg.run_async(self.params, EXTRA)  # the solver runs beside everything below
        Rk, tk = sc.cams[k]
        sources, checker_sources = [], []
        for frame, slot, ktris, kpos, kx in self.kept:
            Rj, tj = sc.cams[frame]
            R = Rk @ Rj.T
            R, t = R.astype(F), (tk - R @ tj).astype(F)
            sources.append(fa.FuseSource(slot=slot, Kinv_src=sc.Kinv32, R=R, t=t, weight=1.0))
            checker_sources.append(dict(tris=ktris, pos=kpos, idepth=kx, Kinv_src=sc.Kinv32, R=R, t=t, weight=1.0))
        sources.append(fa.FuseSource(slot=-1, Kinv_src=sc.Kinv32, weight=2.0))
        checker_sources.append(dict(tris=tris, pos=self.positions, idepth=x, Kinv_src=sc.Kinv32, weight=2.0))
        min_support = min(2, len(sources))
        reg.fuse_views_begin(fa.FuseParams(sources=sources, K_dst=sc.K32, rel_tol=REL_TOL, min_support=min_support, want_layers=True), H, W)
        in_flight = reg.runs_in_flight()
        # the pose-frame that leaves the window is pruned, this frame is kept: both behind the fusion on the side stream
        if len(self.kept) == WINDOW:
            reg.drop_mesh(self.kept[0][1])
            assert reg.kept_mesh_info(self.kept[0][1]) == (-1, -1, False)
            self.kept = self.kept[1:]
        slot = k % 3
        assert all(s != slot for _, s, _, _, _ in self.kept)
        reg.keep_mesh(slot)
        self.kept.append((k, slot, np.asarray(tris, np.int32).reshape(-1, 3).copy(), self.positions.copy(), x.copy()))
        got = reg.fuse_views_end()
        want = fr.fuse_sources(checker_sources, sc.K32, H, W, REL_TOL, min_support)
        fr.assert_same(got, want, "frame %d, %d sources" % (k, len(sources)))
        assert want["coverage"] > 1000 and want["tris_drawn"] > 0 and all(want["present"][s] > 500 for s in range(len(sources)))
        mesh = reg.get_kept_mesh(slot)
        assert mesh["vertices"].tobytes() == self.positions.tobytes() and mesh["idepths"].tobytes() == x.tobytes()
        assert mesh["triangles"].tobytes() == self.kept[-1][2].tobytes()
        print("frame %d: %d sources, coverage %d, support %s, disagreeing pixels %d; runs in flight behind begin: %d, device_ms %.3f" % (
            k, len(sources), want["coverage"], want["support_hist"][:len(sources) + 1], int(((want["present_mask"] & ~want["inlier_mask"]) != 0).sum()),
            in_flight, got["device_ms"]))
        self.checked += 1
        self.sources_seen.append(len(sources))
        dense, _ = reg.interpolate_mesh_end()
        reg.sync()
        return dense


@pytest.mark.gpu
def test_gpu_four_pose_frames_kept_fused_and_pruned(built, monkeypatch):
    import torch  # noqa: F401

    monkeypatch.setattr(tsp, "LAST", tsp.FIRST + 1 + FUSED_FRAMES)  # the graph starts at the second frame
    sc = tsp.make_scene()
    imgs = {c: sc.render(c) for c in sc.cams}
    sides = [PlainChain(sc, imgs), FuseChain(sc, imgs)]
    try:
        _, last, log = tsp.drive(sides, sc)  # (compares the two sides' solver state after every frame's run)
        assert last == tsp.LAST and log["frames_with_graph"] == FUSED_FRAMES and sides[1].checked == FUSED_FRAMES, log
        assert sides[1].sources_seen == [1, 2, 3, 3]  # a slot was dropped and, at the fourth frame, reused
        a, b = sides[0].reg.download_state(), sides[1].reg.download_state()
        assert_state_equal(b, a, keys=tuple(a), what="after the last frame")
    finally:
        for s in sides:
            s.close()
