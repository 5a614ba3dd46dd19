"""The wireframe image inside the per-frame chain of tests/test_select_pipeline.py (its scene, its size, its stages), the way a frame
loop would call it:

    ... -> sync_graph -> run -> interpolate_mesh_begin, mesh_outputs_begin, debug_wireframe_begin (validity from the device, the
    frame's image from the tracker) -> run_async -> the three _ends -> sync

For the first four frames that have a graph, the frame's wireframe is compared byte for byte with the checker
(tests/wireframe_ref.py over the state downloaded before the stages, with tests/mesh_ref.py's triangle validity), while the solver
already iterates again beside the stages."""
import numpy as np
import pytest

from tests import mesh_ref as mr
from tests import test_select_pipeline as sp
from tests import wireframe_ref as wr
from tests.test_debug_images import assert_image
from tests.test_mesh_outputs import bits

FRAMES = 4
COLOR_SCALE = 1.3


class Done(Exception):
    pass


class WireframeChain(sp.HipChain):
    """The product chain; its interpolate stage also draws, and checks, the frame's wireframe."""

    def __init__(self, sc, imgs):
        super().__init__(sc, imgs)
        self.cur, self.checked, self.pos = None, 0, None

    def add_frame(self, k):
        self.cur = k
        super().add_frame(k)

    def select(self, anchors):
        sel = super().select(anchors)
        self.pos = sel["pos"].copy()
        return sel

    def interpolate(self, tris):
        k, H, W, reg = self.cur, sp.H, sp.W, self.reg
        Kinv = self.sc.Kinv32
        before = reg.download_state(("x",))  # the state the map, the mesh outputs and the wireframe describe
        ptr, step = self.tr.frame_image_device(k)
        reg.interpolate_mesh_begin(tris, H, W)
        reg.mesh_outputs_begin(None, Kinv, H, W)
        reg.debug_wireframe_begin(None, H, W, 1.0, self.flame_amd.WireframeParams(scene_color_scale=COLOR_SCALE, validity=2),
                                  img_device=ptr, step_bytes=step)
        reg.run_async(self.params, 300)  # the solver goes on beside the three stages
        dense, _ = reg.interpolate_mesh_end()
        mesh = reg.mesh_outputs_end()
        got = reg.debug_wireframe_end()
        reg.sync()
        after = reg.download_state(("x",))
        assert not np.array_equal(bits(after["x"]), bits(before["x"])), "frame %d: the solver did not run beside the stages" % k
        ref_mesh = mr.mesh_outputs(self.pos, before["x"], tris, Kinv, H, W)
        valid = np.asarray(ref_mesh["tri_valid"], np.uint8)
        assert np.array_equal(mesh["tri_valid"], valid), "frame %d: triangle validity" % k
        ref, nd, ns = wr.draw_wireframe(self.imgs[k], tris, self.pos, ref_mesh["vtx_idepth"], valid, COLOR_SCALE)
        assert (got["lines_drawn"], got["lines_skipped"]) == (nd, ns) == (3 * int(valid.sum()), 0), (k, got["lines_drawn"], got["lines_skipped"], nd, ns)
        assert_image(got["wireframe_img"], ref, "frame %d: wireframe" % k)
        print("frame %d: %d of %d triangles valid, %d entries, refilled %d" % (k, valid.sum(), len(tris), got["entries"], got["refilled"]))
        assert 0 < valid.sum()
        self.checked += 1
        if self.checked == FRAMES:
            raise Done()
        return dense


@pytest.mark.gpu
def test_gpu_chain_draws_the_wireframe_of_four_frames_beside_the_solver(built):
    import torch  # noqa: F401

    sc = sp.make_scene()
    imgs = {c: sc.render(c) for c in sc.cams}
    side = WireframeChain(sc, imgs)
    try:
        with pytest.raises(Done):
            sp.drive([side], sc)
        assert side.checked == FRAMES
    finally:
        side.close()
