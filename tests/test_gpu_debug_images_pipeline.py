"""The three debug images inside the per-frame chain of tests/test_select_pipeline.py (its scene, its size, its stages):

    ... -> sync_graph -> run -> interpolate_mesh -> debug_images (idepth colours, normals) + draw_features

For the first four frames that have a graph, each frame's three pictures are compared byte for byte with the checker
(tests/debug_ref.py over the raster checker's maps of the downloaded state).  No image is uploaded twice: the regulariser takes
the frame's grey image from the tracker's resident frame (frame_image_device), so add_frame is the only upload of a frame."""
import numpy as np
import pytest

from oracle import capi as oracle
from tests import debug_ref as dr
from tests import test_select_pipeline as sp
from tests.test_debug_images import assert_image
from tests.test_mesh_outputs import bits

FRAMES = 4
COLOR_SCALE = 1.3


class Done(Exception):
    pass


class DebugChain(sp.HipChain):
    """The product chain; its interpolate stage also draws, and checks, the frame's debug images."""

    def __init__(self, sc, imgs):
        super().__init__(sc, imgs)
        self.cur, self.uploads, self.checked, self.pos = None, [], 0, None

    def add_frame(self, k):
        self.uploads.append(k)
        self.cur = k
        super().add_frame(k)

    def select(self, anchors):
        sel = super().select(anchors)
        self.pos = sel["pos"].copy()
        return sel

    def interpolate(self, tris):
        k, K, H, W = self.cur, self.sc.K32, sp.H, sp.W
        self.reg.interpolate_mesh_begin(tris, H, W)
        ptr, step = self.tr.frame_image_device(k)
        assert ptr and step == W + 2 * self.tr.border
        self.reg.debug_images_begin(None, K, H, W, self.flame_amd.DebugImageParams(scene_color_scale=COLOR_SCALE), img_device=ptr, step_bytes=step)
        dense, _ = self.reg.interpolate_mesh_end()
        got = self.reg.debug_images_end()
        st = self.reg.download_state(("x", "w1", "w2"))
        ref_dense = oracle.raster_interpolate_mesh(tris, self.pos, st["x"], H, W)
        w1m = oracle.raster_interpolate_mesh(tris, self.pos, st["w1"], H, W)
        w2m = oracle.raster_interpolate_mesh(tris, self.pos, st["w2"], H, W)
        assert np.array_equal(bits(dense), bits(ref_dense)), "frame %d: dense map" % k
        assert np.array_equal(bits(got["w1_map"]), bits(w1m)) and np.array_equal(bits(got["w2_map"]), bits(w2m)), "frame %d: w maps" % k
        img = self.imgs[k]
        assert_image(got["idepthmap_img"], dr.draw_inverse_depth_map(img, ref_dense, COLOR_SCALE), "frame %d: idepth image" % k)
        assert_image(got["normals_img"], dr.draw_normals(img, K, ref_dense, w1m, w2m), "frame %d: normals image" % k)
        thr = float(self.gp.idepth_var_max_graph)
        fimg, nc, nu = self.tr.draw_features(k, thr, COLOR_SCALE)
        ref, rc, ru = dr.draw_features(img, self.tr.get_projected(), thr, COLOR_SCALE)
        assert (nc, nu) == (rc, ru) and nc > 0, (k, nc, nu, rc, ru)
        assert_image(fimg, ref, "frame %d: features image" % k)
        painted = (got["normals_img"] != np.repeat(img[:, :, None], 3, axis=2)).any(axis=2).sum()
        print("frame %d: %d covered pixels, %d painted in the normals image, %d / %d features drawn" % (k, (~np.isnan(dense)).sum(), painted, nc, nc + nu))
        self.checked += 1
        if self.checked == FRAMES:
            raise Done()
        return dense


@pytest.mark.gpu
def test_gpu_chain_draws_the_three_debug_images_of_four_frames(built):
    import torch  # noqa: F401

    sc = sp.make_scene()
    imgs = {c: sc.render(c) for c in sc.cams}
    side = DebugChain(sc, imgs)
    try:
        with pytest.raises(Done):
            sp.drive([side], sc)
        assert side.checked == FRAMES
        assert len(side.uploads) == len(set(side.uploads)), "an image was uploaded twice"
    finally:
        side.close()
