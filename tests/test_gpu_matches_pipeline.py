"""The matches picture inside the per-frame chain of tests/test_select_pipeline.py (its scene, its size, its stages), the way a frame loop
would call it: recording on, and draw_matches right behind every update_resident.

Three sides run the first eight frames of the chain, every stage of each, side by side: the chained CPU checkers, whose update is the sequential walk of
tests/matches_ref.py (held against the oracle's own update on every frame); the product with recording off; the product with recording
on.  After every stage of every frame all three hold the same bits (tests.test_select_pipeline.drive compares them), and the picture
of every frame equals the checker's, byte for byte and counter for counter."""
import numpy as np
import pytest

from flame_amd import synth_stereo as ss
from oracle import stereo_capi as so
from tests import matches_ref as mref
from tests import test_select_pipeline as sp
from tests.test_feature_frontend import PAD

FRAMES = 8


class Done(Exception):
    pass


class MatchesChecker(sp.CheckerChain):
    """The checkers chained; the update is the walk that also draws."""

    def __init__(self, sc, imgs, pictures):
        super().__init__(sc, imgs)
        self.pictures = pictures

    def update(self, k, curr_pf, anchors):
        sc = self.sc
        frs = [dict(p, img_pad=self.frames[p["id"]][0]) for p in ss.poses_for(sc, anchors, k, curr_pf)]
        want = self.feats.copy()
        rc, st = so.update_feature_idepths(so.Params(), sc.K32, sc.Kinv32, sc.width, sc.height, PAD, frs, self.frames[k], curr_pf, want)
        res = mref.update_and_draw(so.Params(), sc.K32, sc.Kinv32, sc.width, sc.height, PAD, frs, self.frames[k], self.imgs[k],
                                   curr_pf, self.feats)
        assert rc == 0 and res["rc"] == 0 and self.feats.tobytes() == want.tobytes() and list(res["stats"]) == list(st)
        self.pictures[k] = res
        return [int(v) for v in st[:7]]


class MatchesHip(sp.HipChain):
    """The product chain with recording on; every update is followed by its picture."""

    def __init__(self, sc, imgs, pictures):
        super().__init__(sc, imgs)
        self.pictures, self.checked, self.draws = pictures, 0, 0
        self.tr.set_record_matches(True)

    def update(self, k, curr_pf, anchors):
        st = super().update(k, curr_pf, anchors)
        pic, ref = self.tr.draw_matches(), self.pictures[k]
        assert pic["num_features"] == self.tr.features_device()[1]
        for key in ("kind_count", "lines_drawn", "lines_skipped", "rings_skipped", "entries"):
            assert pic[key] == ref[key], (k, key, pic[key], ref[key])
        assert np.array_equal(pic["img"], ref["img"]), "frame %d: %d pixels differ" % (k, np.any(pic["img"] != ref["img"], axis=2).sum())
        assert pic["kind_count"][mref.GREEN] + ref["green_skipped"] == st[1] and pic["kind_count"][mref.BLUE] + ref["blue_skipped"] == st[2]
        print("frame %d: %d features, kinds %s, %d segments, %d entries" % (k, pic["num_features"], pic["kind_count"], pic["lines_drawn"],
                                                                             pic["entries"]))
        self.draws += sum(pic["kind_count"]) + pic["lines_drawn"]
        self.checked += 1
        return st

    def add_frame(self, k):
        if self.checked == FRAMES:
            raise Done()  # the ninth frame begins: every stage of eight frames was run on all sides and compared by the driver
        super().add_frame(k)


@pytest.mark.gpu
def test_gpu_chain_draws_the_matches_of_eight_frames(built):
    import torch  # noqa: F401

    sc = sp.make_scene()
    imgs = {c: sc.render(c) for c in sc.cams}
    pictures = {}
    sides = [MatchesChecker(sc, imgs, pictures), sp.HipChain(sc, imgs), MatchesHip(sc, imgs, pictures)]
    try:
        with pytest.raises(Done):
            sp.drive(sides, sc)
        assert sides[2].checked == FRAMES and len(pictures) == FRAMES
        assert sides[2].draws > 50, "the chain's pictures are all but empty"
    finally:
        for s in sides:
            s.close()
