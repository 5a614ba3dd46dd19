"""The detections picture inside the front half of the per-frame chain (detect_features -> update_resident -> project_features,
four pose-frames at 320x240, as tests/test_feature_frontend.py drives it): draw_detections right after every detect_features with
the same arguments.  Every picture must equal the checker's on the checker's own frames, and every stage output must equal the run
that never draws."""
import numpy as np
import pytest

from oracle import stereo_capi as so
from tests import detections_ref as dt
from tests.test_feature_frontend import PAD, HipSide, assert_records_equal, geometry, plane_scene, true_map

pytestmark = pytest.mark.gpu
POSE_FRAMES = (10, 12, 14, 16)
MAX_SCORE = 48.0


class DrawingSide(HipSide):
    def __init__(self, sc, imgs):
        super().__init__(sc, imgs)
        self.pictures = {}

    def detect(self, ref, prev, idepthmap, use_mask, first_id):
        n = super().detect(ref, prev, idepthmap, use_mask, first_id)
        q, t = self.sc.relative(ref, prev)
        flip = ref % 4 == 0
        self.pictures[ref] = (self.tr.draw_detections(self.sp, self.dp, ref, q, t, max_score=MAX_SCORE, flip=flip), flip)
        return n


def test_gpu_chain_with_drawing_equals_the_chain_without(built):
    sc = plane_scene(320, 240)
    imgs = {c: sc.render(c) for c in sc.cams}
    sides = [HipSide(sc, imgs), DrawingSide(sc, imgs)]

    def same(what):
        a, b = sides[0].state(), sides[1].state()
        assert_records_equal(b[0], a[0], what + ": resident set")
        assert_records_equal(b[1], a[1], what + ": projected set")

    try:
        for s in sides:
            for k in (9, 10):
                s.add_frame(k)
        counts = [s.detect(10, 9, None, False, 0) for s in sides]
        assert counts[0] == counts[1] > 100
        same("detect pf 10")
        next_id, anchors, curr_pf = counts[0], [10], 10
        for k in range(11, 17):
            for s in sides:
                s.add_frame(k)
            stats = [s.update(k, curr_pf, anchors) for s in sides]
            assert stats[0] == stats[1], (k, stats)
            same("frame %d update" % k)
            kept = [s.project(k, anchors) for s in sides]
            assert kept[0] == kept[1] > 0, (k, kept)
            same("frame %d project" % k)
            if k in POSE_FRAMES:
                m = true_map(sc, k)
                counts = [s.detect(k, k - 1, m, True, next_id) for s in sides]
                assert counts[0] == counts[1], (k, counts)
                same("detect pf %d" % k)
                next_id += counts[0]
                anchors, curr_pf = anchors + [k], k
        pictures = sides[1].pictures
    finally:
        for s in sides:
            s.close()
    assert sorted(pictures) == list(POSE_FRAMES)
    for ref, ((got, st), flip) in pictures.items():
        _, gx, gy = so.make_frame(imgs[ref], PAD)  # the checker's own frame
        rc, _, score = dt.detection_score(gx, gy, PAD, 320, 240, geometry(sc, ref, ref - 1))
        want = dt.draw_detections(imgs[ref], score, MAX_SCORE, flip)
        assert rc == 0 and got.tobytes() == want.tobytes(), "picture of pose-frame %d" % ref
        assert st == dict(num_scored=int((~np.isnan(score)).sum()), num_examined=dt.num_examined(320, 240), error_pixel=-1)
