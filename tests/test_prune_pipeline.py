"""A long run of the resident front-end with pose-frames let go (include/flame_stereo.h): add_frame, update_resident,
project_features, detect_features on every third frame, then prune_pose_frames down to the last four pose-frames with
first_new at the detections just appended -- 25 frames, in the manner of tests/test_pipeline.py.  After every stage the
resident set and the projected set equal the chained CPU checkers (the oracle's update, tests/frontend_ref.py,
tests/prune_ref.py) bit for bit, and the tracker never holds more frames than the kept pose-frames + 2."""
import numpy as np
import pytest

from flame_amd import synth_stereo as ss
from oracle import stereo_capi as so
from tests import prune_ref as pr
from tests.test_feature_frontend import CheckerSide, HipSide, assert_records_equal, geometry, true_map

gpu = pytest.mark.gpu
FIRST, LAST, EVERY, KEEP = 10, 35, 3, 4  # pose-frames 10, 13, ..., 34; frames 11 .. 35


def long_scene(w=320, h=240, seed=5):
    sc = ss.PlaneScene(w, h, seed=seed, normal=(0.2, -0.1, 1.0), distance=2.2)
    sc.add_camera(FIRST - 1, ss.rot([0, 1, 0], -0.004), [0.03, -0.002, 0.01])
    sc.add_camera(FIRST, np.eye(3), [0, 0, 0])
    for i, k in enumerate(range(FIRST + 1, LAST + 1)):
        sc.add_camera(k, ss.rot([0.1, 1, 0.05], 0.003 + 0.002 * i), [-0.02 - 0.017 * i, 0.003 + 0.001 * i, -0.008 - 0.004 * i])
    return sc


class PruningChecker(CheckerSide):
    def prune(self, keep, dropped, first_new):
        target = pr.target_of(keep)
        rc, st, out = pr.prune_pose_frames(self.feats, keep, {a: geometry(self.sc, a, target) for a in dropped}, target,
                                           self.sc.width, self.sc.height, first_new=first_new)
        assert rc == 0
        self.feats = out
        for a in dropped:
            del self.frames[a]
        return [st[k] for k in pr.STAT_NAMES] + [len(dropped)]

    def drop(self, k):
        del self.frames[k]

    def frame_count(self):
        return len(self.frames)


class PruningHip(HipSide):
    def prune(self, keep, dropped, first_new):
        target = max(keep)
        st = self.tr.prune_pose_frames(self.sp, target, keep,
                                       [dict(id=a, q_to_new=self.sc.relative(a, target)[0],
                                             t_to_new=self.sc.relative(a, target)[1]) for a in dropped], first_new)
        return [st[k] for k in pr.STAT_NAMES] + [st["num_frames_dropped"]]

    def drop(self, k):
        self.tr.drop_frame(k)

    def frame_count(self):
        return self.tr.frame_count()


def drive(sides, sc):
    def same(what):
        st = [s.state() for s in sides]
        for other in st[1:]:
            assert_records_equal(other[0], st[0][0], what + ": resident set")
            assert_records_equal(other[1], st[0][1], what + ": projected set")

    for s in sides:
        for k in (FIRST - 1, FIRST):
            s.add_frame(k)
    counts = [s.detect(FIRST, FIRST - 1, None, False, 0) for s in sides]
    assert len(set(counts)) == 1 and counts[0] > 100, counts
    same("detect pf %d" % FIRST)
    next_id, anchors, curr_pf = counts[0], [FIRST], FIRST
    log = dict(moved=0, invalidated=0, prunes=0, max_frames=0)
    for k in range(FIRST + 1, LAST + 1):
        for s in sides:
            if k - 2 not in anchors:  # the frame before the previous one, unless it is a pose-frame
                s.drop(k - 2)
            s.add_frame(k)
        stats = [s.update(k, curr_pf, anchors) for s in sides]
        assert all(x == stats[0] for x in stats), (k, stats)
        same("frame %d update" % k)
        kept = [s.project(k, anchors) for s in sides]
        assert len(set(kept)) == 1 and kept[0] > 0, (k, kept)
        same("frame %d project" % k)
        if (k - FIRST) % EVERY == 0:
            first_new = kept[0]
            counts = [s.detect(k, k - 1, true_map(sc, k), True, next_id) for s in sides]
            assert len(set(counts)) == 1, counts
            same("detect pf %d" % k)
            next_id += counts[0]
            anchors, curr_pf = anchors + [k], k
            if len(anchors) > KEEP:
                keep, dropped = anchors[-KEEP:], anchors[:-KEEP]
                st = [s.prune(keep, dropped, first_new) for s in sides]
                assert all(x == st[0] for x in st), (k, st)
                same("prune at pf %d" % k)
                assert st[0][-1] == len(dropped) == 1
                log["moved"] += st[0][1]
                log["invalidated"] += st[0][2]
                log["prunes"] += 1
                anchors = keep
                feats = sides[0].state()[0]
                assert np.isin(feats["frame_id"], anchors).all()
        for s in sides:
            # kept pose-frames + the current and the previous frame
            assert s.frame_count() <= len(anchors) + 2, (k, s.frame_count(), anchors)
            log["max_frames"] = max(log["max_frames"], s.frame_count())
    return sides[0].state()[0], log


def test_checker_long_run_prunes_and_keeps_tracking():
    """CPU only: the chained checkers alone.  The prune has work every time (features are moved, some are invalidated),
    the run goes on tracking afterwards and its memory stays bounded."""
    sc = long_scene()
    imgs = {c: sc.render(c) for c in sc.cams}
    feats, log = drive([PruningChecker(sc, imgs)], sc)
    print(log, feats.shape[0])
    assert log["prunes"] == 5 and log["moved"] > 50 and log["max_frames"] <= KEEP + 2
    assert feats.shape[0] > 100 and (feats["num_updates"] >= 2).sum() > 50


@gpu
@pytest.mark.parametrize("size", [(320, 240), (640, 480)])
def test_gpu_long_run_with_prunes_matches_checker(built, size):
    sc = long_scene(*size)
    imgs = {c: sc.render(c) for c in sc.cams}
    hip = PruningHip(sc, imgs)
    try:
        feats, log = drive([PruningChecker(sc, imgs), hip], sc)
    finally:
        hip.close()
    print(size, log, feats.shape[0])
    assert log["prunes"] == 5 and log["moved"] > 50 and log["max_frames"] <= KEEP + 2
