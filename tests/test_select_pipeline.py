"""The whole per-frame chain the way Flame::update() runs it, with the selection of the graph's vertices
(flame_stereo_select_graph_features) between the front-end and the regulariser and NO Python between the stages on the
product side:

    detect_features -> update_resident -> project_features -> select_graph_features -> flame_delaunay_triangulate ->
    project_graph -> sync_graph -> run -> interpolate_mesh -> (the map feeds the next detect_features)

twelve frames, four pose-frames, two prunes, once through the HIP library (C-ABI) and once through the chained CPU
checkers (the oracle's update, tests/frontend_ref.py, tests/select_ref.py, tests/prune_ref.py, oracle/sync_oracle.py,
oracle.run, the raster oracle), each side feeding its own outputs forward.  After every stage of every frame both sides
must hold the same bits.

The oracle-only variant runs on the CPU.  It asserts that every frame after the first graph both adds and removes at
least one vertex, and that the final map is close to the scene's closed-form truth.  The knobs that make it so:
  * STEP, the sideways motion per frame (0.04 m at 2.2 m: about 5 pixels): every frame some vertices leave the valid region on one
    side of the image -- removed --, while features that were detected a few frames ago converge below
    idepth_var_max_graph, and the ones the moving band edge passes come into the band -- added;
  * MIN_HEIGHT = -0.35: the band [-0.35, 4] cuts the image at about 70 % of its height (the plane is 2.2 m away: rows
    below cy + 0.35 / 2.2 * f are below the band), so the height test decides for every frame's set, and the camera
    sinks (TY per frame), which moves that edge across features.
"""
import numpy as np
import pytest

from flame_amd import synth
from flame_amd import synth_stereo as ss
from oracle import capi as oracle
from oracle import sync_oracle
from tests import select_ref as sr
from tests.helpers import OUT_KEYS, assert_state_equal
from tests.test_feature_frontend import assert_records_equal
from tests.test_prune_pipeline import PruningChecker, PruningHip

gpu = pytest.mark.gpu
W, H = 320, 240
FIRST, LAST, EVERY, KEEP = 10, 22, 3, 3  # pose-frames 10, 13, 16, 19, 22; prunes at 19 and 22
STEP, TY = 0.04, 0.006
MIN_HEIGHT, MAX_HEIGHT = -0.35, 4.0
GP = dict(min_height=MIN_HEIGHT, max_height=MAX_HEIGHT)
N_ITERS = 60
MIN_VERTICES = 20  # the graph starts with the first frame that selects this many
MARGIN = 8.0
REGION = (MARGIN, MARGIN, W - 2 * MARGIN, H - 2 * MARGIN)  # projectGraph's valid region


def make_scene():
    sc = ss.PlaneScene(W, H, seed=5, normal=(0.2, -0.1, 1.0), distance=2.2)
    sc.add_camera(FIRST - 1, ss.rot([0, 1, 0], -0.004), [0.03, -0.002, 0.01])
    sc.add_camera(FIRST, np.eye(3), [0, 0, 0])
    for i, k in enumerate(range(FIRST + 1, LAST + 1)):
        # (R, t) maps world points into the camera: t_y < 0 puts the camera BELOW the origin's height (y is down)
        sc.add_camera(k, ss.rot([0.1, 1, 0.05], 0.003 + 0.002 * i), [-0.02 - STEP * i, -TY * i, -0.008 - 0.004 * i])
    return sc


def world_poses(sc, ids):
    out = []
    for k in ids:
        R, t = sc.cams[k]
        out.append(dict(id=k, q=ss.quat_from_rot(R.T).astype(np.float32), t=(-R.T @ t).astype(np.float32)))
    return out


def projection_between(sc, a, b):
    q, t = sc.relative(a, b)
    R = (sc.cams[b][0] @ sc.cams[a][0].T).astype(np.float32)
    return q, t, (sc.K32 @ R @ sc.Kinv32).astype(np.float32)


class CheckerChain(PruningChecker):
    """The CPU checkers chained."""

    def __init__(self, sc, imgs):
        super().__init__(sc, imgs)
        self.ref, self.fid = None, None

    def select(self, anchors):
        rc, res = sr.select(self.feats, self.proj, self.sc.Kinv32, world_poses(self.sc, anchors), 1.0, GP)
        assert rc == 0
        return res

    def triangulate(self, pos):
        import flame_amd

        return flame_amd.delaunay(pos)  # host code of the library: needs no GPU

    def first_graph(self, g, fid):
        self.ref, self.fid = sync_oracle.RefGraph.from_flat(g, fid), fid

    def project_graph(self, q, t, KRKinv):
        flat = sync_oracle.flatten(self.ref, self.fid)
        keep = oracle.graph_project(flat["pos"], flat["x"], 1.0, self.sc.K32, self.sc.Kinv32, q, t, KRKinv, REGION)
        sync_oracle.absorb(self.ref, flat, self.fid)
        for i, f in enumerate(self.fid):
            self.ref.v[int(f)]["pos"] = flat["pos"][i].copy()
        return keep

    def sync_graph(self, sel, edges):
        sync_oracle.sync(self.ref, sel["feat_id"], sel["pos"], sel["data_term"], sel["data_weight"], edges)
        self.fid = sel["feat_id"]

    def run(self, n):
        flat = sync_oracle.flatten(self.ref, self.fid)
        assert oracle.run(flat, n) == 0
        sync_oracle.absorb(self.ref, flat, self.fid)

    def graph_state(self):
        return sync_oracle.flatten(self.ref, self.fid)

    def interpolate(self, tris):
        flat = sync_oracle.flatten(self.ref, self.fid)
        return oracle.raster_interpolate_mesh(tris, flat["pos"], flat["x"], H, W)

    def close(self):
        pass


class HipChain(PruningHip):
    """The product: flame_amd.stereo.FeatureTracker + flame_amd.Regularizer over the C-ABI."""

    def __init__(self, sc, imgs):
        import flame_amd
        from flame_amd.stereo import GraphParams

        super().__init__(sc, imgs)
        self.flame_amd = flame_amd
        self.reg = flame_amd.Regularizer(0)
        self.params = flame_amd.Params()
        self.gp = GraphParams(**GP)

    def select(self, anchors):
        return self.tr.select_graph_features(self.gp, 1.0, world_poses(self.sc, anchors))

    def triangulate(self, pos):
        return self.flame_amd.delaunay(pos)

    def first_graph(self, g, fid):
        self.reg.upload_graph(g)
        self.reg.set_feature_ids(fid)

    def project_graph(self, q, t, KRKinv):
        return self.reg.project_graph(self.sc.K32, self.sc.Kinv32, KRKinv, q, t, REGION, graph_scale=1.0)[0]

    def sync_graph(self, sel, edges):
        self.reg.sync_graph(sel["feat_id"], sel["pos"], sel["data_term"], sel["data_weight"], edges)

    def run(self, n):
        self.reg.run(self.params, n)

    def graph_state(self):
        return self.reg.download_state()

    def interpolate(self, tris):
        return self.reg.interpolate_mesh(tris, H, W)[0]

    def close(self):
        self.reg.close()
        super().close()


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
    prev, dense, prev_ids = None, None, None
    log = dict(prunes=0, frames_with_graph=0, added=[], removed=[], V=[], rejected=np.zeros(3, np.int64))
    for k in range(FIRST + 1, LAST + 1):
        for s in sides:
            if k - 2 not in anchors:
                s.drop(k - 2)
            s.add_frame(k)
        stats = [s.update(k, curr_pf, anchors) for s in sides]
        assert all(x == stats[0] for x in stats), (k, stats)
        same("frame %d update" % k)
        kept = [s.project(k, anchors) for s in sides]
        assert len(set(kept)) == 1 and kept[0] > 0, (k, kept)
        same("frame %d project" % k)
        # ---- which features become vertices
        sels = [s.select(anchors) for s in sides]
        for other in sels[1:]:
            for key in ("V",) + sr.COUNTERS:
                assert other[key] == sels[0][key], (k, key, other[key], sels[0][key])
            for key in sr.ARRAYS:
                assert other[key].tobytes() == sels[0][key].tobytes(), "frame %d select: %s" % (k, key)
        same("frame %d select (the stage only reads)" % k)
        sel = sels[0]
        log["V"].append(sel["V"])
        log["rejected"] += [sel["num_invalid"], sel["num_fail_var"], sel["num_fail_height"]]
        if sel["V"] >= MIN_VERTICES:
            trs = [s.triangulate(sl["pos"]) for s, sl in zip(sides, sels)]
            for tr_ in trs[1:]:
                assert np.array_equal(tr_[0], trs[0][0]) and np.array_equal(tr_[1], trs[0][1]), "frame %d triangulation" % k
            if prev is None:
                g = synth.assemble_graph(sel["pos"], sel["data_term"], trs[0][1], weight=sel["data_weight"])
                for s in sides:
                    s.first_graph(g, sel["feat_id"])
            else:
                q, t, KRKinv = projection_between(sc, prev, k)
                keeps = [s.project_graph(q, t, KRKinv) for s in sides]
                for kp in keeps[1:]:
                    assert np.array_equal(kp, keeps[0]), "frame %d: projectGraph keep mask" % k
                for s, sl, tr_ in zip(sides, sels, trs):
                    s.sync_graph(sl, tr_[1])
                now, before = set(sel["feat_id"].tolist()), set(prev_ids.tolist())
                log["added"].append(len(now - before))
                log["removed"].append(len(before - now))
            for s in sides:
                s.run(N_ITERS)
            states = [s.graph_state() for s in sides]
            for st in states[1:]:
                assert np.array_equal(st["x"].shape, states[0]["x"].shape)
                assert_state_equal(st, states[0], keys=OUT_KEYS, what="frame %d after %d steps" % (k, N_ITERS))
            maps = [s.interpolate(tr_[0]) for s, tr_ in zip(sides, trs)]
            for m in maps[1:]:
                assert np.array_equal(m, maps[0], equal_nan=True), "frame %d: dense inverse depth map" % k
            prev, dense, prev_ids = k, maps, sel["feat_id"]
            log["frames_with_graph"] += 1
        if (k - FIRST) % EVERY == 0:
            first_new = kept[0]
            # the rasteriser's map of this frame (where there is one) initialises the new features
            counts = [s.detect(k, k - 1, None if dense is None or prev != k else dense[i], True, next_id)
                      for i, s in enumerate(sides)]
            assert len(set(counts)) == 1, counts
            same("detect pf %d" % k)
            next_id += counts[0]
            anchors, curr_pf = anchors + [k], k
            if len(anchors) > KEEP:
                keep, dropped = anchors[-KEEP:], anchors[:-KEEP]
                st = [s.prune(keep, dropped, first_new) for s in sides]
                assert all(x == st[0] for x in st), (k, st)
                same("prune at pf %d" % k)
                log["prunes"] += 1
                anchors = keep
    return dense[0], prev, log


def check_run(sc, dense, last, log):
    print(log)
    assert last == LAST and log["prunes"] >= 1 and log["frames_with_graph"] >= 6, log
    # every frame after the first graph both adds and removes at least one vertex
    assert len(log["added"]) == log["frames_with_graph"] - 1
    assert min(log["added"]) >= 1 and min(log["removed"]) >= 1, log
    assert (log["rejected"][1:] > 0).all(), log  # the variance and the height test both reject something
    # the final map against the closed-form truth, as tests/test_pipeline.py does (the band leaves the lower part of the
    # image without vertices, so the map covers less of it than there)
    ys, xs = np.mgrid[0:H, 0:W]
    truth = sc.true_idepth(last, np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)).reshape(H, W)
    ok = ~np.isnan(dense)
    assert ok.mean() > 0.3, ok.mean()
    rel = np.abs(dense[ok] - truth[ok]) / truth[ok]
    print("coverage", ok.mean(), "median", np.median(rel), "p90", np.percentile(rel, 90))
    assert np.median(rel) < 0.02 and np.percentile(rel, 90) < 0.08, (np.median(rel), np.percentile(rel, 90))


def test_checker_chain_with_selection_recovers_the_plane():
    """CPU only: the chained checkers alone."""
    sc = make_scene()
    imgs = {c: sc.render(c) for c in sc.cams}
    dense, last, log = drive([CheckerChain(sc, imgs)], sc)
    check_run(sc, dense, last, log)


@gpu
def test_gpu_chain_with_selection_matches_checker_chain(built):
    import torch  # noqa: F401

    sc = make_scene()
    imgs = {c: sc.render(c) for c in sc.cams}
    sides = [CheckerChain(sc, imgs), HipChain(sc, imgs)]
    try:
        dense, last, log = drive(sides, sc)
    finally:
        for s in sides:
            s.close()
    check_run(sc, dense, last, log)
