"""What the host code behind include/flame_stereo.h shares between its entry points (flame_amd/csrc/stereo_context.hpp: the
arrays and how they grow, the ping-pong swaps, the front-stage skeleton, the decode of the error words), on a 64x48 camera:

  * the resident set is appended to across a reallocation (grow_keep): the old records move, the new ones are the checker's;
  * the two ping-pong pairs over project, project, prune (one record removed), project: after every step the host copies
    equal the checker and the device pointers name the records just read;
  * a set with a record of an unknown frame and a record that trips an assert, in both orders, through update_resident,
    project_features, prune_pose_frames and the arrays form of select: status and error_feature are the checkers';
  * create / every stage / set_camera to another size / every stage / destroy, three times in one process, without a HIP error.

Every device result is compared bit for bit with tests/frontend_ref.py, tests/prune_ref.py, tests/select_ref.py (and the oracle
for the update).  The pure functions behind all this have their own program, tests/cpp/stereo_host_test.cc.

The update's rule.  Flame::updateFeatureIDepths and projectFeatures run their feature loops under OpenMP (flame.cc:1307, 1777),
so which of pfs.at()'s exception and a FLAME_ASSERT ends the process is not defined there; include/flame_stereo.h fixes it as
"an unknown frame first" for both, and so do frontend_ref / prune_ref.  The oracle walks the update on one thread and stops at
the lower index; its two indices are taken from runs with one defect each and combined by the header's rule."""
import numpy as np
import pytest

from flame_amd import synth_stereo as ss
from oracle import stereo_capi as so
from tests import frontend_ref as fr
from tests import prune_cases as pc
from tests import prune_ref as pr
from tests import select_cases as sc_
from tests import select_ref as sr
from tests.test_feature_frontend import PAD, assert_records_equal, checker_detect

gpu = pytest.mark.gpu
W, H = 64, 48
INVALID_ARG, ASSERT = -1, -8
_SCENES = {}


def scene(w=W, h=H):
    """tests/prune_cases.scene at another size: pose-frames 10 .. 22, then frames 23 and 24."""
    if (w, h) not in _SCENES:
        sc = ss.PlaneScene(w, h, seed=5, normal=(0.2, -0.1, 1.0), distance=2.2)
        for i, k in enumerate(pc.PF_IDS):
            sc.add_camera(k, ss.rot([0.1, 1, 0.05], 0.006 * i), [-0.13 * i, 0.01 * i, -0.05 * i])
        sc.add_camera(23, ss.rot([0.1, 1, 0.05], 0.026), [-0.55, 0.042, -0.21])
        sc.add_camera(24, ss.rot([0.1, 1, 0.05], 0.028), [-0.58, 0.044, -0.22])
        _SCENES[(w, h)] = sc
    return _SCENES[(w, h)]


def grown(count):
    """Elements a device array gets when `count` no longer fit (stereo_host.hpp)."""
    return count + count // 2 + 16


def tracker(sc):
    from flame_amd.stereo import FeatureTracker

    return FeatureTracker(sc.K32, sc.Kinv32, sc.width, sc.height, border=PAD)


def view(feats):
    from flame_amd.stereo import FEATURE_DTYPE

    return np.ascontiguousarray(feats).view(FEATURE_DTYPE)


def poses_to(sc, anchors, k):
    return [dict(id=a, q_to_new=sc.relative(a, k)[0], t_to_new=sc.relative(a, k)[1]) for a in anchors]


def geos_to(sc, anchors, k):
    return {a: so.load_geometry(sc.K32, sc.Kinv32, *sc.relative(a, k)) for a in anchors}


def assert_device_sets(tr, feats, proj, what):
    """features_device / projected_device name the records get_features / get_projected just read."""
    from tests.metric_helpers import fetch

    for (ptr, n), host, name in ((tr.features_device(), feats, "resident"), (tr.projected_device(), proj, "projected")):
        assert n == host.shape[0], (what, name, n, host.shape)
        if n:
            assert ptr and fetch(ptr, (n,), host.dtype).tobytes() == host.tobytes(), (what, name)


# ---- append across a reallocation ------------------------------------------------------------------------------------

def detect_case():
    sc = scene()
    img = sc.render(22)
    base = pc.features(sc, 3, seed=11, anchors=(19,), special=False)
    return sc, img, base


def test_detect_case_crosses_both_capacities():
    sc, img, base = detect_case()
    cap0 = grown(3 + 1)  # set_features asks for n + 1
    rc, _, first, cells = checker_detect(sc, img, fr_geo(sc), 22, win=4, first_id=100)
    assert rc == 0 and cells == 16 * 12 == 192 and first.shape[0] > 0
    assert 3 + cells + 1 > cap0  # detect_features asks for n_res + n_cells + 1: the first call reallocates
    cap1 = grown(3 + cells + 1)
    rc, _, second, cells3 = checker_detect(sc, img, fr_geo(sc), 22, win=3, first_id=1000)
    assert rc == 0 and cells3 == 22 * 16 == 352 > 256 and second.shape[0] > first.shape[0]
    assert 3 + first.shape[0] + cells3 + 1 > cap1  # and so does the second, with 3 + len(first) records to move


def fr_geo(sc):
    return so.load_geometry(sc.K32, sc.Kinv32, *sc.relative(22, 19))


@gpu
def test_gpu_detect_appends_across_a_reallocation(built):
    from flame_amd.stereo import DetectParams, StereoParams

    sc, img, base = detect_case()
    q, t = sc.relative(22, 19)
    _, _, first, _ = checker_detect(sc, img, fr_geo(sc), 22, win=4, first_id=100)
    _, _, second, _ = checker_detect(sc, img, fr_geo(sc), 22, win=3, first_id=1000)
    with tracker(sc) as tr:
        tr.add_frame(22, img)
        tr.set_features(view(base))
        n1 = tr.detect_features(StereoParams(), DetectParams(detection_win_size=4), 22, q, t, first_id=100)
        out = tr.get_features()
        assert n1 == first.shape[0] and out.shape[0] == 3 + n1
        assert out[:3].tobytes() == base.tobytes()  # moved to the new buffer unchanged
        assert_records_equal(out[3:], first, "window 4")
        n2 = tr.detect_features(StereoParams(), DetectParams(detection_win_size=3), 22, q, t, first_id=1000)
        out2 = tr.get_features()
        assert n2 == second.shape[0] and out2.shape[0] == 3 + n1 + n2
        assert out2[:3 + n1].tobytes() == out.tobytes()
        assert_records_equal(out2[3 + n1:], second, "window 3")
        assert_device_sets(tr, out2, tr.get_projected(), "after two appends")


# ---- the ping-pong pairs -----------------------------------------------------------------------------------------------

ANCHORS = (16, 19, 22)


def ping_pong_case():
    """300 records; the checker's sets after project -> 23, project -> 24, prune 19 and 22 into 16 with one record removed (the
    records of the newer pose-frames leave 16's image on the side the camera came from), project -> 24."""
    sc = scene()
    feats = pc.features(sc, 300, seed=21, anchors=ANCHORS)
    steps = []
    rc, _, kept, cur = fr.project_features(feats, geos_to(sc, ANCHORS, 23), 23, W, H)
    assert rc == 0
    steps.append((kept, cur))
    rc, _, kept2, cur2 = fr.project_features(kept, geos_to(sc, ANCHORS, 24), 24, W, H)
    assert rc == 0
    steps.append((kept2, cur2))
    first_new = None
    for cand in range(kept2.shape[0], -1, -1):  # the largest first_new at which exactly one record goes
        rc, st, pruned = pr.prune_pose_frames(kept2, [16], geos_to(sc, (19, 22), 16), 16, W, H, cand)
        assert rc == 0
        if st["num_removed"] == 1:
            first_new = cand
            break
        assert st["num_removed"] == 0
    assert first_new is not None, "no orphan fails its move into pose-frame 16"
    steps.append((pruned, cur2))  # (the projected set is not touched)
    rc, _, kept4, cur4 = fr.project_features(pruned, geos_to(sc, (16,), 24), 24, W, H)
    assert rc == 0
    steps.append((kept4, cur4))
    return sc, feats, first_new, steps


def test_ping_pong_case_spans_two_groups_and_shrinks():
    sc, feats, first_new, steps = ping_pong_case()
    sizes = [feats.shape[0]] + [s[0].shape[0] for s in steps]
    print("records per step", sizes, "first_new", first_new)
    assert sizes[0] == 300 > 256 > 0 and sizes[1] < sizes[0] and sizes[3] == sizes[2] - 1 and sizes[4] > 0
    assert (steps[2][0]["frame_id"] == 16).all() and (steps[1][0]["frame_id"] != 16).any()


@gpu
def test_gpu_ping_pong_project_project_prune_project(built):
    from flame_amd.stereo import StereoParams

    sc, feats, first_new, steps = ping_pong_case()
    sp = StereoParams()
    with tracker(sc) as tr:
        tr.set_features(view(feats))
        calls = (("project 23", lambda: tr.project_features(sp, 23, poses_to(sc, ANCHORS, 23))),
                 ("project 24", lambda: tr.project_features(sp, 24, poses_to(sc, ANCHORS, 24))),
                 ("prune into 16", lambda: tr.prune_pose_frames(sp, 16, [16], poses_to(sc, (19, 22), 16), first_new)),
                 ("project 24 again", lambda: tr.project_features(sp, 24, poses_to(sc, (16,), 24))))
        for (what, call), (want_feats, want_proj) in zip(calls, steps):
            res = call()
            if what.startswith("prune"):
                assert res["num_removed"] == 1 and res["num_features"] == want_feats.shape[0], res
            else:
                assert res == want_feats.shape[0], (what, res)
            got, proj = tr.get_features(), tr.get_projected()
            assert_records_equal(got, want_feats, what + ": resident set")
            assert_records_equal(proj, want_proj, what + ": projected set")
            assert_device_sets(tr, got, proj, what)


# ---- which record fails first ------------------------------------------------------------------------------------------

def decode_case(order):
    """120 valid records in pose-frames 19 and 22; record i names frame 77, record j (of frame 19) has a negative idepth."""
    sc = scene()
    feats = pc.features(sc, 120, seed=31, anchors=(19, 22), special=False)
    feats["valid"] = 1
    i, j = (17, 64) if order == "unknown_first" else (64, 17)
    only_unknown, only_assert = feats.copy(), feats.copy()
    for f in (feats, only_unknown):
        f["frame_id"][i] = 77
    for f in (feats, only_assert):
        f["frame_id"][j] = 19
        f["idepth_mu"][j] = -0.5
    return sc, feats, only_unknown, only_assert, i, j


def oracle_update(sc, imgs, feats):
    poses = ss.poses_for(sc, [19, 22], 23, 22)
    frames = [dict(p, img_pad=so.make_frame(imgs[p["id"]], PAD)[0]) for p in poses]
    return so.update_feature_idepths(so.Params(), sc.K32, sc.Kinv32, W, H, PAD, frames, so.make_frame(imgs[23], PAD), 22,
                                     feats.copy())[0]


def expected_errors(order):
    """(status, error_feature) of the four entry points from the checkers alone."""
    sc, feats, only_unknown, only_assert, i, j = decode_case(order)
    imgs = {k: sc.render(k) for k in (19, 22, 23)}
    # the update: the oracle's index of each defect alone, an unknown frame first (see the module's docstring)
    assert oracle_update(sc, imgs, only_unknown) == 1 + i and oracle_update(sc, imgs, only_assert) == -(1 + j)
    assert oracle_update(sc, imgs, feats) == (1 + i if i < j else -(1 + j))  # (one thread: the lower index)
    want = {"update_resident": (INVALID_ARG, i)}
    want["project_features"] = fr.project_features(feats, geos_to(sc, (19, 22), 23), 23, W, H)[:2]
    rc, st, _ = pr.prune_pose_frames(feats, [22], geos_to(sc, (19,), 22), 22, W, H, 60)
    want["prune_pose_frames"] = (rc, st["error_feature"])
    rc, res = sr.select(feats, feats, sc.Kinv32, sc_.world_poses(sc, (19, 22)), 1.0)
    want["select_arrays"] = (rc, res["error_feature"])
    return sc, feats, imgs, want


@pytest.mark.parametrize("order", ["unknown_first", "assert_first"])
def test_checkers_name_the_three_rules(order):
    _, _, _, want = expected_errors(order)
    i, j = (17, 64) if order == "unknown_first" else (64, 17)
    assert want["update_resident"] == want["project_features"] == want["prune_pose_frames"] == (INVALID_ARG, i)
    assert want["select_arrays"] == ((INVALID_ARG, i) if i < j else (ASSERT, j))


@gpu
@pytest.mark.parametrize("order", ["unknown_first", "assert_first"])
def test_gpu_first_failing_record(built, order):
    from flame_amd.stereo import GraphParams, StereoParams

    sc, feats, imgs, want = expected_errors(order)
    sp = StereoParams()
    with tracker(sc) as tr:
        for k, img in imgs.items():
            tr.add_frame(k, img)
        got = {}
        tr.set_features(view(feats))
        rc, st = tr.update_resident(sp, 23, 22, ss.poses_for(sc, [19, 22], 23, 22), raise_on_error=False)
        got["update_resident"] = (rc, st["error_feature"])
        tr.set_features(view(feats))
        rc, st = tr.project_features(sp, 23, poses_to(sc, (19, 22), 23), raise_on_error=False)
        got["project_features"] = (rc, st["error_feature"])
        assert tr.get_features().tobytes() == feats.tobytes()
        rc, st = tr.prune_pose_frames(sp, 22, [22], poses_to(sc, (19,), 22), 60, raise_on_error=False)
        got["prune_pose_frames"] = (rc, st["error_feature"])
        assert tr.get_features().tobytes() == feats.tobytes() and tr.frame_count() == 3
        rc, res = tr.select_graph_features(GraphParams(), 1.0, sc_.world_poses(sc, (19, 22)), view(feats), view(feats),
                                           raise_on_error=False)
        got["select_arrays"] = (rc, res["error_feature"])
        assert res["V"] == 0
    print(order, got)
    assert got == want


# ---- create, use, resize, use, destroy -----------------------------------------------------------------------------------

def use_every_stage(tr, sc, hip_error):
    """One call of every stage at sc's size; project / detect / prune / select against their checkers."""
    from flame_amd.stereo import AlignParams, DetectParams, GraphParams, StereoParams

    w, h = sc.width, sc.height
    sp = StereoParams()
    imgs = {k: sc.render(k) for k in (16, 19, 22, 23)}
    for k in (16, 19, 22):
        tr.add_frame(k, imgs[k])
    tr.set_input(format=0, remap=0, raw_width=w, raw_height=h)
    assert tr.add_raw_frame(23, imgs[23])["n_outside"] == 0
    pad, gx, gy = tr.download_frame(23)
    assert pad.tobytes() == so.make_frame(imgs[23], PAD)[0].tobytes()
    hip_error("frames")
    feats = pc.features(sc, 150, seed=41, anchors=ANCHORS, special=False)
    # the update, on a host array and on the resident set, with the matches recorded; then their picture
    tr.set_record_matches(True)
    host = view(feats.copy())
    poses = ss.poses_for(sc, list(ANCHORS), 23, 22)
    rc, st = tr.update_feature_idepths(sp, 23, 22, poses, host)
    tr.set_features(view(feats))
    rc2, st2 = tr.update_resident(sp, 23, 22, poses)
    assert rc == rc2 == 0 and st == st2 and tr.get_features().tobytes() == host.tobytes()
    frames = [dict(p, img_pad=so.make_frame(imgs[p["id"]], PAD)[0]) for p in poses]
    want = feats.copy()
    rc_o, st_o = so.update_feature_idepths(so.Params(), sc.K32, sc.Kinv32, w, h, PAD, frames, so.make_frame(imgs[23], PAD), 22, want)
    assert rc_o == 0 and st["num_idepth_updates"] == st_o[0] > 0 and host.tobytes() == want.tobytes()
    assert tr.draw_matches()["num_features"] == 150
    tr.set_record_matches(False)
    hip_error("update")
    # project, the pictures over the projected set, select, detect, prune
    updated = host.view(so.FEATURE_DTYPE)
    rc, _, kept, cur = fr.project_features(updated, geos_to(sc, ANCHORS, 23), 23, w, h)
    assert rc == 0 and tr.project_features(sp, 23, poses_to(sc, ANCHORS, 23)) == kept.shape[0] > 0
    assert_records_equal(tr.get_features(), kept, "project")
    assert_records_equal(tr.get_projected(), cur, "projected")
    img, nc, nu = tr.draw_features(23, 1e-2)
    assert img.shape == (h, w, 3) and 0 < nc + nu <= cur.shape[0]
    world = sc_.world_poses(sc, ANCHORS)
    rc, want = sr.select(kept, cur, sc.Kinv32, world, 1.0)
    for res in (tr.select_graph_features(GraphParams(), 1.0, world),
                tr.select_graph_features(GraphParams(), 1.0, world, view(kept), view(cur))):
        assert rc == 0 and res["V"] == want["V"] and res["feat_index"].tolist() == want["feat_index"].tolist()
        assert res["data_term"].tobytes() == want["data_term"].tobytes() and res["pos"].tobytes() == want["pos"].tobytes()
    q, t = sc.relative(22, 19)
    geo = so.load_geometry(sc.K32, sc.Kinv32, q, t)
    rc, _, new, _ = checker_detect(sc, imgs[22], geo, 22, win=8, first_id=5000)
    assert rc == 0 and tr.detect_features(sp, DetectParams(detection_win_size=8), 22, q, t, first_id=5000) == new.shape[0] > 0
    both = np.concatenate([kept, new])
    assert_records_equal(tr.get_features(), both, "detect")
    img, st = tr.draw_detections(sp, DetectParams(detection_win_size=8), 22, q, t)
    assert st["error_pixel"] == -1 and st["num_examined"] == (w - 8) * (h - 8)
    rc, st_c, pruned = pr.prune_pose_frames(both, [19, 22], geos_to(sc, (16,), 22), 22, w, h, kept.shape[0])
    st = tr.prune_pose_frames(sp, 22, [19, 22], poses_to(sc, (16,), 22), kept.shape[0])
    assert rc == 0 and all(st[k] == st_c[k] for k in pr.STAT_NAMES) and st["num_frames_dropped"] == 1
    assert_records_equal(tr.get_features(), pruned, "prune")
    hip_error("front end")
    # the pyramid and one linearisation against a flat map
    for k in (22, 23):
        tr.build_pyramid(k, 2)
    sys = tr.align_linearize(AlignParams(), 22, 23, 1, np.full((h, w), 0.45, np.float32), *[np.float64(v) for v in sc.relative(22, 23)])
    assert sys["n_used"] > 0
    hip_error("alignment")


@gpu
def test_gpu_lifecycle_create_use_resize_destroy(built):
    small, other = scene(), scene(80, 56)
    for turn in range(3):
        tr = tracker(small)
        try:
            def hip_error(what):
                assert tr._L.flame_stereo_last_hip_error(tr._ctx) == 0, (turn, what)

            use_every_stage(tr, small, hip_error)
            assert tr.frame_count() == 3
            tr.set_camera(other.K32, other.Kinv32, other.width, other.height, border=PAD)  # drops the frames and the spares
            assert tr.frame_count() == 0
            hip_error("set_camera")
            use_every_stage(tr, other, hip_error)
            assert tr.frame_count() == 3
        finally:
            tr.close()
