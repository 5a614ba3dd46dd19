"""The four feature stages of flame_amd/csrc/feature_kernels.hip past 256 workgroups and at the edges of projection and
detection (the inputs: tests/feature_edge_cases.py).

CPU part: on the checkers' output alone, every case reaches the path it names -- records move at or past workgroup 256,
the keep patterns keep what they say, the rectangle's known answers hold, the special values take their branches.
GPU part: the HIP stages are bit-equal to the checkers on the same inputs; no comparison has a tolerance.

Left out: nothing of the issue's list.  65 536 records are exactly 256 workgroups (indices 0..255): no record lies at or
past workgroup 256 there, so the floor of 1 000 such records cannot apply to that count (nor, as stated, to 65 537); it is
kept as the largest count at which group_base's loop takes a single turn."""
import numpy as np
import pytest

from oracle import stereo_capi as so
from tests import feature_edge_cases as fe
from tests import frontend_ref as fr
from tests import prune_cases as pc
from tests import prune_ref as pr
from tests import select_cases as sc_
from tests.test_feature_frontend import assert_records_equal
from tests.test_select_graph_features import assert_same_result

gpu = pytest.mark.gpu
F32 = np.float32
ASSERT = -8  # FLAME_NLTGV2_ERR_ASSERT


# ---- CPU, A: every case moves records at or past workgroup 256 -----------------------------------------------------------

def assert_reaches_past_256(source, n_items, what):
    """source: the input index (or cell) of every record of the compacted output."""
    groups = (n_items + fe.GROUP - 1) // fe.GROUP
    past = int((source >= fe.FIRST_PAST).sum())
    print(what, "items", n_items, "workgroups", groups, "output", source.size, "at or past workgroup 256", past)
    assert groups >= 256 and (groups > 256 or n_items == fe.BIG_COUNTS[0]), (what, groups)
    assert (source < fe.FIRST_PAST).any(), what  # a workgroup before number 256 has a non-zero count
    assert np.all(np.diff(source) > 0), what     # (stable order)
    if fe.floor_applies(n_items):
        assert past >= fe.FLOOR, (what, past)
    else:
        assert past <= 1, (what, past)


@pytest.mark.parametrize("letterbox", [0, 1])
@pytest.mark.parametrize("n", fe.BIG_COUNTS)
def test_big_projection_keeps_records_past_workgroup_256(n, letterbox):
    rc, err, kept, cur = fe.big_project(n, letterbox)
    assert rc == 0 and kept.shape == cur.shape and np.array_equal(kept["id"], cur["id"])
    assert kept.shape[0] < n  # (a compaction, not a copy)
    assert_reaches_past_256(kept["id"].astype(np.int64), n, "project %d letterbox %d" % (n, letterbox))


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("n", fe.BIG_COUNTS)
def test_big_prune_keeps_records_past_workgroup_256(n, which):
    first_new = fe.big_first_new(n)[which]
    rc, st, out = fe.big_prune(n, first_new)
    assert rc == 0 and st["num_examined"] == n and st["num_moved"] > n // 5 and st["num_invalidated"] > 0
    if which == 0:  # committed in place: the three totals are sums over all workgroups
        assert st["num_removed"] == 0 and out.shape[0] == n
    else:           # compacted into the other buffer
        assert st["num_removed"] > 0 and out.shape[0] == n - st["num_removed"]
    assert_reaches_past_256(out["id"].astype(np.int64), n, "prune %d first_new %d" % (n, first_new))
    if fe.floor_applies(n):  # moved and invalidated records behind workgroup 256 too: their counts are summed the same way
        tail = out[out["id"] >= fe.FIRST_PAST]
        keep, dropped, target = pc.split(2)
        src = fe.big_features(n)[tail["id"]]
        assert (np.isin(src["frame_id"], dropped) & (tail["valid"] == 1)).sum() >= 100
        if which == 0:  # (behind first_new a failing record is removed, not marked)
            assert (np.isin(src["frame_id"], dropped) & (tail["valid"] == 0) & (src["valid"] == 1)).sum() >= 10


@pytest.mark.parametrize("form", ["arrays", "resident"])
@pytest.mark.parametrize("n", fe.BIG_COUNTS)
def test_big_selection_takes_records_past_workgroup_256(n, form):
    feats, cur = fe.big_select_inputs(n, form)
    assert feats.shape[0] == cur.shape[0] == n  # the resident form too: the projection kept every record
    rc, res = fe.big_select(n, form)
    assert rc == 0 and res["V"] + res["num_invalid"] + res["num_fail_var"] + res["num_fail_height"] == n
    assert res["num_fail_var"] > n // 10 and res["num_fail_height"] > 0
    assert (res["num_invalid"] > n // 20) if form == "arrays" else (res["num_invalid"] == 0)
    assert_reaches_past_256(res["feat_index"].astype(np.int64), n, "select %d %s" % (n, form))


@pytest.mark.parametrize("shape", fe.BIG_DETECT)
def test_big_detection_emits_cells_past_workgroup_256(shape):
    w, h, win = shape
    rc, _, out, n_cells = fe.big_detect(w, h, win, 0)
    assert rc == 0 and n_cells == 76800 and np.array_equal(out["id"], np.arange(out.shape[0]))
    assert_reaches_past_256(fe.cells_of(out, win, w), n_cells, "detect %dx%d window %d" % shape)
    rc, _, out2, _ = fe.big_detect(w, h, win, fe.PREFIX_COUNT)
    assert np.array_equal(out2["id"], fe.PREFIX_COUNT + np.arange(out.shape[0]))


# ---- CPU, B: projection ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", fe.PROJECT_COUNTS)
def test_projection_keep_patterns_keep_what_they_name(n):
    for pattern in fe.PATTERNS:
        feats, (rc, _, kept, cur) = fe.shape_case(n, pattern)
        assert rc == 0, (n, pattern)
        want = {"all": np.arange(n), "none": np.zeros(0, np.int64), "first": np.array([0]), "last": np.array([n - 1]),
                "half": np.nonzero(feats["valid"])[0]}[pattern]
        assert kept["id"].tolist() == want.tolist() == cur["id"].tolist(), (n, pattern)
        assert (cur["frame_id"] == 14).all() and (cur["valid"] == 1).all()
    if n > 1:
        half = fe.shape_case(n, "half")[0]["valid"]
        assert 0 < half.sum() < n


@pytest.mark.parametrize("letterbox", [0, 1])
def test_projection_rectangle_known_answers(letterbox):
    feats, inside, finite = fe.rect_case(letterbox)
    assert fe.region(letterbox) == ((4, 4, 312, 232), (4, 84, 312, 72))[letterbox]
    geo = fe.geos_of(fe.RECT_POSES)[10]
    assert np.array_equal(np.float32(list(geo.KRKinv)), np.eye(3, dtype=np.float32).ravel())
    # maxDepthProjection under the identity returns the input bit for bit
    x, y, nid, ok = fr.project_idepth(geo, feats["x"][finite], feats["y"][finite], feats["idepth_mu"][finite])
    assert ok.all() and (fe.bits(x) == fe.bits(feats["x"][finite])).all() and (fe.bits(y) == fe.bits(feats["y"][finite])).all()
    assert (fe.bits(nid) == 0).all()
    rc, _, kept, cur = fr.project_features(feats, fe.geos_of(fe.RECT_POSES), 14, fe.W, fe.H, do_letterbox=bool(letterbox))
    assert rc == 0
    # the half-open rule: the low edge is in, the high edge is out, one ulp below the high edge is in, ...
    assert kept["id"].tolist() == feats["id"][inside].tolist()
    assert (fe.bits(cur["x"]) == fe.bits(feats["x"][inside])).all() and (fe.bits(cur["y"]) == fe.bits(feats["y"][inside])).all()
    assert inside.sum() == 9 and (~inside).sum() == 17 and (~finite).sum() == 7


def test_projection_special_inverse_depths_take_their_branches():
    feats, at = fe.special_case()
    assert fe.SUBNORMAL > 0 and fe.SUBNORMAL < np.finfo(np.float32).tiny
    assert float(fe.E6) < 1e-6 <= float(fe.ulp_up(fe.E6))  # (double)idepth_mu < 1e-6 splits the nearest float from its upper neighbour
    rc, err, kept, cur = fr.project_features(feats, fe.geos_of(fe.SPECIAL_POSES), 14, fe.W, fe.H)
    assert rc == 0, (rc, err)  # none of them asserts
    got = {int(i): k for k, i in enumerate(kept["id"])}
    for frame in (10, 11):
        i = at["neg_zero@%d" % frame]  # -0.0 is not negative and takes the max-depth branch: +0 comes back, the variance x 1
        c = cur[got[i]]
        assert fe.bits(c["idepth_mu"]) == 0 and fe.bits(c["idepth_var"]) == fe.bits(feats["idepth_var"][i])
        assert fe.bits(kept["idepth_mu"][got[i]]) == 0x80000000  # (the resident record is not rewritten)
    for name in ("e6_lo", "e6", "e6_hi"):
        i = at[name + "@11"]
        same_var = fe.bits(cur["idepth_var"][got[i]]) == fe.bits(feats["idepth_var"][i])
        assert same_var == (float(feats["idepth_mu"][i]) < 1e-6), name
        assert 0 < cur["idepth_mu"][got[i]] < feats["idepth_mu"][i]
    # the camera centre (idepth +inf) seen from 131 072 m behind it: idepth 2^-17, the variance x (2^-17 / inf)^4 = 0
    c = cur[got[at["inf@11"]]]
    assert c["idepth_mu"] == F32(2.0 ** -17) and fe.bits(c["idepth_var"]) == 0
    # a subnormal inverse depth is a depth of 2^127: K p overflows, the point is dropped (not an assert)
    assert at["subnormal@10"] not in got and at["subnormal@11"] not in got
    # variances are carried through
    assert np.isinf(cur["idepth_var"][got[at["var_inf"]]]) and np.isnan(cur["idepth_var"][got[at["var_nan"]]])
    assert np.isinf(cur["idepth_var"][got[at["var_inf_mu0"]]]) and np.isnan(cur["idepth_var"][got[at["var_nan_mu0"]]])


def test_projection_onto_the_camera_plane_asserts_at_the_lowest_index():
    feats = fe.plane_case()
    geos = fe.geos_of(fe.PLANE_POSES)
    i = fe.PLANE_AT[1]
    x, y, nid, ok = fr.project_idepth(geos[12], feats["x"][i:i + 1], feats["y"][i:i + 1], feats["idepth_mu"][i:i + 1])
    assert not ok[0]  # the third coordinate is 2 - 2 = 0 exactly
    rc, err, kept, cur = fr.project_features(feats, geos, 14, fe.W, fe.H)
    assert (rc, err, kept, cur) == (ASSERT, fe.PLANE_AT[1], None, None)  # PLANE_AT[0] is invalid: never projected


def test_projection_pose_table_of_32_uses_first_middle_and_last():
    feats, (rc, _, kept, cur) = fe.table_case()
    assert rc == 0 and len(fe.TABLE_POSES) == 32
    for a in fe.TABLE_USED:
        assert (kept["frame_id"] == a).sum() > 100
    assert 0 < kept.shape[0] < (feats["valid"] == 1).sum()  # some leave the image


# ---- CPU, C: detection ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", fe.DETECT_SHAPES)
def test_detection_shapes_reach_their_paths(shape):
    w, h, win, letterbox, what = shape
    rc, _, out, n_cells = fe.shape_detect(w, h, win, letterbox)
    r_lo, r_hi, c_lo, c_hi = fe.candidate_range(w, h, letterbox)
    assert rc == 0 and n_cells == -(-w // win) * -(-h // win)
    if shape in fe.EMPTY_RANGE:
        assert (r_hi <= r_lo or c_hi <= c_lo) and out.shape[0] == 0
        return
    assert out.shape[0] > 0 and np.array_equal(out["id"], 11 + np.arange(out.shape[0]))
    assert ((out["y"] >= r_lo) & (out["y"] < r_hi) & (out["x"] >= c_lo) & (out["x"] < c_hi)).all()
    if win >= 64:
        assert n_cells == 1 and out.shape[0] == 1 and win * win > 64 * 64 - 1
    if (w, h) == (9, 9):
        assert out.shape[0] == 1 and (out["x"][0], out["y"][0]) == (4, 4)  # the only candidate pixel
    if win == 1:
        assert out.shape[0] > 0.8 * (r_hi - r_lo) * (c_hi - c_lo)  # random bytes: nearly every cell emits


@pytest.mark.parametrize("win", fe.MASK_WINS)
def test_mask_points_block_the_cell_the_float_division_names(win):
    w, h = fe.SMALL
    pts = fe.mask_points(win)
    rc, _, base, _ = fe.mask_detect(win, None)
    assert rc == 0
    base_cells = fe.cells_of(base, win, w)
    kinds = set()
    for i, (x, y, kind) in enumerate(pts):
        rc, _, out, _ = fe.mask_detect(win, i)
        cell = fe.cell_named(x, y, win)
        assert rc == 0, (win, i)
        left = base_cells != cell
        assert np.array_equal(fe.cells_of(out, win, w), base_cells[left]), (win, i, kind)
        assert np.array_equal(out["x"], base["x"][left]) and np.array_equal(out["y"], base["y"][left])
        if kind in ("boundary", "below"):
            assert cell in base_cells, (win, i, kind)  # the point takes a cell away that would have emitted
        if kind == "boundary":  # on the boundary the point belongs to the cell that starts there
            assert cell == (int(y) // win) * -(-w // win) + int(x) // win
        kinds.add(kind)
    assert kinds == {"boundary", "below", "partial", "zero", "corner"}
    # one ulp below a boundary the float quotient may round up to the boundary's cell: the rule is the division's, not floor's
    below = [(x, y) for x, y, kind in pts if kind == "below"]
    assert all(fe.cell_named(x, y, win) in base_cells for x, y in below)
    rc, _, out_all, _ = fe.mask_detect(win, "all")
    named = {fe.cell_named(x, y, win) for x, y, _ in pts}
    assert rc == 0 and np.array_equal(fe.cells_of(out_all, win, w), base_cells[~np.isin(base_cells, list(named))])
    # as the projected set: the points inside the valid region, unchanged by the projection
    f, cur = fe.mask_projected(win)
    assert 4 <= cur.shape[0] < f.shape[0]
    sel = np.isin(f["id"], cur["id"])
    assert (fe.bits(cur["x"]) == fe.bits(f["x"][sel])).all() and (fe.bits(cur["y"]) == fe.bits(f["y"][sel])).all()
    rc, _, out_p, _ = fe.mask_detect(win, "projected")
    assert rc == 0 and out_p.shape[0] < base.shape[0]


def test_idepth_map_specials_are_copied_and_only_nan_falls_back():
    m, winners, (rc, _, out, _) = fe.map_case()
    assert rc == 0 and out.shape[0] == winners.shape[0] >= 2 * len(fe.MAP_SPECIALS)
    want = np.array(fe.MAP_SPECIALS, np.float32)[np.arange(out.shape[0]) % len(fe.MAP_SPECIALS)]
    nan = np.isnan(want)
    assert (fe.bits(out["idepth_mu"][~nan]) == fe.bits(want[~nan])).all()
    assert (out["idepth_mu"][nan] == F32(0.01)).all() and nan.sum() >= 2
    assert {int(b) for b in fe.bits(out["idepth_mu"])} >= {0, 0x80000000, 0x7f800000, 0xff800000, int(fe.bits(F32(2.0 ** -130))[0])}


def test_thresholds_pass_on_equality():
    w, h = fe.SMALL
    _, gx, gy = so.make_frame(fe.ramp_image(), fe.PAD)
    inner = (slice(fe.PAD + 4, fe.PAD + h - 4), slice(fe.PAD + 4, fe.PAD + w - 4))
    assert (gx[inner] == 2).all() and (gy[inner] == 0).all()
    ex, ey, ok = fr.reference_epiline(so.load_geometry(fe.K_SMALL, fe.KINV_SMALL, fe.IDENT_Q, fe.MASK_T), F32([5, 20]), F32([7, 30]))
    assert ok.all() and (np.abs(ex) == 1).all() and (ey == 0).all()
    rc, _, out, n_cells = fe.ramp_detect(2.0)  # g2 = 4 = |gradient|^2 = score: both tests are `<`
    assert rc == 0 and out.shape[0] == n_cells == 12
    rc, _, none, _ = fe.ramp_detect(float(fe.ulp_up(2.0)))
    assert rc == 0 and none.shape[0] == 0


@pytest.mark.parametrize("first_id", fe.WRAP_IDS)
def test_ids_wrap_as_uint32(first_id):
    rc, _, out, _ = fe.wrap_detect(first_id)
    assert rc == 0 and out.shape[0] >= 4
    assert out["id"][:4].tolist() == [(first_id + k) % 2 ** 32 for k in range(4)]
    if first_id == 2 ** 32 - 2:
        assert out["id"][2] == 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _tracker(K, Kinv, w, h):
    from flame_amd.stereo import FeatureTracker

    return FeatureTracker(K, Kinv, w, h, border=fe.PAD)


def _hd_tracker():
    sc = fe.hd_scene()
    return _tracker(sc.K32, sc.Kinv32, sc.width, sc.height)


def _view(a):
    from flame_amd.stereo import FEATURE_DTYPE

    return np.ascontiguousarray(a).view(FEATURE_DTYPE)


# A

@gpu
@pytest.mark.parametrize("letterbox", [0, 1])
@pytest.mark.parametrize("n", fe.BIG_COUNTS)
def test_gpu_big_project_matches_checker(built, n, letterbox):
    from flame_amd.stereo import StereoParams

    sc = fe.hd_scene()
    rc, _, kept, cur = fe.big_project(n, letterbox)
    with _hd_tracker() as tr:
        tr.set_features(_view(fe.big_features(n, letterbox)))
        m = tr.project_features(StereoParams(do_letterbox=letterbox), sc_.CUR, sc_.project_poses(sc))
        assert m == kept.shape[0] and tr.features_device()[1] == m and tr.projected_device()[1] == m
        assert_records_equal(tr.get_features(), kept, "project %d: resident set" % n)
        assert_records_equal(tr.get_projected(), cur, "project %d: projected set" % n)


@gpu
@pytest.mark.parametrize("form", ["resident", "host"])
@pytest.mark.parametrize("n", fe.BIG_COUNTS)
def test_gpu_big_prune_matches_checker(built, n, form):
    from flame_amd.stereo import StereoParams

    sc = fe.hd_scene()
    keep, dropped, target = pc.split(2)
    poses = pc.dropped_poses(sc, dropped, target)
    with _hd_tracker() as tr:
        for first_new in fe.big_first_new(n):
            rc_c, st_c, ref = fe.big_prune(n, first_new)
            if form == "resident":
                tr.set_features(_view(fe.big_features(n)))
                rc, st = tr.prune_pose_frames(StereoParams(), target, keep, poses, first_new, raise_on_error=False)
                out = tr.get_features()
                assert tr.features_device()[1] == ref.shape[0]
            else:
                rc, out, st = tr.prune_features(StereoParams(), target, keep, poses, _view(fe.big_features(n).copy()), first_new,
                                                raise_on_error=False)
            assert rc == rc_c == 0
            for k in pr.STAT_NAMES:
                assert st[k] == st_c[k], (n, form, first_new, k, st, st_c)
            assert_records_equal(out, ref, "prune %d %s first_new %d" % (n, form, first_new))


@gpu
@pytest.mark.parametrize("form", ["arrays", "resident"])
@pytest.mark.parametrize("n", fe.BIG_COUNTS)
def test_gpu_big_select_matches_checker(built, n, form):
    from flame_amd.stereo import GraphParams, StereoParams

    sc = fe.hd_scene()
    world = sc_.world_poses(sc)
    feats, cur = fe.big_select_inputs(n, form)
    rc_c, ref = fe.big_select(n, form)
    with _hd_tracker() as tr:
        if form == "resident":
            tr.set_features(_view(fe.big_survivors(n)))
            assert tr.project_features(StereoParams(), sc_.CUR, sc_.project_poses(sc)) == n
        for copy_mode in (0, 1):
            tr.set_graph_copy(copy_mode)
            args = (_view(feats), _view(cur)) if form == "arrays" else ()
            rc, got = tr.select_graph_features(GraphParams(**fe.SELECT_GP), fe.SELECT_SCALE, world, *args, raise_on_error=False)
            assert rc == rc_c == 0
            assert_same_result(got, ref, "select %d %s copy %d" % (n, form, copy_mode))
        if form == "resident":  # the stage only reads
            assert tr.get_features().tobytes() == feats.tobytes() and tr.get_projected().tobytes() == cur.tobytes()


@gpu
@pytest.mark.parametrize("prefix", [0, 1])
@pytest.mark.parametrize("shape", fe.BIG_DETECT)
def test_gpu_big_detect_matches_checker(built, shape, prefix):
    from flame_amd import synth_stereo as ss
    from flame_amd.stereo import DetectParams, StereoParams

    w, h, win = shape
    first_id = fe.PREFIX_COUNT if prefix else 0
    rc, _, ref, n_cells = fe.big_detect(w, h, win, first_id)
    K, Kinv = ss.intrinsics(w, h)
    with _tracker(K, Kinv, w, h) as tr:
        tr.add_frame(7, fe.random_image(w, h))
        head = _view(fe.big_features(fe.PREFIX_COUNT))[:fe.PREFIX_COUNT if prefix else 0]
        if prefix:
            tr.set_features(head)
        rc, st = tr.detect_features(StereoParams(), DetectParams(detection_win_size=win), 7, fe.DETECT_Q, fe.DETECT_T,
                                    first_id=first_id, raise_on_error=False)
        assert rc == 0 and st["num_examined"] == n_cells and st["num_features"] == ref.shape[0]
        out = tr.get_features()
        assert out.shape[0] == head.shape[0] + ref.shape[0]
        assert out[:head.shape[0]].tobytes() == head.tobytes()  # the resident prefix comes back byte-identical
        assert_records_equal(out[head.shape[0]:], ref, "detect %dx%d window %d prefix %d" % (w, h, win, prefix))


# B

def _gpu_project(tr, feats, poses, cur_id=14, letterbox=0):
    from flame_amd.stereo import StereoParams

    tr.set_features(_view(feats))
    rc, st = tr.project_features(StereoParams(do_letterbox=letterbox), cur_id, list(poses), raise_on_error=False)
    return rc, st


def _same_as_checker(tr, st, kept, cur, what):
    assert st["num_features"] == kept.shape[0] and st["error_feature"] == -1, (what, st)
    assert_records_equal(tr.get_features(), kept, what + ": resident set")
    assert_records_equal(tr.get_projected(), cur, what + ": projected set")


@gpu
@pytest.mark.parametrize("n", fe.PROJECT_COUNTS)
def test_gpu_project_shapes_and_keep_patterns(built, n):
    with _tracker(fe.K_EXACT, fe.KINV_EXACT, fe.W, fe.H) as tr:
        for pattern in fe.PATTERNS:
            feats, (rc_c, _, kept, cur) = fe.shape_case(n, pattern)
            rc, st = _gpu_project(tr, feats, fe.SHAPE_POSES)
            assert rc == rc_c == 0 and st["num_examined"] == n
            _same_as_checker(tr, st, kept, cur, "project %d %s" % (n, pattern))


@gpu
@pytest.mark.parametrize("letterbox", [0, 1])
def test_gpu_project_rectangle_edges(built, letterbox):
    feats, inside, _ = fe.rect_case(letterbox)
    rc_c, _, kept, cur = fr.project_features(feats, fe.geos_of(fe.RECT_POSES), 14, fe.W, fe.H, do_letterbox=bool(letterbox))
    with _tracker(fe.K_EXACT, fe.KINV_EXACT, fe.W, fe.H) as tr:
        rc, st = _gpu_project(tr, feats, fe.RECT_POSES, letterbox=letterbox)
        assert rc == rc_c == 0
        assert tr.get_features()["id"].tolist() == feats["id"][inside].tolist()  # the known answers
        _same_as_checker(tr, st, kept, cur, "rectangle letterbox %d" % letterbox)


@gpu
def test_gpu_project_special_inverse_depths(built):
    feats, at = fe.special_case()
    rc_c, _, kept, cur = fr.project_features(feats, fe.geos_of(fe.SPECIAL_POSES), 14, fe.W, fe.H)
    with _tracker(fe.K_EXACT, fe.KINV_EXACT, fe.W, fe.H) as tr:
        rc, st = _gpu_project(tr, feats, fe.SPECIAL_POSES)
        assert rc == rc_c == 0
        _same_as_checker(tr, st, kept, cur, "special inverse depths")


@gpu
def test_gpu_project_onto_the_camera_plane_is_an_assert(built):
    feats = fe.plane_case()
    with _tracker(fe.K_EXACT, fe.KINV_EXACT, fe.W, fe.H) as tr:
        rc, st = _gpu_project(tr, feats, fe.PLANE_POSES)
        assert (rc, st["error_feature"], st["num_features"]) == (ASSERT, fe.PLANE_AT[1], 0)
        assert tr.get_features().tobytes() == feats.tobytes() and tr.get_projected().shape[0] == 0  # nothing committed
        ok = feats.copy()
        ok["valid"][list(fe.PLANE_AT)] = 0
        rc_c, _, kept, cur = fr.project_features(ok, fe.geos_of(fe.PLANE_POSES), 14, fe.W, fe.H)
        rc, st = _gpu_project(tr, ok, fe.PLANE_POSES)
        assert rc == rc_c == 0
        _same_as_checker(tr, st, kept, cur, "after the assert")


@gpu
def test_gpu_project_pose_table_of_32(built):
    from flame_amd import synth_stereo as ss

    feats, (rc_c, _, kept, cur) = fe.table_case()
    K, Kinv = ss.intrinsics(fe.W, fe.H)
    with _tracker(K, Kinv, fe.W, fe.H) as tr:
        rc, st = _gpu_project(tr, feats, fe.TABLE_POSES, cur_id=200)
        assert rc == rc_c == 0
        _same_as_checker(tr, st, kept, cur, "pose table of 32")


# C

def _gpu_detect(tr, img, q, t, ref_id=7, letterbox=0, **kw):
    from flame_amd.stereo import DetectParams, StereoParams

    dp = DetectParams(**{k: kw.pop(k) for k in ("detection_win_size", "min_grad_mag") if k in kw})
    tr.add_frame(ref_id, np.ascontiguousarray(img))
    return tr.detect_features(StereoParams(do_letterbox=letterbox), dp, ref_id, q, t, raise_on_error=False, **kw)


@gpu
@pytest.mark.parametrize("shape", fe.DETECT_SHAPES)
def test_gpu_detect_shapes(built, shape):
    from flame_amd import synth_stereo as ss
    from flame_amd.stereo import DetectParams, StereoParams

    w, h, win, letterbox, what = shape
    rc_c, _, ref, n_cells = fe.shape_detect(w, h, win, letterbox)
    K, Kinv = ss.intrinsics(w, h)
    with _tracker(K, Kinv, w, h) as tr:
        rc, st = _gpu_detect(tr, fe.random_image(w, h), fe.DETECT_Q, fe.DETECT_T, letterbox=letterbox, detection_win_size=win,
                             first_id=11)
        assert rc == rc_c == 0 and st["num_examined"] == n_cells and st["num_features"] == ref.shape[0] and st["error_feature"] == -1
        assert_records_equal(tr.get_features(), ref, "detect %r" % (shape,))
        if shape in fe.EMPTY_RANGE:
            assert st["num_features"] == 0
            img, ds = tr.draw_detections(StereoParams(do_letterbox=letterbox), DetectParams(detection_win_size=win), 7,
                                         fe.DETECT_Q, fe.DETECT_T)
            assert ds["num_examined"] == 0 and ds["num_scored"] == 0


@gpu
@pytest.mark.parametrize("win", fe.MASK_WINS)
def test_gpu_detect_mask_points_on_cell_boundaries(built, win):
    w, h = fe.SMALL
    pts = np.float32([p[:2] for p in fe.mask_points(win)])
    img = fe.random_image(w, h)
    with _tracker(fe.K_SMALL, fe.KINV_SMALL, w, h) as tr:
        for which in [None, "all"] + list(range(len(pts))):
            rc_c, _, ref, _ = fe.mask_detect(win, which)
            mask = None if which is None else (pts if which == "all" else pts[which:which + 1])
            tr.clear_features()
            rc, st = _gpu_detect(tr, img, fe.IDENT_Q, fe.MASK_T, detection_win_size=win, mask_xy=mask, first_id=5)
            assert rc == rc_c == 0
            assert_records_equal(tr.get_features(), ref, "mask window %d point %r" % (win, which))
        # the same points as the projected set, where they are a valid projection
        f, cur = fe.mask_projected(win)
        rc, st = _gpu_project(tr, f, fe.RECT_POSES, cur_id=12)
        assert rc == 0 and st["num_features"] == cur.shape[0]
        assert_records_equal(tr.get_projected(), cur, "mask points as the projected set")
        head = tr.get_features()
        rc_c, _, ref, _ = fe.mask_detect(win, "projected")
        rc, st = _gpu_detect(tr, img, fe.IDENT_Q, fe.MASK_T, detection_win_size=win, mask_xy="projected", first_id=5)
        assert rc == rc_c == 0
        out = tr.get_features()
        assert out[:head.shape[0]].tobytes() == head.tobytes()
        assert_records_equal(out[head.shape[0]:], ref, "projected mask window %d" % win)


@gpu
@pytest.mark.parametrize("path", ["host", "device"])
def test_gpu_detect_idepth_map_specials(built, path):
    import torch

    from flame_amd import synth_stereo as ss

    w, h = fe.SMALL
    m, winners, (rc_c, _, ref, _) = fe.map_case()
    K, Kinv = ss.intrinsics(w, h)
    with _tracker(K, Kinv, w, h) as tr:
        arg = np.array(m)
        if path == "device":
            dm = torch.from_numpy(np.array(m)).cuda()
            torch.cuda.synchronize()
            arg = dm.data_ptr()
        rc, st = _gpu_detect(tr, fe.random_image(w, h), fe.DETECT_Q, fe.DETECT_T, detection_win_size=7, idepthmap=arg)
        assert rc == rc_c == 0
        out = tr.get_features()
        assert out.tobytes() == ref.tobytes()  # bit for bit: -0.0, the infinities and the subnormal are copied


@gpu
def test_gpu_detect_thresholds_pass_on_equality(built):
    w, h = fe.SMALL
    with _tracker(fe.K_SMALL, fe.KINV_SMALL, w, h) as tr:
        for mag in (2.0, float(fe.ulp_up(2.0))):
            rc_c, _, ref, _ = fe.ramp_detect(mag)
            tr.clear_features()
            rc, st = _gpu_detect(tr, fe.ramp_image(), fe.IDENT_Q, fe.MASK_T, min_grad_mag=mag)
            assert rc == rc_c == 0 and st["num_features"] == ref.shape[0] == (12 if mag == 2.0 else 0)
            assert_records_equal(tr.get_features(), ref, "min_grad_mag %r" % mag)


@gpu
@pytest.mark.parametrize("first_id", fe.WRAP_IDS)
def test_gpu_detect_ids_wrap_as_uint32(built, first_id):
    from flame_amd import synth_stereo as ss

    w, h = fe.SMALL
    rc_c, _, ref, _ = fe.wrap_detect(first_id)
    K, Kinv = ss.intrinsics(w, h)
    with _tracker(K, Kinv, w, h) as tr:
        rc, st = _gpu_detect(tr, fe.random_image(w, h), fe.DETECT_Q, fe.DETECT_T, first_id=first_id)
        assert rc == rc_c == 0
        assert_records_equal(tr.get_features(), ref, "first_id %d" % first_id)
        assert tr.get_features()["id"][:4].tolist() == [(first_id + k) % 2 ** 32 for k in range(4)]
