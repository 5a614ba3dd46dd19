"""prunePoseFrames on the resident feature set (include/flame_stereo.h: flame_stereo_prune_pose_frames,
flame_stereo_prune_features, flame_stereo_clear_features): the CPU checker (tests/prune_ref.py) against hand-computed
cases and the pinned projection of oracle/, the conditions on the test inputs (tests/prune_cases.py), the C-ABI surface,
and -- on the GPU -- the HIP kernels bit-equal to the checker, the error contracts and the gap the call closes."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from flame_amd import synth_stereo as ss
from oracle import stereo_capi as so
from tests import frontend_ref as fr
from tests import prune_cases as pc
from tests import prune_ref as pr
from tests.conftest import HAS_GPU, ROOT

gpu = pytest.mark.gpu
PAD = 5
NO_DEVICE = -2  # FLAME_NLTGV2_ERR_NO_DEVICE
NEW_SYMBOLS = ("flame_stereo_prune_pose_frames", "flame_stereo_prune_features", "flame_stereo_clear_features")
F32 = np.float32


def assert_records_equal(a, b, what):
    a = np.ascontiguousarray(a).view(so.FEATURE_DTYPE)
    b = np.ascontiguousarray(b).view(so.FEATURE_DTYPE)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.tobytes() == b.tobytes():
        return
    for name in a.dtype.names:
        bad = np.nonzero((a[name].view(np.uint8).reshape(len(a), -1) != b[name].view(np.uint8).reshape(len(b), -1)).any(axis=1))[0]
        if bad.size:
            i = int(bad[0])
            raise AssertionError("%s: %s differs on %d records, first %d: %r vs %r" % (what, name, bad.size, i, a[i], b[i]))
    raise AssertionError("%s: bytes differ" % what)


# ---- CPU: the C-ABI surface (fails before the entry points existed) ------------------------------------------------

def test_prune_symbols_are_exported_listed_and_callable(built):
    import flame_amd
    from flame_amd.regularizer import NLTGV2Error
    from flame_amd.stereo import STEREO_ABI_SYMBOLS, FeatureTracker, StereoParams, _lib, _Pose, _PruneStats

    nm = subprocess.check_output(["nm", "-D", "--defined-only", flame_amd.library_path()], text=True)
    hdr = open(os.path.join(ROOT, "include", "flame_stereo.h")).read()
    for name in NEW_SYMBOLS:
        assert name in STEREO_ABI_SYMBOLS, name
        assert (" T %s\n" % name) in nm, name
        assert name + "(" in hdr, name
    L = _lib()
    p, st = StereoParams(), _PruneStats()
    ids = (C.c_uint32 * 1)(22)
    n = C.c_int(0)
    assert L.flame_stereo_prune_pose_frames(None, C.byref(p), 22, 1, ids, 0, (_Pose * 1)(), 0, C.byref(st)) == -1
    assert L.flame_stereo_prune_features(None, C.byref(p), 22, 1, ids, 0, (_Pose * 1)(), 0, C.byref(n), None, C.byref(st)) == -1
    assert L.flame_stereo_clear_features(None) == -1
    for m in ("prune_pose_frames", "prune_features", "clear_features"):
        assert callable(getattr(FeatureTracker, m))
    if not HAS_GPU:  # through the mirror: up to the "no device" status
        K, Kinv = ss.intrinsics(320, 240)
        with pytest.raises(NLTGV2Error) as e:
            FeatureTracker(K, Kinv, 320, 240, border=PAD)
        assert e.value.status == NO_DEVICE, e.value


def test_prune_stats_struct_is_plain_c99(built, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "flame_stereo.h"\n'
                   'int main(void) { flame_stereo_prune_stats s; s.num_removed = 0; s.num_frames_dropped = 0;\n'
                   '  return (int)sizeof s - 28 + s.num_removed + FLAME_NLTGV2_ABI_VERSION - 7; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "t.o")])
    from flame_amd.stereo import _PruneStats

    assert C.sizeof(_PruneStats) == 28


# ---- CPU: the checker against hand-computed cases ------------------------------------------------------------------

# a camera whose K and Kinv are dyadic, so that the identity pose and power-of-two depths round nowhere
W, H = 320, 240
K32 = np.float32([256, 0, 160, 0, 256, 120, 0, 0, 1])
KINV32 = np.float32([1 / 256, 0, -160 / 256, 0, 1 / 256, -120 / 256, 0, 0, 1])
IDENT = ([1, 0, 0, 0], [0, 0, 0])


def one_feature(x, y, mu, var=0.02, frame=10, valid=1):
    f = np.zeros(1, so.FEATURE_DTYPE)
    f["id"], f["frame_id"], f["x"], f["y"], f["idepth_mu"], f["idepth_var"], f["valid"] = 7, frame, x, y, mu, var, valid
    f["num_updates"], f["num_dropouts"], f["search_status"] = 3, 1, 2
    return f


def prune_one(f, q, t, first_new=None, **kw):
    geo = so.load_geometry(K32, KINV32, q, t)
    return pr.prune_pose_frames(f, [13, 22], {10: geo}, 22, W, H, first_new=first_new, **kw)


def test_checker_identity_pose_rewrites_only_frame_id():
    # K, Kinv, the coordinates and the depth are dyadic: every step is exact and the record is bit-unchanged but for frame_id
    g = one_feature(100.25, 77.75, 0.5, var=0.03)
    rc, st, out = prune_one(g, *IDENT)
    assert rc == 0 and st["num_moved"] == 1 and st["num_invalidated"] == 0 and st["num_features"] == 1
    exp = g.copy()
    exp["frame_id"] = 22
    assert out.tobytes() == exp.tobytes()
    # a feature of a kept pose-frame is untouched
    k = one_feature(100.25, 77.75, 0.5, frame=13)
    rc, st, out = prune_one(k, *IDENT)
    assert rc == 0 and out.tobytes() == k.tobytes() and st["num_moved"] == 0


def test_checker_invalid_features_are_moved_too_and_stay_invalid():
    g = one_feature(100.25, 77.75, 0.5, valid=0)
    rc, st, out = prune_one(g, *IDENT)
    assert rc == 0 and st["num_moved"] == 1 and out["frame_id"][0] == 22 and out["valid"][0] == 0


def test_checker_point_behind_the_target_camera():
    # depth 2 along the axis, the target camera 3 further on: z = 2 - 3 = -1, idepth -1 -> predict gives 0 and fails
    f = one_feature(160.0, 120.0, 0.5, var=0.04)
    rc, st, out = prune_one(f, [1, 0, 0, 0], [0, 0, -3.0])
    assert rc == 0 and st["num_invalidated"] == 1 and st["num_behind"] == 1 and st["num_features"] == 1
    r = out[0]
    # overwritten BEFORE the success test: the projected point (K p / z = the principal point), idepth 0, variance x 1
    assert (r["frame_id"], float(r["x"]), float(r["y"]), float(r["idepth_mu"]), r["valid"]) == (22, 160.0, 120.0, 0.0, 0)
    assert r["idepth_var"].tobytes() == F32(0.04).tobytes()
    assert (r["num_updates"], r["num_dropouts"], r["search_status"]) == (3, 1, 2)
    # the same record as a new feature is removed, not rewritten
    rc, st, out = prune_one(f, [1, 0, 0, 0], [0, 0, -3.0], first_new=0)
    assert rc == 0 and st["num_removed"] == 1 and st["num_invalidated"] == 0 and out.shape[0] == 0


def test_checker_rectangle_rounds_ties_to_even():
    """border 4: the rectangle is x in [4, 316), y in [4, 236) on ROUNDED coordinates.  3.5 -> 4 (inside), 4.5 -> 4,
    2.5 -> 2 (outside), 315.5 -> 316 (outside), 314.5 -> 314 (inside), 316.5 -> 316: ties go to the even integer."""
    assert pr.valid_region(W, H) == (4, 4, 312, 232)
    assert [pr.cv_round(v) for v in (2.5, 3.5, 4.5, -0.5, 0.5, 1.5, float("nan"), 3e9, -3e9)] == \
        [2, 4, 4, 0, 0, 2, -2 ** 31, -2 ** 31, -2 ** 31]
    cases = [(3.5, 100.0, True), (2.5, 100.0, False), (3.25, 100.0, False), (315.5, 100.0, False), (314.5, 100.0, True),
             (315.25, 100.0, True), (100.0, 3.5, True), (100.0, 2.5, False), (100.0, 235.5, False), (100.0, 234.5, True),
             (100.0, 235.25, True)]
    for x, y, inside in cases:
        f = one_feature(x, y, 0.5)
        rc, st, out = prune_one(f, *IDENT)
        assert rc == 0 and float(out["x"][0]) == F32(x) and float(out["y"][0]) == F32(y), (x, y)
        assert bool(out["valid"][0]) == inside and st["num_moved"] == int(inside) and st["num_outside"] == int(not inside), (x, y)
        rc, st, out = prune_one(f, *IDENT, first_new=0)
        assert out.shape[0] == int(inside), (x, y)
    # a float rectangle (projectFeatures' rule) would decide 3.5 and 315.5 the other way round
    assert not (F32(4) <= F32(3.5)) and F32(315.5) < F32(316)
    # the letterbox moves the rows only: y in [4 + 80, 4 + 80 + 232 - 160)
    assert pr.valid_region(W, H, do_letterbox=True) == (4, 84, 312, 72)
    f = one_feature(100.0, 83.5, 0.5)
    assert prune_one(f, *IDENT, do_letterbox=True)[2]["valid"][0] == 1
    assert prune_one(one_feature(100.0, 82.5, 0.5), *IDENT, do_letterbox=True)[2]["valid"][0] == 0
    assert prune_one(one_feature(100.0, 155.5, 0.5), *IDENT, do_letterbox=True)[2]["valid"][0] == 0  # -> 156 = 84 + 72


def test_checker_small_new_idepth_keeps_the_variance():
    # idepth 0: maxDepthProjection, new idepth 0, 0/0 = NaN replaced by 1
    f = one_feature(100.0, 90.0, 0.0, var=0.03)
    rc, st, out = prune_one(f, [1, 0, 0, 0], [0.1, 0, 0])
    assert rc == 0 and st["num_moved"] == 1 and out["idepth_mu"][0] == 0 and out["idepth_var"][0].tobytes() == F32(0.03).tobytes()
    # the test is on the NEW value: old 5e-7, pushed 1e6 m back -> new 3.3e-7 < 1e-6: factor 1
    f = one_feature(100.0, 90.0, 5e-7, var=0.03)
    rc, st, out = prune_one(f, [1, 0, 0, 0], [0, 0, 1e6])
    assert rc == 0 and 0 < out["idepth_mu"][0] < 1e-6 and out["idepth_var"][0].tobytes() == F32(0.03).tobytes()
    # old 5e-7 (< 1e-6) brought to about 1 m: the new idepth is NOT below 1e-6, the factor ~(1 / 5e-7)^4 = 1.6e25 applies
    rc, st, out = prune_one(f, [1, 0, 0, 0], [0, 0, -1999999.0])
    assert rc == 0 and out["idepth_mu"][0] > 0.5 and out["idepth_var"][0] > 1e22
    # two squarings: ((a / b)^2)^2 in float
    f = one_feature(160.0, 120.0, 0.5, var=0.03)
    rc, st, out = prune_one(f, [1, 0, 0, 0], [0, 0, 0.3])
    new = F32(1) / (F32(2) + F32(0.3))
    v = F32(new / F32(0.5))
    v = F32(v * v)
    v = F32(v * v)
    assert out["idepth_mu"][0].tobytes() == new.tobytes() and out["idepth_var"][0].tobytes() == F32(F32(0.03) * v).tobytes()


def test_checker_first_new_splits_the_same_failing_record():
    f = np.concatenate([one_feature(2.0, 100.0, 0.5), one_feature(50.0, 100.0, 0.5, frame=13), one_feature(2.0, 100.0, 0.5),
                        one_feature(60.0, 100.0, 0.5)])
    f["id"] = [0, 1, 2, 3]
    rc, st, out = prune_one(f, *IDENT, first_new=2)
    assert rc == 0 and list(out["id"]) == [0, 1, 3] and list(out["valid"]) == [0, 1, 1]
    assert (st["num_moved"], st["num_invalidated"], st["num_removed"], st["num_features"]) == (1, 1, 1, 3)
    rc, st, out4 = prune_one(f, *IDENT, first_new=4)
    assert list(out4["id"]) == [0, 1, 2, 3] and list(out4["valid"]) == [0, 1, 0, 1] and st["num_invalidated"] == 2
    rc, st, out0 = prune_one(f, *IDENT, first_new=0)
    assert list(out0["id"]) == [1, 3] and st["num_removed"] == 2


def test_checker_errors():
    f = np.concatenate([one_feature(50.0, 50.0, 0.5), one_feature(50.0, 50.0, -0.5), one_feature(50.0, 50.0, np.nan),
                        one_feature(50.0, 50.0, -0.5, frame=13)])
    rc, st, out = prune_one(f, *IDENT)
    assert (rc, st["error_feature"], out) == (fr.ASSERT, 1, None)
    rc, st, out = prune_one(f[[0, 3, 2]], *IDENT)  # a negative idepth in a KEPT pose-frame is never projected
    assert (rc, st["error_feature"]) == (fr.ASSERT, 2)
    z = one_feature(160.0, 120.0, 0.5)
    rc, st, out = prune_one(z, [1, 0, 0, 0], [0, 0, -2.0])  # a zero third coordinate
    assert (rc, st["error_feature"]) == (fr.ASSERT, 0)
    u = np.concatenate([one_feature(50.0, 50.0, -0.5), one_feature(50.0, 50.0, 0.5, frame=42, valid=0)])
    rc, st, out = prune_one(u, *IDENT)  # the unknown frame is reported before the assert
    assert (rc, st["error_feature"]) == (fr.INVALID_ARG, 1)
    geo = so.load_geometry(K32, KINV32, *IDENT)
    assert pr.prune_pose_frames(z, [13], {10: geo}, 22, W, H)[0] == fr.INVALID_ARG  # the target is not kept
    assert pr.prune_pose_frames(z, [13, 22], {13: geo}, 22, W, H)[0] == fr.INVALID_ARG  # kept and dropped
    assert pr.prune_pose_frames(z, [13, 22], {10: geo}, 22, W, H, first_new=2)[0] == fr.INVALID_ARG
    assert pr.target_of([16, 22, 19]) == 22  # crbegin() of a std::map: the largest id


def test_checker_projection_step_is_bit_equal_to_the_oracle():
    """The checker's projection is frontend_ref.project_idepth on the geometry of target^-1 * pf; against the pinned
    EpipolarGeometry::project of oracle/ on the inputs of a real case."""
    case = pc.make("small")
    sc, f = case["sc"], case["feats"]
    for a, geo in pc.dropped_geos(sc, case["dropped"], case["target"]).items():
        sel = np.nonzero(f["frame_id"] == a)[0][:1500]
        px, py, pd, ok = fr.project_idepth(geo, f["x"][sel], f["y"][sel], f["idepth_mu"][sel])
        assert ok.all() and sel.size > 100
        for k, i in enumerate(sel):
            assert (px[k], py[k], pd[k]) == so.project_idepth(geo, float(f["x"][i]), float(f["y"][i]), float(f["idepth_mu"][i])), i


# ---- CPU: the conditions on the inputs of the GPU parity tests ------------------------------------------------------

@functools.lru_cache(maxsize=None)
def checker_result(name, first_new):
    case = pc.make(name)
    sc = case["sc"]
    return pr.prune_pose_frames(case["feats"], case["keep"], pc.dropped_geos(sc, case["dropped"], case["target"]),
                                case["target"], sc.width, sc.height, first_new=first_new,
                                do_letterbox=bool(case["letterbox"]))


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_parity_inputs_exercise_every_path(name):
    """In every parity case with more than 1000 features at least a fifth of the features are moved successfully, at
    least one in twenty fails the region test and at least one fails behind the camera -- on the checker's own output
    for the very inputs the GPU tests use."""
    case = pc.make(name)
    n = case["feats"].shape[0]
    rc, st, out = checker_result(name, n)
    assert rc == 0 and st["num_examined"] == n
    print(name, n, st)
    if n > 1000:
        assert st["num_moved"] >= n / 5, st
        assert st["num_outside"] >= n / 20, st
        assert st["num_behind"] >= 1, st
        rc, st0, out0 = checker_result(name, n // 3)
        assert rc == 0 and 0 < st0["num_removed"] and 0 < st0["num_invalidated"] and out0.shape[0] == n - st0["num_removed"]
    if name == "nothing-to-move":
        assert st["num_moved"] == 0 and out.tobytes() == case["feats"].tobytes()
    if name == "everything-to-move":
        assert st["num_moved"] + st["num_invalidated"] == n and (out["frame_id"] == case["target"]).all()


@pytest.mark.parametrize("name", ["group+1", "small", "vga-letterbox"])
def test_vectorised_host_version_equals_the_checker(name):
    case = pc.make(name)
    sc, n = case["sc"], case["feats"].shape[0]
    for first_new in pc.first_new_values(n):
        out = pr.prune_vectorised(case["feats"], case["keep"], pc.dropped_geos(sc, case["dropped"], case["target"]),
                                  case["target"], sc.width, sc.height, first_new=first_new,
                                  do_letterbox=bool(case["letterbox"]))
        assert_records_equal(out, checker_result(name, first_new)[2], "%s first_new %d" % (name, first_new))


# ---- GPU: bit-equal to the checker --------------------------------------------------------------------------------

def _tracker(sc):
    from flame_amd.stereo import FeatureTracker

    return FeatureTracker(sc.K32, sc.Kinv32, sc.width, sc.height, border=PAD)


def _view(tr, feats):
    from flame_amd.stereo import FEATURE_DTYPE

    return np.ascontiguousarray(feats).view(FEATURE_DTYPE)


def _gpu_prune(tr, case, first_new, form, feats=None, keep=None, dropped=None, target=None):
    from flame_amd.stereo import StereoParams

    sc = case["sc"]
    sp = StereoParams(do_letterbox=case["letterbox"])
    feats = case["feats"] if feats is None else feats
    keep = case["keep"] if keep is None else keep
    dropped = case["dropped"] if dropped is None else dropped
    target = case["target"] if target is None else target
    poses = pc.dropped_poses(sc, dropped, target) if dropped and not isinstance(dropped[0], dict) else dropped
    if form == "resident":
        tr.set_features(_view(tr, feats))
        rc, st = tr.prune_pose_frames(sp, target, keep, poses, first_new, raise_on_error=False)
        return rc, st, tr.get_features()
    arr = _view(tr, feats.copy())
    rc, out, st = tr.prune_features(sp, target, keep, poses, arr, first_new, raise_on_error=False)
    return rc, st, out


@gpu
@pytest.mark.parametrize("form", ["resident", "host"])
@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_gpu_prune_matches_checker(built, name, form):
    case = pc.make(name)
    n = case["feats"].shape[0]
    with _tracker(case["sc"]) as tr:
        for first_new in pc.first_new_values(n):
            rc_c, st_c, ref = checker_result(name, first_new)
            rc, st, out = _gpu_prune(tr, case, first_new, form)
            print(name, form, first_new, st)
            assert rc == rc_c == 0
            for k in pr.STAT_NAMES:
                assert st[k] == st_c[k], (name, form, first_new, k, st, st_c)
            assert st["num_frames_dropped"] == 0  # (no frames were added)
            assert_records_equal(out, ref, "%s %s first_new %d" % (name, form, first_new))
            if form == "resident":
                assert tr.features_device()[1] == ref.shape[0]


@gpu
def test_gpu_prune_is_in_place_when_nothing_is_removed(built):
    case = pc.make("vga")
    n = case["feats"].shape[0]
    with _tracker(case["sc"]) as tr:
        from flame_amd.stereo import StereoParams

        tr.set_features(_view(tr, case["feats"]))
        before, _ = tr.features_device()
        st = tr.prune_pose_frames(StereoParams(), case["target"], case["keep"],
                                  pc.dropped_poses(case["sc"], case["dropped"], case["target"]))  # first_new = n
        assert st["num_removed"] == 0 and st["num_invalidated"] > 0 and tr.features_device() == (before, n)
        assert tr.last_kernel_ms() > 0
        # pruning again finds nothing to move: every feature is in a kept pose-frame now
        once = tr.get_features()
        st = tr.prune_pose_frames(StereoParams(), case["target"], case["keep"], [], 0)
        assert (st["num_moved"], st["num_invalidated"], st["num_removed"], st["num_features"]) == (0, 0, 0, n)
        assert tr.get_features().tobytes() == once.tobytes() and tr.features_device() == (before, n)
        tr.clear_features()
        assert tr.features_device()[1] == 0 and tr.get_features().shape[0] == 0 and tr.get_projected().shape[0] == 0
        st = tr.prune_pose_frames(StereoParams(), case["target"], case["keep"], [], 0)
        assert st["num_examined"] == 0 and st["num_features"] == 0


def _with_frames(tr, sc, ids):
    blank = np.zeros((sc.height, sc.width), np.uint8)
    for k in ids:
        tr.add_frame(k, blank)


@gpu
@pytest.mark.parametrize("form", ["resident", "host"])
def test_gpu_prune_error_contracts(built, form):
    """Unknown frame, target not kept, asserting idepth: each leaves the set, the projected set and frame_count alone."""
    from flame_amd.stereo import StereoParams

    case = pc.make("small")
    sc, feats = case["sc"], case["feats"]
    n = feats.shape[0]
    proj_pose = [dict(id=a, q_to_new=sc.relative(a, 23)[0], t_to_new=sc.relative(a, 23)[1]) for a in pc.PF_IDS]
    with _tracker(sc) as tr:
        _with_frames(tr, sc, pc.PF_IDS + (23, 24))
        tr.set_features(_view(tr, feats))
        tr.project_features(StereoParams(), 23, proj_pose)
        base, proj = tr.get_features(), tr.get_projected()
        assert proj.shape[0] > 100 and tr.frame_count() == 7
        base_c = base.view(so.FEATURE_DTYPE)
        geos = pc.dropped_geos(sc, case["dropped"], case["target"])

        def unchanged(feats_now):
            assert tr.get_features().tobytes() == feats_now.tobytes()
            assert tr.get_projected().tobytes() == proj.tobytes() and tr.frame_count() == 7

        orphans = np.nonzero(np.isin(base_c["frame_id"], case["dropped"]))[0]
        kept = np.nonzero(~np.isin(base_c["frame_id"], case["dropped"]))[0]
        # 1. a feature whose frame is neither kept nor listed
        bad = base_c.copy()
        bad["frame_id"][[orphans[5], orphans[40]]] = 77
        bad["idepth_mu"][orphans[2]] = -1.0  # (an assert at a lower index: the unknown frame is reported first)
        rc, st, out = _gpu_prune(tr, case, n // 2, form, feats=bad)
        assert rc == -1 and st["error_feature"] == orphans[5], st
        assert pr.prune_pose_frames(bad, case["keep"], geos, case["target"], sc.width, sc.height, n // 2)[1]["error_feature"] == orphans[5]
        unchanged(bad if form == "resident" else base)
        # 2. the asserting inverse depths: negative, NaN; only in a dropped pose-frame
        bad = base_c.copy()
        bad["idepth_mu"][kept[0]] = -1.0
        bad["idepth_mu"][orphans[7]] = np.nan
        bad["idepth_mu"][orphans[9]] = -0.25
        bad["valid"][orphans[7]] = 0  # `valid` is not tested
        rc, st, out = _gpu_prune(tr, case, n // 2, form, feats=bad)
        assert rc == -8 and st["error_feature"] == orphans[7], st
        assert pr.prune_pose_frames(bad, case["keep"], geos, case["target"], sc.width, sc.height, n // 2)[:2][0] == -8
        unchanged(bad if form == "resident" else base)
        if form == "resident":
            tr.set_features(base)
        # 3. the arguments: target not kept, target dropped, an id in both lists, first_new out of range, no kept id
        poses = pc.dropped_poses(sc, case["dropped"], case["target"])
        for kw in (dict(keep=[16, 19]), dict(keep=[16, 19, 22], dropped=pc.dropped_poses(sc, [10, 13, 22], 22)),
                   dict(keep=[13, 16, 19, 22]), dict(keep=[])):
            rc, st, out = _gpu_prune(tr, case, n // 2, form, feats=base_c, **kw)
            assert rc == -1 and st["error_feature"] == -1, kw
            unchanged(base)
        for first_new in (-1, n + 1):
            rc, st, out = _gpu_prune(tr, case, first_new, form, feats=base_c)
            assert rc == -1
            unchanged(base)
        # and then it works, releasing the dropped frames (both forms do)
        rc, st, out = _gpu_prune(tr, case, n // 2, form, feats=base_c)
        assert rc == 0 and st["num_frames_dropped"] == len(case["dropped"]) and tr.frame_count() == 7 - len(case["dropped"])
        assert tr.get_projected().tobytes() == proj.tobytes()  # the projected set is not touched
        assert_records_equal(out, pr.prune_pose_frames(base_c, case["keep"], geos, case["target"], sc.width, sc.height, n // 2)[2],
                             "after the errors")
        assert len(poses) == len(case["dropped"])


@gpu
def test_gpu_prune_releases_frames_and_bounds_the_spares(built):
    from flame_amd.stereo import StereoParams

    case = pc.make("wave")
    sc = case["sc"]
    with _tracker(sc) as tr:
        ids = tuple(range(30, 38)) + pc.PF_IDS
        _with_frames(tr, sc, ids)
        tr.set_features(_view(tr, case["feats"]))
        assert tr.frame_count() == 13
        # eight frames without features and two with: more than the spare list holds
        dropped = pc.dropped_poses(sc, case["dropped"], case["target"]) + \
            [dict(id=k, q_to_new=[1, 0, 0, 0], t_to_new=[0, 0, 0]) for k in range(30, 38)] + \
            [dict(id=99, q_to_new=[1, 0, 0, 0], t_to_new=[0, 0, 0])]  # (not resident: nothing to release)
        st = tr.prune_pose_frames(StereoParams(), case["target"], case["keep"], dropped)
        assert st["num_frames_dropped"] == 10 and tr.frame_count() == 3
        assert_records_equal(tr.get_features(), checker_result("wave", 64)[2], "prune with many drops")
        _with_frames(tr, sc, range(40, 46))  # from the spares, then fresh
        assert tr.frame_count() == 9


@gpu
def test_gpu_prune_closes_the_gap_drop_frame_leaves(built):
    """After a plain drop_frame of a pose-frame that still anchors features the next update_resident / project_features
    answer ERR_INVALID_ARG; after prune_pose_frames of the same frame they succeed."""
    from flame_amd.stereo import StereoParams

    sc = pc.scene("320x240")
    imgs = {k: sc.render(k) for k in (19, 22, 23)}
    feats = ss.make_features(sc, so.FEATURE_DTYPE, [19, 22], 400, 3)
    sp = StereoParams()
    only22 = ss.poses_for(sc, [22], 23, 22)
    for how in ("drop_frame", "prune"):
        with _tracker(sc) as tr:
            for k, img in imgs.items():
                tr.add_frame(k, img)
            tr.set_features(_view(tr, feats))
            if how == "drop_frame":
                tr.drop_frame(19)
            else:
                st = tr.prune_pose_frames(sp, 22, [22], pc.dropped_poses(sc, [19], 22))
                assert st["num_moved"] > 300 and st["num_frames_dropped"] == 1
            assert tr.frame_count() == 2
            rc_u, st_u = tr.update_resident(sp, 23, 22, only22, raise_on_error=False)
            rc_p, st_p = tr.project_features(sp, 23, [dict(id=22, q_to_new=sc.relative(22, 23)[0],
                                                           t_to_new=sc.relative(22, 23)[1])], raise_on_error=False)
            if how == "drop_frame":
                assert rc_u == -1 and st_u["error_feature"] == 0 and rc_p == -1 and st_p["error_feature"] == 0
                # naming the dropped pose-frame does not help: it is not resident
                assert tr.update_resident(sp, 23, 22, ss.poses_for(sc, [19, 22], 23, 22), raise_on_error=False)[0] == -1
            else:
                assert rc_u == 0 and st_u["num_idepth_updates"] > 100 and rc_p == 0 and st_p["num_features"] > 300
