"""The selection of the graph's vertices (include/flame_stereo.h: flame_stereo_select_graph_features and
flame_stereo_select_graph_features_arrays -- the preprocessing of Flame::syncGraph, flame.cc:1954-1980): the CPU checker
(tests/select_ref.py) against hand-computed records, a float64 statement of the height and the reference's set logic
restated; the conditions on the test inputs (tests/select_cases.py); the C-ABI surface; and -- on the GPU -- the HIP
kernels bit-equal to the checker in both forms, and the error contracts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from flame_amd import synth_stereo as ss
from oracle import stereo_capi as so
from tests import frontend_ref as fr
from tests import prune_cases as pc
from tests import select_cases as sc_
from tests import select_ref as sr
from tests.conftest import HAS_GPU, ROOT

gpu = pytest.mark.gpu
PAD = 5
NO_DEVICE = -2  # FLAME_NLTGV2_ERR_NO_DEVICE
NEW_SYMBOLS = ("flame_stereo_default_graph_params", "flame_stereo_select_graph_features",
               "flame_stereo_select_graph_features_arrays")
F32 = np.float32
U = 2.0 ** -24  # the unit roundoff of float32


# ---- CPU: the C-ABI surface (fails before the entry points existed) ------------------------------------------------

def test_select_symbols_are_exported_listed_and_callable(built):
    import flame_amd
    from flame_amd.regularizer import NLTGV2Error
    from flame_amd.stereo import STEREO_ABI_SYMBOLS, FeatureTracker, GraphParams, _GraphInputs, _lib, _WorldPose

    nm = subprocess.check_output(["nm", "-D", "--defined-only", flame_amd.library_path()], text=True)
    hdr = open(os.path.join(ROOT, "include", "flame_stereo.h")).read()
    for name in NEW_SYMBOLS:
        assert name in STEREO_ABI_SYMBOLS, name
        assert (" T %s\n" % name) in nm, name
        assert name + "(" in hdr, name
    L = _lib()
    gp, out = GraphParams(), _GraphInputs()
    assert abs(gp.idepth_var_max_graph - 1e-2) < 1e-9 and abs(gp.min_height - 0.1) < 1e-8 and gp.max_height == 4.0
    assert gp.adaptive_data_weights == 0
    out.V, out.error_feature = 5, 7
    assert L.flame_stereo_select_graph_features(None, C.byref(gp), 1.0, 0, (_WorldPose * 1)(), C.byref(out)) == -1
    assert (out.V, out.error_feature, bool(out.feat_id)) == (0, -1, False)  # never a stale result
    assert L.flame_stereo_select_graph_features_arrays(None, C.byref(gp), 1.0, 0, (_WorldPose * 1)(), 0, None, None,
                                                       C.byref(out)) == -1
    for m in ("select_graph_features", "get_raw_idepths"):
        assert callable(getattr(FeatureTracker, m))
    if not HAS_GPU:  # through the mirror: up to the "no device" status
        K, Kinv = ss.intrinsics(320, 240)
        with pytest.raises(NLTGV2Error) as e:
            FeatureTracker(K, Kinv, 320, 240, border=PAD)
        assert e.value.status == NO_DEVICE, e.value


def test_select_structs_are_plain_c99(built, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "flame_stereo.h"\n'
                   'int main(void) { flame_stereo_graph_inputs s; flame_stereo_graph_params g; flame_stereo_world_pose p;\n'
                   '  s.V = 0; g.adaptive_data_weights = 0; p.frame_id = 0;\n'
                   '  return (int)sizeof g - 16 + (int)sizeof p - 32 + s.V + g.adaptive_data_weights + (int)p.frame_id\n'
                   '         + FLAME_NLTGV2_ABI_VERSION - 7; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "t.o")])
    from flame_amd.stereo import GraphParams, _GraphInputs, _WorldPose

    assert C.sizeof(GraphParams) == 16 and C.sizeof(_WorldPose) == 32
    assert C.sizeof(_GraphInputs) == 8 + 5 * C.sizeof(C.c_void_p) + 5 * 4 + 4  # (V + padding, 5 pointers, 5 ints + padding)


# ---- CPU: the checker against hand-computed records -----------------------------------------------------------------

# a camera whose K and Kinv are dyadic, so that power-of-two depths round nowhere
K32 = np.float32([256, 0, 160, 0, 256, 120, 0, 0, 1])
KINV32 = np.float32([1 / 256, 0, -160 / 256, 0, 1 / 256, -120 / 256, 0, 0, 1])
IDENT = dict(id=10, q=[1, 0, 0, 0], t=[0, 0, 0])


def rec(x, y, mu, var=0.005, frame=10, valid=1, fid=7):
    f = np.zeros(1, so.FEATURE_DTYPE)
    f["id"], f["frame_id"], f["x"], f["y"], f["idepth_mu"], f["idepth_var"], f["valid"] = fid, frame, x, y, mu, var, valid
    return f


def cur_rec(x=11.5, y=22.25, mu=0.25, var=0.125, valid=1, fid=99):
    return rec(x, y, mu, var=var, frame=23, valid=valid, fid=fid)


def one(f, pose=IDENT, scale=1.0, c=None, **gp):
    rc, res = sr.select(f, cur_rec() if c is None else c, KINV32, [pose], scale, gp)
    return rc, res


def test_checker_identity_pose():
    # x = 160, y = 56, idepth 0.5: pix = (320, 112, 2); X = 1.25 - 1.25 = 0, Y = 0.4375 - 0.9375 = -0.5, Z = 2: height 0.5
    f = rec(160.0, 56.0, 0.5)
    h, known = sr.heights32(f, KINV32, [IDENT])
    assert known.all() and h[0] == F32(0.5)
    rc, res = one(f)
    assert rc == 0 and res["V"] == 1 and (res["num_invalid"], res["num_fail_var"], res["num_fail_height"]) == (0, 0, 0)
    # the outputs come from the PROJECTED record; feat_id from the resident one
    assert res["feat_id"].tolist() == [7] and res["feat_index"].tolist() == [0]
    assert res["pos"].tolist() == [[11.5, 22.25]] and res["data_term"].tolist() == [0.25] and res["data_weight"].tolist() == [1.0]
    rc, res = one(f, scale=0.5, adaptive_data_weights=1)
    assert res["data_term"].tolist() == [0.5] and res["data_weight"].tolist() == [8.0]  # 0.25 / 0.5, 1 / 0.125
    # the projected record's valid flag and id are not read; a zeroed record gives zeros (and 1 / 0 = inf as a weight)
    rc, res = one(f, c=np.zeros(1, so.FEATURE_DTYPE), adaptive_data_weights=1)
    assert rc == 0 and res["V"] == 1 and res["pos"].tolist() == [[0, 0]] and res["data_term"][0] == 0 and np.isinf(res["data_weight"][0])
    # an invalid resident record is counted as invalid whatever else fails
    rc, res = one(rec(160.0, 56.0, 0.5, var=0.5, valid=0))
    assert (res["V"], res["num_invalid"], res["num_fail_var"], res["num_fail_height"]) == (0, 1, 0, 0)
    # below the image centre the point is below the camera: height -0.5
    rc, res = one(rec(160.0, 184.0, 0.5))
    assert sr.heights32(rec(160.0, 184.0, 0.5), KINV32, [IDENT])[0][0] == F32(-0.5)
    assert (res["V"], res["num_fail_height"]) == (0, 1)


def test_checker_pure_translation():
    # the camera half a metre below the world's origin (world.y is down): world.y = -0.5 + 0.5 = 0, height 0
    pose = dict(id=10, q=[1, 0, 0, 0], t=[3.0, 0.5, -7.0])  # only t[1] matters
    f = rec(160.0, 56.0, 0.5)
    assert sr.heights32(f, KINV32, [pose])[0][0] == F32(0)
    assert one(f, pose)[1]["num_fail_height"] == 1  # 0 < 0.1
    assert one(f, pose, min_height=-0.5, max_height=1.5)[1]["V"] == 1
    assert one(f, pose, min_height=0.0)[1]["V"] == 1  # -0.0 >= 0.0
    pose["t"] = [0, -1.0, 0]
    assert sr.heights32(f, KINV32, [pose])[0][0] == F32(1.5) and one(f, pose)[1]["V"] == 1


def test_checker_roll_of_90_degrees():
    """A roll by +90 degrees about the optical axis: world.y = camera x.  q = (c, 0, 0, c) with c = float32(sqrt(1/2)):
    tz = 2c; R10 = tz*w = 2c*c, R11 = 1 - tz*z = 1 - 2c*c, R12 = 0 -- the float32 steps written out."""
    c = F32(np.sqrt(0.5))
    pose = dict(id=10, q=[c, 0, 0, c], t=[0, 0, 0])
    r10, r11, r12 = sr.rotation_row1(pose["q"])
    tz = F32(2) * c
    assert r10 == F32(0) + tz * c and r11 == F32(1) - (F32(0) + tz * c) and r12 == F32(0)
    assert abs(float(r10) - 1.0) <= 2 * U and abs(float(r11)) <= 2 * U
    # x = 32, y = 120, idepth 0.5: X = 64/256 - 1.25 = -1, Y = 0: world.y = R10 * -1 + R11 * 0: height = R10
    f = rec(32.0, 120.0, 0.5)
    h = sr.heights32(f, KINV32, [pose])[0][0]
    assert h == -(((r10 * F32(-1) + r11 * F32(0)) + r12 * F32(2)) + F32(0)) and abs(float(h) - 1.0) <= 2 * U
    assert one(f, pose)[1]["V"] == 1
    # the same pixel without the roll sits at height 0
    assert sr.heights32(f, KINV32, [IDENT])[0][0] == F32(0) and one(f)[1]["num_fail_height"] == 1
    # and mirrored in x it is a metre below
    assert one(rec(288.0, 120.0, 0.5), pose)[1]["num_fail_height"] == 1


def test_checker_idepth_zero_and_tiny():
    # idepth 0: x / 0 = inf, Kinv[1] * inf = 0 * inf = NaN: every comparison false, counted under the height
    with np.errstate(all="ignore"):
        h = sr.heights32(rec(160.0, 56.0, 0.0), KINV32, [IDENT])[0][0]
    assert np.isnan(h)
    rc, res = one(rec(160.0, 56.0, 0.0))
    assert rc == 0 and (res["V"], res["num_invalid"], res["num_fail_var"], res["num_fail_height"]) == (0, 0, 0, 1)
    rc, res = one(rec(160.0, 56.0, 0.0), min_height=-np.inf, max_height=np.inf)
    assert res["num_fail_height"] == 1  # NaN passes no band
    rc, res = one(rec(160.0, 56.0, 0.0, var=0.5))
    assert res["num_fail_var"] == 1  # the variance test comes first
    # idepth 5e-7: two thousand kilometres away, a finite height far above the band; below the centre far below it
    for y, sign in ((56.0, 1), (184.0, -1)):
        f = rec(160.0, y, 5e-7)
        h = sr.heights32(f, KINV32, [IDENT])[0][0]
        assert np.isfinite(h) and sign * h > 4e5
        assert one(f)[1]["num_fail_height"] == 1
        assert one(f, max_height=1e6)[1]["V"] == (1 if sign > 0 else 0)


def test_checker_thresholds_are_exact():
    f = rec(160.0, 56.0, 0.5)  # height exactly 0.5
    thr = F32(1e-2)
    assert one(rec(160.0, 56.0, 0.5, var=thr))[1]["num_fail_var"] == 1  # var < max, not <=
    assert one(rec(160.0, 56.0, 0.5, var=np.nextafter(thr, F32(0))))[1]["V"] == 1
    assert one(f, min_height=0.5)[1]["V"] == 1  # >=
    assert one(f, min_height=np.nextafter(F32(0.5), F32(1)))[1]["num_fail_height"] == 1
    assert one(f, max_height=0.5)[1]["V"] == 1  # <=
    assert one(f, max_height=np.nextafter(F32(0.5), F32(0)))[1]["num_fail_height"] == 1
    assert one(f, min_height=0.5, max_height=0.5)[1]["V"] == 1


def test_checker_errors():
    f = np.concatenate([rec(160.0, 56.0, 0.5, fid=0), rec(160.0, 56.0, -0.5, valid=0, fid=1), rec(160.0, 56.0, np.nan, fid=2),
                        rec(160.0, 56.0, 0.5, frame=42, valid=0, fid=3)])
    c = np.concatenate([cur_rec()] * 4)
    rc, res = sr.select(f, c, KINV32, [IDENT], 1.0)  # the assert runs for an INVALID record too
    assert (rc, res["error_feature"], res["V"], res["feat_id"].size) == (fr.ASSERT, 1, 0, 0)
    rc, res = sr.select(f[[0, 2, 3]], c[:3], KINV32, [IDENT], 1.0)  # NaN
    assert (rc, res["error_feature"]) == (fr.ASSERT, 1)
    rc, res = sr.select(f[[0, 3, 1]], c[:3], KINV32, [IDENT], 1.0)  # the unknown frame comes first in the loop
    assert (rc, res["error_feature"]) == (fr.INVALID_ARG, 1)
    both = rec(160.0, 56.0, -1.0, frame=42)
    rc, res = sr.select(np.concatenate([f[:1], both]), c[:2], KINV32, [IDENT], 1.0)  # within a record the assert is first
    assert (rc, res["error_feature"]) == (fr.ASSERT, 1)
    big = np.concatenate([rec(160.0, 184.0, 0.5, fid=2 ** 31), rec(160.0, 56.0, 0.5, fid=2 ** 31 + 5), rec(160.0, 56.0, 0.5, fid=3)])
    rc, res = sr.select(big, c[:3], KINV32, [IDENT], 1.0)  # only a SELECTED id must fit
    assert (rc, res["error_feature"], res["V"]) == (fr.INVALID_ARG, 1, 0)
    rc, res = sr.select(big[[0, 2]], c[:2], KINV32, [IDENT], 1.0)
    assert rc == 0 and res["feat_id"].tolist() == [3] and res["feat_index"].tolist() == [1]
    rc, res = sr.select(f[:0], c[:0], KINV32, [], 1.0)
    assert rc == 0 and res["V"] == 0 and res["num_examined"] == 0


# ---- CPU: the conditions on the inputs of the GPU parity tests ------------------------------------------------------

BIG = tuple(n for n in sc_.SIZES if n >= 1000)


@pytest.mark.parametrize("n", BIG)
def test_parity_inputs_exercise_every_path(n):
    """Conditions, not measurements: selected >= 10 %, invalid, variance and below-band each >= 5 %,
    above-band-or-non-finite >= 0.5 % -- on the checker's own output for the very arrays the GPU tests use."""
    case = sc_.make(n)
    rc, res = sr.select(case["feats"], case["proj"], case["sc"].Kinv32, case["world"], 1.0)
    h, known = sr.heights32(case["feats"], case["sc"].Kinv32, case["world"])
    with np.errstate(all="ignore"):
        below = int((h < F32(0.1)).sum())
        above = int((~(h <= F32(4.0))).sum())
    print(n, {k: res[k] for k in ("V",) + sr.COUNTERS}, "below", below, "above or non-finite", above)
    assert rc == 0 and known.all()
    assert res["V"] + res["num_invalid"] + res["num_fail_var"] + res["num_fail_height"] == n == res["num_examined"]
    assert res["V"] >= 0.10 * n
    assert (case["feats"]["valid"] == 0).sum() >= 0.05 * n and res["num_invalid"] >= 0.05 * n
    assert (case["feats"]["idepth_var"] >= F32(1e-2)).sum() >= 0.05 * n and res["num_fail_var"] >= 0.05 * n
    assert below >= 0.05 * n and above >= 0.005 * n and res["num_fail_height"] >= 0.05 * n
    # a selected feature whose projected record is the zeroed one: its zeros are part of the output
    zero_sel = case["proj"]["valid"][res["feat_index"]] == 0
    assert zero_sel.any() and (res["pos"][zero_sel] == 0).all() and (res["data_term"][zero_sel] == 0).all()
    # the resident form: all valid after the projection, invalid again after the in-place prune
    kept, cur = sc_.resident_sets(n)
    rc, r2 = sr.select(kept, cur, case["sc"].Kinv32, case["world"], 1.0)
    assert rc == 0 and r2["num_invalid"] == 0 and r2["V"] >= 0.10 * kept.shape[0] and r2["num_fail_var"] > 0 and r2["num_fail_height"] > 0
    kept, cur = sc_.resident_sets(n, prune=True)
    rc, r3 = sr.select(kept, cur, case["sc"].Kinv32, case["world"], 1.0)
    assert rc == 0 and r3["num_invalid"] > 0 and r3["V"] > 0 and r3["num_fail_var"] > 0 and r3["num_fail_height"] > 0


def height_bound(feats, K, R, t):
    """A bound on |float32 height - float64 height| per record, from the operation count and the magnitudes of the terms
    (u = 2^-24, first order, then doubled for the second-order terms and the float64 statement's own error):
      pix        one division each: relative u;
      Kinv       float32(inv(K)): relative u per entry;
      X, Y, Z    each term Kinv_ij * p_j carries <= 3 roundings (entry, p_j, product) and <= 2 additions: 5 u S_i with
                 S_i = sum_j |Kinv_ij p_j|;
      R row 1    q is rounded to float32 (<= u/2 per component, |q| <= 1: <= 3 u on an entry of R) and each entry takes <= 4
                 roundings on magnitudes <= 3: <= 15 u, taken as 16 u absolute;
      world.y    each term R1j * Xj: 16 u |Xj| + |R1j| 5 u S_j + 4 u |R1j Xj| (product + three additions); t[1]: its rounding
                 and one addition, 2 u |t1|."""
    Ki = np.linalg.inv(np.asarray(K, np.float64).reshape(3, 3))
    mu = feats["idepth_mu"].astype(np.float64)
    with np.errstate(all="ignore"):
        p = np.stack([feats["x"].astype(np.float64) / mu, feats["y"].astype(np.float64) / mu, 1.0 / mu], axis=0)
        S = np.abs(Ki) @ np.abs(p)  # S_i >= |X_i|
        r = np.abs(np.asarray(R, np.float64)[1])
        first = (16.0 * S + 5.0 * r[:, None] * S + 4.0 * r[:, None] * S).sum(axis=0) + 2.0 * abs(float(t[1]))
    return 2.0 * U * first


@pytest.mark.parametrize("n", BIG)
def test_float32_checker_agrees_with_the_float64_statement(n):
    """Every record whose float64 height lies farther from both thresholds than its bound is classified alike (a
    non-finite float64 height passes no band in either); at most 0.1 % of the records may lie inside the bound."""
    case = sc_.make(n)
    sc, feats = case["sc"], case["feats"]
    h32, _ = sr.heights32(feats, sc.Kinv32, case["world"])
    inside_total, worst = 0, 0.0
    for band in sc_.BANDS:
        gp = dict(sr.DEFAULT_GP, **band)
        lo, hi = float(F32(gp["min_height"])), float(F32(gp["max_height"]))
        for a in pc.PF_IDS:
            sel = feats["frame_id"] == a
            f = feats[sel]
            R, t = sc_.world_pose64(sc, a)
            h64 = sr.height64(f, sc.K, R, t)
            B = height_bound(f, sc.K, R, t)
            with np.errstate(all="ignore"):
                band32 = (h32[sel] >= F32(lo)) & (h32[sel] <= F32(hi))
                band64 = (h64 >= lo) & (h64 <= hi)
                finite = np.isfinite(h64) & np.isfinite(B)
                near = finite & ((np.abs(h64 - lo) <= B) | (np.abs(h64 - hi) <= B))
                err = np.abs(h32[sel].astype(np.float64) - h64)
            decided = ~near
            assert (band32[decided] == band64[decided]).all(), (n, a, band)
            assert not band32[~finite].any() and not band64[~finite].any()
            assert (err[finite] <= B[finite]).all(), (n, a, float((err[finite] / B[finite]).max()))
            worst = max(worst, float((err[finite] / B[finite]).max()))
            inside_total += int(near.sum())
    print(n, "inside the bound:", inside_total, "of", 2 * n, "; largest error / bound:", worst)
    assert inside_total <= 0.001 * 2 * n


@pytest.mark.parametrize("n", (257, 1500, 8400))
def test_reference_set_logic_gives_the_checkers_mask(n):
    case = sc_.make(n)
    feats, proj = case["feats"], case["proj"]
    h32, _ = sr.heights32(feats, case["sc"].Kinv32, case["world"])
    for gp in (dict(), dict(adaptive_data_weights=1, min_height=-0.5, max_height=1.5)):
        rc, res = sr.select(feats, proj, case["sc"].Kinv32, case["world"], 0.37, gp)
        seq = sr.select_sequential(feats, proj, h32, 0.37, gp)
        assert rc == 0 and sorted(seq) == res["feat_id"].tolist()
        for k, fid in enumerate(res["feat_id"].tolist()):
            ii, x, y, term, weight = seq[fid]
            assert ii == res["feat_index"][k]
            got = (res["pos"][k, 0], res["pos"][k, 1], res["data_term"][k], res["data_weight"][k])
            assert np.array([x, y, term, weight], np.float32).tobytes() == np.array(got, np.float32).tobytes(), (fid, k)


# ---- GPU: bit-equal to the checker --------------------------------------------------------------------------------

def _tracker(sc):
    from flame_amd.stereo import FeatureTracker

    return FeatureTracker(sc.K32, sc.Kinv32, sc.width, sc.height, border=PAD)


def _view(a):
    from flame_amd.stereo import FEATURE_DTYPE

    return np.ascontiguousarray(a).view(FEATURE_DTYPE)


def assert_same_result(got, ref, what):
    for k in ("V",) + sr.COUNTERS:
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    for k in sr.ARRAYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.nonzero((a.view(np.uint32).reshape(len(a), -1) != b.view(np.uint32).reshape(len(b), -1)).any(axis=1))[0]
            raise AssertionError("%s: %s differs at %d places, first %d: %r vs %r" % (what, k, bad.size, bad[0], a[bad[0]], b[bad[0]]))


def _combos():
    for adaptive in (0, 1):
        for scale in sc_.SCALES:
            for band in sc_.BANDS:
                yield dict(band, adaptive_data_weights=adaptive), scale


def _gpu_select(tr, world, gp, scale, feats=None, proj=None):
    from flame_amd.stereo import GraphParams

    if feats is not None:
        feats, proj = _view(feats), _view(proj)
    return tr.select_graph_features(GraphParams(**gp), scale, world, feats, proj, raise_on_error=False)


@gpu
@pytest.mark.parametrize("copy_mode", [0, 1])
@pytest.mark.parametrize("n", sc_.SIZES)
def test_gpu_select_arrays_matches_checker(built, n, copy_mode):
    case = sc_.make(n)
    sc = case["sc"]
    seen = np.zeros(4, np.int64)
    with _tracker(sc) as tr:
        tr.set_graph_copy(copy_mode)
        for gp, scale in _combos():
            rc_c, ref = sr.select(case["feats"], case["proj"], sc.Kinv32, case["world"], scale, gp)
            rc, got = _gpu_select(tr, case["world"], gp, scale, case["feats"], case["proj"])
            assert rc == rc_c == 0
            assert_same_result(got, ref, "n %d %r scale %g" % (n, gp, scale))
            seen += [got["V"], got["num_invalid"], got["num_fail_var"], got["num_fail_height"]]
        assert tr.last_kernel_ms() > 0
        assert tr.features_device()[1] == 0 and tr.projected_device()[1] == 0  # neither resident set is touched
    print(n, copy_mode, "selected / invalid / variance / height over the settings:", seen.tolist())
    if n >= 1000:
        assert (seen > 0).all()


@gpu
@pytest.mark.parametrize("n", sc_.SIZES)
def test_gpu_select_resident_matches_checker(built, n):
    """set_features + project_features, then the selection on the resident and the projected set: against the checker
    applied to the checker's own post-projection sets.  The stage only reads: both sets are byte-identical afterwards."""
    from flame_amd.stereo import StereoParams

    case = sc_.make(n)
    sc = case["sc"]
    kept, cur = sc_.resident_sets(n)
    with _tracker(sc) as tr:
        tr.set_features(_view(case["feats"]))
        assert tr.project_features(StereoParams(), sc_.CUR, sc_.project_poses(sc)) == kept.shape[0]
        assert tr.get_features().tobytes() == kept.tobytes() and tr.get_projected().tobytes() == cur.tobytes()
        for copy_mode in (0, 1):
            tr.set_graph_copy(copy_mode)
            for gp, scale in _combos():
                rc_c, ref = sr.select(kept, cur, sc.Kinv32, case["world"], scale, gp)
                rc, got = _gpu_select(tr, case["world"], gp, scale)
                assert rc == rc_c == 0
                assert_same_result(got, ref, "resident n %d %r scale %g" % (n, gp, scale))
                if n >= 1000 and "min_height" not in gp:
                    assert got["V"] > 0 and got["num_invalid"] == 0 and got["num_fail_var"] > 0 and got["num_fail_height"] > 0
        assert tr.get_features().tobytes() == kept.tobytes() and tr.get_projected().tobytes() == cur.tobytes()
        xy, mu, var = tr.get_raw_idepths()  # Flame::getRawIDepths: the valid records of the projected set
        assert xy.tobytes() == np.stack([cur["x"], cur["y"]], 1).tobytes() and mu.tobytes() == cur["idepth_mu"].tobytes()
        assert var.tobytes() == cur["idepth_var"].tobytes()


@gpu
@pytest.mark.parametrize("n", (1500, 8400, 61441))
def test_gpu_select_resident_after_an_in_place_prune_sees_invalid_records(built, n):
    from flame_amd.stereo import StereoParams

    case = sc_.make(n)
    sc = case["sc"]
    kept, cur = sc_.resident_sets(n, prune=True)
    keep, dropped, target = sc_.PRUNE
    with _tracker(sc) as tr:
        tr.set_features(_view(case["feats"]))
        m = tr.project_features(StereoParams(), sc_.CUR, sc_.project_poses(sc))
        st = tr.prune_pose_frames(StereoParams(), target, keep, pc.dropped_poses(sc, dropped, target), first_new=m)
        assert st["num_removed"] == 0 and st["num_invalidated"] > 0
        assert tr.get_features().tobytes() == kept.tobytes() and tr.get_projected().tobytes() == cur.tobytes()
        for gp, scale in _combos():
            rc_c, ref = sr.select(kept, cur, sc.Kinv32, case["world"], scale, gp)
            rc, got = _gpu_select(tr, case["world"], gp, scale)
            assert rc == rc_c == 0
            assert_same_result(got, ref, "pruned n %d %r scale %g" % (n, gp, scale))
            assert got["V"] > 0 and got["num_invalid"] > 0 and got["num_fail_var"] > 0 and got["num_fail_height"] > 0
        assert tr.get_features().tobytes() == kept.tobytes() and tr.get_projected().tobytes() == cur.tobytes()
        # a prune that REMOVES a record breaks the alignment
        tr.set_features(_view(case["feats"]))
        m = tr.project_features(StereoParams(), sc_.CUR, sc_.project_poses(sc))
        st = tr.prune_pose_frames(StereoParams(), target, keep, pc.dropped_poses(sc, dropped, target), first_new=0)
        assert st["num_removed"] > 0
        rc, got = _gpu_select(tr, case["world"], {}, 1.0)
        assert rc == -1 and got["V"] == 0


@gpu
def test_gpu_second_call_does_not_depend_on_the_first(built):
    """Shrinking and growing V and n on one context, both forms and both ways of copying out interleaved."""
    sc = sc_.scene_for(8400)
    big, small, mid = sc_.make(16000), sc_.make(8400), None
    with _tracker(sc) as tr:
        for k, (case, gp, scale, mode) in enumerate([(big, dict(), 1.0, 0), (small, dict(adaptive_data_weights=1), 0.37, 1),
                                                     (big, dict(min_height=-0.5, max_height=1.5), 2.5, 1),
                                                     (small, dict(idepth_var_max_graph=0.003), 1.0, 0),
                                                     (big, dict(idepth_var_max_graph=1.0, min_height=-100.0, max_height=100.0), 1.0, 0),
                                                     (small, dict(), 1.0, 0)]):
            tr.set_graph_copy(mode)
            rc_c, ref = sr.select(case["feats"], case["proj"], sc.Kinv32, case["world"], scale, gp)
            rc, got = _gpu_select(tr, case["world"], gp, scale, case["feats"], case["proj"])
            assert rc == rc_c == 0
            assert_same_result(got, ref, "call %d" % k)
            print(k, got["V"])
    assert mid is None


def _raw(tr):
    from flame_amd.stereo import _lib

    return _lib(), tr._ctx


@gpu
@pytest.mark.parametrize("form", ["arrays", "resident"])
def test_gpu_select_error_contracts(built, form):
    """Points 4, 6, 7 and 8 of the header, NULL and negative arguments; after each failing call a valid call gives the
    right answer, and the resident and the projected set are byte-identical before and after every call."""
    from flame_amd.stereo import DetectParams, GraphParams, StereoParams, _GraphInputs, _WorldPose

    n = 1500
    case = sc_.make(n)
    sc, world = case["sc"], case["world"]
    kept, cur = sc_.resident_sets(n)
    feats, proj = (case["feats"], case["proj"]) if form == "arrays" else (kept, cur)
    sp = StereoParams()
    with _tracker(sc) as tr:
        for k in pc.PF_IDS + (23, 24):
            tr.add_frame(k, sc.render(k))
        if form == "resident":  # point 7: no projection yet
            assert _gpu_select(tr, world, {}, 1.0)[0] == -1
            tr.set_features(_view(case["feats"]))
            assert _gpu_select(tr, world, {}, 1.0)[0] == -1
        tr.set_features(_view(case["feats"]))
        tr.project_features(sp, sc_.CUR, sc_.project_poses(sc))
        res0, proj0 = tr.get_features(), tr.get_projected()
        assert res0.tobytes() == kept.tobytes() and proj0.tobytes() == cur.tobytes()

        def call(f=None, c=None, w=world, gp=None, scale=1.0):
            f = feats if f is None else f
            c = proj if c is None else c
            if form == "arrays":
                out = _gpu_select(tr, w, gp or {}, scale, f, c)
            else:
                if f is not feats:  # bring the edited records into the resident set
                    tr.set_features(_view(f))
                    st = tr.project_features(sp, sc_.CUR, sc_.project_poses(sc), raise_on_error=False)
                    assert st[0] == 0 and st[1]["num_features"] == f.shape[0], st
                out = _gpu_select(tr, w, gp or {}, scale)
            return out

        def good(what):
            if form == "resident" and tr.get_features().tobytes() != kept.tobytes():
                tr.set_features(_view(case["feats"]))
                tr.project_features(sp, sc_.CUR, sc_.project_poses(sc))
            rc_c, ref = sr.select(feats, proj, sc.Kinv32, world, 0.37, dict(adaptive_data_weights=1))
            rc, got = call(gp=dict(adaptive_data_weights=1), scale=0.37)
            assert rc == rc_c == 0
            assert_same_result(got, ref, what)
            assert tr.get_features().tobytes() == res0.tobytes() and tr.get_projected().tobytes() == proj0.tobytes()

        def failed(rc, got, want_rc, want_index, f=None, c=None, w=world):
            rc_c, ref = sr.select(feats if f is None else f, proj if c is None else c, sc.Kinv32, w, 1.0)
            assert (rc, got["error_feature"]) == (want_rc, want_index) == (rc_c, ref["error_feature"]), (rc, got["error_feature"])
            assert got["V"] == 0 and all(got[k].size == 0 for k in sr.ARRAYS)

        good("first")
        # point 4: an unknown frame (a pose list that misses pose-frame 16), for every record, valid or not
        w = [p for p in world if p["id"] != 16]
        first16 = int(np.nonzero(feats["frame_id"] == 16)[0][0])
        rc, got = call(w=w)
        failed(rc, got, -1, first16, w=w)
        good("after the unknown frame")
        rc, got = call(w=[])
        failed(rc, got, -1, 0, w=[])
        good("after no poses")
        if form == "arrays":
            # point 4: the assert runs for every record, valid or not; the lowest index decides between the two errors
            inv = np.nonzero(feats["valid"] == 0)[0]
            bad = feats.copy()
            bad["idepth_mu"][inv[3]] = -0.25
            bad["idepth_mu"][inv[7]] = np.nan
            rc, got = call(f=bad)
            failed(rc, got, -8, int(inv[3]), f=bad)
            good("after the negative idepth")
            bad = feats.copy()
            bad["idepth_mu"][inv[7]] = np.nan
            bad["frame_id"][inv[9]] = 42
            rc, got = call(f=bad)
            failed(rc, got, -8, int(inv[7]), f=bad)
            bad["frame_id"][inv[2]] = 42
            rc, got = call(f=bad)
            failed(rc, got, -1, int(inv[2]), f=bad)
            bad["idepth_mu"][inv[2]] = -1.0  # both in one record: the assert comes first
            rc, got = call(f=bad)
            failed(rc, got, -8, int(inv[2]), f=bad)
            good("after the mixed errors")
        # point 6: an id >= 2^31 among the selected; among the others it does not matter
        rc_c, ref = sr.select(feats, proj, sc.Kinv32, world, 1.0)
        taken = ref["feat_index"]
        others = np.setdiff1d(np.arange(feats.shape[0]), taken)
        bad = feats.copy()
        bad["id"][others[:50]] = 2 ** 31 + np.arange(50)
        bad_c = proj.copy()
        bad_c["id"] = bad["id"] if form == "resident" else bad_c["id"]
        rc, got = call(f=bad)
        rc_c, ref_b = sr.select(bad, bad_c, sc.Kinv32, world, 1.0)
        assert rc == rc_c == 0
        assert_same_result(got, ref_b, "big ids among the rejected")
        bad["id"][taken[5]] = 2 ** 31
        bad["id"][taken[9]] = 2 ** 32 - 1
        rc, got = call(f=bad)
        failed(rc, got, -1, int(taken[5]), f=bad)
        good("after the big id")
        # NULL and negative arguments
        L, ctx = _raw(tr)
        gp, out = GraphParams(), _GraphInputs()
        wp = tr._world_poses(world)
        a, b = _view(feats), _view(proj)
        if form == "resident":
            fn = L.flame_stereo_select_graph_features
            bad_calls = [(ctx, None, 1.0, len(world), wp, C.byref(out)), (ctx, C.byref(gp), 1.0, len(world), wp, None),
                         (ctx, C.byref(gp), 1.0, -1, wp, C.byref(out)), (ctx, C.byref(gp), 1.0, len(world), None, C.byref(out)),
                         (None, C.byref(gp), 1.0, len(world), wp, C.byref(out))]
        else:
            fn = L.flame_stereo_select_graph_features_arrays
            m = feats.shape[0]
            bad_calls = [(ctx, None, 1.0, len(world), wp, m, a.ctypes.data, b.ctypes.data, C.byref(out)),
                         (ctx, C.byref(gp), 1.0, len(world), wp, m, a.ctypes.data, b.ctypes.data, None),
                         (ctx, C.byref(gp), 1.0, -1, wp, m, a.ctypes.data, b.ctypes.data, C.byref(out)),
                         (ctx, C.byref(gp), 1.0, len(world), None, m, a.ctypes.data, b.ctypes.data, C.byref(out)),
                         (ctx, C.byref(gp), 1.0, len(world), wp, -1, a.ctypes.data, b.ctypes.data, C.byref(out)),
                         (ctx, C.byref(gp), 1.0, len(world), wp, m, None, b.ctypes.data, C.byref(out)),
                         (ctx, C.byref(gp), 1.0, len(world), wp, m, a.ctypes.data, None, C.byref(out)),
                         (None, C.byref(gp), 1.0, len(world), wp, m, a.ctypes.data, b.ctypes.data, C.byref(out))]
        for args in bad_calls:
            out.V, out.error_feature = 3, 3
            assert fn(*args) == -1, args
            assert (out.V, out.error_feature, bool(out.pos)) == ((0, -1, False) if args[-1] is not None else (3, 3, False))
            good("after a bad argument")
        # point 8: no features
        if form == "arrays":
            rc, got = _gpu_select(tr, world, {}, 1.0, feats[:0], proj[:0])
            assert rc == 0 and got["V"] == 0 and got["num_examined"] == 0 and got["error_feature"] == -1
            assert fn(ctx, C.byref(gp), 1.0, 0, None, 0, None, None, C.byref(out)) == 0 and out.V == 0 and not out.feat_id
            good("after the empty call")
            return
        # point 7 (resident): update_resident between the two calls keeps the flag, whatever changes membership clears it
        rc, st = tr.update_resident(sp, 24, 22, ss.poses_for(sc, pc.PF_IDS, 24, 22))
        assert rc == 0 and st["num_idepth_updates"] > 0
        now = tr.get_features()
        assert now.tobytes() != kept.tobytes() and tr.get_projected().tobytes() == proj0.tobytes()
        rc_c, ref = sr.select(now.view(so.FEATURE_DTYPE), cur, sc.Kinv32, world, 1.0)
        rc, got = _gpu_select(tr, world, {}, 1.0)
        assert rc == rc_c == 0
        assert_same_result(got, ref, "after update_resident")
        assert tr.get_features().tobytes() == now.tobytes()
        q, t = sc.relative(23, 22)
        added = tr.detect_features(sp, DetectParams(), 23, q, t, mask_xy="projected", first_id=10 ** 6)
        assert added > 0 and _gpu_select(tr, world, {}, 1.0)[0] == -1  # records without a projected counterpart
        tr.project_features(sp, 24, sc_.project_poses(sc, pc.PF_IDS + (23,), cur=24))
        w23 = sc_.world_poses(sc, pc.PF_IDS + (23,))
        rc_c, ref = sr.select(tr.get_features().view(so.FEATURE_DTYPE), tr.get_projected().view(so.FEATURE_DTYPE), sc.Kinv32, w23, 1.0)
        rc, got = _gpu_select(tr, w23, {}, 1.0)
        assert rc == rc_c == 0 and got["num_examined"] > kept.shape[0] - 5
        assert_same_result(got, ref, "after detection and projection")
        tr.clear_features()
        assert _gpu_select(tr, w23, {}, 1.0)[0] == -1
        tr.set_features(_view(feats[:0]))
        assert tr.project_features(sp, sc_.CUR, sc_.project_poses(sc)) == 0
        rc, got = _gpu_select(tr, world, {}, 1.0)  # point 8
        assert rc == 0 and got["V"] == 0 and got["num_examined"] == 0
