"""The pyramid levels and the direct alignment on the GPU, through the C-ABI (flame_amd.stereo): every plane of every level, the 28
sums and the 5 counts of every linearisation, compared with the checker (tests/align_ref.py) as bits -- .view(uint32) / .view(uint64), no
tolerance.  In each test the checker runs alone first and must show that the classes the case is about are populated, so that nothing
passes by being empty.  The driver's loop is checked from its own trace."""
import numpy as np
import pytest

from tests import align_cases as ac
from tests import align_ref as ar

pytestmark = pytest.mark.gpu
INVALID_ARG, NO_GRAPH = -1, -4
F = np.float32
IDENT = (np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3))


def _tracker(w, h, K, border=3):
    from flame_amd.stereo import FeatureTracker

    Km, Ki = ac.K_matrices(K)
    return FeatureTracker(Km, Ki, w, h, border=border)


def _assert_level(got, want, what):
    for name, g, w_ in zip(("img", "gradx", "grady"), got, want):
        assert g.shape == w_.shape and g.dtype == w_.dtype, (what, name, g.shape, w_.shape)
        gb = g.view(np.uint32) if g.dtype == F else g
        wb = np.ascontiguousarray(w_).view(np.uint32) if w_.dtype == F else w_
        bad = np.argwhere(gb != wb)
        assert bad.shape[0] == 0, "%s: %s differs at %d places, first %s: %r vs %r" % (what, name, bad.shape[0], bad[0], g[tuple(bad[0])],
                                                                                    w_[tuple(bad[0])])


# ---- 1. pyramid levels ----
@pytest.mark.parametrize("w,h,n_levels", [(33, 17, 3), (67, 45, 3), (9, 8, 2)])
def test_gpu_pyramid_levels_equal_the_checker(built, w, h, n_levels):
    """67 x 45: three workgroups across and six down at level 1 (34 x 23), an odd size at every level; 9 x 8 -> 5 x 4: the 5 x 5 window
    reflects more than once."""
    img = ac.random_image(w, h, 100 + w)
    want = ar.build_pyramid(img, n_levels)
    assert [p[0].shape for p in want] == [ar.level_size(w, h, l)[::-1] for l in range(n_levels)]
    assert all(p[0].std() > 1 and np.abs(p[1]).max() > 0 and np.abs(p[2]).max() > 0 for p in want)  # nothing flat
    with _tracker(w, h, (64.0, 64.0, w / 2, h / 2)) as tr:
        tr.add_frame(7, img)
        tr.build_pyramid(7, n_levels)
        for l in range(n_levels):
            _assert_level(tr.download_pyramid_level(7, l), want[l], "%dx%d level %d" % (w, h, l))
        assert tr.download_pyramid_level(7, n_levels, raise_on_error=False)[0] == INVALID_ARG
        assert tr.build_pyramid(7, n_levels) == 0  # again: a no-op
        _assert_level(tr.download_pyramid_level(7, n_levels - 1), want[n_levels - 1], "after the second build")


def test_gpu_pyramid_lifetime_and_errors(built):
    w, h = 67, 45
    a, b = ac.random_image(w, h, 1), ac.random_image(w, h, 2)
    pa, pb = ar.build_pyramid(a, 3), ar.build_pyramid(b, 3)
    assert not np.array_equal(pa[2][0], pb[2][0])
    with _tracker(w, h, (64.0, 64.0, 33.0, 22.0)) as tr:
        tr.add_frame(1, a)
        assert tr.download_pyramid_level(1, 1, raise_on_error=False)[0] == INVALID_ARG  # not built yet
        _assert_level(tr.download_pyramid_level(1, 0), pa[0], "level 0 needs no build")
        tr.build_pyramid(1, 3)
        # the error cases leave the frame count and the levels as they were
        for frame, n in ((1, 0), (1, 6), (1, 5), (2, 3), (1, -1)):  # 67 x 45 over 5 levels: 5 x 3 at the last
            assert tr.build_pyramid(frame, n, raise_on_error=False) == INVALID_ARG, (frame, n)
        assert tr.frame_count() == 1
        for l in range(3):
            _assert_level(tr.download_pyramid_level(1, l), pa[l], "after the failed builds, level %d" % l)
        tr.build_pyramid(1, 2)  # another n_levels: rebuilt, level 2 is gone
        _assert_level(tr.download_pyramid_level(1, 1), pa[1], "rebuilt with 2 levels")
        assert tr.download_pyramid_level(1, 2, raise_on_error=False)[0] == INVALID_ARG
        tr.build_pyramid(1, 3)
        # replacing the frame releases its levels
        tr.add_frame(1, b)
        assert tr.download_pyramid_level(1, 1, raise_on_error=False)[0] == INVALID_ARG
        tr.build_pyramid(1, 3)
        _assert_level(tr.download_pyramid_level(1, 2), pb[2], "the replaced frame's level 2")
        # drop_frame releases them; the buffers go to the next frame, whose levels are not built
        tr.drop_frame(1)
        assert tr.frame_count() == 0 and tr.download_pyramid_level(1, 0, raise_on_error=False)[0] == INVALID_ARG
        tr.add_frame(2, a)
        assert tr.download_pyramid_level(2, 1, raise_on_error=False)[0] == INVALID_ARG
        tr.build_pyramid(2, 3)
        _assert_level(tr.download_pyramid_level(2, 2), pa[2], "a frame on recycled buffers")
        # set_camera releases everything
        Km, Ki = ac.K_matrices((64.0, 64.0, 16.0, 8.0))
        tr.set_camera(Km, Ki, 33, 17, border=3)
        assert tr.frame_count() == 0 and tr.build_pyramid(2, 3, raise_on_error=False) == INVALID_ARG
        c = ac.random_image(33, 17, 3)
        tr.add_frame(2, c)
        tr.build_pyramid(2, 3)
        _assert_level(tr.download_pyramid_level(2, 2), ar.build_pyramid(c, 3)[2], "after set_camera")


# ---- 2. one padded chunk ----
def _scene(w, h, seed, d_lo=0.3, d_hi=0.9):
    rng = np.random.default_rng(seed)
    ref, new = ac.random_image(w, h, seed), ac.random_image(w, h, seed + 1)
    d = rng.uniform(d_lo, d_hi, (h, w)).astype(F)
    return ref, new, d


def _reference(ref_pyr, new_pyr, d, level, K, border, huber_k, q, t):
    return ar.linearize(ref_pyr[level][0], new_pyr[level], d, level, K, border, huber_k, q, t)


def test_gpu_linearisation_of_one_padded_chunk(built):
    """33 x 17 = 561 pixels: one chunk of 1024, padded; border 1: the taps reach the level's last row and column."""
    import torch
    from flame_amd.stereo import AlignParams

    w, h, K = 33, 17, (32.0, 32.0, 16.0, 8.0)
    ref, new, d = _scene(w, h, 5)
    q, t = ac.small_pose()
    want = _reference(ar.build_pyramid(ref, 1), ar.build_pyramid(new, 1), d, 0, K, 1, 10.0, q, t)
    assert want["n_used"] > 300 and want["n_outside"] > 0 and want["n_huber"] > 50 and want["n_huber"] < want["n_used"]
    assert np.count_nonzero(want["sums"]) == 28
    P = AlignParams(border=1, huber_k=10.0)
    with _tracker(w, h, K) as tr:
        tr.add_frame(1, ref)
        tr.add_frame(2, new)
        host = tr.align_linearize(P, 1, 2, 0, d, q, t)
        ar.assert_same_system(host, want, "map from the host")
        assert tr.last_kernel_ms() > 0
        dev = torch.from_numpy(d.copy()).cuda()
        torch.cuda.synchronize()
        first = tr.align_linearize(P, 1, 2, 0, int(dev.data_ptr()), q, t)
        again = tr.align_linearize(P, 1, 2, 0, int(dev.data_ptr()), q, t)
        ar.assert_same_system(first, want, "map from a device buffer")
        assert first["sums"].tobytes() == again["sums"].tobytes() and all(first[n] == again[n] for n in ar.COUNTS)
        # the error returns, with nothing changed
        bad = [
            dict(ref=9), dict(new=9), dict(level=1), dict(level=-1), dict(P=AlignParams(border=8, huber_k=10.0)),  # 2 * 8 + 2 > 17
            dict(P=AlignParams(border=0, huber_k=10.0)), dict(P=AlignParams(border=1, huber_k=0.0)), dict(P=AlignParams(border=1, huber_k=-1.0)),
            dict(q=(1.0, np.nan, 0.0, 0.0)), dict(t=(0.0, np.inf, 0.0)), dict(m=None),
        ]
        for kw in bad:
            rc, _ = tr.align_linearize(kw.get("P", P), kw.get("ref", 1), kw.get("new", 2), kw.get("level", 0), kw.get("m", d),
                                       kw.get("q", q), kw.get("t", t), raise_on_error=False)
            assert rc == INVALID_ARG, kw
        ar.assert_same_system(tr.align_linearize(P, 1, 2, 0, d, q, t), want, "after the refused calls")
        assert tr.frame_count() == 2
    with _tracker(w, h, (32.0, 32.0, 16.0, 8.0)) as tr:  # a camera with a skew is refused
        Km, Ki = ac.K_matrices(K)
        Km[1] = 0.5
        tr.set_camera(Km, Ki, w, h, border=3)
        tr.add_frame(1, ref)
        tr.add_frame(2, new)
        assert tr.align_linearize(P, 1, 2, 0, d, q, t, raise_on_error=False)[0] == INVALID_ARG


# ---- 3. every class of pixel ----
CLASS_W, CLASS_H, CLASS_K, CLASS_BORDER, CLASS_HUBER = 64, 48, (64.0, 64.0, 16.0, 8.0), 2, 10.0


def _class_case():
    """ref, new, map and three poses.  With the identity pose and this K every eligible pixel lands on itself, u = x and v = y exactly, so
    r = new - ref is the integer the images were crafted with and the inside test meets both of its bounds with equality."""
    w, h = CLASS_W, CLASS_H
    rng = np.random.default_rng(42)
    ref = rng.integers(40, 200, (h, w), dtype=np.uint8)
    new = ref.copy()
    new[:, 8:16] += 10   # |r| == huber_k exactly: weight 1
    new[:, 16:24] += 11  # just above
    new[:, 24:32] -= 15  # r < 0, above
    new[:, 32:40] -= 10  # r == -huber_k exactly
    new[:, 40:48] += 3
    d = np.full((h, w), 0.5, F)
    d[4:8, 4:12] = np.nan
    d[8:12, 4:12] = 0.0
    d[12:16, 4:12] = -1.0
    d[16:20, 4:12] = np.inf
    d[24:40, 20:44] = 1.0  # behind the camera once t_z = -1.5 (t_z d < -1), in front (Xz = 0.25) where d = 0.5
    poses = {
        "identity": IDENT,
        "behind": (np.array([1.0, 0.0, 0.0, 0.0]), np.array([0.0, 0.0, -1.5])),
        "outside": (ac.small_pose()[0], np.array([0.4, -0.3, 0.1])),
    }
    return ref, new, d, poses


def test_gpu_every_class_of_pixel(built):
    from flame_amd.stereo import AlignParams

    ref, new, d, poses = _class_case()
    w, h, b = CLASS_W, CLASS_H, CLASS_BORDER
    rp, npyr = ar.build_pyramid(ref, 3), ar.build_pyramid(new, 3)
    want = {(name, l): _reference(rp, npyr, d, l, CLASS_K, b, CLASS_HUBER, *pose) for name, pose in poses.items() for l in range(3)}
    # the checker alone: every class is there
    for (name, l), s in want.items():
        wl, hl = ar.level_size(w, h, l)
        assert s["n_used"] + s["n_no_depth"] + s["n_behind"] + s["n_outside"] == (wl - 2 * b) * (hl - 2 * b), (name, l)
        assert s["n_no_depth"] > 0 and s["n_huber"] <= s["n_used"]
    ident = want[("identity", 0)]
    px = ident["px"]
    assert ident["n_no_depth"] == 4 * 4 * 8 and ident["n_behind"] == 0
    ring = px["ring"] & ~px["no_depth"]
    xx, yy = np.meshgrid(np.arange(w), np.arange(h))
    assert (px["u"][ring] == xx[ring]).all() and (px["v"][ring] == yy[ring]).all()  # exact
    assert px["used"][ring & (xx == b) & (yy > b) & (yy < h - 1 - b)].all()  # u == border: inside
    assert px["outside"][ring & (xx == w - 1 - b)].all() and px["outside"][ring & (yy == h - 1 - b)].all()  # u == w - 1 - border: outside
    assert ident["n_outside"] == int((ring & ((xx == w - 1 - b) | (yy == h - 1 - b))).sum()) > 0
    r = px["r"][px["used"]]
    assert set(np.unique(r).tolist()) == {-15.0, -10.0, 0.0, 3.0, 10.0, 11.0}
    assert ident["n_huber"] == int((np.abs(r) > 10).sum()) and 0 < ident["n_huber"] < int((np.abs(r) >= 10).sum())
    wg = px["wgt"][px["used"]]
    assert (wg[np.abs(r) == 10] == 1).all() and (wg[r == 11] == F(10) / F(11)).all() and (wg[r == -15] == F(10) / F(15)).all()
    assert want[("behind", 0)]["n_behind"] == 16 * 24 and want[("behind", 0)]["n_used"] > 0
    assert all(want[("behind", l)]["n_behind"] > 0 for l in range(3))
    assert all(want[("outside", l)]["n_outside"] > want[("identity", l)]["n_outside"] and want[("outside", l)]["n_used"] > 0 for l in range(3))
    P = AlignParams(border=b, huber_k=CLASS_HUBER)
    with _tracker(w, h, CLASS_K) as tr:
        tr.add_frame(1, ref)
        tr.add_frame(2, new)
        tr.build_pyramid(1, 3)
        assert tr.align_linearize(P, 1, 2, 1, d, *IDENT, raise_on_error=False)[0] == INVALID_ARG  # built for one frame only
        tr.build_pyramid(2, 3)
        for (name, l), s in want.items():
            got = tr.align_linearize(P, 1, 2, l, d, *poses[name])
            ar.assert_same_system(got, s, "%s pose, level %d" % (name, l))


# ---- 4. more than 1024 chunks ----
def test_gpu_linearisation_of_more_than_1024_chunks(built):
    """1200 x 881 = 1 057 200 pixels: 1033 chunks, the last one padded; the partials are combined strided (two rounds), then pairwise."""
    from flame_amd.stereo import AlignParams

    w, h, K = 1200, 881, (1024.0, 1024.0, 600.0, 440.0)
    assert (w * h + 1023) // 1024 == 1033 and (w * h) % 1024 != 0
    r0, n0 = ac.driver_scene()[:2]
    ref, new = (np.ascontiguousarray(np.tile(a, (13, 13))[:h, :w]) for a in (r0, n0))
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    d = (0.5 + 0.2 * np.sin(xx / 97.0) * np.cos(yy / 61.0)).astype(F)
    q, t = ac.small_pose()
    want = _reference(ar.build_pyramid(ref, 1), ar.build_pyramid(new, 1), d, 0, K, 2, 10.0, q, t)
    assert want["n_used"] > 900 * 1024 and want["n_outside"] > 0 and want["n_huber"] > 0 and np.count_nonzero(want["sums"]) == 28
    with _tracker(w, h, K) as tr:
        tr.add_frame(1, ref)
        tr.add_frame(2, new)
        got = tr.align_linearize(AlignParams(border=2, huber_k=10.0), 1, 2, 0, d, q, t)
        ar.assert_same_system(got, want, "1033 chunks")


# ---- 5. nothing eligible ----
def test_gpu_nothing_eligible(built):
    from flame_amd.stereo import ALIGN_TOO_FEW, AlignParams

    ref, new, d, _, _ = ac.driver_scene()
    nan_map = np.full_like(d, np.nan)
    P = AlignParams(**ac.DRIVER_PARAMS)
    with _tracker(ac.DRIVER_W, ac.DRIVER_H, ac.DRIVER_K) as tr:
        tr.add_frame(1, ref)
        tr.add_frame(2, new)
        tr.build_pyramid(1, 3)
        tr.build_pyramid(2, 3)
        q, t = np.array([1.0, 0.0, 0.0, 0.0]), np.array([0.1, 0.0, 0.0])
        for level in range(3):
            s = tr.align_linearize(P, 1, 2, level, nan_map, q, t)
            wl, hl = ar.level_size(ac.DRIVER_W, ac.DRIVER_H, level)
            assert s["n_used"] == 0 and s["n_no_depth"] == (wl - 4) * (hl - 4) and s["n_behind"] == s["n_outside"] == s["n_huber"] == 0
            assert (s["sums"].view(np.uint64) == 0).all()  # +0.0, every one
        res = tr.align_frame(P, 1, 2, nan_map, q, t)
        assert res["status"] == ALIGN_TOO_FEW and res["n_evals"] == 1 and len(res["trace"]) == 1 and res["trace"][0]["level"] == 2
        assert res["q"].tobytes() == q.tobytes() and res["t"].tobytes() == t.tobytes() and res["iters"] == [0] * 5


# ---- 6. the driver ----
def test_gpu_driver_is_what_its_trace_says(built):
    """96 x 72, levels 2 -> 0, from the identity.  Everything is derived from the recorded trace: (a) the checker's linearisation at
    every recorded double pose gives the recorded sums and counts, bit for bit; (b) every accept / reject is the rule recomputed from the
    recorded sums; (c) every recorded delta solves its system to 1e-9 (||H|| ||delta|| + ||b||): a 6 x 6 Cholesky in double is backward
    stable near 1e-15, a wrong factor is off by orders; (d) every next pose is numpy's exp(delta) T within 1e-12 per component (|t| <= 1:
    four orders above double rounding over a few dozen operations, five below the float32 step a wrong formula would move); (e) the final
    float32 R, t are the roundings of the final double pose; (f) the final pose is nearer the truth than the start."""
    from flame_amd.stereo import ALIGN_FLAG_REJECTED, ALIGN_OK, AlignParams

    ref, new, d, q_true, t_true = ac.driver_scene()
    alone = ac.driver_reference()  # the checker alone: the scene converges and every branch of the loop is taken
    assert alone["status"] == ar.OK and any(e["accepted"] == 0 for e in alone["trace"]) and sum(alone["iters"]) >= 3
    rp, npyr = ar.build_pyramid(ref, 3), ar.build_pyramid(new, 3)
    PK = ac.DRIVER_PARAMS
    with _tracker(ac.DRIVER_W, ac.DRIVER_H, ac.DRIVER_K) as tr:
        tr.add_frame(1, ref)
        tr.add_frame(2, new)
        tr.build_pyramid(1, 3)
        tr.build_pyramid(2, 3)
        res = tr.align_frame(AlignParams(**PK), 1, 2, d, *IDENT)
        rc, _ = tr.align_frame(AlignParams(**dict(PK, coarsest_level=3)), 1, 2, d, *IDENT, raise_on_error=False)
        assert rc == INVALID_ARG  # level 3 is not built
    trace = res["trace"]
    assert res["status"] == ALIGN_OK and res["n_evals"] == len(trace) >= 6 and [e["level"] for e in trace] == sorted((e["level"] for e in trace), reverse=True)
    assert {e["level"] for e in trace} == {0, 1, 2}
    cur_q, cur_t, base, level = IDENT[0], IDENT[1], None, None
    iters = [0] * 5
    for k, e in enumerate(trace):
        what = "evaluation %d (level %d)" % (k, e["level"])
        ar.assert_same_system(e, _reference(rp, npyr, d, e["level"], ac.DRIVER_K, PK["border"], PK["huber_k"], e["q"], e["t"]), what)  # (a)
        if e["level"] != level:  # a level's first evaluation: at the pose reached so far, no step
            assert not e["delta"].any() and e["accepted"] == 1, what
            assert e["q"].tobytes() == cur_q.tobytes() and e["t"].tobytes() == cur_t.tobytes(), what
            base, level = e, e["level"]
            continue
        H, b, delta = ar.full_H(base["sums"]), base["sums"][21:27], e["delta"]
        A = H + PK["lm_lambda"] * np.diag(np.diag(H))
        resid = np.abs(A @ delta + b).max()
        bound = 1e-9 * (np.abs(A).sum(axis=1).max() * np.abs(delta).max() + np.abs(b).max())
        assert resid <= bound, (what, resid, bound)  # (c)
        q2, t2 = ar.exp_left(delta, cur_q, cur_t)
        assert np.abs(e["q"] - q2).max() <= 1e-12 and np.abs(e["t"] - t2).max() <= 1e-12 and np.abs(e["t"]).max() <= 1, what  # (d)
        assert bool(e["accepted"]) == ar.accept(e["sums"][27], e["n_used"], base["sums"][27], base["n_used"]), what  # (b)
        if e["accepted"]:
            cur_q, cur_t, base = e["q"], e["t"], e
            iters[level] += 1
            if k + 1 < len(trace) and trace[k + 1]["level"] == level:  # the level went on: the step was not yet below min_step
                assert np.abs(delta).max() >= PK["min_step"] and iters[level] < PK["max_iters_per_level"], what
        else:
            assert k + 1 == len(trace) or trace[k + 1]["level"] < level, what  # a rejection ends the level
    assert res["iters"] == iters and bool(res["flags"] & ALIGN_FLAG_REJECTED) == any(e["accepted"] == 0 for e in trace)
    assert res["q"].tobytes() == cur_q.tobytes() and res["t"].tobytes() == cur_t.tobytes()
    assert res["first_mean_cost"] == trace[0]["sums"][27] / trace[0]["n_used"] and res["last_mean_cost"] == base["sums"][27] / base["n_used"]
    assert res["q_f32"].tobytes() == res["q"].astype(F).tobytes() and res["t_f32"].tobytes() == res["t"].astype(F).tobytes()  # (e)
    assert res["R_f32"].tobytes() == ar.quat_to_rot(res["q"]).astype(F).tobytes()
    r0, t0 = ar.pose_error(*IDENT, q_true, t_true)
    r1, t1 = ar.pose_error(res["q"], res["t"], q_true, t_true)
    print("start", r0, t0, "end", r1, t1, "evaluations", len(trace), "iters", res["iters"])
    assert r1 < r0 and t1 < t0  # (f)
