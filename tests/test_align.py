"""The checker of the pyramid levels and the direct alignment (tests/align_ref.py restates include/flame_stereo.h) against known
answers and against the properties of the formulas it restates.  No device: the device is compared with this checker, bit for bit, in
tests/test_gpu_align.py."""
import numpy as np

from tests import align_cases as ac
from tests import align_ref as ar
from tests import map_error_ref as mer

F = np.float32


# ---- pyrDown known answers ----
def test_pyr_down_keeps_a_constant_image_constant_at_every_level():
    for value in (0, 1, 77, 255):
        pyr = ar.build_pyramid(np.full((45, 67), value, np.uint8), 4)
        assert [p[0].shape for p in pyr] == [(45, 67), (23, 34), (12, 17), (6, 9)]
        for img, gx, gy in pyr:
            assert (img == value).all() and (gx == 0).all() and (gy == 0).all()


def test_pyr_down_of_an_impulse_is_the_kernel():
    img = np.zeros((21, 25), np.uint8)
    img[10, 12] = 255  # even coordinates: the centre tap of output (5, 6)
    out = ar.pyr_down(img)
    k = np.array([1, 4, 6, 4, 1])
    want = np.zeros_like(out)
    # output (y, x) reads source (2y + i, 2x + j): the impulse at (10, 12) meets outputs y = 4, 5, 6 with i = 2, 0, -2
    for y, i in ((4, 2), (5, 0), (6, -2)):
        for x, j in ((5, 2), (6, 0), (7, -2)):
            want[y, x] = (k[i + 2] * k[j + 2] * 255 + 128) >> 8
    assert np.array_equal(out, want)
    assert out[5, 6] == (36 * 255 + 128) >> 8 and out[4, 5] == (1 * 255 + 128) >> 8
    img = np.zeros((21, 25), np.uint8)
    img[9, 11] = 255  # odd coordinates: taps i, j = +-1 of the four outputs around
    out = ar.pyr_down(img)
    assert out[4, 5] == out[5, 6] == out[4, 6] == out[5, 5] == (16 * 255 + 128) >> 8 and out.sum() == 4 * out[4, 5]


def test_pyr_down_sizes_are_rounded_up():
    for w, h in ((33, 17), (67, 45), (9, 8), (4, 4), (5, 7)):
        assert ar.pyr_down(np.zeros((h, w), np.uint8)).shape == ((h + 1) // 2, (w + 1) // 2)
    assert ar.level_size(33, 17, 2) == (9, 5) and ar.level_size(67, 45, 2) == (17, 12) and ar.level_size(9, 8, 1) == (5, 4)
    assert ar.levels_valid(33, 17, 3) and not ar.levels_valid(33, 17, 4) and ar.levels_valid(9, 8, 2) and not ar.levels_valid(9, 8, 3)
    assert not ar.levels_valid(640, 480, 0) and not ar.levels_valid(640, 480, 6) and ar.levels_valid(640, 480, 5)


def test_pyr_down_of_a_4x4_image_reflects_repeatedly():
    # len 4: period 6; source coordinates -2 .. 8 fold to 2 1 0 1 2 3 2 1 0 1 2
    assert ar.reflect_101(np.arange(-2, 9), 4).tolist() == [2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]
    assert ar.reflect_101(np.arange(-5, 6), 2).tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1]  # len 2 alternates
    img = ac.random_image(4, 4, 5)
    out = ar.pyr_down(img)
    k = [1, 4, 6, 4, 1]
    for y in range(2):
        for x in range(2):
            acc = 0
            for i in range(-2, 3):
                for j in range(-2, 3):
                    sy, sx = 2 * y + i, 2 * x + j
                    while not 0 <= sy < 4:  # the rule as cv::borderInterpolate loops it
                        sy = -sy if sy < 0 else 6 - sy
                    while not 0 <= sx < 4:
                        sx = -sx if sx < 0 else 6 - sx
                    acc += k[i + 2] * k[j + 2] * int(img[sy, sx])
            assert out[y, x] == (acc + 128) >> 8


def test_central_gradient_is_level_zero_of_add_frame():
    from oracle import stereo_capi as so

    img = ac.random_image(33, 17, 2)
    pad, gx_pad, gy_pad = so.make_frame(img, 3)
    gx, gy = ar.central_gradient(img)
    assert np.array_equal(gx.view(np.uint32), np.ascontiguousarray(gx_pad[3:-3, 3:-3]).view(np.uint32))
    assert np.array_equal(gy.view(np.uint32), np.ascontiguousarray(gy_pad[3:-3, 3:-3]).view(np.uint32))


# ---- the Jacobian ----
RAMP_W, RAMP_H, RAMP_K = 64, 48, (64.0, 64.0, 32.0, 24.0)
ALPHA, BETA, RAMP_D = 0.5, 0.25, 0.5


def ramp_level(dtype):
    yy, xx = np.meshgrid(np.arange(RAMP_H), np.arange(RAMP_W), indexing="ij")
    img = (ALPHA * xx + BETA * yy).astype(dtype)
    gx, gy = ar.central_gradient(img, dtype)
    assert (gx == ALPHA).all() and (gy == BETA).all()  # a ramp's differences are exact, at the edges too
    return img, gx, gy


def ramp_terms(q, t, dtype):
    R, tf = ar.pose_floats(q, t, dtype)
    ref = np.zeros((RAMP_H, RAMP_W), dtype)
    d = np.full((RAMP_H, RAMP_W), RAMP_D, dtype)
    return ar.pixel_terms(ref, ramp_level(dtype), d, 0, RAMP_K, 4, 1e9, R, tf, dtype)


def test_translation_columns_are_exact_on_a_ramp_in_float32():
    """fx = fy = 64, d = 0.5, t_z = 0, R = I: every operation of the warp and of the bilinear taps is exact in float32, so J0 and J1 are
    fx alpha d and fy beta d to the bit and r moves by exactly J0 delta under a pure x-translation."""
    q = (1.0, 0.0, 0.0, 0.0)
    base = ramp_terms(q, (0.0625, 0.0, 0.0), F)
    used = base["used"]
    assert used.sum() > 1000
    assert (base["J"][0][used] == F(64 * ALPHA * RAMP_D)).all() and (base["J"][1][used] == F(64 * BETA * RAMP_D)).all()
    delta = 1.0 / 256  # an eighth of a pixel
    moved = ramp_terms(q, (0.0625 + delta, 0.0, 0.0), F)
    both = used & moved["used"]
    assert both.sum() > 1000
    assert ((moved["r"] - base["r"])[both] == base["J"][0][both] * F(delta)).all()
    assert (base["r"][both] == (F(ALPHA) * base["u"] + F(BETA) * base["v"])[both]).all()  # the sampling itself is exact


def test_second_order_remainder_of_every_column():
    """|r(exp(delta) T) - r(T) - J delta| in float64 on the ramp, delta along one column.  Columns 2 .. 5 (v_z and the rotation): the
    remainder, as a norm over the pixels that stay inside, falls by a factor between 3.5 and 4.5 when delta is halved -- a property, no
    tolerance on the value.  Columns 0 and 1: with
    omega = 0, exp(delta) T only adds v to t, and r is affine in t_x and t_y on a ramp, so the remainder is zero in exact arithmetic and a
    ratio of two roundings means nothing; there the remainder itself is bounded by rounding, 1e-9 of |J delta| (float64 carries 1e-16; the
    bound leaves room for the cancellation in r' - r), which asks more of these two columns than second order does."""
    q, t = ac.small_pose()
    base = ramp_terms(q, t, np.float64)
    for col in range(6):
        rem = []
        masks = []
        for eps in (2e-3, 1e-3):
            delta = np.zeros(6)
            delta[col] = eps
            q2, t2 = ar.exp_left(delta, q, t)
            moved = ramp_terms(q2, t2, np.float64)
            masks.append(moved["used"])
            rem.append(moved["r"] - base["r"] - base["J"][col] * eps)
        both = base["used"] & masks[0] & masks[1]  # no sample crosses the inside test among these
        assert both.sum() > 1000
        a, b = np.abs(rem[0][both]), np.abs(rem[1][both])
        if col < 2:
            lin = np.abs(base["J"][col][both] * 2e-3)
            assert (a <= 1e-9 * lin).all() and (b <= 1e-9 * lin).all()
            continue
        # over the common pixels, in the 2-norm and in the max-norm (a single pixel whose second-order term happens to vanish has a
        # remainder of third order and no such ratio)
        for ratio in (np.linalg.norm(a) / np.linalg.norm(b), a.max() / b.max()):
            print("column", col, "ratio", ratio)
            assert 3.5 < ratio < 4.5, (col, ratio)


def test_weights_and_classes_of_the_checker():
    ref, new, d, q, t = ac.driver_scene()
    lv = ar.build_pyramid(new, 1)[0]
    s = ar.linearize(ref, lv, d, 0, ac.DRIVER_K, 2, 10.0, q, t)
    inner = (ac.DRIVER_W - 4) * (ac.DRIVER_H - 4)
    assert s["n_used"] + s["n_no_depth"] + s["n_behind"] + s["n_outside"] == inner and s["n_huber"] <= s["n_used"]
    H = ar.full_H(s["sums"])
    assert np.allclose(H, H.T) and (np.linalg.eigvalsh(H) > 0).all()


# ---- the sum rule ----
def test_sum_rule_is_the_map_errors():
    rng = np.random.default_rng(11)
    for n in (1, 1023, 1024, 1025, 33 * 17, 1025 * 1024 + 37):  # the last: 1026 chunks, a padded last chunk, two strided rounds
        e = (rng.standard_normal(n) * 100).astype(F)
        a, b = np.float64(ar.ordered_sum(e.astype(np.float64))), np.float64(mer.ordered_sum(e))
        assert a.tobytes() == b.tobytes(), n
    assert ar.CHUNK == mer.CHUNK == 1024


# ---- the loop ----
def test_checker_loop_on_a_synthetic_scene():
    """A smooth texture, a smooth known inverse depth, the true pose (about 2 degrees, |t| = 0.075) and the identity as the start.
    Measured with this checker (float32, levels 2 -> 0): rotation error 3.51e-2 rad -> 8.5e-5 rad, translation error 7.48e-2 -> 9.6e-5;
    15 evaluations, 9 accepted steps.  Asserted: nearer the truth than at the start in both, and the mean cost of the accepted evaluations
    falls strictly within each level (levels are different images, so their costs are not compared with each other)."""
    _, _, _, q_true, t_true = ac.driver_scene()
    res = ac.driver_reference()
    r0, t0 = ar.pose_error((1, 0, 0, 0), (0, 0, 0), q_true, t_true)
    r1, t1 = ar.pose_error(res["q"], res["t"], q_true, t_true)
    print("start", r0, t0, "end", r1, t1, "evaluations", len(res["trace"]), "iters", res["iters"])
    assert res["status"] == ar.OK and r1 < r0 and t1 < t0
    assert sum(res["iters"]) >= 3 and all(res["iters"][l] >= 1 for l in (0, 1, 2))
    for level in (2, 1, 0):
        costs = [e["sums"][27] / e["n_used"] for e in res["trace"] if e["level"] == level and e["accepted"]]
        assert len(costs) >= 2 and all(b < a for a, b in zip(costs, costs[1:])), (level, costs)
    assert res["trace"][0]["level"] == 2 and not res["trace"][0]["delta"].any()


def test_checker_loop_ends_with_too_few_on_an_empty_map():
    ref, new, d, _, _ = ac.driver_scene()
    rp, npyr = ar.build_pyramid(ref, 3), ar.build_pyramid(new, 3)
    res = ar.align_frame(rp, npyr, np.full_like(d, np.nan), ac.DRIVER_K, (1, 0, 0, 0), (0.1, 0, 0), **ac.DRIVER_PARAMS)
    assert res["status"] == ar.TOO_FEW and len(res["trace"]) == 1 and res["trace"][0]["n_used"] == 0
    assert res["q"].tolist() == [1, 0, 0, 0] and res["t"].tolist() == [0.1, 0, 0]
    assert (res["trace"][0]["sums"].view(np.uint64) == 0).all()  # +0.0, every one


def test_exp_left_small_and_large_angles_agree_and_compose():
    q, t = ac.small_pose()
    for scale in (1e-6, 0.9e-5, 1.1e-5, 1e-3, 0.3):  # both sides of theta^2 = 1e-10
        d = scale * np.array([0.3, -0.2, 0.5, 0.6, -0.7, 0.2])
        q1, t1 = ar.exp_left(d, q, t)
        qh, th = ar.exp_left(0.5 * d, q, t)
        q2, t2 = ar.exp_left(0.5 * d, qh, th)  # exp(d/2) exp(d/2) = exp(d)
        assert np.allclose(q1, q2, atol=1e-13) and np.allclose(t1, t2, atol=1e-13) and abs(np.linalg.norm(q1) - 1) < 1e-15
        R = ar.quat_to_rot(q1).reshape(3, 3)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-14)
