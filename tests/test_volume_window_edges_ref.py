"""The window's shift past one grid and at its extremes, on the CPU alone: the preconditions of every case of
tests/test_gpu_volume_window_edges.py (tests/volume_window_cases.py, check_big), the shift stated by hand against the checker
tests/volume_window_ref.py bit for bit, and the algebra of two shifts on the checker, so that a failure on the device points at the device.
No GPU here."""
import numpy as np
import pytest

from tests import volume_ref as vr
from tests import volume_window_cases as wc

F = np.float32


def same(a, b):
    return np.array_equal(vr.bits(a), vr.bits(b))


@pytest.mark.parametrize("name", list(wc.BIG_SHIFTS))
def test_the_shifts_past_one_grid_meet_their_preconditions(name):
    walk = wc.check_big(name)
    # the table's arithmetic, once more from the dimensions alone
    p, per = wc.BIG_SHIFTS[name]["params"], wc.units_of(wc.BIG_SHIFTS[name])[3]
    n = p["nx"] * p["ny"] * p["nz"] // per
    assert walk["rounds"] == -(-n // (wc.MAX_GRID * wc.BLOCK)) >= 2 and 8 * n * per <= 8_800_000


def test_the_cases_are_the_ones_they_are_meant_to_be():
    assert list(wc.BIG_SHIFTS) == ["131x65x62", "101x89x97", "258x47x90", "258x47x90 odd", "1024x3x180", "1024x1x540", "258x47x90 zero"]
    assert 0 < wc.BIG_SHIFTS["131x65x62"]["tail"] < 64  # the last workgroup ends inside its first wave
    # the two paths over the same bytes, and the count alone
    assert [wc.BIG_SHIFTS[k]["record_bytes"] for k in ("258x47x90", "258x47x90 odd", "258x47x90 zero")] == [16, 8, 0]
    assert wc.rounds_and_carries(wc.BIG_SHIFTS["1024x1x540"])["step"] == (0, 0, 512)
    assert wc.rounds_and_carries(wc.BIG_SHIFTS["1024x3x180"])["step"] == (0, 2, 170)
    # 67x63x63 would be no test of the walk: the row carry never fires, alone or with the column carry
    walk = wc.rounds_and_carries(dict(params=dict(vr.SCENE, nx=67, ny=63, nz=63), shift=(3, -2, 1)))
    assert (walk["rounds"], walk["none"] + walk["column"], walk["row"], walk["both"], walk["row_by_column"]) == (2, 3779, 0, 0, 0)
    # the extremes: per volume and axis +-(n - 1), +-n, +-(n + 1), +-(n + 1001), alone and beside small steps along the other axes
    assert len(wc.EXTREMES) == 2 * 3 * 4 * 2 * 2 + 1 == len(set(wc.EXTREMES))
    assert {("16x12x10", (17, 0, 0)), ("16x12x10", (-17, 1, 0)), ("16x12x10", (0, 12, 0)), ("16x12x10", (0, 0, -10))} <= set(wc.EXTREMES)
    for name, s in wc.EXTREMES:
        p = wc.SMALL[name]
        dims = (p["nx"], p["ny"], p["nz"])
        assert sum(1 for a in range(3) if abs(s[a]) >= dims[a] - 1) == 1
    # the clamp changes the parity of s.x and with it the path
    assert wc.record_bytes((16, 12, 10), (17, 0, 0)) == 16 and wc.record_bytes((16, 12, 10), (15, 0, 0)) == 8
    assert wc.record_bytes((16, 12, 10), (-17, 1, 0)) == 16 and wc.record_bytes((16, 12, 10), (-15, 1, 0)) == 8
    assert wc.record_bytes((16, 12, 10), (1017, 0, 0)) == 16 and wc.record_bytes((15, 7, 5), (16, 0, 0)) == 8
    assert wc.record_bytes((16, 12, 10), (0, 0, 0)) == 0


def against_the_checker(params, content, s, what):
    v = wc.volume_of(params, content)
    hand = wc.by_hand(v, s)
    want = v.shift(s)
    assert hand[2] == want, (what, hand[2], want)
    wc.assert_same_as_by_hand(v, hand, what)
    n = params["nx"] * params["ny"] * params["nz"]
    assert want["kept"] + want["entered"] == n and want["kept_seen"] + want["lost_seen"] == np.count_nonzero(content[1] > 0)
    return v, want


@pytest.mark.parametrize("name", list(wc.BIG_SHIFTS))
def test_the_shift_by_hand_is_the_checkers_past_one_grid(name):
    case = wc.BIG_SHIFTS[name]
    content = wc.random_content(name)
    v, want = against_the_checker(case["params"], content, case["shift"], name)
    assert (want["entered"] > 0) == any(case["shift"]) and want["kept_seen"] > 0
    # and back: the second shift of the device test
    back = tuple(-c for c in case["shift"])
    hand = wc.by_hand(v, back)
    assert hand[2] == v.shift(back)
    wc.assert_same_as_by_hand(v, hand, name + " and back")
    wc.assert_back_again(v, content, case["shift"], name + " and back")
    assert v.base.tolist() == [0, 0, 0]


def test_the_shift_by_hand_is_the_checkers_at_the_extremes():
    nothing_kept = 0
    for name, s in wc.EXTREMES:
        p = wc.SMALL[name]
        v, want = against_the_checker(p, wc.random_content(name), s, "%s %s" % (name, s))
        assert v.base.tolist() == list(s)  # the base takes the shift unclamped
        dims = (p["nx"], p["ny"], p["nz"])
        assert (want["kept"] == 0) == any(abs(s[a]) >= dims[a] for a in range(3))
        nothing_kept += want["kept"] == 0
        if want["kept"]:
            assert 0 < want["kept"] <= dims[0] * dims[1] * dims[2] // min(dims)  # one plane, or less beside the small steps
    assert nothing_kept == 2 * 3 * 3 * 2 * 2 + 1


PAIRS = [((3, -2, 1), (-1, 4, 2)), ((5, 0, 0), (-5, 0, 0)), ((-4, 1, 0), (2, -3, 1)), ((15, 0, 0), (-14, 0, 0)), ((0, 6, -4), (0, -6, 4)),
         ((14, 0, 0), (-14, 3, 0)), ((2, 2, 2), (0, 0, 0)), ((9, 0, 0), (9, 0, 0))]


@pytest.mark.parametrize("name", list(wc.SMALL))
def test_two_shifts_are_their_sum_on_the_box_kept_by_both(name):
    p = wc.SMALL[name]
    dims = np.array([p["nx"], p["ny"], p["nz"]])
    content = wc.random_content(name)
    fresh_t, fresh_w = vr.bits(np.ones(1, F))[0], vr.bits(np.zeros(1, F))[0]
    k, j, i = np.indices(content[0].shape)
    d = np.stack([i, j, k], axis=-1)
    boxes = []
    for a, b in PAIRS:
        a, b = np.array(a), np.array(b)
        two, one = wc.volume_of(p, content), wc.volume_of(p, content)
        two.shift(a), two.shift(b)
        one.shift(a + b)
        assert two.base.tolist() == one.base.tolist() == (a + b).tolist()
        # destination d of the pair holds source d + b of the first shift's result, which held source d + b + a of the content
        both = np.all((d + b >= 0) & (d + b < dims) & (d + a + b >= 0) & (d + a + b < dims), axis=-1)
        boxes.append(int(np.count_nonzero(both)))
        for x, y, fresh in ((two.tsdf, one.tsdf, fresh_t), (two.weight, one.weight, fresh_w)):
            assert np.array_equal(vr.bits(x)[both], vr.bits(y)[both]), (a, b)
            assert np.all(vr.bits(x)[~both] == fresh), (a, b)
    # (9 + 9 keeps nothing on either volume's x; a zero second shift keeps the first one's box)
    assert min(boxes) == 0 and sum(b > 0 for b in boxes) >= 6 and max(boxes) < content[0].size


@pytest.mark.parametrize("name", list(wc.SMALL))
def test_a_shift_and_its_inverse_restore_the_kept_box(name):
    p = wc.SMALL[name]
    content = wc.random_content(name)
    for s in [(3, -2, 1), (2, 0, 0), (-1, 0, 0), (0, 0, 4), (p["nx"] - 1, 0, 0), (0, -(p["ny"] - 1), 1), (p["nx"], 0, 0), (0, 0, -(p["nz"] + 1001))]:
        v = wc.volume_of(p, content)
        v.shift(s), v.shift(tuple(-c for c in s))
        assert v.base.tolist() == [0, 0, 0]
        wc.assert_back_again(v, content, s, "%s %s and back" % (name, s))
        boxes = wc.kept_boxes((p["nx"], p["ny"], p["nz"]), s)
        if boxes is None:
            assert same(v.tsdf, np.ones_like(v.tsdf)) and not v.weight.view(np.uint32).any()
        else:
            assert same(v.tsdf[boxes[1]], content[0][boxes[1]]) and same(v.weight[boxes[1]], content[1][boxes[1]])
