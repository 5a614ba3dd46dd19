"""flame_stereo_draw_matches (getDebugImageMatches) on the GPU, through the Python surface: every byte of the picture and every counter
against the sequential checker tests/matches_ref.py, no tolerance and no pixel left out.  The cases and the checker's results come from
tests/test_matches.py, which also asserts that together they draw every kind."""
import numpy as np
import pytest

from tests import matches_ref as mr
from tests.test_matches import KIND_CASES, KIND_CASES_640, case, reference, run_checker

pytestmark = pytest.mark.gpu

INVALID_ARG, ERR_ASSERT = -1, -8
STAT_NAMES = ("num_idepth_updates", "num_fail_max_var", "num_fail_max_dropouts", "num_fail_ref_patch_grad",
              "num_fail_ambiguous_match", "num_fail_max_cost", "success")


def _tracker(c):
    from flame_amd.stereo import FeatureTracker

    tr = FeatureTracker(c["K"], c["Kinv"], c["width"], c["height"], border=c["pad"])
    for fid, img in c["imgs"].items():
        tr.add_frame(fid, img)
    return tr


def _update(tr, c, feats, entry="host", wait=True, raise_on_error=True):
    """One update through one of the three entry points -> (rc, stats or None, the records afterwards)."""
    from flame_amd.stereo import FEATURE_DTYPE, StereoParams

    P = StereoParams(**c["pkw"])
    f = feats.copy().view(FEATURE_DTYPE)
    if entry == "host":
        rc, st = tr.update_feature_idepths(P, c["new"], c["curr_pf"], c["poses"], f, raise_on_error=raise_on_error)
        return rc, st, f
    if entry == "resident":
        tr.set_features(f)
        rc, st = tr.update_resident(P, c["new"], c["curr_pf"], c["poses"], wait=wait, raise_on_error=raise_on_error)
        return rc, st, None  # (read back by the caller, after the picture: get_features waits for the stream)
    import torch

    dev = torch.from_numpy(f.view(np.uint8).reshape(-1, 40).copy()).cuda()
    torch.cuda.synchronize()
    st = tr.update_feature_idepths_device(P, c["new"], c["curr_pf"], c["poses"], f.shape[0], dev.data_ptr(), wait=wait)
    return 0, st, dev


def _run(c, feats=None, entry="host", lanes=0, record=True, wait=True, flip=False):
    feats = c["feats"] if feats is None else feats
    tr = _tracker(c)
    try:
        if lanes:
            tr.set_lanes_per_feature(lanes)
        tr.set_record_matches(record)
        rc, st, out = _update(tr, c, feats, entry, wait)
        assert rc == 0
        pic = tr.draw_matches(flip=flip) if record else None
        if entry == "resident":
            out = tr.get_features()
        elif entry == "device":
            import torch

            torch.cuda.synchronize()
            out = out.cpu().numpy().reshape(-1).view(feats.dtype)
        ms = tr.last_kernel_ms()
    finally:
        tr.close()
    if record:
        assert ms > 0
    return st, out, pic


def _same(pic, ref, st=None, out=None, refilled=0):
    """Every byte, every counter; the records and statistics of the update; the invariants between the two sets of counters."""
    assert pic["num_features"] == ref["feats"].shape[0]
    for k in ("kind_count", "lines_drawn", "lines_skipped", "rings_skipped", "entries"):
        assert pic[k] == ref[k], (k, pic[k], ref[k])
    assert pic["refilled"] == refilled
    if not np.array_equal(pic["img"], ref["img"]):
        bad = np.argwhere(np.any(pic["img"] != ref["img"], axis=2))
        y, x = bad[0]
        raise AssertionError("%d pixels differ, first (x %d, y %d): gpu %r checker %r" % (len(bad), x, y, pic["img"][y, x], ref["img"][y, x]))
    if out is not None:
        assert out.tobytes() == ref["feats"].tobytes()
    if st is not None:
        assert [st[n] for n in STAT_NAMES] == [int(v) for v in ref["stats"]]
    else:  # an enqueue-only update reports nothing: the checker's statistics of the same update stand in
        st = dict(zip(STAT_NAMES, (int(v) for v in ref["stats"])))
    assert pic["kind_count"][mr.GREEN] + ref["green_skipped"] == st["num_fail_max_var"]
    assert pic["kind_count"][mr.BLUE] + ref["blue_skipped"] == st["num_fail_max_dropouts"]


@pytest.mark.parametrize("name", KIND_CASES + KIND_CASES_640)
def test_every_kind_of_draw(built, name):
    """Brown, magenta, black, cyan, white, red, yellow, the blended segment and both rings: at 320x240 (r1 = 1, r2 = 4) and at
    640x480 (r1 = 2, r2 = 8)."""
    st, out, pic = _run(case(name))
    _same(pic, reference(name), st, out)
    assert sum(pic["kind_count"]) > 0


@pytest.mark.parametrize("reverse", [False, True])
def test_draw_order(built, reverse):
    """Segments over later rectangles, rectangles under later segments, segments of two colours on one pixel (tests/test_matches.py
    asserts that the two pictures differ)."""
    c = case("order")
    st, out, pic = _run(c, feats=c["feats"][::-1].copy() if reverse else None)
    _same(pic, reference("order", reverse), st, out)


@pytest.mark.parametrize("name", ["order", "scene"])
def test_lanes_per_feature_and_option_off(built, name):
    c, ref = case(name), reference(name)
    st0, out0, _ = _run(c, record=False)
    for lanes in (16, 1):
        st, out, pic = _run(c, lanes=lanes)
        _same(pic, ref, st, out)
        assert st == st0 and out.tobytes() == out0.tobytes(), "recording changed what the update computes"
        st_off, out_off, _ = _run(c, lanes=lanes, record=False)
        assert st_off == st0 and out_off.tobytes() == out0.tobytes()


def test_clipping_at_every_edge_and_corner(built):
    st, out, pic = _run(case("clip"))
    _same(pic, reference("clip"), st, out)


def test_single_pixel_radii(built):
    """160x120: r1 = r2 = 0."""
    st, out, pic = _run(case("small"))
    _same(pic, reference("small"), st, out)
    assert pic["kind_count"][mr.GREEN] > 0 and pic["kind_count"][mr.BLUE] > 0


def test_wide_image_radii(built):
    """1280 columns: r1 = 4, r2 = 16, radii no other case has."""
    st, out, pic = _run(case("wide"))
    _same(pic, reference("wide"), st, out)
    assert pic["kind_count"][mr.GREEN] > 0 and pic["kind_count"][mr.BLUE] > 0


def test_flip(built):
    c = case("textureless")
    ref = dict(reference("textureless"))
    ref["img"] = run_checker(c, flip=True)["img"]
    assert np.array_equal(ref["img"].reshape(-1, 3), reference("textureless")["img"].reshape(-1, 3)[::-1])
    st, out, pic = _run(c, flip=True)
    _same(pic, ref, st, out)


@pytest.mark.parametrize("entry", ["host", "resident", "device"])
def test_all_three_update_entry_points(built, entry):
    st, out, pic = _run(case("variants"), entry=entry)
    _same(pic, reference("variants"), st, out)


@pytest.mark.parametrize("entry", ["resident", "device"])
def test_enqueue_only_update_then_draw(built, entry):
    """stats = NULL: the update is only enqueued; draw_matches is ordered behind it on the context's stream."""
    st, out, pic = _run(case("textureless"), entry=entry, wait=False)
    assert st is None
    _same(pic, reference("textureless"), None, out)


@pytest.mark.parametrize("name", ["empty", "success"])
def test_empty_pictures(built, name):
    """No features, and a frame where every feature succeeds: the grey image, every counter 0."""
    c = case(name)
    st, out, pic = _run(c)
    _same(pic, reference(name), st, out)
    assert pic["kind_count"] == [0] * 9 and pic["lines_drawn"] == pic["lines_skipped"] == pic["rings_skipped"] == pic["entries"] == 0
    assert np.array_equal(pic["img"], np.repeat(c["imgs"][c["new"]][:, :, None], 3, axis=2))
    assert st["num_idepth_updates"] == c["feats"].shape[0]


def test_entry_buffer_overflow(built):
    """More entries than 2 * rows * cols: a fresh context grows the buffer and repeats fill and fold; the next call does not."""
    c, ref = case("overflow"), reference("overflow")
    assert ref["entries"] > 2 * c["width"] * c["height"]
    tr = _tracker(c)
    try:
        tr.set_record_matches(True)
        rc, st, out = _update(tr, c, c["feats"])
        _same(tr.draw_matches(), ref, st, out, refilled=1)
        _same(tr.draw_matches(), ref, st, out, refilled=0)
        rc, st, out = _update(tr, c, c["feats"])
        _same(tr.draw_matches(), ref, st, out, refilled=0)
    finally:
        tr.close()


def test_errors(built):
    from flame_amd import NLTGV2Error
    from flame_amd.stereo import OPT_RECORD_MATCHES

    c = case("scene")
    tr = _tracker(c)
    try:
        assert tr.draw_matches(raise_on_error=False) == (INVALID_ARG, None)      # option off, no update
        _update(tr, c, c["feats"])
        assert tr.draw_matches(raise_on_error=False) == (INVALID_ARG, None)      # option off
        tr.set_record_matches(True)
        assert tr.draw_matches(raise_on_error=False) == (INVALID_ARG, None)      # no update since the option went on
        with pytest.raises(NLTGV2Error) as ei:
            tr._chk(tr._L.flame_stereo_set_option(tr._ctx, OPT_RECORD_MATCHES, 2), "set_option")
        assert ei.value.status == INVALID_ARG
        rc, st, out = _update(tr, c, c["feats"])
        _same(tr.draw_matches(), reference("scene"), st, out)
        bad = c["feats"].copy()
        bad["idepth_mu"][5] = -0.5                                                # FLAME_ASSERT(idepth >= 0)
        rc, st, _ = _update(tr, c, bad, raise_on_error=False)
        assert rc == ERR_ASSERT and st["error_feature"] == 5
        assert tr.draw_matches(raise_on_error=False) == (INVALID_ARG, None)      # the last update returned an error
        for entry in ("resident", "device"):                                      # ... also when nobody has read its status yet
            rc, st, _ = _update(tr, c, bad, entry=entry, wait=False)
            assert tr.draw_matches(raise_on_error=False) == (INVALID_ARG, None)
        rc, st, out = _update(tr, c, c["feats"])
        tr.set_record_matches(False)
        assert tr.draw_matches(raise_on_error=False) == (INVALID_ARG, None)      # switched off: the records do not stand
        tr.set_record_matches(True)
        assert tr.draw_matches(raise_on_error=False) == (INVALID_ARG, None)
        rc, st, out = _update(tr, c, c["feats"])
        tr.drop_frame(c["new"])
        assert tr.draw_matches(raise_on_error=False) == (INVALID_ARG, None)      # the new frame is no longer resident
        with pytest.raises(NLTGV2Error):                                          # an update that names it fails before it runs ...
            _update(tr, c, c["feats"])
        tr.add_frame(c["new"], c["imgs"][c["new"]])
        assert tr.draw_matches(raise_on_error=False) == (INVALID_ARG, None)      # ... and the records of the one before do not stand
        rc, st, out = _update(tr, c, c["feats"])
        tr.drop_frame(c["new"])
        tr.add_frame(c["new"], c["imgs"][c["new"]])
        _same(tr.draw_matches(), reference("scene"), st, out)
    finally:
        tr.close()
