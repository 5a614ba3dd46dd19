"""Frame::create level 0 on the device at tiny frames and wide borders: img_pad, gradx_pad and grady_pad of
flame_stereo_add_frame and flame_stereo_add_raw_frame against tests/frame_ref.py, a numpy checker that shares no index
arithmetic with k_frame_pad_gradient or with oracle/stereo_oracle.c.  No tolerance anywhere: every comparison is of bytes.

CPU: the checker's known answers by hand; what every case of tests/frame_cases.py is there to reach; the oracle's
stereo_make_frame pinned to the checker on 637 tiny frames (so that the rest of the suite, which checks the device against
the oracle, vouches for both).  GPU: frames from 2x2, borders wider than the frame (BORDER_REFLECT_101 reflects repeatedly),
padded widths at the edges of the 256-lane row blocks, the largest dimension; row strides through the C entry; the unpadded
view; buffers across cameras in one context; and k_input_rectify at outputs of 4 to 15 pixels, every store tail."""
import ctypes as C

import numpy as np
import pytest

from oracle import stereo_capi as so
from tests import frame_cases as fc
from tests import frame_ref as fr
from tests import input_ref as ir

gpu = pytest.mark.gpu
INVALID_ARG = -1
CASES = sorted(fc.FRAME_CASES)
MANY_CASES = [c for c in CASES if fc.FRAME_CASES[c][0] == fc.MANY]


# ---------------------------------------------------------------- CPU: the checker's known answers


def test_reflect_101_is_the_opencv_loop():
    # len 2: period 2, the source index is the parity of p
    assert [fr.reflect_101(p, 2)[0] for p in range(-5, 7)] == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0]
    # len 3: period 4: ... 2 1 0 1 2 1 0 1 2 ...
    assert [fr.reflect_101(p, 3)[0] for p in range(-5, 8)] == [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1]
    # len 4: period 6
    assert [fr.reflect_101(p, 4)[0] for p in range(-7, 11)] == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2]
    # the number of reflections: none inside, one up to a frame's length away, then one more per len - 1
    assert [fr.reflect_101(p, 4)[1] for p in range(-7, 11)] == [3, 2, 2, 2, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 3]
    assert fr.reflect_101(-64, 2) == (0, 64) and fr.reflect_101(65, 2) == (1, 64)


def test_checker_2x2_by_hand():
    img = np.array([[10, 20], [30, 40]], np.uint8)
    pad, gx, gy = fr.make_frame(img, 0)
    assert pad.tolist() == [[10, 20], [30, 40]]
    # width == 2: the first column is forward, the last backward, both the same whole difference; likewise the rows
    assert gx.tolist() == [[10, 10], [10, 10]] and gy.tolist() == [[20, 20], [20, 20]]
    pad, gx, gy = fr.make_frame(img, 1)
    assert pad.tolist() == [[40, 30, 40, 30], [20, 10, 20, 10], [40, 30, 40, 30], [20, 10, 20, 10]]
    assert gx.tolist() == [[0, 0, 0, 0], [0, 10, 10, 0], [0, 10, 10, 0], [0, 0, 0, 0]]
    assert gy.tolist() == [[0, 0, 0, 0], [0, 20, 20, 0], [0, 20, 20, 0], [0, 0, 0, 0]]
    # border 2, the first a single reflection gets wrong: the whole 6x6 plane is the image tiled
    pad, gx, gy = fr.make_frame(img, 2)
    assert pad.tolist() == [[10, 20, 10, 20, 10, 20],
                            [30, 40, 30, 40, 30, 40],
                            [10, 20, 10, 20, 10, 20],
                            [30, 40, 30, 40, 30, 40],
                            [10, 20, 10, 20, 10, 20],
                            [30, 40, 30, 40, 30, 40]]
    want_gx = np.zeros((6, 6), np.float32)
    want_gx[2:4, 2:4] = 10
    assert np.array_equal(gx, want_gx) and np.array_equal(gy, 2 * want_gx) and gx.dtype == np.float32
    # border 5 (odd): the parity flips, pad[y, x] = img[(y + 1) % 2, (x + 1) % 2]
    pad, gx, gy = fr.make_frame(img, 5)
    assert pad.shape == (12, 12) and all(pad[y, x] == img[(y + 1) % 2, (x + 1) % 2] for y in range(12) for x in range(12))
    assert np.count_nonzero(gx) == 4 and (gx[5:7, 5:7] == 10).all() and (gy[5:7, 5:7] == 20).all()


def test_checker_3x2_by_hand():
    img = np.array([[1, 5, 11], [100, 90, 70]], np.uint8)
    pad, gx, gy = fr.make_frame(img, 0)
    assert pad.tobytes() == img.tobytes()
    assert gx.tolist() == [[4, 5, 6], [-10, -15, -20]]  # forward, half of the central difference, backward
    assert gy.tolist() == [[99, 85, 59], [99, 85, 59]]  # height == 2: both rows the same one-sided difference
    pad, _, _ = fr.make_frame(img, 1)
    assert pad.tolist() == [[90, 100, 90, 70, 90], [5, 1, 5, 11, 5], [90, 100, 90, 70, 90], [5, 1, 5, 11, 5]]
    pad, gx, gy = fr.make_frame(img, 2)
    # columns: p = -2 .. 4 -> 2 1 0 1 2 1 0 (period 4); rows: p = -2 .. 3 -> 0 1 0 1 0 1 (period 2)
    top, bottom = [11, 5, 1, 5, 11, 5, 1], [70, 90, 100, 90, 70, 90, 100]
    assert pad.tolist() == [top, bottom, top, bottom, top, bottom]
    assert gx[2:4, 2:5].tolist() == [[4, 5, 6], [-10, -15, -20]] and np.count_nonzero(gx) == 6
    assert gy[2:4, 2:5].tolist() == [[99, 85, 59], [99, 85, 59]] and np.count_nonzero(gy) == 6
    pad, _, _ = fr.make_frame(img, 5)
    # columns: p = -5 .. 7 -> 1 0 1 2 1 0 1 2 1 0 1 2 1; rows: p = -5 .. 6 -> 1 0 1 0 ...
    cols = [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1]
    assert pad.shape == (12, 13) and pad.tolist() == [[int(img[(y + 1) % 2, c]) for c in cols] for y in range(12)]


@pytest.mark.parametrize("w,h,border", [(9, 6, 14), (6, 9, 20), (2, 5, 7), (35, 17, 64)])
def test_checker_ramp_padded_wider_than_the_frame(w, h, border):
    """img[y, x] = (7 x + 13 y) % 251 names its own pixel as long as no two pixels share a value (all but the 35x17 one): the
    source (sx, sy) of every padded pixel is recomputed from its value and is the one the OpenCV loop gives."""
    img = fr.ramp(w, h)
    pad, gx, gy = fr.make_frame(img, border)
    unique = len(set(img.reshape(-1).tolist())) == w * h
    assert unique == ((w, h) != (35, 17))
    where = {int(img[y, x]): (x, y) for y in range(h) for x in range(w)}
    for y in range(h + 2 * border):
        sy, _ = fr.reflect_101(y - border, h)
        for x in range(w + 2 * border):
            sx, _ = fr.reflect_101(x - border, w)
            if unique:
                assert where[int(pad[y, x])] == (sx, sy), (x, y)  # the source recomputed from the value
            assert int(pad[y, x]) == (7 * sx + 13 * sy) % 251
    # a pixel more than two frame lengths out, by hand: p = -14 on len 9 (period 16) -> 14 -> 2; p = 9 + 13 = 22 -> 6 -> 6
    if (w, border) == (9, 14):
        assert fr.reflect_101(-14, 9) == (2, 2) and fr.reflect_101(22, 9) == (6, 2)
        assert pad[border, 0] == 7 * 2 and pad[border, w + 2 * border - 1] == 7 * 6


def test_checker_ramp_gradients_at_the_rim_and_inside():
    w, h, b = 9, 6, 14  # no wrap of the ramp: 7 * 8 + 13 * 5 = 121 < 251
    _, gx, gy = fr.make_frame(fr.ramp(w, h), b)
    ix, iy = gx[b:b + h, b:b + w], gy[b:b + h, b:b + w]
    # the ramp's slope is (7, 13): central differences halve 14 and 26, the one-sided ones are the slope itself
    assert (ix == 7).all() and (iy == 13).all()
    assert np.count_nonzero(gx) == w * h and np.count_nonzero(gy) == w * h  # zeros everywhere outside
    # with a wrap the rim and the interior differ: 36 columns, 7 * 35 = 245, so row 1 (13 + 7 x) wraps at x = 34
    img = fr.ramp(36, 3)
    gx, gy = fr.central_gradient(img)
    assert img[1, 33] == 244 and img[1, 34] == 0 and img[1, 35] == 7
    assert gx[1, 33] == 0.5 * (0 - 237) and gx[1, 34] == 0.5 * (7 - 244) and gx[1, 35] == 7 - 0 and gx[1, 0] == 7
    assert gy[0, 34] == 0 - 238 and gy[1, 34] == 0.5 * (13 - 238) and gy[2, 34] == 13 - 0
    assert gx.dtype == np.float32 and gy.dtype == np.float32


@pytest.mark.parametrize("w,h", [(2, 2), (2, 7), (7, 2)])
def test_checker_two_wide_or_two_high(w, h):
    """width == 2: the first and the last column are both one-sided and the two differences are the same number."""
    img = fc.random_image(w, h, 3)
    gx, gy = fr.central_gradient(img)
    f = img.astype(np.int64)
    if w == 2:
        assert np.array_equal(gx[:, 0], gx[:, 1]) and np.array_equal(gx[:, 0], (f[:, 1] - f[:, 0]).astype(np.float32))
    if h == 2:
        assert np.array_equal(gy[0], gy[1]) and np.array_equal(gy[0], (f[1] - f[0]).astype(np.float32))
    if w > 2:
        assert np.array_equal(gx[:, 1:-1], ((f[:, 2:] - f[:, :-2]) / 2.0).astype(np.float32))
    if h > 2:
        assert np.array_equal(gy[1:-1], ((f[2:] - f[:-2]) / 2.0).astype(np.float32))


def test_checker_loop_and_np_pad_agree_and_would_notice():
    img = fc.random_image(5, 4, 1)
    for b in (0, 3, 4, 5, 9, 64):
        assert fr.padded_image(img, b).tobytes() == fr.padded_image_loop(img, b).tobytes()
    # numpy's other modes are not the rule: the assertion inside padded_image is not vacuous
    assert np.pad(img, 5, mode="symmetric").tobytes() != fr.padded_image_loop(img, 5).tobytes()
    big = fc.random_image(300, 250, 2)  # above LOOP_LIMIT: the per-axis index map stands in for the loop
    assert big.size + 1 > fr.LOOP_LIMIT and fr.padded_image(big, 5).shape == (260, 310)


# ---------------------------------------------------------------- CPU: the cases reach what they name


def test_the_case_tables_are_complete():
    assert len(CASES) == 20 and len(MANY_CASES) == 13
    assert [c for c in CASES if fc.FRAME_CASES[c][0] == fc.NONE] == [(2, 2, 0), (256, 2, 0), (257, 2, 0), (16384, 2, 0)]
    assert [c for c in CASES if fc.FRAME_CASES[c][0] == fc.ONE] == [(2, 2, 1), (2, 16384, 1), (65, 65, 64)]
    assert sorted(c[0] + 2 * c[2] for c in CASES if fc.FRAME_CASES[c][1] is not None) == [255, 256, 256, 257, 257]
    assert fc.RAW_TAILS == tuple((w * h) % 4 for w, h in fc.RAW_SIZES) and set(fc.RAW_TAILS) == {0, 1, 2, 3}
    assert [w * h for w, h in fc.RAW_SIZES] == [4, 6, 6, 9, 15, 14]
    assert len(fc.SWEEP_DIMS) ** 2 * len(fc.SWEEP_BORDERS) == 637


@pytest.mark.parametrize("case", CASES, ids=fc.case_id)
def test_case_reaches_what_it_names(case):
    fc.check_reaches(case)


@pytest.mark.parametrize("case", CASES, ids=fc.case_id)
def test_one_reflection_differs_exactly_where_two_are_needed(case):
    """The index arithmetic k_frame_pad_gradient had (one round of the rule), read on the CPU: in every case that needs two
    reflections or more it leaves an index outside the frame, so the plane would differ from the checker's (the device would
    have read outside its staging buffer: never run); in every other case it is the checker's index map."""
    w, h, b = case
    xs, ys = fc.check_reaches(case)
    old_x = np.array([fc.single_reflection(q - b, w) for q in range(w + 2 * b)])
    old_y = np.array([fc.single_reflection(q - b, h) for q in range(h + 2 * b)])
    same = np.array_equal(old_x, xs) and np.array_equal(old_y, ys)
    outside = old_x.min() < 0 or old_y.min() < 0 or old_x.max() >= w or old_y.max() >= h
    assert same == (case not in MANY_CASES) and outside == (case in MANY_CASES)


# ---------------------------------------------------------------- CPU: the oracle against the checker


@pytest.mark.parametrize("w", fc.SWEEP_DIMS)
def test_oracle_make_frame_equals_the_checker(w):
    """Every (w, h) in {2, 3, 4, 5, 7, 8, 33}^2 with every border in {0 .. 5, 7, 8, 9, 32, 33, 63, 64}: all three planes byte for
    byte.  The rest of the suite checks the device against the oracle; this makes the oracle answer to the checker."""
    n = 0
    for h in fc.SWEEP_DIMS:
        img = fc.random_image(w, h, 5)
        for b in fc.SWEEP_BORDERS:
            fr.assert_planes_equal(so.make_frame(img, b), fr.make_frame(img, b), "oracle %dx%d b%d" % (w, h, b))
            n += 1
    assert n == 7 * 13


def test_oracle_make_frame_equals_the_checker_on_the_ramp():
    for w, h, b in ((2, 2, 64), (4, 7, 9), (33, 32, 64), (65, 65, 64), (247, 3, 5)):
        fr.assert_planes_equal(so.make_frame(fr.ramp(w, h), b), fr.make_frame(fr.ramp(w, h), b), "oracle, ramp %dx%d b%d" % (w, h, b))


# ---------------------------------------------------------------- GPU: add_frame


def _camera(w, h):
    return ir.cam(float(w), float(w), 0.5 * (w - 1), 0.5 * (h - 1))


def _tracker(w, h, border):
    from flame_amd.stereo import FeatureTracker

    K, Kinv = _camera(w, h)
    return FeatureTracker(K, Kinv, w, h, border=border)


@gpu
@pytest.mark.parametrize("image", fc.IMAGES)
@pytest.mark.parametrize("case", CASES, ids=fc.case_id)
def test_gpu_add_frame_equals_the_checker(built, case, image):
    fc.check_reaches(case)
    w, h, b = case
    img, want = fc.frame_expected(case, image)
    with _tracker(w, h, b) as tr:
        tr.add_frame(4, img)
        fr.assert_planes_equal(tr.download_frame(4), want, "%s, %s" % (fc.case_id(case), image))
        assert tr.frame_count() == 1


def _c_add_frame(tr, frame_id, ptr, stride):
    return tr._L.flame_stereo_add_frame(tr._ctx, frame_id, C.c_void_p(ptr), stride)


@gpu
@pytest.mark.parametrize("extra", fc.STRIDE_EXTRA)
@pytest.mark.parametrize("case", fc.STRIDE_CASES, ids=fc.case_id)
def test_gpu_add_frame_strides_through_the_c_entry(built, case, extra):
    """The Python wrapper always passes a tight image; the C entry takes any stride of at least the width.  Pixels are below
    200 and the bytes behind each row are 255: a padding byte read as a pixel shows."""
    w, h, b = case
    buf, img = fc.strided_image(w, h, extra)
    assert buf.strides == (w + extra, 1) and img.max() < 200 and (extra == 0 or (buf[:, w:] == 255).all())
    want = fr.make_frame(img, b)
    assert want[0].max() < 200
    with _tracker(w, h, b) as tr:
        assert _c_add_frame(tr, 9, buf.ctypes.data, w + extra) == 0
        fr.assert_planes_equal(tr.download_frame(9), want, "%s, stride w + %d" % (fc.case_id(case), extra))


@gpu
@pytest.mark.parametrize("case", fc.STRIDE_CASES, ids=fc.case_id)
def test_gpu_add_frame_refuses_a_stride_below_the_width(built, case):
    w, h, b = case
    buf, img = fc.strided_image(w, h, 0)
    want = fr.make_frame(img, b)
    with _tracker(w, h, b) as tr:
        tr.add_frame(1, img)
        for frame_id in (1, 2):  # an existing id and a new one
            assert _c_add_frame(tr, frame_id, buf.ctypes.data, w - 1) == INVALID_ARG
            assert tr.frame_count() == 1
            fr.assert_planes_equal(tr.download_frame(1), want, "after the refused stride")


@gpu
@pytest.mark.parametrize("case", [(5, 4, 5), (64, 64, 64)], ids=fc.case_id)
def test_gpu_frame_image_device_is_the_image_that_was_added(built, case):
    from tests import metric_helpers as mh

    w, h, b = case
    img, want = fc.frame_expected(case, "random")
    with _tracker(w, h, b) as tr:
        tr.add_frame(3, img)
        ptr, step = tr.frame_image_device(3)
        assert ptr and step == w + 2 * b
        rows = np.stack([mh.fetch(ptr + y * step, (w,), np.uint8) for y in range(h)])
        assert rows.tobytes() == img.tobytes()
        fr.assert_planes_equal(tr.download_frame(3), want, fc.case_id(case))


@gpu
def test_gpu_buffers_across_cameras_in_one_context(built):
    """320x240 b5: six frames added and dropped (the spare list fills and the rest is freed); 4x7 b9: another padded size and the
    repeated reflection; back to 320x240 b5.  Every resident frame is compared after every step."""
    big, small = (320, 240, 5), (4, 7, 9)
    resident = {}

    def image(case, k):
        return fc.random_image(case[0], case[1], 40 + k)

    def check(tr, case, what):
        assert tr.frame_count() == len(resident), what
        for frame_id, img in sorted(resident.items()):
            fr.assert_planes_equal(tr.download_frame(frame_id), fr.make_frame(img, case[2]), "%s, frame %d" % (what, frame_id))

    with _tracker(*big) as tr:
        for k in range(6):
            resident[k] = image(big, k)
            tr.add_frame(k, resident[k])
            check(tr, big, "big, added %d" % k)
        for k in range(6):
            tr.drop_frame(k)
            del resident[k]
            check(tr, big, "big, dropped %d" % k)
        K, Kinv = _camera(small[0], small[1])
        tr.set_camera(K, Kinv, small[0], small[1], border=small[2])
        assert tr.frame_count() == 0
        for k in (10, 11):
            resident[k] = image(small, k)
            tr.add_frame(k, resident[k])
            check(tr, small, "small, added %d" % k)
        # an existing id with other content: replaced, and no frame more
        resident[10] = image(small, 12)
        assert resident[10].tobytes() != image(small, 10).tobytes()
        tr.add_frame(10, resident[10])
        check(tr, small, "small, replaced 10")
        resident.clear()
        K, Kinv = _camera(big[0], big[1])
        tr.set_camera(K, Kinv, big[0], big[1], border=big[2])
        assert tr.frame_count() == 0
        for k in (20, 21):
            resident[k] = image(big, k)
            tr.add_frame(k, resident[k])
            check(tr, big, "big again, added %d" % k)
        resident[21] = image(big, 22)
        tr.add_frame(21, resident[21])
        check(tr, big, "big again, replaced 21")
        assert tr.frame_count() == 2


# ---------------------------------------------------------------- GPU: the rectifier at widths and tails it has never run


def _raw_case(tr, size, border, fmt, pad, source):
    """add_raw_frame of one case into a tracker of (size, border); the expectation chains input_ref.rectify and frame_ref."""
    w, h = size
    raw, grey, n_outside, K, Kinv, p = fc.raw_expected(w, h, fmt, pad, source)
    assert raw.strides[0] == p["raw_width"] * ir.BYTES[fmt] + pad
    tr.set_input(format=fmt, **p)
    what = "%dx%d b%d format %d pad %d from %s" % (w, h, border, fmt, pad, source)
    assert tr.add_raw_frame(6, raw) == dict(n_outside=n_outside), what
    fr.assert_planes_equal(tr.download_frame(6), fr.make_frame(grey, border), what)
    assert tr.frame_count() == 1


@gpu
@pytest.mark.parametrize("size", fc.RAW_SIZES, ids=lambda s: "%dx%d" % s)
def test_gpu_raw_frame_remap_0_at_tiny_outputs(built, size):
    """Outputs of 4 to 15 pixels: one thread owns four pixels of up to three rows; store tails 0, 2, 2, 1, 3, 2 (2x2: a single
    full dword and nothing else).  All five formats with a stride of raw_width * bytes + 5; BGRA8 and RGBA8 also tight, which
    reads the taps as dwords.  Border 0, and one of at least the width."""
    w, h = size
    assert (w * h) % 4 == fc.RAW_TAILS[fc.RAW_SIZES.index(size)]
    for border in fc.raw_borders(w, h):
        assert border == 0 or border >= w
        with _tracker(w, h, border) as tr:
            for fmt in (ir.GREY8, ir.BGR8, ir.RGB8, ir.BGRA8, ir.RGBA8):
                _raw_case(tr, size, border, fmt, 5, None)
            for fmt in (ir.BGRA8, ir.RGBA8):
                _raw_case(tr, size, border, fmt, 0, None)


@gpu
@pytest.mark.parametrize("source", fc.RAW_SOURCES, ids=lambda s: "from_%dx%d" % s)
@pytest.mark.parametrize("size", fc.RAW_SIZES, ids=lambda s: "%dx%d" % s)
def test_gpu_raw_frame_remap_1_at_tiny_outputs(built, size, source):
    """The same outputs through the map, from a raw frame of 2x2 (every inside pixel has x0 = y0 = 0) and of 4x3, with a small
    radial distortion, as GREY8 and as tight BGRA8; every case has inside and outside pixels (tests/frame_cases.raw_expected
    asserts it on the checker's output)."""
    w, h = size
    for border in fc.raw_borders(w, h):
        with _tracker(w, h, border) as tr:
            for fmt in (ir.GREY8, ir.BGRA8):
                _, _, n_outside, _, _, _ = fc.raw_expected(w, h, fmt, 0, source)
                assert 0 < n_outside < w * h
                _raw_case(tr, size, border, fmt, 0, source)


@pytest.mark.parametrize("source", fc.RAW_SOURCES, ids=lambda s: "from_%dx%d" % s)
@pytest.mark.parametrize("size", fc.RAW_SIZES, ids=lambda s: "%dx%d" % s)
def test_raw_cases_have_inside_and_outside_pixels(size, source):
    """CPU: what the remapped cases promise, on the checker's output."""
    w, h = size
    for fmt in (ir.GREY8, ir.BGRA8):
        raw, grey, n_outside, K, Kinv, p = fc.raw_expected(w, h, fmt, 0, source)
        xs, ys, inside = ir.source_map(p["K_raw"], p["dist"], Kinv, w, h, *source)
        assert 0 < n_outside < w * h and n_outside == int((~inside).sum())
        assert (grey[~inside] == 0).all()
        if source == (2, 2):
            assert (xs[inside].astype(np.int32) == 0).all() and (ys[inside].astype(np.int32) == 0).all()
        else:
            assert xs[inside].astype(np.int32).max() >= 1 or ys[inside].astype(np.int32).max() >= 1
