"""flame_nltgv2_map_error_begin / _end through the C-ABI against the checker tests/map_error_ref.py, bit for bit: the error image as
uint32, the histogram and the ranks equal, the sum equal as a double, the picture's bytes.  Every case hands its map in through
map_device, so the shapes are free: tiny images around the border and a wave, validity patterns, a projection that leaves the image,
windows that straddle the tile's edges (the box kernel's tile is 64 x 16 outputs), the true-map source with its special values, one
bin under contention, the outputs one by one, and every error before anything is enqueued."""
import ctypes as C

import numpy as np
import pytest

from flame_amd import synth
from tests import map_error_ref as er
from tests.metric_helpers import fetch, on_device

F = np.float32
NAN, INF = F(np.nan), F(np.inf)
B = 3  # the border of the PHOTO cases
IDENTITY = (np.eye(3, dtype=F), np.zeros(3, F))
# cx = x + 1.5 + 2 * idepth, cy = y - 0.75 + idepth: a parallax of a few pixels
PARALLAX = (np.array([[1, 0, 1.5], [0, 1, -0.75], [0, 0, 1]], F), np.array([2.0, 1.0, 0.0], F))
# a shear: the projection leaves the comparison frame along a diagonal
SHEAR = (np.array([[1, 0.6, -20], [0.3, 1, -12], [0, 0, 1]], F), np.array([3.0, -2.0, 0.0], F))


@pytest.fixture(scope="module")
def gpu(built):
    import torch  # noqa: F401

    import flame_amd

    assert hasattr(flame_amd.load_library(), "flame_nltgv2_map_error_begin")
    return flame_amd


@pytest.fixture(scope="module")
def reg(gpu):
    with gpu.Regularizer(0) as r:
        r.upload_graph(synth.make_graph("320x240", seed=9))
        yield r


def images(shape, seed, step=None):
    """Two u8 images; with `step`, views of wider buffers (rows of `step` bytes)."""
    rng = np.random.default_rng(seed)
    rows, cols = shape
    step = cols if step is None else step
    bufs = [rng.integers(0, 256, (rows, step), dtype=np.uint8) for _ in range(2)]
    return bufs[0][:, :cols], bufs[1][:, :cols]


def random_map(shape, seed, p_nan=0.0, lo=0.05, hi=2.0):
    rng = np.random.default_rng(seed)
    v = rng.uniform(lo, hi, shape).astype(F)
    if p_nan:
        v[rng.random(shape) < p_nan] = NAN
    return v


def pow2_map(shape, seed, p_nan=0.0):
    """Inverse depths that are powers of two: x * depth and * (1 / depth) are exact, so the identity geometry projects every pixel onto
    itself exactly (an arbitrary depth may land a pixel of the band's first column one ulp outside it)."""
    rng = np.random.default_rng(seed)
    v = np.array([0.25, 0.5, 1.0, 2.0], F)[rng.integers(0, 4, shape)]
    if p_nan:
        v[rng.random(shape) < p_nan] = NAN
    return v


def photo_case(gpu, reg, v, ref, cmp, geo, what, border=B, **kw):
    rows, cols = v.shape
    keep = [on_device(v), on_device(ref.base if ref.base is not None else ref), on_device(cmp.base if cmp.base is not None else cmp)]
    p = gpu.MapErrorParams(source=gpu.MAP_ERROR_PHOTO, KRKinv=geo[0], Kt=geo[1], border=border, map_device=keep[0].data_ptr(),
                           ref_device=keep[1].data_ptr(), cmp_device=keep[2].data_ptr(), image_step_bytes=ref.strides[0], **kw)
    got = reg.map_error(p, rows, cols)
    ref_kw = {k: kw[k] for k in ("win_size", "hist_scale", "ptile_num", "ptile_den", "max_error", "flip", "want_image") if k in kw}
    want = er.map_error(v, er.PHOTO, geo[0], geo[1], ref, cmp, border, **ref_kw)
    er.assert_same(got, want, what)
    assert got["win_size"] == want["win_size"] and got["hist_scale"] == want["hist_scale"], what
    return got, want


def truth_case(gpu, reg, v, t, what, device_truth=False, gray=None, **kw):
    rows, cols = v.shape
    keep = [on_device(v)]
    if device_truth:
        keep.append(on_device(t))
        src = dict(truth_device=keep[1].data_ptr())
    else:
        src = dict(truth=t)
    p = gpu.MapErrorParams(source=gpu.MAP_ERROR_TRUTH, map_device=keep[0].data_ptr(), gray=gray, **src, **kw)
    got = reg.map_error(p, rows, cols)
    ref_kw = {k: kw[k] for k in ("relative", "win_size", "hist_scale", "ptile_num", "ptile_den", "max_error", "flip", "want_image") if k in kw}
    want = er.map_error(v, er.TRUTH, truth=t, gray=gray, **ref_kw)
    er.assert_same(got, want, what)
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2 * B + 1, 2 * B + 1), (2 * B + 1, 2 * B + 63), (2 * B + 1, 2 * B + 64), (2 * B + 1, 2 * B + 65),
                                   (2 * B + 3, 2 * B + 70), (37, 29)])
def test_gpu_tiny_photo_images_around_the_border_and_a_wave(gpu, reg, shape):
    ref, cmp = images(shape, 10 * shape[0] + shape[1])
    v = random_map(shape, shape[1])
    # the identity: every pixel of the band projects onto itself, so the band is exactly what is valid
    got, _ = photo_case(gpu, reg, pow2_map(shape, 3), ref, cmp, IDENTITY, f"{shape} identity", win_size=1)
    band = (shape[0] - 2 * B) * (shape[1] - 2 * B)
    assert got["n_valid"] == band  # (one pixel at (7, 7))
    assert np.array_equal(~np.isnan(got["error_map"][B:shape[0] - B, B:shape[1] - B]), np.ones((shape[0] - 2 * B, shape[1] - 2 * B), bool))
    for win in (0, 11):  # 0: 5 here, cols < 640; 11: wider than the valid band of every shape here but (37, 29), whose band it fills a third of
        got, want = photo_case(gpu, reg, v, ref, cmp, PARALLAX, f"{shape} parallax win {win}", win_size=win)
        assert got["win_size"] == (5 if win == 0 else 11)
        if shape[1] > 2 * B + 6:
            assert 0 < got["n_valid"] < band, (shape, got["n_valid"])
    # an image inside a wider buffer: rows of step bytes
    ref, cmp = images(shape, 7, step=shape[1] + 13)
    photo_case(gpu, reg, v, ref, cmp, PARALLAX, f"{shape} step {shape[1] + 13}", win_size=3)


def validity_patterns(shape, seed):
    """Maps for the PHOTO source with the identity geometry, where the band [B, size - B) is what can be valid."""
    rows, cols = shape
    base = pow2_map(shape, seed)
    none, first, last = (np.full(shape, NAN, F) for _ in range(3))
    first[B, B], last[rows - B - 1, cols - B - 1] = base[B, B], base[-1, -1]
    half = pow2_map(shape, seed + 1, p_nan=0.5)
    band = base.copy()
    band[rows // 2 - 7:rows // 2 + 7] = NAN  # 14 rows: wider than the window of 11
    band[:, cols // 2 - 6:cols // 2 + 7] = NAN
    signs = base.copy()
    rng = np.random.default_rng(seed + 2)
    pick = rng.integers(0, 4, shape)
    signs[pick == 0], signs[pick == 1], signs[pick == 2] = F(-0.5), F(0.0), F(-0.0)
    return dict(none=none, first=first, last=last, half=half, band=band, signs=signs)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(37, 29), (45, 150)])
def test_gpu_validity_patterns(gpu, reg, shape):
    ref, cmp = images(shape, 21)
    band = (shape[0] - 2 * B) * (shape[1] - 2 * B)
    for name, v in validity_patterns(shape, 5).items():
        for win in (1, 11):
            got, want = photo_case(gpu, reg, v, ref, cmp, IDENTITY, f"{shape} {name} win {win}", win_size=win)
            if name == "none":
                assert (got["n_valid"], got["median_bin"], got["ptile_bin"], got["sum"], got["mean"]) == (0, -1, -1, 0.0, 0.0)
                assert np.isnan(got["error_map"]).all() and not got["hist"].any()
            if name in ("first", "last"):
                at = (B, B) if name == "first" else (shape[0] - B - 1, shape[1] - B - 1)
                assert got["n_valid"] == 1 and not np.isnan(got["error_map"][at])
                assert got["median_bin"] == got["ptile_bin"] == int(np.flatnonzero(got["hist"])[0])
            if name == "signs":  # a negative value is a hole, both zeros take the infinite-depth projection
                neg = (v < 0)[B:shape[0] - B, B:shape[1] - B]
                assert got["n_valid"] == band - int(neg.sum()) and 0 < neg.sum() < band
        # the same patterns against a true map: every pixel counts, the first and the last of the image too
        t = np.full(shape, 0.75, F)
        vt = v.copy()
        if name in ("first", "last"):
            vt[:] = NAN
            vt.reshape(-1)[0 if name == "first" else -1] = F(1.0)
        got, _ = truth_case(gpu, reg, vt, t, f"{shape} {name} truth", win_size=5)
        assert got["n_valid"] == int((~np.isnan(vt)).sum())


@pytest.mark.gpu
def test_gpu_projection_leaves_the_comparison_frame_along_a_diagonal(gpu, reg):
    shape = (70, 200)
    ref, cmp = images(shape, 31)
    v = np.full(shape, 0.5, F)
    got, want = photo_case(gpu, reg, v, ref, cmp, SHEAR, "shear", win_size=1)
    ok = ~np.isnan(got["error_map"])
    per_row = ok.sum(axis=1)[B:shape[0] - B]
    first = np.array([np.flatnonzero(r)[0] if r.any() else -1 for r in ok[B:shape[0] - B]])
    assert 0 < got["n_valid"] < (shape[0] - 2 * B) * (shape[1] - 2 * B)
    assert len(set(per_row.tolist())) > 10 and len(set(first[first >= 0].tolist())) > 10, (per_row, first)  # the cut moves from row to row
    photo_case(gpu, reg, random_map(shape, 32, p_nan=0.2), ref, cmp, SHEAR, "shear, random map, smoothed", win_size=5)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(37, 29), (70, 200)])  # 70 = 4 * 16 + 6, 200 = 3 * 64 + 8: neither a multiple of the 64 x 16 tile
@pytest.mark.parametrize("win", [1, 3, 5, 11, 31])
def test_gpu_window_sizes_across_tile_edges(gpu, reg, shape, win):
    ref, cmp = images(shape, 41)
    v = random_map(shape, 42, p_nan=0.5)
    got, want = photo_case(gpu, reg, v, ref, cmp, PARALLAX, f"{shape} win {win}", win_size=win)
    assert got["n_valid"] > 50
    _, cnt = er.box_mean(want["raw_error"], win)
    valid = ~np.isnan(want["raw_error"])
    if win > 1:
        assert cnt[valid].min() < cnt[valid].max()  # (the counts vary: the mean is not the plain box's)
        assert not np.array_equal(er.bits(got["error_map"]), er.bits(want["raw_error"]))
    # the true-map source has no border: windows reach over the image's own edge
    t = random_map(shape, 43, lo=0.2, hi=1.5)
    truth_case(gpu, reg, v, t, f"{shape} truth win {win}", win_size=win)


def special_truth():
    """Every kind of v against every kind of t."""
    vs = np.array([NAN, 0.0, -1.0, INF, 6e-39, 0.5, 3e38, 1.0], F)
    ts = np.array([NAN, 0.0, -1.0, INF, 6e-39, 0.5, 1e-30, 2.0, -0.0, 1e-45], F)
    v = np.repeat(vs[:, None], ts.size, axis=1)
    t = np.repeat(ts[None, :], vs.size, axis=0)
    return v, t


@pytest.mark.gpu
@pytest.mark.parametrize("relative", [False, True])
@pytest.mark.parametrize("hist_scale", [1.0, 1000.0, 0.0])
def test_gpu_truth_mode_special_values_and_overflow(gpu, reg, relative, hist_scale):
    v, t = special_truth()
    for device_truth in (False, True):
        got, want = truth_case(gpu, reg, v, t, f"special values relative={relative} scale={hist_scale}", device_truth=device_truth,
                               relative=relative, hist_scale=hist_scale, win_size=1)
        e = got["error_map"]
        assert np.isnan(e[0]).all() and np.isnan(e[:, [0, 1, 2, 8]]).all()  # NaN v; NaN, zero, negative, -0 t
        assert np.isinf(e[3, 5]) and got["sum"] == np.inf and np.isinf(got["mean"])  # |inf - 0.5|: bin 255, an infinite sum
        assert np.isinf(e[6, 4]) == relative and e[6, 4] >= F(3e38)  # 3e38 / 6e-39 overflows
        assert got["hist"][255] >= 4 and got["ptile_bin"] == 255
        assert got["hist_scale"] == (hist_scale or 1000.0)
        # t = 1e-45 is > 0: a valid pixel; t = +inf too, with an infinite absolute error and no relative one (inf / inf)
        assert not np.isnan(e[5, 9]) and np.isinf(e[5, 3]) != relative and np.isnan(e[3, 3])
    # ordinary values, smoothed, both kinds of error
    v, t = random_map((37, 29), 51, p_nan=0.3), random_map((37, 29), 52)
    t[::7, ::5] = 0
    got, _ = truth_case(gpu, reg, v, t, f"ordinary relative={relative} scale={hist_scale}", relative=relative, hist_scale=hist_scale, win_size=5,
                        ptile_num=90, ptile_den=100)
    assert 0 <= got["median_bin"] <= got["ptile_bin"]


@pytest.mark.gpu
def test_gpu_1080p_one_bin_under_contention_and_every_level_of_the_sum(gpu, reg):
    shape = (1080, 1920)
    # every error equal: 0.25 in bin 250 of the 0.001 bins; 0.25 * count is exact, so the box mean leaves it
    t = np.full(shape, 1.0, F)
    v = np.full(shape, 1.25, F)
    got, want = truth_case(gpu, reg, v, t, "1080p one bin", device_truth=True, relative=False, win_size=11)
    print("1080p, every error in one bin: device_ms", got["device_ms"])
    assert got["hist"][250] == got["n_valid"] == v.size and got["median_bin"] == got["ptile_bin"] == 250
    assert got["sum"] == 0.25 * v.size and got["mean"] == F(0.25)
    # random, half of it NaN: 2025 blocks of 1024 pixels, two rounds of the second level
    ref, cmp = images(shape, 61)
    v = random_map(shape, 62, p_nan=0.5)
    v[400:500] = NAN
    got, want = photo_case(gpu, reg, v, ref, cmp, PARALLAX, "1080p random", win_size=11)
    print("1080p, random half-NaN photo: device_ms", got["device_ms"], "n_valid", got["n_valid"], "median", got["median_bin"], "p99", got["ptile_bin"])
    assert 850_000 < got["n_valid"] < 1_050_000 and np.count_nonzero(got["hist"]) > 20


@pytest.mark.gpu
def test_gpu_repeat_calls_outputs_one_by_one_and_on_the_device_only(gpu, reg):
    shape = (45, 150)
    rows, cols = shape
    ref, cmp = images(shape, 71)
    v = random_map(shape, 72, p_nan=0.3)
    keep = [on_device(v), on_device(ref), on_device(cmp)]
    base = dict(source=gpu.MAP_ERROR_PHOTO, KRKinv=PARALLAX[0], Kt=PARALLAX[1], border=B, map_device=keep[0].data_ptr(),
                ref_device=keep[1].data_ptr(), cmp_device=keep[2].data_ptr(), image_step_bytes=cols, win_size=5, max_error=20.0)
    want = er.map_error(v, er.PHOTO, PARALLAX[0], PARALLAX[1], ref, cmp, B, win_size=5, max_error=20.0, want_image=True)
    first = reg.map_error(gpu.MapErrorParams(want_image=True, **base), rows, cols)
    again = reg.map_error(gpu.MapErrorParams(want_image=True, **base), rows, cols)
    er.assert_same(first, want, "all outputs")
    er.assert_same(again, first, "a repeated begin")
    assert again["image"].tobytes() == first["image"].tobytes() and again["error_map"].tobytes() == first["error_map"].tobytes()
    view = reg.map_error_end(copy=False)  # a second _end of the same begin: the same view
    er.assert_same(view, first, "a second _end")
    # each flag alone
    flags = dict(want_stats="stats", want_error_map="error_map", want_image="image")
    off = {k: False for k in flags}
    for flag, key in flags.items():
        got = reg.map_error(gpu.MapErrorParams(**{**base, **off, flag: True}), rows, cols)
        er.assert_same(got, want, flag, keys=(key,))
        assert set(got["device"]) == {key}, flag
        assert ("hist" in got) == (key == "stats") and ("error_map" in got) == (key == "error_map") and ("image" in got) == (key == "image"), flag
    with pytest.raises(gpu.NLTGV2Error) as ei:
        reg.map_error(gpu.MapErrorParams(**{**base, **off}), rows, cols)  # nothing wanted
    assert ei.value.status == -1
    # copy_out = 0: the statistics travel, the arrays are fetched through the device pointers
    got = reg.map_error(gpu.MapErrorParams(want_image=True, copy_out=False, **base), rows, cols)
    assert "error_map" not in got and "image" not in got and set(got["device"]) == {"stats", "error_map", "image"}
    er.assert_same(got, want, "copy_out = 0", keys=("stats",))
    fetched = dict(error_map=fetch(got["device"]["error_map"], shape, F), image=fetch(got["device"]["image"], shape + (3,), np.uint8))
    er.assert_same(fetched, want, "through the device pointers", keys=("error_map", "image"))
    stats = fetch(got["device"]["stats"], (262,), np.int32)
    assert np.array_equal(stats[:256], want["hist"]) and stats[256:259].tolist() == [want["n_valid"], want["median_bin"], want["ptile_bin"]]
    assert stats[260:262].view(np.float64)[0] == want["sum"] and stats[259:260].view(F)[0] == want["mean"]
    # the synchronous entry point: the arrays that are not NULL
    lib = gpu.load_library()
    err, st = np.empty(shape, F), gpu.MapErrorStats()
    p = gpu.MapErrorParams(copy_out=False, want_stats=False, want_error_map=False, **base)
    rc = lib.flame_nltgv2_map_error(reg._ctx, C.byref(p), rows, cols, err.ctypes.data_as(C.POINTER(C.c_float)), None, C.byref(st))
    assert rc == 0
    one_shot = dict(error_map=err, hist=np.ctypeslib.as_array(st.hist), n_valid=st.n_valid, median_bin=st.median_bin, ptile_bin=st.ptile_bin,
                    sum=st.sum, mean=F(st.mean))
    er.assert_same(one_shot, want, "synchronous", keys=("error_map", "stats"))
    # the images of photo_set_images instead of device pointers
    reg.photo_set_images(ref, cmp)
    kw = {k: base[k] for k in base if k not in ("ref_device", "cmp_device", "image_step_bytes")}
    got = reg.map_error(gpu.MapErrorParams(want_image=True, **kw), rows, cols)
    er.assert_same(got, want, "the images of photo_set_images")


@pytest.mark.gpu
@pytest.mark.parametrize("flip", [False, True])
def test_gpu_picture(gpu, reg, flip):
    shape = (37, 61)  # 2257 pixels: the last thread of the picture kernel has one
    ref, cmp = images(shape, 81, step=80)
    v = random_map(shape, 82, p_nan=0.3)
    got, want = photo_case(gpu, reg, v, ref, cmp, PARALLAX, f"photo picture flip={flip}", win_size=3, max_error=24.0, flip=flip, want_image=True)
    img = got["image"][::-1, ::-1] if flip else got["image"]
    hole = np.isnan(got["error_map"])
    assert hole.any() and (~hole).any()
    assert (img[hole] == ref[hole][:, None]).all()  # grey shows through where no error is defined
    assert (img[~hole].max(axis=1) != img[~hole].min(axis=1)).all()  # the jet has no grey
    # the true-map source draws over a grey image of the caller's, from the host or the device
    t = random_map(shape, 83)
    gray = ref
    got, want = truth_case(gpu, reg, v, t, f"truth picture flip={flip}", gray=gray, win_size=5, max_error=0.5, flip=flip, want_image=True, relative=True)
    keep = [on_device(v), on_device(gray.base)]
    p = gpu.MapErrorParams(source=gpu.MAP_ERROR_TRUTH, map_device=keep[0].data_ptr(), truth=t, gray_device=keep[1].data_ptr(), gray_step_bytes=80,
                           win_size=5, max_error=0.5, flip=flip, want_image=True)
    er.assert_same(reg.map_error(p, *shape), want, f"truth picture over a device grey image flip={flip}")
    # errors beyond max_error take the last colour, +inf too
    t2 = t.copy()
    t2[5, 5] = F(6e-39)
    got, _ = truth_case(gpu, reg, np.full(shape, 3.0, F), t2, f"truth picture with +inf flip={flip}", gray=gray, win_size=1, max_error=0.5, flip=flip,
                        want_image=True)
    assert np.isinf(got["error_map"][5, 5])


@pytest.mark.gpu
def test_gpu_every_error_comes_before_anything_is_enqueued_and_leaves_the_previous_outputs(gpu):
    shape = (37, 29)
    rows, cols = shape
    ref, cmp = images(shape, 91)
    v, t = random_map(shape, 92, p_nan=0.3), random_map(shape, 93)
    keep = [on_device(v), on_device(ref), on_device(cmp)]
    dev = dict(map_device=keep[0].data_ptr())
    img = dict(ref_device=keep[1].data_ptr(), cmp_device=keep[2].data_ptr(), image_step_bytes=cols)
    P, lib = gpu.MapErrorParams, gpu.load_library()
    with gpu.Regularizer(0) as reg:
        good = P(want_image=True, **dev, **img)
        assert lib.flame_nltgv2_map_error_begin(reg._ctx, C.byref(good), rows, cols) == -4  # no graph
        reg.upload_graph(synth.make_graph("320x240", seed=9))
        with pytest.raises(gpu.NLTGV2Error):
            reg.map_error_end()  # no begin has succeeded
        first = reg.map_error(good, rows, cols)
        er.assert_same(first, er.map_error(v, er.PHOTO, IDENTITY[0], IDENTITY[1], ref, cmp, 3, want_image=True), "the good call")
        bad = dict(
            no_images=P(**dev),
            one_image=P(ref_device=img["ref_device"], image_step_bytes=cols, **dev),
            short_step=P(**{**img, "image_step_bytes": cols - 1}, **dev),
            border_0=P(border=0, **dev, **img), border_negative=P(border=-3, **dev, **img),
            even_window=P(win_size=4, **dev, **img), negative_window=P(win_size=-1, **dev, **img), wide_window=P(win_size=33, **dev, **img),
            ptile=P(ptile_num=101, ptile_den=100, **dev, **img), ptile_den_0=P(ptile_num=0, ptile_den=0, **dev, **img),
            ptile_negative=P(ptile_num=-1, **dev, **img),
            scale_negative=P(hist_scale=-1.0, **dev, **img), scale_nan=P(hist_scale=float("nan"), **dev, **img),
            scale_inf=P(hist_scale=float("inf"), **dev, **img),
            source=P(source=2, **dev, **img),
            truth_without_a_map=P(source=gpu.MAP_ERROR_TRUTH, **dev),
            truth_twice=P(source=gpu.MAP_ERROR_TRUTH, truth=t, truth_device=keep[0].data_ptr(), **dev),
            truth_picture_without_grey=P(source=gpu.MAP_ERROR_TRUTH, truth=t, want_image=True, **dev),
            truth_picture_short_step=P(source=gpu.MAP_ERROR_TRUTH, truth=t, want_image=True, gray_device=keep[1].data_ptr(), gray_step_bytes=cols - 1, **dev),
            picture_max_error_0=P(want_image=True, max_error=0.0, **dev, **img),
            nothing_wanted=P(want_stats=False, want_error_map=False, want_image=False, **dev, **img),
            no_resident_map=P(**img), no_filtered_map=P(use_filtered_map=True, **img),
        )
        for name, p in bad.items():
            with pytest.raises(gpu.NLTGV2Error) as ei:
                reg.map_error_begin(p, rows, cols)
            assert ei.value.status == -1, name
        for r, c in ((0, cols), (rows, -1), (65536, 65536)):
            with pytest.raises(gpu.NLTGV2Error):
                reg.map_error_begin(good, r, c)
        assert lib.flame_nltgv2_map_error_begin(reg._ctx, None, rows, cols) == -1
        assert lib.flame_nltgv2_map_error_end(reg._ctx, None) == -1
        # the images of photo_set_images must have the map's size
        reg.photo_set_images(*images((rows + 1, cols), 94))
        with pytest.raises(gpu.NLTGV2Error) as ei:
            reg.map_error_begin(P(**dev), rows, cols)
        assert ei.value.status == -1
        # a resident map of another size than the call's
        g = synth.make_graph("320x240", seed=9)
        reg.interpolate_mesh(synth.delaunay_triangles_scipy(g["pos"]), 240, 320)
        with pytest.raises(gpu.NLTGV2Error):
            reg.map_error_begin(P(**img), rows, cols)
        kept = reg.map_error_end()
        er.assert_same(kept, first, "after the errors")
        assert kept["image"].tobytes() == first["image"].tobytes()
        # ... and the resident map itself, at its own size, against a true map
        dense = reg.interpolate_mesh(synth.delaunay_triangles_scipy(g["pos"]), 240, 320)[0]
        truth = np.full((240, 320), 0.5, F)
        got = reg.map_error(P(source=gpu.MAP_ERROR_TRUTH, truth=truth), 240, 320)
        er.assert_same(got, er.map_error(dense, er.TRUTH, truth=truth), "the resident map")
        assert got["n_valid"] == int((~np.isnan(dense)).sum()) > 1000
