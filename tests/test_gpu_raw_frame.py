"""flame_stereo_add_raw_frame on the GPU, through the Python surface: the three planes of the resident frame byte for byte
against oracle.stereo_capi.make_frame of the checker's rectified image (tests/input_ref.py), with no tolerance and no pixel left
out, and the count of the outside pixels; every format with a padded, odd stride; host and device source; that the call changes
nothing else in the context; and its error returns."""
import ctypes as C

import numpy as np
import pytest

from oracle import stereo_capi as so
from tests import input_ref as ir
from tests import raw_frame_cases as rc
from tests.test_feature_frontend import PAD, plane_scene

pytestmark = pytest.mark.gpu
INVALID_ARG, NO_GRAPH = -1, -4


def _tracker(case):
    from flame_amd.stereo import FeatureTracker

    w, h, K, Kinv, p = rc.setup(case)
    return FeatureTracker(K, Kinv, w, h, border=PAD), p


def _assert_frame(tr, frame_id, grey, what):
    want = so.make_frame(grey, PAD)
    got = tr.download_frame(frame_id)
    for name, g, w_ in zip(("img_pad", "gradx_pad", "grady_pad"), got, want):
        if g.tobytes() != w_.tobytes():
            bad = np.argwhere(g != w_)
            raise AssertionError("%s: %s differs at %d places, first (row %d, col %d): %r vs %r"
                                 % (what, name, bad.shape[0], bad[0][0], bad[0][1], g[tuple(bad[0])], w_[tuple(bad[0])]))


@pytest.mark.parametrize("case", sorted(rc.CASES))
def test_gpu_cases_equal_the_checker(built, case):
    """61x37 = 2257 pixels: the dword store's odd tail.  denominator_zero and overflow: inf and NaN coordinates are outside."""
    raw, (grey, n_outside) = rc.expected(case)
    tr, p = _tracker(case)
    with tr:
        tr.set_input(format=ir.GREY8, **p)
        st = tr.add_raw_frame(10, raw)
        assert st == dict(n_outside=n_outside)
        _assert_frame(tr, 10, grey, case)
        assert tr.frame_count() == 1 and tr.last_kernel_ms() > 0


@pytest.mark.parametrize("fmt", [ir.GREY8, ir.BGR8, ir.RGB8, ir.BGRA8, ir.RGBA8])
def test_gpu_every_format_with_a_padded_odd_stride(built, fmt):
    """Stride = raw_width * bytes + 5: rows and 3-byte pixels at every alignment."""
    raw, (grey, n_outside) = rc.expected("pincushion", fmt, 5)
    assert raw.strides[0] == 61 * ir.BYTES[fmt] + 5 and n_outside == 433
    tr, p = _tracker("pincushion")
    with tr:
        tr.set_input(format=fmt, **p)
        assert tr.add_raw_frame(10, raw) == dict(n_outside=n_outside)
        _assert_frame(tr, 10, grey, "format %d" % fmt)


@pytest.mark.parametrize("fmt", [ir.BGRA8, ir.RGBA8])
def test_gpu_four_byte_formats_with_an_aligned_stride(built, fmt):
    """A tight 4-byte format from the host: base and stride are multiples of 4, the taps are read as dwords."""
    raw, (grey, n_outside) = rc.expected("pincushion", fmt, 0)
    tr, p = _tracker("pincushion")
    with tr:
        tr.set_input(format=fmt, **p)
        assert tr.add_raw_frame(10, raw) == dict(n_outside=n_outside)
        _assert_frame(tr, 10, grey, "format %d, tight" % fmt)


def test_gpu_bgr_and_rgb_read_the_same_bytes_differently(built):
    raw, (grey_bgr, _) = rc.expected("pincushion", ir.BGR8, 5)
    raw2, (grey_rgb, _) = rc.expected("pincushion", ir.RGB8, 5)
    assert raw.tobytes() == raw2.tobytes() and grey_bgr.tobytes() != grey_rgb.tobytes()
    tr, p = _tracker("pincushion")
    with tr:
        planes = []
        for fmt, grey in ((ir.BGR8, grey_bgr), (ir.RGB8, grey_rgb)):
            tr.set_input(format=fmt, **p)
            tr.add_raw_frame(10, raw)
            _assert_frame(tr, 10, grey, "format %d" % fmt)
            planes.append(tr.download_frame(10)[0])
        assert planes[0].tobytes() != planes[1].tobytes() and tr.frame_count() == 1


def test_gpu_remap_0(built):
    """GREY8 with a tight stride: the very bytes add_frame gives; BGRA8 with a padded stride: the checker's."""
    w, h, K, Kinv, p = rc.setup("pincushion")
    p = dict(p, remap=0)
    tr, _ = _tracker("pincushion")
    with tr:
        img = rc.raw_bytes(w, h, ir.GREY8)
        tr.add_frame(1, img)
        tr.set_input(format=ir.GREY8, **p)
        assert tr.add_raw_frame(2, img) == dict(n_outside=0)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(tr.download_frame(1), tr.download_frame(2)))
        raw = rc.raw_bytes(w, h, ir.BGRA8, 5)
        grey, n_outside = ir.rectify(raw, ir.BGRA8, p, K, Kinv, w, h)
        tr.set_input(format=ir.BGRA8, **p)
        assert tr.add_raw_frame(3, raw) == dict(n_outside=0) and n_outside == 0
        _assert_frame(tr, 3, grey, "BGRA8, remap 0")
        assert tr.frame_count() == 3


@pytest.mark.parametrize("lead", [0, 1])
def test_gpu_device_source(built, lead):
    """The raw frame in device memory, `lead` bytes into an allocation (1: an unaligned base): enqueue-only without stats (the
    next download_frame waits for the stream), then with the count; the bytes are those of the host-source call."""
    import torch

    fmt = ir.BGRA8
    raw, (grey, n_outside) = rc.expected("pincushion", fmt, 4 * lead)  # (lead 1: an aligned stride behind an unaligned base)
    stride = raw.strides[0]
    dev = torch.zeros(lead + raw.size, dtype=torch.uint8, device="cuda")
    dev[lead:] = torch.from_numpy(raw.copy().reshape(-1)).cuda()
    torch.cuda.synchronize()
    tr, p = _tracker("pincushion")
    with tr:
        tr.set_input(format=fmt, **p)
        tr.add_raw_frame(1, raw)
        host_planes = tr.download_frame(1)
        assert tr.add_raw_frame(2, None, device_ptr=dev.data_ptr() + lead, stride=stride, want_stats=False) is None
        dev_planes = tr.download_frame(2)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(dev_planes, host_planes))
        _assert_frame(tr, 2, grey, "device source")
        st = tr.add_raw_frame(3, None, device_ptr=dev.data_ptr() + lead, stride=stride, want_stats=True)
        assert st == dict(n_outside=n_outside)
        _assert_frame(tr, 3, grey, "device source with stats")
        # the same id again, enqueue-only twice in a row: the second replaces the first, no buffer is added
        for _ in range(2):
            tr.add_raw_frame(2, None, device_ptr=dev.data_ptr() + lead, stride=stride, want_stats=False)
        _assert_frame(tr, 2, grey, "device source, replaced")
        assert tr.frame_count() == 3
    del dev


def test_gpu_nothing_else_moves(built):
    """The resident features, the projected set and another resident frame are byte-identical before and after."""
    from flame_amd import synth_stereo as ss
    from flame_amd.stereo import FeatureTracker, StereoParams

    sc = plane_scene(320, 240)
    with FeatureTracker(sc.K32, sc.Kinv32, 320, 240, border=PAD) as tr:
        for k in (10, 13):
            tr.add_frame(k, sc.render(k))
        tr.set_features(ss.make_features(sc, so.FEATURE_DTYPE, [10], 500, 3).view(tr.get_features().dtype))
        tr.project_features(StereoParams(), 13, [dict(id=10, q_to_new=sc.relative(10, 13)[0], t_to_new=sc.relative(10, 13)[1])])
        before = (tr.get_features(), tr.get_projected(), tr.download_frame(13), tr.download_frame(10))
        assert before[0].shape[0] > 0 and before[1].shape[0] > 0
        Kraw, _ = ir.cam(300, 298, 200.3, 140.6)
        p = dict(remap=1, raw_width=400, raw_height=280, K_raw=Kraw, dist=np.float32([-0.2, 0.05, 1e-3, -1e-3]))
        raw = rc.raw_bytes(400, 280, ir.BGR8, 3)
        grey, n_outside = ir.rectify(raw, ir.BGR8, p, sc.K32, sc.Kinv32, 320, 240)
        tr.set_input(format=ir.BGR8, **p)
        assert tr.add_raw_frame(20, raw) == dict(n_outside=n_outside)
        _assert_frame(tr, 20, grey, "400x280 BGR8 -> 320x240")
        after = (tr.get_features(), tr.get_projected(), tr.download_frame(13), tr.download_frame(10))
        assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
        for a, b in zip(after[2] + after[3], before[2] + before[3]):
            assert a.tobytes() == b.tobytes()
        assert tr.frame_count() == 3


def _raw_call(tr, frame_id, ptr, stride, on_device=0):
    return tr._L.flame_stereo_add_raw_frame(tr._ctx, frame_id, C.c_void_p(ptr), stride, on_device, None)


def test_gpu_error_returns_leave_the_frames_alone(built):
    from flame_amd import NLTGV2Error
    from flame_amd.stereo import InputParams, _lib

    w, h, K, Kinv, p = rc.setup("pincushion")
    raw, (grey, _) = rc.expected("pincushion", ir.BGR8, 5)
    tr, _ = _tracker("pincushion")
    with tr:
        tr.add_frame(1, rc.raw_bytes(w, h, ir.GREY8))
        kept = tr.download_frame(1)

        def unchanged():
            return tr.frame_count() == 1 and all(a.tobytes() == b.tobytes() for a, b in zip(tr.download_frame(1), kept))

        # no set_input yet
        assert _raw_call(tr, 1, raw.ctypes.data, raw.strides[0]) == INVALID_ARG and unchanged()
        assert _raw_call(tr, 2, raw.ctypes.data, raw.strides[0]) == INVALID_ARG and unchanged()
        # what set_input refuses: an unknown format, a raw dimension below 2, remap 0 with another size
        for bad in (dict(format=5), dict(format=-1), dict(raw_width=1), dict(raw_height=1), dict(raw_height=0),
                    dict(remap=0, raw_width=w + 1), dict(remap=0, raw_height=h - 1), dict(remap=2)):
            with pytest.raises(NLTGV2Error) as ei:
                tr.set_input(**dict(dict(p, format=ir.BGR8), **bad))
            assert ei.value.status == INVALID_ARG, bad
            assert _raw_call(tr, 2, raw.ctypes.data, raw.strides[0]) == INVALID_ARG and unchanged(), bad
        assert tr._L.flame_stereo_set_input(tr._ctx, None) == INVALID_ARG
        # with an input: a NULL frame, a stride below the row's pixels
        tr.set_input(format=ir.BGR8, **p)
        assert _raw_call(tr, 2, None, raw.strides[0]) == INVALID_ARG and unchanged()
        assert _raw_call(tr, 2, None, raw.strides[0], on_device=1) == INVALID_ARG and unchanged()
        assert _raw_call(tr, 1, raw.ctypes.data, 61 * 3 - 1) == INVALID_ARG and unchanged()
        assert _raw_call(tr, 2, raw.ctypes.data, 0) == INVALID_ARG and unchanged()
        assert _raw_call(tr, 2, raw.ctypes.data, -raw.strides[0]) == INVALID_ARG and unchanged()
        # a refused set_input leaves the earlier one standing, and after all of it the call still works
        with pytest.raises(NLTGV2Error):
            tr.set_input(**dict(p, format=9))
        assert _raw_call(tr, 2, raw.ctypes.data, raw.strides[0]) == 0 and tr.frame_count() == 2
        _assert_frame(tr, 2, grey, "after the errors")
        # set_camera forgets the input (and drops the frames) until set_input is called again
        tr.set_camera(K, Kinv, w, h, border=PAD)
        assert tr.frame_count() == 0
        assert _raw_call(tr, 2, raw.ctypes.data, raw.strides[0]) == INVALID_ARG and tr.frame_count() == 0
        tr.set_input(format=ir.BGR8, **p)
        assert _raw_call(tr, 2, raw.ctypes.data, raw.strides[0]) == 0 and tr.frame_count() == 1
        _assert_frame(tr, 2, grey, "after set_camera and set_input")
    # no camera: FLAME_NLTGV2_ERR_NO_GRAPH, from both entry points
    L = _lib()
    ctx = C.c_void_p()
    assert L.flame_stereo_create(C.byref(ctx), 0) == 0
    try:
        ip = InputParams(format=ir.BGR8, **p)
        assert L.flame_stereo_set_input(ctx, C.byref(ip)) == NO_GRAPH
        assert L.flame_stereo_add_raw_frame(ctx, 1, C.c_void_p(raw.ctypes.data), raw.strides[0], 0, None) == NO_GRAPH
        assert L.flame_stereo_frame_count(ctx) == 0
    finally:
        L.flame_stereo_destroy(ctx)
    assert L.flame_stereo_add_raw_frame(None, 1, C.c_void_p(raw.ctypes.data), raw.strides[0], 0, None) == INVALID_ARG
