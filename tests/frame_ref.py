"""The checker of utils::Frame::create level 0 (frame.cc:33-71) as flame_stereo_add_frame leaves it on the device: the three
padded planes of a frame, in plain numpy.  It shares no index arithmetic with k_frame_pad_gradient or with
oracle/stereo_oracle.c: the padding is numpy's own, the gradients are slices.

img_pad     cv::copyMakeBorder(img, border, BORDER_REFLECT_101): the padded pixel whose source coordinate along an axis of length
            `len` is p takes cv::borderInterpolate's loop -- while p lies outside [0, len): p < 0 -> -p, p >= len ->
            2 (len - 1) - p -- REPEATED until p lies inside, as often as a border wider than the frame needs.  That is
            np.pad(mode="reflect"); `reflect_101` below is the loop itself, and `padded_image` asserts the two agree.
gradx_pad,  getCentralGradient (image_utils.h:426-474), then cv::copyMakeBorder(BORDER_CONSTANT 0): 0.5 * (right - left) and
grady_pad   0.5 * (down - up) inside; the first column / row right - self and down - self, the last self - left and
            self - up, both without the half.  float32: a difference of two bytes and its half are exact.
"""
import numpy as np

F = np.float32


def reflect_101(p, length):
    """(source index, number of reflections) of coordinate p along an axis of `length` >= 2: the OpenCV loop, literally."""
    assert length >= 2
    n = 0
    while p < 0 or p >= length:
        p = -p if p < 0 else 2 * (length - 1) - p
        n += 1
    return p, n


def index_map(length, border):
    """(source index, reflections) of each of the length + 2 * border padded coordinates of one axis: two int arrays."""
    pairs = [reflect_101(q - border, length) for q in range(length + 2 * border)]
    return np.array([s for s, _ in pairs], np.int64), np.array([n for _, n in pairs], np.int64)


LOOP_LIMIT = 1 << 16  # padded planes up to this many pixels are also walked pixel by pixel


def padded_image_loop(img, border):
    """img_pad by the rule as it is stated: every padded pixel fetches img[reflect(y), reflect(x)], one at a time."""
    h, w = img.shape
    out = np.empty((h + 2 * border, w + 2 * border), np.uint8)
    sxs = [reflect_101(x - border, w)[0] for x in range(out.shape[1])]  # (the same for every row: taken once)
    for y in range(out.shape[0]):
        sy, _ = reflect_101(y - border, h)
        for x, sx in enumerate(sxs):
            out[y, x] = img[sy, sx]
    return out


def padded_image(img, border):
    """np.pad(mode="reflect"); checked against the per-pixel loop (planes above LOOP_LIMIT pixels: against the loop's index map
    of each axis, which is the same rule taken once per row and column)."""
    img = np.ascontiguousarray(img, np.uint8)
    assert img.ndim == 2 and min(img.shape) >= 2 and border >= 0
    out = np.pad(img, border, mode="reflect")
    if out.size <= LOOP_LIMIT:
        want = padded_image_loop(img, border)
    else:
        want = img[np.ix_(index_map(img.shape[0], border)[0], index_map(img.shape[1], border)[0])]
    assert out.dtype == np.uint8 and out.tobytes() == want.tobytes(), "np.pad(reflect) and the OpenCV loop disagree"
    return out


def central_gradient(img):
    """(gx, gy) of getCentralGradient<uint8_t, float>, unpadded, float32."""
    f = np.ascontiguousarray(img, np.uint8).astype(F)
    gx, gy = np.empty_like(f), np.empty_like(f)
    gx[:, 1:-1] = F(0.5) * (f[:, 2:] - f[:, :-2])
    gx[:, 0] = f[:, 1] - f[:, 0]
    gx[:, -1] = f[:, -1] - f[:, -2]
    gy[1:-1] = F(0.5) * (f[2:] - f[:-2])
    gy[0] = f[1] - f[0]
    gy[-1] = f[-1] - f[-2]
    assert gx.dtype == F and gy.dtype == F
    return gx, gy


def make_frame(img, border):
    """(img_pad u8, gradx_pad f32, grady_pad f32), each (h + 2 border, w + 2 border)."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    pad = padded_image(img, border)
    planes = []
    for g in central_gradient(img):
        p = np.zeros(pad.shape, F)
        p[border:border + h, border:border + w] = g
        planes.append(p)
    return pad, planes[0], planes[1]


def ramp(w, h):
    """img[y, x] = (7 x + 13 y) % 251."""
    y, x = np.mgrid[0:h, 0:w]
    return ((7 * x + 13 * y) % 251).astype(np.uint8)


def assert_planes_equal(got, want, what):
    """Bit for bit, all three planes; names the first place that differs."""
    for name, g, w_ in zip(("img_pad", "gradx_pad", "grady_pad"), got, want):
        assert g.shape == w_.shape and g.dtype == w_.dtype, "%s: %s is %s %s, expected %s %s" % (what, name, g.shape, g.dtype,
                                                                                                 w_.shape, w_.dtype)
        if g.tobytes() != w_.tobytes():
            bad = np.argwhere(g.view(np.uint32 if g.dtype == F else np.uint8) != w_.view(np.uint32 if g.dtype == F else np.uint8))
            raise AssertionError("%s: %s differs at %d places, first (row %d, col %d): %r vs %r"
                                 % (what, name, bad.shape[0], bad[0][0], bad[0][1], g[tuple(bad[0])], w_[tuple(bad[0])]))
