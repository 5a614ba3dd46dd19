"""numpy restatement of flame_nltgv2_map_error_begin (include/flame_nltgv2.h states the rules), the checker of the map-error stage.
float32 where the device computes in float, float64 for the sum, no FMA anywhere; the device must agree bit for bit.

  error image   PHOTO: oracle.capi.photo_residual on the pixel grid u = (col, row) with the map's values (graph_scale 1);
                TRUTH: |v - t| or |v - t| / t where !(v != v) and t > 0, NaN elsewhere
  box mean      sum / (float)count over the non-NaN errors of the window, the sum separably: per row left to right from +0.0f, then
                those row sums top to bottom from +0.0f; a NaN or a position outside the image adds +0.0f
  bins          s = err * hist_scale; bin = 255 if s >= 255 else (int)(s + 0.5f)
  ranks         median: the smallest m with 2 * cum[m] > n; percentile: the smallest m with den * cum[m] > num * n, in integers
  sum           float -> double terms, holes +0.0; blocks of 1024 consecutive pixels pairwise p[t] += p[t + s], s = 512 .. 1; the block
                partials b: q[t] = b[t] + b[t + 1024] + ... from +0.0, then q pairwise in the same way
  picture       the grey image, jet(err, 0, max_error) (tests/debug_ref.py) where the error is not NaN; flip: reversed pixel order
"""
import numpy as np

from tests import debug_ref as dr

F = np.float32
PHOTO, TRUTH = 0, 1
CHUNK = 1024
STAT_KEYS = ("n_valid", "median_bin", "ptile_bin")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def default_window(win_size, cols):
    return (5 if cols < 640 else 11) if win_size == 0 else win_size


def photo_error(idepthmap, KRKinv, Kt, ref, cmp, border):
    from oracle import capi as oracle

    m = np.ascontiguousarray(idepthmap, F)
    rows, cols = m.shape
    jj, ii = np.meshgrid(np.arange(cols, dtype=F), np.arange(rows, dtype=F))
    pos = np.stack([jj.reshape(-1), ii.reshape(-1)], axis=1)
    return oracle.photo_residual(pos, m.reshape(-1), 1.0, KRKinv, Kt, ref, cmp, border).reshape(rows, cols)


def truth_error(idepthmap, truth, relative=True):
    v, t = np.asarray(idepthmap, F), np.asarray(truth, F)
    with np.errstate(all="ignore"):
        valid = ~np.isnan(v) & (t > F(0))
        e = np.abs((v - t).astype(F))
        if relative:
            e = (e / t).astype(F)
    return np.where(valid & ~np.isnan(e), e, F(np.nan)).astype(F)  # (inf - inf, inf / inf: the hole's own quiet NaN)


def box_mean(err, win_size):
    """-> (the smoothed image, the counts)."""
    err = np.asarray(err, F)
    rows, cols = err.shape
    ok = ~np.isnan(err)
    if win_size == 1:
        return err.copy(), ok.astype(np.int64)
    assert win_size % 2 == 1 and win_size >= 1
    h = win_size // 2
    z = np.zeros((rows + 2 * h, cols + 2 * h), F)  # +0.0f outside the image and on NaNs
    z[h:h + rows, h:h + cols] = np.where(ok, err, F(0))
    c = np.zeros((rows + 2 * h, cols + 2 * h), np.int64)
    c[h:h + rows, h:h + cols] = ok
    with np.errstate(all="ignore"):
        hs, hc = np.zeros((rows + 2 * h, cols), F), np.zeros((rows + 2 * h, cols), np.int64)
        for k in range(win_size):  # left to right
            hs = (hs + z[:, k:k + cols]).astype(F)
            hc += c[:, k:k + cols]
        s, n = np.zeros((rows, cols), F), np.zeros((rows, cols), np.int64)
        for k in range(win_size):  # top to bottom
            s = (s + hs[k:k + rows]).astype(F)
            n += hc[k:k + rows]
        mean = (s / np.maximum(n, 1).astype(F)).astype(F)
    assert (n[ok] >= 1).all()
    return np.where(ok, mean, F(np.nan)).astype(F), n


def bin_of(err, hist_scale):
    """The bins of non-NaN errors."""
    e = np.asarray(err, F)
    with np.errstate(all="ignore"):
        s = (e * F(hist_scale)).astype(F)
        top = s >= F(255)
        b = (np.where(top, F(0), s) + F(0.5)).astype(F).astype(np.int64)  # (int): truncation
    return np.where(top, 255, b)


def histogram(err, hist_scale):
    e = np.asarray(err, F).reshape(-1)
    e = e[~np.isnan(e)]
    return np.bincount(bin_of(e, hist_scale), minlength=256).astype(np.int32)


def ranks(hist, ptile_num=99, ptile_den=100):
    """-> (n_valid, median_bin, ptile_bin), in Python integers."""
    n = int(sum(int(h) for h in hist))
    median = ptile = -1
    cum = 0
    for m, h in enumerate(hist):
        if n == 0:
            break
        cum += int(h)
        if median < 0 and 2 * cum > n:
            median = m
        if ptile < 0 and ptile_den * cum > ptile_num * n:
            ptile = m
    return n, median, ptile


def _pairwise(p):
    """p[..., t] += p[..., t + s] for s = 512 .. 1 -> p[..., 0]."""
    s = CHUNK // 2
    with np.errstate(all="ignore"):
        while s >= 1:
            p = p[..., :s] + p[..., s:2 * s]
            s //= 2
    return p[..., 0]


def ordered_sum(err):
    e = np.asarray(err, F).reshape(-1)
    terms = np.where(np.isnan(e), 0.0, e.astype(np.float64))
    chunks = (terms.size + CHUNK - 1) // CHUNK
    padded = np.zeros(chunks * CHUNK, np.float64)
    padded[:terms.size] = terms
    b = _pairwise(padded.reshape(chunks, CHUNK))
    rounds = (chunks + CHUNK - 1) // CHUNK
    bp = np.zeros(rounds * CHUNK, np.float64)
    bp[:chunks] = b
    q = np.zeros(CHUNK, np.float64)
    with np.errstate(all="ignore"):
        for j in range(rounds):  # thread t: b[t], b[t + 1024], ... in turn
            q = q + bp[j * CHUNK:(j + 1) * CHUNK]
    return float(_pairwise(q))


def statistics(err, hist_scale, ptile_num=99, ptile_den=100):
    hist = histogram(err, hist_scale)
    n, median, ptile = ranks(hist, ptile_num, ptile_den)
    total = ordered_sum(err)
    with np.errstate(all="ignore"):
        mean = F(np.float64(total) / np.float64(n)) if n > 0 else F(0)
    return dict(hist=hist, n_valid=n, median_bin=median, ptile_bin=ptile, sum=total, mean=mean)


def picture(gray, err, max_error, flip=False):
    out = dr._gray3(gray)
    e = np.asarray(err, F)
    ok = ~np.isnan(e)
    with np.errstate(all="ignore"):
        col = dr.jet(e, 0.0, max_error)
    out[ok] = col[ok]
    return dr._flip(out, flip)


def map_error(idepthmap, source=PHOTO, KRKinv=None, Kt=None, ref=None, cmp=None, border=3, truth=None, relative=True, win_size=0,
              hist_scale=0.0, ptile_num=99, ptile_den=100, gray=None, max_error=32.0, flip=False, want_image=False):
    m = np.asarray(idepthmap, F)
    raw = photo_error(m, KRKinv, Kt, ref, cmp, border) if source == PHOTO else truth_error(m, truth, relative)
    win = default_window(win_size, m.shape[1])
    err, _ = box_mean(raw, win)
    scale = hist_scale if hist_scale != 0.0 else (1.0 if source == PHOTO else 1000.0)
    out = statistics(err, scale, ptile_num, ptile_den)
    out.update(error_map=err, raw_error=raw, win_size=win, hist_scale=scale)
    if want_image:
        out["image"] = picture(ref if source == PHOTO else gray, err, max_error, flip)
    return out


def assert_same(got, ref, what="", keys=("error_map", "stats", "image")):
    """Bit for bit: the error map as uint32, the histogram and the ranks equal, the sum equal as a double, the picture's bytes."""
    if "error_map" in keys:
        g, r = bits(got["error_map"]), bits(ref["error_map"])
        nan = np.isnan(ref["error_map"])
        assert np.array_equal(np.isnan(got["error_map"]), nan), f"{what}: the holes differ"
        bad = g != r  # (the holes too: both sides write the quiet NaN 0x7fc00000)
        assert not bad.any(), f"{what}: error_map differs at {np.argwhere(bad)[:5].tolist()} ({int(bad.sum())} pixels)"
    if "stats" in keys:
        assert np.array_equal(got["hist"], ref["hist"]), f"{what}: hist differs in bins {np.flatnonzero(got['hist'] != ref['hist'])[:8].tolist()}"
        for k in STAT_KEYS:
            assert got[k] == ref[k], f"{what}: {k} {got[k]} != {ref[k]}"
        a, b = np.float64(got["sum"]), np.float64(ref["sum"])
        assert a.tobytes() == b.tobytes(), f"{what}: sum {a!r} != {b!r}"
        assert F(got["mean"]).tobytes() == F(ref["mean"]).tobytes(), f"{what}: mean {got['mean']!r} != {ref['mean']!r}"
    if "image" in keys and "image" in ref:
        assert np.array_equal(got["image"], ref["image"]), f"{what}: the picture differs in {int((got['image'] != ref['image']).any(axis=2).sum())} pixels"
