"""BASELINE config 5 at its edges: the per-vertex photometric residual (photo_residual_at, nltgv2_device.hpp) on every path that
computes it, where kernels go wrong.

CPU: the checker (oracle/photometric_oracle.c) against an independent float64 statement of the residual (tests/photo_ref64.py)
  on smooth, noisy and x/y-asymmetric textures and on rotation, forward, backward, lateral and behind-the-camera motion.
GPU: vertices placed on and one float32 ulp either side of the border lines, at integer and .5 pixels and on the last interior
  row and column; x = 0, -0, negative, NaN, very large; graph scales that push idepth to 0 or to infinity; odd image sizes,
  borders 1, 2, 4 and one wider than half the image; rows padded with non-zero bytes.  Every output equals the checker bit for
  bit, through the stand-alone sweep, the canonical path's sweep, the per-step path's packed sweep and the epilogue of every
  persistent form.  Then the standing target (photo_fuse) across every change of the graph, the state and the images."""
import numpy as np
import pytest

from flame_amd import synth
from oracle import capi as oracle
from tests import photo_ref64 as r64
from tests.test_photometric import _rot_y, smooth_texture

EPS32 = float(np.finfo(np.float32).eps)


def _rot_x(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)


def noise_texture(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8)


def asymmetric_texture(rows, cols, seed):
    """Fast in x, slow in y, plus a diagonal ramp: a transposed or mirrored lookup lands on other values."""
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    ph = np.random.default_rng(seed).random() * 6.0
    v = 110 + 70 * np.sin(x / 2.3 + ph) * np.cos(y / 17.0) + 60 * (x / cols) - 30 * (y / rows) ** 2
    return np.clip(v, 0, 255).astype(np.uint8)


TEXTURES = {"smooth": smooth_texture, "noise": noise_texture, "asymmetric": asymmetric_texture}


def camera(rows, cols):
    """fx != fy and an off-centre principal point, so that a swapped x / y cannot pass."""
    return np.array([[0.55 * cols, 0, cols / 2.0 - 3.3], [0, 0.61 * cols, rows / 2.0 + 2.1], [0, 0, 1]], np.float64)


MOTIONS = {  # T_ref->cmp = (R, t); scene depths 0.4 .. 3.3
    "rotation": (_rot_y(0.03) @ _rot_x(-0.02), np.zeros(3)),
    "forward": (_rot_y(0.005), np.array([0.01, 0.0, -0.25])),
    "backward": (_rot_x(0.004), np.array([0.0, 0.02, 0.35])),
    "lateral": (_rot_y(-0.01), np.array([0.12, -0.07, 0.0])),
    "behind": (_rot_y(0.02), np.array([0.03, 0.0, -1.2])),  # every point nearer than 1.2 ends up behind the other camera
}


def geometry32(K, R, t):
    """KRKinv, Kt as the float32 rounding of their float64 values."""
    return (K @ R @ np.linalg.inv(K)).astype(np.float32), (K @ t).astype(np.float32)


def scene(rows, cols, seed, V=3000):
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-6, cols + 6, V), rng.uniform(-6, rows + 6, V)], 1).astype(np.float32)
    x = (1.0 / rng.uniform(0.4, 3.3, V)).astype(np.float32)
    x[::37] = 0.0  # at infinity
    x[5::101] = -0.5
    x[7::103] = np.nan
    return pos, x


def coord_bound(K, R, t, pos, x, graph_scale, c64, z):
    """Per-vertex bound of |checker's projection - float64 projection| (pixels, per axis).  The checker evaluates
    h = KRKinv (u * depth) + Kt with KRKinv, Kt rounded to float32, then h0 / h2, h1 / h2: each of the at most five
    roundings of a term is relative (<= eps), so |h_i error| <= 8 eps T_i with T_i the sum of the terms' magnitudes,
    and c_i = h_i / h2 is off by at most 8 eps (T_i + |c_i| T_2) / |h2| plus 2 eps |c_i| for the division.
    Doubled for margin (16 eps)."""
    A = K @ R @ np.linalg.inv(K)
    kt = K @ t
    u = pos.astype(np.float64)
    idepth = x.astype(np.float64) * graph_scale
    inf = idepth == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.where(inf, 1.0, 1.0 / idepth)
        hom = np.stack([u[:, 0] * depth, u[:, 1] * depth, depth], 1)
        T = np.abs(hom) @ np.abs(A).T + np.where(inf, 0.0, 1.0)[:, None] * np.abs(kt)[None, :]
        h2 = np.where(inf, z, z * depth)  # (K's last row is (0, 0, 1): h2 is the point's z, times depth for a finite point)
        b = 16 * EPS32 * (T[:, :2] + np.abs(c64) * T[:, 2:3]) / np.abs(h2)[:, None] + 2 * EPS32 * np.abs(c64)
    return b, h2


@pytest.mark.parametrize("texture", sorted(TEXTURES))
@pytest.mark.parametrize("motion", sorted(MOTIONS))
def test_checker_against_float64_reference(texture, motion):
    """The checker's projection within a derived per-vertex bound of the float64 projection (and within 2e-3 px for every
    vertex inside both frames whose depth in the other camera is at least a tenth of its depth in this one); its residual
    within (local image range) x (coordinate bound) + float32 interpolation rounding; NaN patterns equal but for vertices
    within the coordinate bound of a border line."""
    rows, cols, border, gs = 479, 641, 3, 1.25
    ref, cmp = TEXTURES[texture](rows, cols, 11), TEXTURES[texture](rows, cols, 12)
    K = camera(rows, cols)
    R, t = MOTIONS[motion]
    KRKinv, Kt = geometry32(K, R, t)
    pos, x = scene(rows, cols, 5)
    x = x / np.float32(gs)
    err32 = oracle.photo_residual(pos, x, gs, KRKinv, Kt, ref, cmp, border)
    err64, c64, z = r64.residual64(pos, x, gs, K, R, t, ref, cmp, border)
    idepth32 = x * np.float32(gs)
    c32 = np.array([oracle.photo_project(KRKinv, Kt, float(pos[v, 0]), float(pos[v, 1]), float(idepth32[v]))
                    if idepth32[v] >= 0 else (np.nan, np.nan) for v in range(len(x))])
    bound, h2 = coord_bound(K, R, t, pos, x, gs, c64, z)
    live = (idepth32 >= 0) & np.isfinite(bound).all(1) & (bound < 0.25).all(1)
    assert live.sum() > 0.8 * len(x)
    dev = np.abs(c32 - c64)
    assert (dev[live] <= bound[live]).all(), (motion, dev[live].max(), bound[live][np.argmax((dev[live] / bound[live]).max(1))])
    in_frame = live & r64.inside64(c64[:, 0], c64[:, 1], rows, cols, 0) & r64.inside64(pos[:, 0], pos[:, 1], rows, cols, 0)
    well_in_front = in_frame & (h2 * np.where(idepth32 == 0, 1.0, idepth32) >= 0.1)
    assert well_in_front.sum() > 200 and dev[well_in_front].max() <= 2e-3
    if motion == "behind":
        assert (z[idepth32 > 0] < 0).sum() > 100  # some of the graph is behind the other camera: projected as it is

    lo, hi = np.float64(border), np.array([cols - border, rows - border], np.float64)
    near_line = ~live | ((np.abs(c64 - lo) <= bound) | (np.abs(c64 - hi) <= bound)).any(1)
    differ = np.isnan(err32) != np.isnan(err64)
    assert not (differ & ~near_line).any(), np.flatnonzero(differ & ~near_line)[:10]
    both = ~np.isnan(err32) & ~np.isnan(err64)
    assert both.sum() > (0.05 if motion == "behind" else 0.4) * len(x)
    slope = r64.local_range(cmp, c64[both, 0], c64[both, 1])
    tol = slope * (bound[both, 0] + bound[both, 1]) + 64 * EPS32 * 255
    assert (np.abs(err32[both] - err64[both]) <= tol).all(), (np.abs(err32[both] - err64[both]) - tol).max()


def test_float64_reference_sees_axes_and_corners():
    """The float64 statement itself: exact corner weights on an image whose pixels are all different, x as the column,
    rows addressed through the stride, a point at infinity moved by the rotation only."""
    img = (np.arange(7 * 9).reshape(7, 9) * 3 % 251).astype(np.uint8)
    buf = np.full((7, 16), 200, np.uint8)
    buf[:, :9] = img
    view = buf[:, :9]
    for xq, yq in ((2.25, 4.5), (6.0, 1.0), (7.75, 5.125)):
        x0, y0, fx, fy = int(xq), int(yq), xq - int(xq), yq - int(yq)
        want = ((1 - fx) * (1 - fy) * img[y0, x0] + fx * (1 - fy) * img[y0, x0 + 1] + (1 - fx) * fy * img[y0 + 1, x0]
                + fx * fy * img[y0 + 1, x0 + 1])
        assert r64.bilinear64(*r64._flat_step(view), xq, yq) == pytest.approx(want, abs=1e-12)
        assert abs(oracle.photo_bilinear_u8(img, xq, yq) - want) < 1e-4
    K = camera(120, 160)
    c_inf, _ = r64.project64(K, _rot_y(0.01), np.array([5.0, 5.0, 5.0]), np.array([[40.0, 30.0]]), np.array([0.0]))
    c_rot, _ = r64.project64(K, _rot_y(0.01), np.zeros(3), np.array([[40.0, 30.0]]), np.array([0.7]))
    assert np.allclose(c_inf, c_rot, atol=1e-9)


# ---- GPU: the edge grid ---------------------------------------------------------------------------------------------------------
def _lines(n, border):
    """Coordinates along an axis of n pixels: both border lines and one float32 ulp either side, integer and .5 pixels, the
    last interior pixel, and the image's own edges."""
    f = np.float32
    vals = []
    for b in (border, n - border):
        vals += [f(b), np.nextafter(f(b), f(-np.inf)), np.nextafter(f(b), f(np.inf))]
    vals += [f(n - border - 1), f(n - border - 0.5), f(border + 0.5), f(n // 2), f(n // 2 + 0.5), f(n - 2), f(n - 1.5),
             f(n - 1), f(0.0), f(1.0), f(0.5), f(n)]
    return np.unique(np.array(vals, np.float32))


SPECIAL_X = np.array([0.7, 0.0, -0.0, -0.3, np.nan, 1e30, 3.0, 1.5e-3, 0.25, 2.0e4, -1e30], np.float32)


def edge_graph(rows, cols, border, base_config, shift, seed):
    """A synthetic graph scaled to the image, part of its vertices moved onto the edge grid: as it is, and moved by -shift (a
    pure image-space shift by +shift then takes them back onto the lines in the other image).  Each grid point takes the
    nearest vertex not yet moved, so every vertex stays close to where it was and the patch layouts keep their locality
    (the two-half-edges form, for one, needs that to apply)."""
    g = synth.make_graph(base_config, seed=seed)
    bw, bh, _ = synth.CONFIGS[base_config]
    pos = g["pos"] * np.array([cols / bw, rows / bh], np.float32)
    xs, ys = _lines(cols, border), _lines(rows, border)
    grid = np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2)
    pts = np.unique(np.concatenate([grid, (grid - np.asarray(shift, np.float32)).astype(np.float32)]), axis=0)
    assert len(pts) <= g["V"] // 2
    slots = np.empty(len(pts), np.int64)
    free = np.ones(g["V"], bool)
    for i, pt in enumerate(pts):
        d = ((pos - pt).astype(np.float64) ** 2).sum(1)
        d[~free] = np.inf
        slots[i] = np.argmin(d)
        free[slots[i]] = False
    pos[slots] = pts
    _, first = np.unique(pos, axis=0, return_index=True)
    assert len(first) == g["V"]  # (no two vertices at one place: every edge keeps a finite length)
    # re-triangulated, as the synthetic graphs are made: the patches of the two-half-edges form then fetch few enough foreign
    # records for it to apply (with the original edges kept, the moved vertices' neighbourhoods exceed that)
    out = synth.assemble_graph(pos, g["data_term"], synth.delaunay_edges_native(pos))
    return out, slots


def padded(img, pad, fill):
    """img as a row-strided view into a wider buffer whose padding bytes are `fill`."""
    rows, cols = img.shape
    buf = np.full((rows, cols + pad), fill, np.uint8)
    buf[:, :cols] = img
    return buf[:, :cols]


def image_pair(rows, cols, pad, seed):
    ref, cmp = asymmetric_texture(rows, cols, seed), noise_texture(rows, cols, seed + 1)
    if pad:
        ref, cmp = padded(ref, pad, 0xC3), padded(cmp, pad, 0x5A)
        assert ref.strides[0] == cols + pad and not ref.flags.c_contiguous
    return ref, cmp


def shift_geometry(sx, sy):
    """KRKinv = [[1, 0, sx], [0, 1, sy], [0, 0, 1]], Kt = 0: at idepth 0 the projection is u + (sx, sy), exactly."""
    return np.array([[1, 0, sx], [0, 1, sy], [0, 0, 1]], np.float32), np.zeros(3, np.float32)


SHIFT = (-3.0, 2.0)


def camera_geometry(rows, cols):
    return geometry32(camera(rows, cols), _rot_y(0.012) @ _rot_x(0.006), np.array([0.03, -0.02, 0.01]))


def _same(got, want, what):
    assert got.shape == want.shape, what
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), (what, np.flatnonzero(bad)[:8], got[bad][:8], want[bad][:8])


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,base", [(479, 641, "640x480"), (61, 97, "320x240")])
def test_gpu_sweep_edge_grid_bit_for_bit(built, rows, cols, base):
    """The stand-alone sweep and the canonical path's sweep against the checker, bit for bit, NaN pattern included: borders
    1, 2, 4 and wider than half the image, contiguous and padded rows, special x through upload_state, graph scales 1, 1.7,
    0 (every idepth 0: -0 and negative x times 0 too), 1e-30 (idepth near 0) and 1e30 (idepth overflows)."""
    import torch  # noqa: F401

    import flame_amd
    from flame_amd.regularizer import OPT_SOLVER

    big = max(rows, cols) // 2 + 1
    seen_finite = 0
    for border in (1, 2, 4, big):
        g, _ = edge_graph(rows, cols, min(border, 4), base, SHIFT, seed=31 + border)
        x = SPECIAL_X[np.arange(g["V"]) * 7 % len(SPECIAL_X)]
        with flame_amd.Regularizer(0) as reg:
            reg.upload_graph(g)
            reg.upload_state({"x": x})
            assert np.array_equal(reg.download_state(("x",))["x"].view(np.uint32), x.view(np.uint32))
            for pad in (0, 37):
                ref, cmp = image_pair(rows, cols, pad, seed=border * 10 + pad)
                reg.photo_set_images(ref, cmp)
                for gname, (KRKinv, Kt) in (("shift", shift_geometry(*SHIFT)), ("camera", camera_geometry(rows, cols))):
                    for gs in (1.0, 1.7, 0.0, 1e-30, 1e30):
                        want = oracle.photo_residual(g["pos"], x, gs, KRKinv, Kt, ref, cmp, border)
                        got = reg.photo_residual(KRKinv, Kt, graph_scale=gs, border=border)
                        _same(got, want, (rows, cols, border, pad, gname, gs))
                        if border == big:
                            assert np.isnan(got).all()
                        seen_finite += int(np.isfinite(got).sum())
                        if pad and gname == "shift" and gs == 0.0:  # a row addressed by cols instead of step reads the wrong bytes
                            dense = oracle.photo_residual(g["pos"], x, gs, KRKinv, Kt, np.ascontiguousarray(ref),
                                                          np.ascontiguousarray(cmp), border)
                            _same(got, dense, "padded rows read as the dense image")
            # the canonical 4-sweep path's appended sweep (k_photo_residual on the run's x)
            reg.set_option(OPT_SOLVER, 1)
            reg.upload_state({"x": np.abs(np.nan_to_num(x, nan=0.5, posinf=2.0, neginf=2.0)).clip(0, 10).astype(np.float32)})
            KRKinv, Kt = camera_geometry(rows, cols)
            reg.photo_fuse(KRKinv, Kt, graph_scale=1.3, border=border)
            reg.run(flame_amd.Params(), 3)
            assert reg.info()["last_run_path"] == 4
            xr = reg.download_state(("x",))["x"]
            _same(reg.photo_residual_last(), oracle.photo_residual(g["pos"], xr, 1.3, KRKinv, Kt, ref, cmp, border),
                  ("canonical", border))
    assert seen_finite > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 1, 3, 4, 6])
def test_gpu_fused_edge_grid_bit_for_bit(built, form):
    """The epilogue of every persistent form (and the per-step path's packed sweep, form 0) on the edge grid, bit for bit.
    data_weight is so large that every primal step lands x on data_term exactly: the run's final x is 0, -0, negative,
    small and large as placed (NaN / infinite x would stop the solver itself, the sweep test covers those)."""
    import torch  # noqa: F401

    import flame_amd

    rows, cols = 1079, 1921  # (a 1080p graph: every form applies to it, the two-half-edges one included)
    want_path = {0: (2, 3), 1: (5, 6, 7), 3: (5,), 4: (6,), 6: (7,)}[form]
    g, slots = edge_graph(rows, cols, 4, "1920x1080", SHIFT, seed=41)
    special = np.array([0.7, 0.0, -0.0, -0.3, 3.0, 1.5e-3, 0.25, 2.0e4, 1e-30], np.float32)
    data = g["data_term"].copy()
    data[slots] = special[np.arange(len(slots)) % len(special)]
    g = synth.assemble_graph(g["pos"], data, np.stack([g["src"], g["dst"]], 1), weight=np.full(g["V"], 1e30, np.float32))
    p = flame_amd.Params(x_min=-1e6, x_max=1e6)
    with flame_amd.Regularizer(0) as reg:
        reg.set_option(5, form)
        reg.upload_graph(g)
        for border, pad, gs, geo in ((4, 0, 1.0, "shift"), (1, 37, 0.0, "shift"), (2, 37, 1.7, "camera"), (4, 0, 1e-30, "camera"),
                                     (4, 37, 1e35, "camera"), (2, 0, 0.0, "camera")):
            ref, cmp = image_pair(rows, cols, pad, seed=border + pad)
            KRKinv, Kt = shift_geometry(*SHIFT) if geo == "shift" else camera_geometry(rows, cols)
            reg.photo_set_images(ref, cmp)
            reg.photo_fuse(KRKinv, Kt, graph_scale=gs, border=border)
            for n in (12, 7):
                reg.run(p, n)
                assert reg.info()["last_run_path"] in want_path, (form, reg.info()["last_run_path"])
                fused = reg.photo_residual_last()
                x = reg.download_state(("x",))["x"]
                assert np.array_equal(x[slots].view(np.uint32), data[slots].view(np.uint32))  # (the placed values, -0 included)
                want = oracle.photo_residual(g["pos"], x, gs, KRKinv, Kt, ref, cmp, border)
                _same(fused, want, (form, border, pad, gs, geo, n))
                if gs < 1e30:  # (at 1e35 every idepth overflows: each vertex projects to Kt's own point, outside the frame)
                    assert np.isfinite(want).sum() > 0.5 * g["V"]
                _same(reg.photo_residual(KRKinv, Kt, graph_scale=gs, border=border), want, ("sweep", form, border, pad, gs, geo))
        if form != 0:
            # on smooth images the epilogue also agrees with the float64 statement, within the CPU test's bounds
            K = camera(rows, cols)
            R, t = _rot_y(0.012) @ _rot_x(0.006), np.array([0.03, -0.02, 0.01])
            ref, cmp = smooth_texture(rows, cols, 8), smooth_texture(rows, cols, 9)
            reg.photo_set_images(ref, cmp)
            reg.photo_fuse(*geometry32(K, R, t), graph_scale=1.0, border=4)
            reg.run(p, 6)
            fused = reg.photo_residual_last()
            x = reg.download_state(("x",))["x"]
            err64, c64, z = r64.residual64(g["pos"], x, 1.0, K, R, t, ref, cmp, 4)
            bound, _ = coord_bound(K, R, t, g["pos"], x, 1.0, c64, z)
            both = np.isfinite(fused) & np.isfinite(err64)
            assert both.sum() > 0.8 * g["V"]
            tol = r64.local_range(cmp, c64[both, 0], c64[both, 1]) * bound[both].sum(1) + 64 * EPS32 * 255
            assert (np.abs(fused[both] - err64[both]) <= tol).all()


# ---- GPU: the standing target across changes ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", [1, 0])
def test_gpu_standing_target_follows_the_graph(built, form):
    """photo_residual_last equals the checker on the CURRENT pos, x, images and target after every change -- with a run behind
    it (the epilogue / the run's sweep) and without (the call's own sweep) --, its length is the current V, and it is an error
    without a standing target."""
    import torch  # noqa: F401

    import flame_amd
    from tests.test_graph_maintenance import quat_wxyz_from_rot

    rows, cols = 480, 640
    K = camera(rows, cols)
    K32, Kinv32 = K.astype(np.float32), np.linalg.inv(K).astype(np.float32)
    p = flame_amd.Params()
    g = synth.make_graph("640x480", seed=61)
    st = {"pos": g["pos"].copy(), "imgs": image_pair(rows, cols, 0, 3), "tgt": camera_geometry(rows, cols) + (1.1, 4)}

    def check(what, x=None):
        got = reg.photo_residual_last()
        assert len(got) == reg.V == len(st["pos"]), what
        x = reg.download_state(("x",))["x"] if x is None else x
        KRKinv, Kt, gs, border = st["tgt"]
        want = oracle.photo_residual(st["pos"], x, gs, KRKinv, Kt, *st["imgs"], border)
        _same(got, want, what)
        assert np.isfinite(want).sum() > 0.5 * reg.V, what

    def sync_to(pos, fid, what, prepared=False):
        rng = np.random.default_rng(len(pos))
        edges = synth.delaunay_edges_native(pos)
        args = (fid, pos, rng.uniform(0.3, 2.0, len(pos)).astype(np.float32), np.ones(len(pos), np.float32), edges)
        if prepared:
            reg.sync_prepare(*args)
            reg.run_async(p, 11)
            reg.run_async(p, 6)
            reg.sync_commit()
        else:
            reg.sync_graph(*args)
        st["pos"] = pos.copy()
        check(what + ", no run since")
        reg.run(p, 9)
        check(what + ", then a run")

    with flame_amd.Regularizer(0) as reg:
        reg.set_option(5, form)
        reg.upload_graph(g)
        reg.photo_set_images(*st["imgs"])
        with pytest.raises(flame_amd.NLTGV2Error):
            reg.photo_residual_last()  # no standing target
        reg.photo_fuse(*st["tgt"][:2], graph_scale=st["tgt"][2], border=st["tgt"][3])
        check("standing target, no run yet")
        reg.run(p, 30)
        check("after a run")
        # the stand-alone sweep with a target of its own: its answer is its target's, the standing one's is untouched
        other = geometry32(K, _rot_y(-0.02), np.array([0.05, 0.01, -0.03])) + (0.8, 7)
        x = reg.download_state(("x",))["x"]
        _same(reg.photo_residual(*other[:2], graph_scale=other[2], border=other[3]),
              oracle.photo_residual(st["pos"], x, other[2], other[0], other[1], *st["imgs"], other[3]), "stand-alone sweep")
        check("standing target after a stand-alone sweep of another one")
        reg.run(p, 5)
        reg.photo_residual(*other[:2], graph_scale=other[2], border=other[3])
        check("standing target after a run and a stand-alone sweep of another one")
        # projectGraph moves pos in place
        R, t = _rot_y(0.015), np.array([0.02, -0.01, 0.01], np.float32)
        KRKinv = (K32 @ R.astype(np.float32) @ Kinv32).astype(np.float32)
        _, st["pos"] = reg.project_graph(K32, Kinv32, KRKinv, quat_wxyz_from_rot(R), t, (8.0, 8.0, cols - 16.0, rows - 16.0), 1.1)
        check("project_graph, no run since")
        reg.run(p, 10)
        check("project_graph, then a run")
        reg.rescale_data(1.1, p)
        check("rescale_data, no run since")
        reg.run(p, 10)
        check("rescale_data, then a run")
        # syncGraph: grow, shrink, prepared beside rounds in flight
        V = reg.V
        rng = np.random.default_rng(5)
        extra = np.stack([rng.uniform(10, cols - 10, 600), rng.uniform(10, rows - 10, 600)], 1).astype(np.float32)
        sync_to(np.concatenate([st["pos"], extra]), np.arange(V + 600, dtype=np.int32), "sync_graph grows")
        assert reg.V == V + 600
        keep = np.sort(rng.permutation(reg.V)[: reg.V * 2 // 3])
        sync_to(st["pos"][keep], keep.astype(np.int32), "sync_graph shrinks")
        assert reg.V < V
        sync_to(np.concatenate([st["pos"], extra[:200] + 0.25]), np.arange(reg.V + 200, dtype=np.int32) + 5000,
                "sync_prepare / sync_commit beside rounds in flight", prepared=True)
        # a re-upload of another size
        g2 = synth.make_graph("320x240", seed=62)
        g2["pos"] = (g2["pos"] * 2).astype(np.float32)
        reg.upload_graph(g2)
        st["pos"] = g2["pos"]
        check("upload_graph of another V, no run since")
        reg.run(p, 8)
        check("upload_graph of another V, then a run")
        # new images while the target stands, rounds in flight
        reg.run_async(p, 20)
        reg.run_async(p, 9)
        st["imgs"] = image_pair(rows, cols, 21, 7)
        reg.photo_set_images(*st["imgs"])
        check("new (padded) images behind rounds in flight")
        reg.run(p, 5)
        check("new images, then a run")
        # a new target
        st["tgt"] = geometry32(K, _rot_x(0.01), np.array([-0.02, 0.03, 0.05])) + (0.9, 2)
        reg.photo_fuse(*st["tgt"][:2], graph_scale=st["tgt"][2], border=st["tgt"][3])
        check("photo_fuse again, no run since")
        reg.run(p, 6)
        check("photo_fuse again, then a run")
        # an open run: settled by photo_residual_last itself
        # an open run (the patch form's open instance carries the epilogue); where none applies (form 0), nothing is enqueued
        before = reg.iterations()
        opened = reg.run_open(p, 400000)
        assert opened == (form != 0)
        if not opened:
            assert reg.iterations() == before
        check("open run, settled by photo_residual_last" if opened else "open run declined: nothing ran")
        reg.run(p, 4)
        check("after the open run")
        reg.photo_fuse(enable=False)
        with pytest.raises(flame_amd.NLTGV2Error):
            reg.photo_residual_last()


def test_photo_set_images_keeps_row_strided_views(monkeypatch):
    """A view with contiguous rows goes to the C-ABI as it is (its strides[0] as the step); other layouts are copied."""
    import flame_amd
    from flame_amd import regularizer as regmod

    seen = []

    class FakeLib:
        def flame_nltgv2_photo_set_images(self, ctx, ref, cmp, rows, cols, step):
            seen.append((C.cast(ref, C.c_void_p).value, rows, cols, step))
            return 0

    import ctypes as C

    reg = object.__new__(flame_amd.Regularizer)
    reg._L, reg._ctx = FakeLib(), None
    img = padded(asymmetric_texture(30, 41, 1), 23, 7)
    reg.photo_set_images(img, padded(noise_texture(30, 41, 2), 23, 9))
    assert seen[-1] == (img.ctypes.data, 30, 41, 64)
    reg.photo_set_images(img[:, ::-1], img[:, ::-1])  # columns not contiguous: copied into dense rows
    assert seen[-1][1:] == (30, 41, 41) and seen[-1][0] != img.ctypes.data
    reg.photo_set_images(img, np.ascontiguousarray(img))  # different steps: both dense
    assert seen[-1][3] == 41
    assert regmod._rows_contiguous_u8(img) and not regmod._rows_contiguous_u8(img.T)
