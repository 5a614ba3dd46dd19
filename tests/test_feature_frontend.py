"""projectFeatures and detectFeatures on the resident feature set (include/flame_stereo.h): the C-ABI surface, the CPU
checker (tests/frontend_ref.py) against the pinned EpipolarGeometry pieces of oracle/, and -- on the GPU -- the HIP
stages bit-equal to the checker, alone and chained with updateFeatureIDepths from an empty set."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from flame_amd import synth_stereo as ss
from oracle import stereo_capi as so
from tests import frontend_ref as fr
from tests.conftest import HAS_GPU, ROOT

gpu = pytest.mark.gpu
PAD = 5
NEW_SYMBOLS = ("flame_stereo_default_detect_params", "flame_stereo_project_features", "flame_stereo_get_projected",
               "flame_stereo_projected_device", "flame_stereo_detect_features")


# ---- scenes ------------------------------------------------------------------------------------------------------

def plane_scene(w, h, seed=5):
    sc = ss.PlaneScene(w, h, seed=seed, normal=(0.2, -0.1, 1.0), distance=2.2)
    sc.add_camera(9, ss.rot([0, 1, 0], -0.004), [0.03, -0.002, 0.01])  # the frame before pose-frame 10
    sc.add_camera(10, np.eye(3), [0, 0, 0])
    for i, k in enumerate(range(11, 17)):
        a = 0.004 + 0.003 * i
        sc.add_camera(k, ss.rot([0.1, 1, 0.05], a), [-0.025 - 0.02 * i, 0.003 + 0.001 * i, -0.01 - 0.006 * i])
    return sc


def geometry(sc, a, b):
    return so.load_geometry(sc.K32, sc.Kinv32, *sc.relative(a, b))


def tie_ramp(w=160, h=96):
    """I = 2 (x mod 128): constant gx = 2 away from the wrap columns, gy = 0; with a pure x-translation the reference
    epiline is (+-1, 0), so every pixel of a cell without a wrap column scores the same."""
    x = np.arange(w)
    return np.tile((2 * (x % 128)).astype(np.uint8), (h, 1))


def true_map(sc, cam, holes=True):
    ys, xs = np.mgrid[0:sc.height, 0:sc.width]
    m = sc.true_idepth(cam, np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)).reshape(sc.height, sc.width)
    m = m.astype(np.float32)
    if holes:
        m[((xs // 13) + (ys // 11)) % 4 == 0] = np.nan
    return m


def checker_detect(sc, img, geo, ref_id, **kw):
    pad_img, gx, gy = so.make_frame(img, PAD)
    return fr.detect_features(gx, gy, PAD, img.shape[1], img.shape[0], geo, ref_id, dtype=so.FEATURE_DTYPE, **kw)


def assert_records_equal(a, b, what):
    a = np.ascontiguousarray(a).view(so.FEATURE_DTYPE)
    b = np.ascontiguousarray(b).view(so.FEATURE_DTYPE)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.tobytes() == b.tobytes():
        return
    for name in a.dtype.names:
        x, y = a[name], b[name]
        bad = np.nonzero(np.any((x != y).reshape(len(x), -1), axis=1) & ~np.all((x != x).reshape(len(x), -1)
                                                                                 & (y != y).reshape(len(y), -1), axis=1))[0]
        if bad.size:
            i = int(bad[0])
            raise AssertionError("%s: %s differs on %d records, first %d: %r vs %r" % (what, name, bad.size, i, a[i], b[i]))
    raise AssertionError("%s: bytes differ" % what)


# ---- CPU: the C-ABI surface ---------------------------------------------------------------------------------------

def test_new_symbols_are_exported_and_listed(built):
    import flame_amd
    from flame_amd.stereo import STEREO_ABI_SYMBOLS

    nm = subprocess.check_output(["nm", "-D", "--defined-only", flame_amd.library_path()], text=True)
    for name in NEW_SYMBOLS:
        assert name in STEREO_ABI_SYMBOLS, name
        assert (" T %s\n" % name) in nm, name
    hdr = open(os.path.join(ROOT, "include", "flame_stereo.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in hdr, name


def test_null_context_is_invalid_arg(built):
    from flame_amd.stereo import DetectParams, StereoParams, _FeatureStats, _lib

    L = _lib()
    p, dp, st = StereoParams(), DetectParams(), _FeatureStats()
    q = (C.c_float * 4)(1, 0, 0, 0)
    t = (C.c_float * 3)(0.1, 0, 0)
    assert L.flame_stereo_project_features(None, C.byref(p), 1, 0, None, C.byref(st)) == -1
    assert L.flame_stereo_detect_features(None, C.byref(p), C.byref(dp), 1, q, t, None, None, 0, None, 0, C.byref(st)) == -1
    n = C.c_int(0)
    assert L.flame_stereo_get_projected(None, 0, None, C.byref(n)) == -1
    assert L.flame_stereo_projected_device(None, None, C.byref(n)) == -1


def test_default_detect_params_are_the_references(built):
    from flame_amd.stereo import DetectParams

    d = DetectParams()
    # params.h:39, 48, 60, 61
    assert (d.detection_win_size, d.min_grad_mag, d.idepth_init, d.idepth_var_init) == \
        (16, np.float32(5.0), np.float32(0.01), np.float32(0.25))


def test_new_structs_are_plain_c99(built, tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "flame_stereo.h"\n'
                   'int main(void) { flame_stereo_detect_params d; flame_stereo_feature_stats s;\n'
                   '  flame_stereo_default_detect_params(&d); s.num_features = 0;\n'
                   '  return (int)sizeof d - 16 + (int)sizeof s - 12 + s.num_features; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                           str(src), "-o", str(tmp_path / "t.o")])


# ---- CPU: the checker checks itself -------------------------------------------------------------------------------

def test_checker_border_is_float_arithmetic():
    assert fr.border_of(1.4, 5) == 4  # 1.4f * 5 / 2 + 1 = 4.5 in float
    assert fr.border_of(2.0, 5) == 6


def test_checker_epiline_is_bit_equal_to_the_oracle():
    sc = plane_scene(320, 240)
    rng = np.random.default_rng(3)
    for a, b in ((10, 9), (13, 12), (10, 16)):
        geo = geometry(sc, a, b)
        ii = rng.integers(0, 240, 5000).astype(np.float32)
        jj = rng.integers(0, 320, 5000).astype(np.float32)
        ex, ey, ok = fr.reference_epiline(geo, ii, jj)  # (row, col) as (x, y), as detectFeatures passes them
        assert ok.all()
        for k in range(ii.size):
            rx, ry = so.reference_epiline(geo, float(ii[k]), float(jj[k]))
            assert (ex[k], ey[k]) == (rx, ry), (k, ii[k], jj[k])


def test_checker_projection_is_bit_equal_to_the_oracle():
    sc = plane_scene(320, 240)
    rng = np.random.default_rng(4)
    geo = geometry(sc, 10, 14)
    x = rng.uniform(-20, 340, 4000).astype(np.float32)
    y = rng.uniform(-20, 260, 4000).astype(np.float32)
    d = rng.uniform(0, 2, 4000).astype(np.float32)
    d[::97] = 0.0
    d[1::89] = 1e-7
    px, py, pd, ok = fr.project_idepth(geo, x, y, d)
    assert ok.all()
    for k in range(x.size):
        assert (px[k], py[k], pd[k]) == so.project_idepth(geo, float(x[k]), float(y[k]), float(d[k])), k
    _, _, _, ok = fr.project_idepth(geo, np.float32([5, 5]), np.float32([5, 5]), np.float32([-0.1, np.nan]))
    assert not ok.any()


def test_checker_ties_go_to_the_last_pixel():
    img = tie_ramp()
    h, w = img.shape
    K, Kinv = ss.intrinsics(w, h)
    geo = so.load_geometry(K, Kinv, [1, 0, 0, 0], [0.1, 0, 0])
    pad_img, gx, gy = so.make_frame(img, PAD)
    rc, _, out, _ = fr.detect_features(gx, gy, PAD, w, h, geo, 3, win=16, min_grad_mag=1.0, dtype=so.FEATURE_DTYPE)
    assert rc == 0
    lit = fr.detect_scan_literal(gx, gy, PAD, w, h, geo, 16, 1.0, fr.border_of(1.4, 5))
    got = {(int(y) // 16, int(x) // 16): (int(x), int(y)) for x, y in zip(out["x"], out["y"])}
    assert got == lit
    # a cell without a wrap column (x = 127, 128): every pixel ties, and the last one in row-major order wins
    assert got[(2, 2)] == (47, 47) and got[(1, 3)] == (63, 31)
    assert got[(0, 0)] == (15, 15)


def test_checker_swap_matters_with_forward_motion():
    """detectFeatures passes (row, col) to referenceEpiline; with t_z != 0 that changes which pixel wins."""
    sc = plane_scene(320, 240)
    img = sc.render(10)
    pad_img, gx, gy = so.make_frame(img, PAD)
    geo = so.load_geometry(sc.K32, sc.Kinv32, [1, 0, 0, 0], [0.02, 0.01, 0.08])
    rc, _, out, _ = fr.detect_features(gx, gy, PAD, 320, 240, geo, 10, dtype=so.FEATURE_DTYPE)
    assert rc == 0
    lit = fr.detect_scan_literal(gx, gy, PAD, 320, 240, geo, 16, 5.0, 4)
    assert {(int(y) // 16, int(x) // 16): (int(x), int(y)) for x, y in zip(out["x"], out["y"])} == lit
    # without the swap other pixels win
    rc2, _, out2, _ = fr.detect_features(gx, gy, PAD, 320, 240, geo, 10, dtype=so.FEATURE_DTYPE, swap=False)
    assert rc2 == 0 and out2.tobytes() != out.tobytes()


# ---- the chain from nothing: detect -> update -> project -> detect with a mask and a map ---------------------------

class CheckerSide:
    def __init__(self, sc, imgs):
        self.sc, self.imgs = sc, imgs
        self.frames = {}
        self.feats = np.zeros(0, so.FEATURE_DTYPE)
        self.proj = np.zeros(0, so.FEATURE_DTYPE)

    def add_frame(self, k):
        self.frames[k] = so.make_frame(self.imgs[k], PAD)

    def detect(self, ref, prev, idepthmap, use_mask, first_id):
        pad_img, gx, gy = self.frames[ref]
        mask = np.stack([self.proj["x"], self.proj["y"]], 1) if use_mask else None
        rc, _, new, _ = fr.detect_features(gx, gy, PAD, self.sc.width, self.sc.height, geometry(self.sc, ref, prev), ref,
                                           idepthmap=idepthmap, mask_xy=mask, first_id=first_id, dtype=so.FEATURE_DTYPE)
        assert rc == 0
        self.feats = np.concatenate([self.feats, new])
        return new.shape[0]

    def update(self, k, curr_pf, anchors):
        frs = [dict(p, img_pad=self.frames[p["id"]][0]) for p in ss.poses_for(self.sc, anchors, k, curr_pf)]
        rc, st = so.update_feature_idepths(so.Params(), self.sc.K32, self.sc.Kinv32, self.sc.width, self.sc.height, PAD,
                                           frs, self.frames[k], curr_pf, self.feats)
        assert rc == 0
        return [int(v) for v in st[:7]]

    def project(self, k, anchors):
        rc, _, kept, cur = fr.project_features(self.feats, {a: geometry(self.sc, a, k) for a in anchors}, k,
                                               self.sc.width, self.sc.height)
        assert rc == 0
        self.feats, self.proj = kept, cur
        return kept.shape[0]

    def state(self):
        return self.feats, self.proj


class HipSide:
    def __init__(self, sc, imgs):
        import torch

        from flame_amd.stereo import DetectParams, FeatureTracker, StereoParams

        self.torch = torch
        self.sc, self.imgs = sc, imgs
        self.tr = FeatureTracker(sc.K32, sc.Kinv32, sc.width, sc.height, border=PAD)
        self.sp, self.dp = StereoParams(), DetectParams()

    def add_frame(self, k):
        self.tr.add_frame(k, self.imgs[k])

    def detect(self, ref, prev, idepthmap, use_mask, first_id):
        q, t = self.sc.relative(ref, prev)
        dmap = None
        if idepthmap is not None:  # the map lives on the device, as the rasteriser's would
            dmap = self.torch.from_numpy(np.ascontiguousarray(idepthmap)).cuda()
            self.torch.cuda.synchronize()
        n = self.tr.detect_features(self.sp, self.dp, ref, q, t, idepthmap=None if dmap is None else dmap.data_ptr(),
                                    mask_xy="projected" if use_mask else None, first_id=first_id)
        del dmap
        return n

    def update(self, k, curr_pf, anchors):
        _, st = self.tr.update_resident(self.sp, k, curr_pf, ss.poses_for(self.sc, anchors, k, curr_pf))
        return [st[n] for n in ("num_idepth_updates", "num_fail_max_var", "num_fail_max_dropouts", "num_fail_ref_patch_grad",
                                "num_fail_ambiguous_match", "num_fail_max_cost", "success")]

    def project(self, k, anchors):
        return self.tr.project_features(self.sp, k, [dict(id=a, q_to_new=self.sc.relative(a, k)[0],
                                                          t_to_new=self.sc.relative(a, k)[1]) for a in anchors])

    def state(self):
        return self.tr.get_features(), self.tr.get_projected()

    def close(self):
        self.tr.close()


def drive_chain(sides, sc):
    """Pose-frame 10 (detected with no map), frames 11-16 (update, project), pose-frame 13 (detected after its
    projection, with the projected set as mask and the true inverse depth with holes as map)."""
    for s in sides:
        for k in (9, 10):
            s.add_frame(k)

    def same(what):
        st = [s.state() for s in sides]
        for other in st[1:]:
            assert_records_equal(other[0], st[0][0], what + ": resident set")
            assert_records_equal(other[1], st[0][1], what + ": projected set")

    counts = [s.detect(10, 9, None, False, 0) for s in sides]
    assert len(set(counts)) == 1 and counts[0] > 100, counts
    same("detect pf 10")
    next_id, anchors, curr_pf = counts[0], [10], 10
    for k in range(11, 17):
        for s in sides:
            s.add_frame(k)
        stats = [s.update(k, curr_pf, anchors) for s in sides]
        assert all(x == stats[0] for x in stats), (k, stats)
        same("frame %d update" % k)
        kept = [s.project(k, anchors) for s in sides]
        assert len(set(kept)) == 1, (k, kept)
        same("frame %d project" % k)
        if k == 13:
            m = true_map(sc, 13)
            counts = [s.detect(13, 12, m, True, next_id) for s in sides]
            assert len(set(counts)) == 1 and counts[0] > 0, counts
            same("detect pf 13")
            next_id += counts[0]
            anchors, curr_pf = [10, 13], 13
    feats = sides[0].state()[0]
    return feats, next_id


def converged_error(sc, feats):
    f = feats[(feats["valid"] == 1) & (feats["num_updates"] >= 2)]
    truth = np.concatenate([sc.true_idepth(int(a), np.stack([f["x"], f["y"]], 1)[f["frame_id"] == a])
                            for a in np.unique(f["frame_id"])])
    mu = np.concatenate([f["idepth_mu"][f["frame_id"] == a] for a in np.unique(f["frame_id"])])
    return f.shape[0], float(np.median(np.abs(mu - truth) / truth))


MEDIAN_REL_ERR = 0.05  # median |idepth - truth| / truth of the features with >= 2 updates


@pytest.mark.parametrize("size", [(320, 240)])
def test_checker_chain_recovers_the_plane(size):
    """CPU only: the chained checkers (detect from nothing, update, project, detect again) converge on the plane."""
    sc = plane_scene(*size)
    imgs = {c: sc.render(c) for c in sc.cams}
    feats, _ = drive_chain([CheckerSide(sc, imgs)], sc)
    n, err = converged_error(sc, feats)
    assert n > 100 and err < MEDIAN_REL_ERR, (n, err)


# ---- GPU: bit-equal to the checker ------------------------------------------------------------------------------

def _tracker(sc_or_shape, K=None, Kinv=None):
    from flame_amd.stereo import FeatureTracker

    if K is None:
        return FeatureTracker(sc_or_shape.K32, sc_or_shape.Kinv32, sc_or_shape.width, sc_or_shape.height, border=PAD)
    h, w = sc_or_shape
    return FeatureTracker(K, Kinv, w, h, border=PAD)


def _gpu_detect(tr, img, ref, q, t, sp=None, dp=None, **kw):
    from flame_amd.stereo import DetectParams, StereoParams

    tr.add_frame(ref, img)
    return tr.detect_features(sp or StereoParams(), dp or DetectParams(), ref, q, t, **kw)


@gpu
@pytest.mark.parametrize("size", [(320, 240), (640, 480), (1920, 1080)])
@pytest.mark.parametrize("win", [16, 10, 24, 7])
@pytest.mark.parametrize("letterbox", [0, 1])
def test_gpu_detect_matches_checker(built, size, win, letterbox):
    from flame_amd.stereo import DetectParams, StereoParams

    sc = plane_scene(*size)
    img = sc.render(10)
    q, t = sc.relative(10, 9)
    rc, _, ref_out, ncells = checker_detect(sc, img, geometry(sc, 10, 9), 10, win=win, do_letterbox=bool(letterbox), first_id=7)
    assert rc == 0 and ref_out.shape[0] > 0
    with _tracker(sc) as tr:
        n = _gpu_detect(tr, img, 10, q, t, StereoParams(do_letterbox=letterbox), DetectParams(detection_win_size=win),
                        first_id=7)
        assert n == ref_out.shape[0]
        assert_records_equal(tr.get_features(), ref_out, "detect %r win %d letterbox %d" % (size, win, letterbox))
        rc, st = tr.detect_features(StereoParams(do_letterbox=letterbox), DetectParams(detection_win_size=win), 10, q, t,
                                    first_id=0, raise_on_error=False)
        assert rc == 0 and st["num_examined"] == ncells and st["error_feature"] == -1


@gpu
@pytest.mark.parametrize("maps", ["none", "host", "device"])
@pytest.mark.parametrize("mask", ["none", "host", "projected"])
def test_gpu_detect_masks_and_maps(built, maps, mask):
    import torch

    sc = plane_scene(640, 480)
    img = sc.render(13)
    q, t = sc.relative(13, 12)
    m = true_map(sc, 13)
    with _tracker(sc) as tr:
        from flame_amd.stereo import StereoParams

        # a resident prefix from an earlier pose-frame, projected into 13: the projected set is a real mask
        tr.add_frame(10, sc.render(10))
        base = ss.make_features(sc, so.FEATURE_DTYPE, [10], 600, 3).view(tr.get_features().dtype)
        tr.set_features(base)
        tr.project_features(StereoParams(), 13, [dict(id=10, q_to_new=sc.relative(10, 13)[0], t_to_new=sc.relative(10, 13)[1])])
        prefix, proj = tr.get_features(), tr.get_projected()
        assert proj.shape[0] > 400
        mask_pts = None
        if mask == "host":
            rng = np.random.default_rng(1)
            mask_pts = np.stack([rng.uniform(0, 639.9, 300), rng.uniform(0, 479.9, 300)], 1).astype(np.float32)
        elif mask == "projected":
            mask_pts = np.stack([proj["x"], proj["y"]], 1)
        rc, _, ref_out, _ = checker_detect(sc, img, geometry(sc, 13, 12), 13, idepthmap=None if maps == "none" else m,
                                           mask_xy=mask_pts, first_id=1000)
        arg_map = None
        if maps == "host":
            arg_map = m
        elif maps == "device":
            dm = torch.from_numpy(m).cuda()
            torch.cuda.synchronize()
            arg_map = dm.data_ptr()
        n = _gpu_detect(tr, img, 13, q, t, idepthmap=arg_map,
                        mask_xy="projected" if mask == "projected" else mask_pts, first_id=1000)
        out = tr.get_features()
        assert n == ref_out.shape[0] and out.shape[0] == prefix.shape[0] + n
        assert out[:prefix.shape[0]].tobytes() == prefix.tobytes()  # the resident prefix is untouched
        assert_records_equal(out[prefix.shape[0]:], ref_out, "detect maps=%s mask=%s" % (maps, mask))
        assert np.array_equal(out["id"][prefix.shape[0]:], np.arange(1000, 1000 + n))
        if maps != "none":
            assert (out["idepth_mu"][prefix.shape[0]:] != np.float32(0.01)).any()


@gpu
def test_gpu_detect_zero_grad_threshold_and_tie_ramp(built):
    from flame_amd.stereo import DetectParams, StereoParams

    sc = plane_scene(320, 240)
    img = sc.render(10)
    q, t = sc.relative(10, 9)
    rc, _, ref_out, _ = checker_detect(sc, img, geometry(sc, 10, 9), 10, min_grad_mag=0.0)
    with _tracker(sc) as tr:
        n = _gpu_detect(tr, img, 10, q, t, dp=DetectParams(min_grad_mag=0.0))
        assert_records_equal(tr.get_features(), ref_out, "min_grad_mag 0")
    # flat image: every score is 0, no cell is emitted
    flat = np.full((240, 320), 77, np.uint8)
    with _tracker(sc) as tr:
        assert _gpu_detect(tr, flat, 10, q, t, dp=DetectParams(min_grad_mag=0.0)) == 0
    img = tie_ramp()
    h, w = img.shape
    K, Kinv = ss.intrinsics(w, h)
    geo = so.load_geometry(K, Kinv, [1, 0, 0, 0], [0.1, 0, 0])
    pad_img, gx, gy = so.make_frame(img, PAD)
    rc, _, ref_out, _ = fr.detect_features(gx, gy, PAD, w, h, geo, 3, win=16, min_grad_mag=1.0, dtype=so.FEATURE_DTYPE)
    with _tracker((h, w), K, Kinv) as tr:
        n = _gpu_detect(tr, img, 3, [1, 0, 0, 0], [0.1, 0, 0], dp=DetectParams(min_grad_mag=1.0))
        assert n == ref_out.shape[0]
        assert_records_equal(tr.get_features(), ref_out, "tie ramp")


@gpu
def test_gpu_detect_forward_motion_swap(built):
    sc = plane_scene(320, 240)
    img = sc.render(10)
    q, t = np.float32([1, 0, 0, 0]), np.float32([0.02, 0.01, 0.08])
    rc, _, ref_out, _ = checker_detect(sc, img, so.load_geometry(sc.K32, sc.Kinv32, q, t), 10)
    with _tracker(sc) as tr:
        _gpu_detect(tr, img, 10, q, t)
        assert_records_equal(tr.get_features(), ref_out, "t_z != 0")


@gpu
def test_gpu_detect_errors_leave_the_set_unchanged(built):
    from flame_amd.stereo import DetectParams, StereoParams

    sc = plane_scene(320, 240)
    img = sc.render(10)
    base = ss.make_features(sc, so.FEATURE_DTYPE, [10], 100, 2)
    with _tracker(sc) as tr:
        tr.add_frame(10, img)
        tr.set_features(base.view(tr.get_features().dtype))
        rc, st = tr.detect_features(StereoParams(), DetectParams(), 10, [1, 0, 0, 0], [0, 0, 0], raise_on_error=False)
        assert rc == -8 and st["num_features"] == 0 and st["error_feature"] >= 0  # FLAME_NLTGV2_ERR_ASSERT
        geo = so.load_geometry(sc.K32, sc.Kinv32, [1, 0, 0, 0], [0, 0, 0])
        rc_c, px, _, _ = checker_detect(sc, img, geo, 10)
        assert rc_c == -8 and st["error_feature"] == px
        assert tr.get_features().tobytes() == base.tobytes()
        rc, _ = tr.detect_features(StereoParams(), DetectParams(), 10, [1, 0, 0, 0], [0.1, 0, 0],
                                   mask_xy=np.float32([[5, 5], [320, 5]]), raise_on_error=False)
        assert rc == -1  # a host mask point outside the image
        rc, _ = tr.detect_features(StereoParams(), DetectParams(), 99, [1, 0, 0, 0], [0.1, 0, 0], raise_on_error=False)
        assert rc == -1  # not a resident frame
        assert tr.get_features().tobytes() == base.tobytes()


def _project_case(sc):
    """Features in pose-frames 10, 11 and 12, some invalid, some leaving the image on each side or going behind the
    camera, some with idepth_mu below 1e-6 and exactly 0."""
    feats = ss.make_features(sc, so.FEATURE_DTYPE, [10, 11, 12], 700, 9, border=0)
    rng = np.random.default_rng(2)
    n = feats.shape[0]
    feats["valid"][rng.random(n) < 0.1] = 0
    feats["num_updates"] = rng.integers(0, 9, n)
    feats["num_dropouts"] = rng.integers(0, 3, n)
    feats["search_status"] = rng.integers(0, 4, n)
    feats["x"][:40] = np.linspace(-3, 6, 40)           # off the left side
    feats["x"][40:80] = sc.width - np.linspace(-2, 7, 40)  # off the right side
    feats["y"][80:120] = np.linspace(-3, 6, 40)        # top
    feats["y"][120:160] = sc.height - np.linspace(-2, 7, 40)  # bottom
    feats["idepth_mu"][160:170] = 0.0
    feats["idepth_mu"][170:180] = 5e-7
    feats["idepth_mu"][180:190] = 60.0                 # in front of the reference, behind the current camera
    feats["idepth_var"][160:190] = 0.3
    return feats


def _poses_to(sc, anchors, k):
    return [dict(id=a, q_to_new=sc.relative(a, k)[0], t_to_new=sc.relative(a, k)[1]) for a in anchors]


@gpu
@pytest.mark.parametrize("letterbox", [0, 1])
def test_gpu_project_matches_checker(built, letterbox):
    from flame_amd.stereo import StereoParams

    sc = plane_scene(640, 480)
    feats = _project_case(sc)
    geos = {a: geometry(sc, a, 14) for a in (10, 11, 12)}
    rc, _, kept, cur = fr.project_features(feats, geos, 14, 640, 480, do_letterbox=bool(letterbox))
    assert rc == 0 and 0 < kept.shape[0] < (feats["valid"] == 1).sum()
    if not letterbox:  # (the letterbox drops the top rows, where the zero and tiny inverse depths are)
        assert (cur["idepth_mu"] == 0).any() and (kept["idepth_mu"] < 1e-6).sum() >= 10
    with _tracker(sc) as tr:
        tr.set_features(feats.view(tr.get_features().dtype))
        n = tr.project_features(StereoParams(do_letterbox=letterbox), 14, _poses_to(sc, (10, 11, 12), 14))
        assert n == kept.shape[0]
        assert_records_equal(tr.get_features(), kept, "project: resident set")
        assert_records_equal(tr.get_projected(), cur, "project: projected set")
        p, m = tr.projected_device()
        assert p and m == n
        # projecting again into the same frame keeps everything that is still inside, in order
        n2 = tr.project_features(StereoParams(do_letterbox=letterbox), 14, _poses_to(sc, (10, 11, 12), 14))
        rc, _, kept2, cur2 = fr.project_features(kept, geos, 14, 640, 480, do_letterbox=bool(letterbox))
        assert n2 == kept2.shape[0]
        assert_records_equal(tr.get_features(), kept2, "project twice: resident set")
        assert_records_equal(tr.get_projected(), cur2, "project twice: projected set")


@gpu
def test_gpu_project_errors(built):
    from flame_amd.stereo import StereoParams

    sc = plane_scene(320, 240)
    feats = _project_case(sc)
    poses = _poses_to(sc, (10, 11, 12), 14)
    with _tracker(sc) as tr:
        bad = feats.copy()
        bad["idepth_mu"][[500, 900, 1300]] = -0.5
        bad["valid"][[500, 900, 1300]] = [0, 1, 1]
        tr.set_features(bad.view(tr.get_features().dtype))
        before = tr.get_features()
        rc, st = tr.project_features(StereoParams(), 14, poses, raise_on_error=False)
        assert rc == -8 and st["error_feature"] == 900  # the lowest VALID feature with a negative idepth
        assert fr.project_features(bad, {a: geometry(sc, a, 14) for a in (10, 11, 12)}, 14, 320, 240)[:2] == (-8, 900)
        assert tr.get_features().tobytes() == before.tobytes() and tr.get_projected().shape[0] == 0
        unknown = feats.copy()
        unknown["frame_id"][700] = 42
        unknown["valid"][700] = 0  # pfs.at() comes before the valid test
        tr.set_features(unknown.view(tr.get_features().dtype))
        rc, st = tr.project_features(StereoParams(), 14, poses, raise_on_error=False)
        assert rc == -1 and st["error_feature"] == 700
        assert tr.get_features().tobytes() == unknown.tobytes()


@gpu
@pytest.mark.parametrize("size", [(320, 240), (640, 480)])
def test_gpu_chain_from_nothing_matches_checker(built, size):
    sc = plane_scene(*size)
    imgs = {c: sc.render(c) for c in sc.cams}
    hip = HipSide(sc, imgs)
    try:
        feats, next_id = drive_chain([CheckerSide(sc, imgs), hip], sc)
    finally:
        hip.close()
    n, err = converged_error(sc, feats)
    assert n > 100 and err < MEDIAN_REL_ERR, (n, err)


def _build_cpp(tmp_path):
    exe = str(tmp_path / "feature_frontend_test")
    lib_dir = os.path.join(ROOT, "flame_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-Wno-invalid-offsetof", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "feature_frontend_test.cc"), "-o", exe,
        "-L", lib_dir, "-lflame_nltgv2_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_frontend_binding_compiles(built, tmp_path):
    exe = _build_cpp(tmp_path)
    if not HAS_GPU:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no usable HIP device" in r.stdout, r.stdout + r.stderr


@gpu
def test_cpp_frontend_binding_end_to_end(built, tmp_path):
    r = subprocess.run([_build_cpp(tmp_path)], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.count(" ok") >= 3, r.stdout + r.stderr
