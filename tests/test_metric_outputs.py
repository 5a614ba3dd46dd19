"""The metric outputs (include/flame_nltgv2.h, flame_nltgv2_metric_outputs_begin): known answers for the checker tests/metric_ref.py,
and the new symbols of the C-ABI.  No GPU here; the device is compared with the checker in tests/test_gpu_metric_outputs*.py."""
import ctypes as C
import os
import re

import numpy as np

from tests import metric_ref as xr
from tests.conftest import ROOT
from tests.metric_helpers import INF, F, pinhole_kinv, rot_z, special_map

NAN_BITS = 0x7FC00000


def test_depth_is_the_reciprocal_with_a_standard_kinv():
    rng = np.random.default_rng(3)
    v = rng.uniform(0.01, 4.0, (37, 29)).astype(F)
    out = xr.metric_points(v, pinhole_kinv())
    assert np.array_equal(xr.bits(out["depth"]), xr.bits(F(1) / v))
    assert out["n_points"] == v.size and np.array_equal(out["cloud_pixel"], np.arange(v.size, dtype=np.uint32))


def test_holes_are_exactly_nan_nonpositive_infinite_and_clipped():
    v = special_map()
    out = xr.metric_points(v, pinhole_kinv())
    with np.errstate(all="ignore"):
        z = F(1) / v
    expect_hole = np.isnan(v) | (v <= 0) | np.isinf(v) | np.isinf(z)
    hole = xr.bits(out["depth"]) == NAN_BITS
    assert np.array_equal(hole, expect_hole)
    assert not expect_hole[0, 5] and not expect_hole[0, 6] and expect_hole[0, 4]  # 6e-39 and 1e-30 are points, 1e-45 overflows
    assert (xr.bits(out["organized"])[hole] == NAN_BITS).all() and not np.isnan(out["organized"][~hole]).any()
    assert (out["depth_mm"][hole] == 0).all()
    # clipping: both bounds are exclusive
    v = np.array([[1.0, 0.5, 0.25, 0.125]], F)  # z = 1, 2, 4, 8
    out = xr.metric_points(v, pinhole_kinv(), min_depth=1.0, max_depth=8.0)
    assert np.array_equal(np.isnan(out["depth"]), [[True, False, False, True]])
    assert out["cloud_pixel"].tolist() == [1, 2] and out["n_points"] == 2
    out = xr.metric_points(v, pinhole_kinv(), min_depth=np.nan)
    assert out["n_points"] == 0  # a NaN bound: every comparison is false
    # the same on the map of special values, whose 0.5 and 2 lie exactly on the window (0.5, 2): only v = 1 is left in each row
    out = xr.metric_points(special_map(), pinhole_kinv(), min_depth=0.5, max_depth=2.0)
    assert out["n_points"] == 3 and (out["depth"][~np.isnan(out["depth"])] == 1.0).all()
    assert xr.metric_points(special_map(), pinhole_kinv(), min_depth=0.49, max_depth=2.01)["n_points"] == 9


def test_cloud_is_organized_at_cloud_pixel_in_ascending_order():
    rng = np.random.default_rng(5)
    for shape in ((1, 1), (1, 65), (3, 70), (80, 91)):  # (the last: the vectorised walk)
        v = rng.uniform(0.05, 3.0, shape).astype(F)
        v[rng.random(shape) < 0.5] = np.nan
        out = xr.metric_points(v, pinhole_kinv(), pose=rot_z(30))
        pix = out["cloud_pixel"].astype(np.int64)
        assert (np.diff(pix) > 0).all() and out["cloud"].shape == (out["n_points"], 3)
        assert np.array_equal(xr.bits(out["cloud"]), xr.bits(out["organized"].reshape(-1, 3)[pix]))
        # the plain row-major loop itself, also where metric_points takes the vectorised walk (80 x 91 is above LOOP_LIMIT)
        assert (v.size > xr.LOOP_LIMIT) == (shape == (80, 91))
        assert np.array_equal(out["cloud_pixel"], xr.valid_pixels_loop(~np.isnan(v).reshape(-1)))
    small = xr.metric_points(np.full((64, 64), 0.5, F), pinhole_kinv())  # 4096 pixels: the plain loop
    large = xr.metric_points(np.full((64, 65), 0.5, F), pinhole_kinv())
    assert small["n_points"] == 4096 and large["n_points"] == 4160


def test_identity_pose_gives_the_points_of_no_pose():
    rng = np.random.default_rng(7)
    v = rng.uniform(0.05, 3.0, (17, 23)).astype(F)
    v[::3, ::2] = 0
    eye = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(F)
    a, b = xr.metric_points(v, pinhole_kinv()), xr.metric_points(v, pinhole_kinv(), pose=eye)
    for k in ("organized", "cloud", "depth"):
        # (x + 0 * y + 0 * z + 0 == x for finite values; -0 cannot occur: z > 0 and the sums start from x itself)
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    moved = xr.metric_points(v, pinhole_kinv(), pose=rot_z(90, t=(0, 0, 0)))
    assert np.array_equal(xr.bits(moved["depth"]), xr.bits(a["depth"]))  # depth stays the camera-frame z
    ok = ~np.isnan(a["depth"])
    np.testing.assert_allclose(moved["organized"][ok][:, 0], -a["organized"][ok][:, 1], rtol=1e-6, atol=1e-6)


def mm_of(z):
    """depth_mm of a single pixel whose depth is exactly z: v = 1 and Kinv(2, 2) = z, so q.z = z and z / 1 = z."""
    out = xr.metric_points(np.ones((1, 1), F), np.diag([1, 1, z]).astype(F))
    assert out["depth"][0, 0] == F(z)
    return int(out["depth_mm"][0, 0])


def test_depth_mm_ties_go_to_even_and_saturate():
    # z * 1000.0f is exactly k + 0.5 in float: z = 2^-9 -> 1.953125 (no tie), z = 0.0625 -> 62.5, z = 0.1875 -> 187.5
    for z, prod, want in ((0.0625, 62.5, 62), (0.1875, 187.5, 188), (0.3125, 312.5, 312), (0.4375, 437.5, 438)):
        assert F(z) * F(1000.0) == F(prod)
        assert mm_of(z) == want
    assert mm_of(0.5) == 500 and mm_of(2.0) == 2000
    assert mm_of(2.0 ** -11) == 0   # 0.488 mm rounds to 0: below 1, not written
    assert mm_of(2.0 ** -10) == 1   # 0.977 mm
    assert mm_of(64.0) == 64000
    assert mm_of(128.0) == 0        # beyond 65.535 m
    # the edge itself: 65.535 m is the last depth with a value, the next float above 65.5355 m has none
    out = xr.metric_points(np.array([[1 / 65.535, 1 / 65.536, 1 / 65.5349]], np.float64).astype(F), np.eye(3, dtype=F))
    z = out["depth"][0]
    want = [int(m) if 1 <= m <= 65535 else 0 for m in np.rint(z * F(1000.0))]
    assert out["depth_mm"][0].tolist() == want and want[0] == 65535 and want[1] == 0 and want[2] == 65535


def test_mesh_checker_poses_vertices_and_normals_and_keeps_the_valid_triangles_in_order():
    pos = np.array([[10, 20], [30, 20], [10, 40], [30, 44]], F)
    x = np.array([0.5, 0.25, 1.0, 2.0], F)
    normals = np.array([[0, 0, -1], [1, 0, 0], [0, 1, 0], [0.6, 0.8, 0]], F)
    tris = np.array([[0, 1, 2], [1, 3, 2], [0, 3, 2]], np.int32)
    m = xr.metric_mesh(pos, x, 2.0, pinhole_kinv(), normals, tris, np.array([1, 0, 7], np.uint8))
    assert m["n_valid"] == 2 and m["mesh_triangles"].tolist() == [[0, 1, 2], [0, 3, 2]]
    assert np.array_equal(m["mesh_vertices"][:, 2], F(1) / (x * F(2)))
    assert np.array_equal(m["mesh_normals"], normals)
    r = xr.metric_mesh(pos, x, 2.0, pinhole_kinv(), normals, tris, np.zeros(3, np.uint8), pose=rot_z(90, t=(1, 2, 3)))
    assert r["n_valid"] == 0 and r["mesh_triangles"].shape == (0, 3)
    np.testing.assert_allclose(r["mesh_normals"][1], [0, 1, 0], atol=1e-6)
    np.testing.assert_allclose(r["mesh_vertices"][:, 2], m["mesh_vertices"][:, 2] + 3, rtol=1e-6)


def test_new_symbols_are_declared_and_exported_and_the_abi_version_stays(built):
    import flame_amd
    from flame_amd.regularizer import ABI_SYMBOLS

    names = ("flame_nltgv2_default_metric_params", "flame_nltgv2_metric_outputs_begin", "flame_nltgv2_metric_outputs_end",
             "flame_nltgv2_metric_outputs")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flame_nltgv2.h")).read(), flags=re.S)
    lib = flame_amd.load_library()
    for n in names:
        assert re.search(r"\b" + n + r"\s*\(", header), n
        assert n in ABI_SYMBOLS and hasattr(lib, n), n
    assert re.search(r"#define FLAME_NLTGV2_ABI_VERSION 7\b", header) and lib.flame_nltgv2_abi_version() == 7
    p = flame_amd.MetricParams(min_depth=3, max_depth=4, use_filtered_map=True, want_depth=False, want_depth_mm=False,
                               want_organized=False, want_cloud=False, want_mesh=True, copy_out=False, map_device=64)
    lib.flame_nltgv2_default_metric_params(C.byref(p))
    d = flame_amd.MetricParams()
    for name, _ in flame_amd.MetricParams._fields_:
        assert getattr(p, name) == getattr(d, name), name
    assert (p.min_depth, p.max_depth, p.want_mesh, p.copy_out, p.map_device) == (0.0, INF, 0, 1, None)
    # the view's layout is the header's: two int32 triples, eight (host, device) pointer pairs, one float
    from flame_amd.regularizer import _MetricOutputsView

    assert C.sizeof(flame_amd.MetricParams) == 48 and C.sizeof(_MetricOutputsView) == 24 + 16 * 8 + 8
