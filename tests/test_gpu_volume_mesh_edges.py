"""flame_nltgv2_volume_mesh_* at its edges, bit for bit against the checker tests/volume_mesh_ref.py: tsdf values of exactly 0.0f and -0.0f
on corners (zero-area triangles are kept), a NaN and two infinities that go through the arithmetic as they are; the checkerboard at its
twelve triangles per cube and a voxel that owns all seven vertices; one volume of 1120 workgroups, so that a thread of the scan takes
two totals; a proper sub-box, the tile pairs of tests/test_volume_mesh_ref.py along every axis, boxes of one layer."""
import numpy as np
import pytest

from tests import volume_mesh_ref as mr
from tests.test_gpu_volume_mesh import gpu, mesh, reg, uploaded  # noqa: F401  (the fixtures)

F = np.float32


@pytest.mark.gpu
def test_gpu_signed_zeros_on_corners_a_nan_and_an_infinity(gpu, reg):
    tsdf, weight = mr.random_signs(9, 6, 5, 21, 4)
    flat = tsdf.reshape(-1)
    flat[::7] = F(0.0)
    flat[3::11] = F(-0.0)
    tsdf[2, 3, 4] = np.nan
    tsdf[1, 1, 6] = np.inf
    tsdf[3, 4, 2] = -np.inf
    ref = uploaded(gpu, reg, tsdf, weight)
    got, want = mesh(gpu, reg, ref, "zeros and non-finite values")
    assert np.isnan(got["vertices"]).any() and np.isnan(want["vertices"]).any()
    with np.errstate(all="ignore"):
        v = want["vertices"].astype(np.float64)[want["triangles"]]
        area = np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1)
    assert np.count_nonzero(area == 0) > 0, "no zero-area triangle: the zeros are on no corner of a surface cube"


@pytest.mark.gpu
def test_gpu_the_checkerboard_has_twelve_triangles_per_cube(gpu, reg):
    ref = uploaded(gpu, reg, mr.checkerboard_tsdf(9, 9, 9))
    got, want = mesh(gpu, reg, ref, "the 9^3 checkerboard")
    assert got["live_cubes"] == got["surface_cubes"] == 512 and got["n_triangles"] == 12 * 512
    # a face diagonal joins two voxels of one colour: the three axis edges and the body diagonal of a voxel carry a vertex, four of the
    # seven it owns.  All seven at once need inside / outside to differ along every offset of E, which no two colours can do
    assert np.bincount(want["keys"] // 7).max() == 4
    # seven per voxel: the owner inside, its seven far ends outside
    tsdf = np.full((3, 3, 3), 0.5, F)
    tsdf[1, 1, 1] = F(-0.25)
    got, want = mesh(gpu, reg, uploaded(gpu, reg, tsdf), "one voxel inside")
    assert np.bincount(want["keys"] // 7).max() == 7


def large_volume():
    """70 x 64 x 64: 1120 workgroups of 256, so a thread of the scan sums two totals.  A tilted plane and a corner of random signs."""
    nx, ny, nz = 70, 64, 64
    k, j, i = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    tsdf = ((0.31 * i + 0.17 * j + 0.93 * k - 58.0) / 6.0).clip(-1, 1).astype(F)
    weight = np.ones((nz, ny, nx), F)
    rs, rw = mr.random_signs(70, 8, 8, 17, 300)
    tsdf[:8, :8, :] = rs
    weight[:8, :8, :] = rw
    return tsdf, weight


@pytest.mark.gpu
def test_gpu_a_volume_of_1120_workgroups(gpu, reg):
    tsdf, weight = large_volume()
    assert (tsdf.size + 255) // 256 == 1120 > 1024
    ref = uploaded(gpu, reg, tsdf, weight, voxel_size=0.05)
    got, want = mesh(gpu, reg, ref, "70x64x64")
    # the plane's part and the corner's part both have triangles, before and behind workgroup 1024
    cube_block = want["tri_cube"] // 256
    assert cube_block.min() < 8 and cube_block.max() > 1030 and got["n_triangles"] > 20000


# ---- boxes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_sub_boxes_tiles_and_a_box_of_one_layer(gpu, reg):
    tsdf, weight = mr.random_signs(70, 9, 8, 5, 60)
    ref = uploaded(gpu, reg, tsdf, weight)
    dims = (70, 9, 8)
    whole, _ = mesh(gpu, reg, ref, "the whole volume")
    sub, _ = mesh(gpu, reg, ref, "a proper sub-box", (3, 1, 2), (67, 8, 7))
    assert 0 < sub["n_triangles"] < whole["n_triangles"]
    for axis in range(3):
        (lo_a, hi_a), (lo_b, hi_b) = mr.tile_boxes(dims, axis, dims[axis] // 2)
        a, _ = mesh(gpu, reg, ref, "tile a along %d" % axis, lo_a, hi_a)
        b, _ = mesh(gpu, reg, ref, "tile b along %d" % axis, lo_b, hi_b)
        assert a["n_triangles"] + b["n_triangles"] == whole["n_triangles"] and a["n_triangles"] > 0 and b["n_triangles"] > 0
    for lo, hi in (((0, 4, 0), (70, 5, 8)), ((69, 0, 0), (70, 9, 8)), ((0, 0, 7), (70, 9, 8))):
        one, _ = mesh(gpu, reg, ref, "a box of one layer", lo, hi)
        assert [one[k] for k in mr.MESH_COUNTERS] == [0, 0, 0, 0, 0]
