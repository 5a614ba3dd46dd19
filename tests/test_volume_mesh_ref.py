"""The volume's surface extraction (include/flame_nltgv2.h, flame_nltgv2_volume_mesh_begin): the checker tests/volume_mesh_ref.py against
properties that are integer or combinatorial -- a sphere is a closed, outward-facing surface of genus 0; random signs with unobserved
voxels give a manifold-with-boundary mesh from live cubes only; a checkerboard reaches the twelve triangles per cube that the int32 bound
assumes; two boxes that overlap by one voxel layer tile an extraction -- the generated table against the committed header, and the
stand-alone layout program.  No GPU here; the device is compared with the checker in tests/test_gpu_volume_mesh*.py."""
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

from tests import volume_mesh_ref as mr
from tests import volume_ref as vr
from tests.conftest import ROOT

F = np.float32


def volume(nx, ny, nz, tsdf=None, weight=None, voxel_size=0.1, origin=(-0.3, 0.2, 0.5)):
    v = vr.Volume(nx, ny, nz, voxel_size, origin, 0.3, 2.0)
    if tsdf is not None:
        v.tsdf = np.ascontiguousarray(tsdf, F)
    v.weight = np.ones((nz, ny, nx), F) if weight is None else np.ascontiguousarray(weight, F)
    return v


def directed_edges(triangles):
    t = np.asarray(triangles, np.int64)
    return Counter(zip(np.concatenate([t[:, 0], t[:, 1], t[:, 2]]).tolist(), np.concatenate([t[:, 1], t[:, 2], t[:, 0]]).tolist()))


def face_normals(m):
    v, t = m["vertices"].astype(np.float64), m["triangles"]
    return np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])


def sphere():
    return volume(14, 14, 14, mr.sphere_tsdf(14, 14, 14, (6.3, 6.6, 6.4), 4.7), voxel_size=1.0, origin=(0, 0, 0))


def test_a_sphere_is_closed_of_genus_zero_and_faces_outwards():
    v = sphere()
    m = mr.extract(v)
    edges = directed_edges(m["triangles"])
    assert m["n_triangles"] > 0 and max(edges.values()) == 1
    assert all((b, a) in edges for a, b in edges), "a directed edge without its reverse"
    V, Eu, Fc = m["n_vertices"], len(edges) // 2, m["n_triangles"]
    print("sphere: V - E + F = %d - %d + %d" % (V, Eu, Fc))
    assert V - Eu + Fc == 2
    fn = face_normals(m)
    t = m["triangles"]
    centroid = m["vertices"].astype(np.float64)[t].mean(axis=1)
    assert np.all(np.einsum("ij,ij->i", fn, centroid - np.array([6.3, 6.6, 6.4])) > 0)
    for c in range(3):
        assert np.all(np.einsum("ij,ij->i", fn, m["normals"].astype(np.float64)[t[:, c]]) > 0)
    assert m["live_cubes"] == 13 ** 3 and 0 < m["surface_cubes"] < m["live_cubes"] and m["overflow"] == 0
    assert np.all(np.diff(m["keys"]) > 0)


def test_random_signs_with_unobserved_voxels():
    tsdf, weight = mr.random_signs(6, 7, 8, 11, 9)
    v = volume(6, 7, 8, tsdf, weight)
    m = mr.extract(v)
    assert m["n_triangles"] > 0 and 0 < m["live_cubes"] < 5 * 6 * 7
    assert max(directed_edges(m["triangles"]).values()) == 1
    assert np.array_equal(np.unique(m["triangles"]), np.arange(m["n_vertices"]))
    live = set(m["cube_lin"][m["live"]].tolist())
    assert set(m["tri_cube"].tolist()) <= live
    assert np.all(np.diff(m["tri_cube"]) >= 0)


def test_a_checkerboard_has_twelve_triangles_per_cube():
    v = volume(5, 5, 5, mr.checkerboard_tsdf(5, 5, 5))
    m = mr.extract(v)
    assert m["live_cubes"] == m["surface_cubes"] == 64 and m["n_triangles"] == 12 * 64
    assert np.all(np.bincount(np.unique(m["tri_cube"], return_inverse=True)[1]) == 12)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_two_boxes_that_overlap_by_one_layer_tile_the_extraction(axis):
    tsdf, weight = mr.random_signs(6, 7, 8, 5, 7)
    v = volume(6, 7, 8, tsdf, weight)
    whole = mr.extract(v)
    dims = (6, 7, 8)
    (lo_a, hi_a), (lo_b, hi_b) = mr.tile_boxes(dims, axis, dims[axis] // 2)
    a, b = mr.extract(v, lo_a, hi_a), mr.extract(v, lo_b, hi_b)
    ta, tb = [set(map(tuple, m["tri_keys"].tolist())) for m in (a, b)]
    assert ta and tb and not (ta & tb)
    assert ta | tb == set(map(tuple, whole["tri_keys"].tolist()))
    assert a["n_triangles"] + b["n_triangles"] == whole["n_triangles"]
    for m in (a, b):
        at = np.searchsorted(whole["keys"], m["keys"])
        assert np.array_equal(whole["keys"][at], m["keys"])
        assert np.array_equal(mr.bits(whole["vertices"][at]), mr.bits(m["vertices"]))
        assert np.array_equal(mr.bits(whole["normals"][at]), mr.bits(m["normals"]))
    assert np.intersect1d(a["keys"], b["keys"]).size > 0  # the shared layer's vertices are in both


def test_boxes_and_degenerate_volumes():
    assert mr.box_ok((4, 4, 4), (0, 0, 0), (0, 0, 0)) == ([0, 0, 0], [4, 4, 4])
    for lo, hi in (((0, 0, 0), (5, 4, 4)), ((2, 0, 0), (2, 4, 4)), ((-1, 0, 0), (4, 4, 4)), ((0, 0, 0), (4, 0, 4)), ((3, 0, 0), (2, 4, 4))):
        assert mr.box_ok((4, 4, 4), lo, hi) is None
    assert mr.box_ok((1024, 1024, 256), (0, 0, 0), (1024, 1024, 64)) is not None
    assert mr.box_ok((1024, 1024, 256), (0, 0, 0), (1024, 1024, 65)) is None
    for dims in ((1, 1, 1), (4, 1, 4)):
        m = mr.extract(volume(*dims, np.full(dims[::-1], -1, F)))
        assert [m[k] for k in mr.MESH_COUNTERS] == [0, 0, 0, 0, 0]
    # a box of one layer has no cube either
    m = mr.extract(volume(5, 5, 5, mr.checkerboard_tsdf(5, 5, 5)), (0, 2, 0), (5, 3, 5))
    assert m["n_triangles"] == 0 and m["live_cubes"] == 0


def test_signed_zeros_and_non_finite_values_go_through_as_they_are():
    tsdf = np.full((3, 3, 3), 0.5, F)
    tsdf[1, 1, 1] = F(-0.0)  # inside
    tsdf[0, 0, 0] = F(0.0)   # inside, on the corner
    tsdf[2, 2, 1] = np.nan   # outside
    tsdf[2, 0, 2] = -np.inf  # inside
    m = mr.extract(volume(3, 3, 3, tsdf))
    assert m["n_triangles"] > 0 and np.isnan(m["vertices"]).any()
    k = m["keys"]
    centre = (1 * 3 + 1) * 3 + 1
    own = m["vertices"][(k // 7) == centre]
    assert own.shape[0] == 7  # every edge the centre owns leaves it
    overflow = mr.extract(volume(3, 3, 3, tsdf), max_vertices=m["n_vertices"] - 1, max_triangles=m["n_triangles"])
    assert overflow["overflow"] == 1 and mr.extract(volume(3, 3, 3, tsdf), max_vertices=m["n_vertices"], max_triangles=m["n_triangles"])["overflow"] == 0


def test_the_table_is_the_committed_header():
    path = os.path.join(ROOT, "flame_amd", "csrc", "volume_mesh_table.h")
    with open(path) as f:
        text = f.read()
    assert text == mr.table_header(), "flame_amd/csrc/volume_mesh_table.h is not what tests/volume_mesh_ref.py generates"
    assert mr.parse_table_header(text) == mr.table_codes()
    counts, _ = mr.table_codes()
    for p in range(6):
        assert counts[p][0] == counts[p][15] == 0 and all(counts[p][m] == (2 if bin(m).count("1") == 2 else 1) for m in range(1, 15))
    # Kuhn's tets: each of the 19 tet edges of a cube is an edge of E from its lower corner; the body diagonal is in all six
    used = Counter()
    for p in range(6):
        c = mr.tet_corners(p)
        for x in range(4):
            for y in range(x + 1, 4):
                used[mr._edge(c, x, y)] += 1
    assert len(used) == 19 and used[((0, 0, 0), 6)] == 6


def test_volume_mesh_layout_under_the_sanitizers(tmp_path):
    """tests/cpp/volume_mesh_layout_test.cc: a stand-alone program that walks the layout and the box check; nothing is loaded into Python."""
    exe = str(tmp_path / "volume_mesh_layout_test")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-Werror", "-I", os.path.join(ROOT, "flame_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "volume_mesh_layout_test.cc"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 violations" in r.stdout, r.stdout + r.stderr
