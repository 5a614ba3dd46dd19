"""The checker of the metric outputs (include/flame_nltgv2.h, flame_nltgv2_metric_outputs_begin): the semantics stated there in numpy
float32, operation for operation.  Nothing here has a counterpart in the reference; the conventions are the library's own, the ones of
flame_nltgv2_mesh_outputs (tests/mesh_ref.py): every sum of three products left to right, no FMA, IEEE division.

    q = Kinv * (col, row, 1);  P = q / v;  z = P.z
    valid  iff  v > 0 and z > min_depth and z < max_depth        (every comparison with a NaN is false)
    P_w = ((r0 * x + r1 * y) + r2 * z) + t, row by row           (pose = T_world_cam, 12 floats row-major [R | t]; None: P untouched)
    depth      z where valid, the quiet NaN 0x7fc00000 on holes
    depth_mm   rint(z * 1000) (ties to even) where valid and in [1, 65535], else 0
    organized  P or P_w where valid, three quiet NaNs on holes
    cloud, cloud_pixel   the valid pixels' points and linear indices in ascending row-major order

Results are compared with the device's as bit patterns (`bits`, `.view(uint32)`): no tolerance.  Every array op below is an
elementwise IEEE float32 operation; numpy neither contracts nor reorders them.
"""
import numpy as np

F = np.float32
QNAN = np.uint32(0x7FC00000).view(np.float32)
POINT_KEYS = ("depth", "depth_mm", "organized", "cloud", "cloud_pixel")
MESH_KEYS = ("mesh_vertices", "mesh_normals", "mesh_triangles")


def bits(a):
    """The bit patterns of a float32 array, as they are."""
    return np.ascontiguousarray(a, F).view(np.uint32)


def pose_points(pose, x, y, z, translate=True):
    """((r0 * x + r1 * y) + r2 * z) + t for the three rows of pose -> three arrays."""
    T = np.asarray(pose, F).reshape(-1)[:12].reshape(3, 4)
    with np.errstate(all="ignore"):
        rows = [(T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z for r in range(3)]
        return [rows[r] + T[r, 3] for r in range(3)] if translate else rows


def pixel_points(idepthmap, Kinv, min_depth=0.0, max_depth=np.inf):
    """-> (x, y, z, valid): the camera-frame points of every pixel, (rows, cols) each, and the validity."""
    v = np.ascontiguousarray(idepthmap, F)
    rows, cols = v.shape
    K = np.asarray(Kinv, F).reshape(9)
    col = np.broadcast_to(np.arange(cols, dtype=F)[None, :], (rows, cols))
    row = np.broadcast_to(np.arange(rows, dtype=F)[:, None], (rows, cols))
    one = F(1)
    with np.errstate(all="ignore"):
        q = [(K[3 * r] * col + K[3 * r + 1] * row) + K[3 * r + 2] * one for r in range(3)]
        x, y, z = [(c / v).astype(F) for c in q]
        valid = (v > F(0)) & (z > F(min_depth)) & (z < F(max_depth))
    return x, y, z, valid


LOOP_LIMIT = 4096  # maps up to this many pixels are compacted by the plain loop itself


def valid_pixels_loop(flat_valid):
    """The compaction as the specification states it: a plain row-major walk that keeps the linear indices of the valid pixels."""
    return np.array([i for i in range(len(flat_valid)) if flat_valid[i]], np.uint32)


def valid_pixels(flat_valid):
    """valid_pixels_loop; above LOOP_LIMIT pixels np.flatnonzero, which returns the indices of the non-zero entries in ascending
    order -- the same list (tests/test_metric_outputs.py walks a map above the limit both ways)."""
    if len(flat_valid) <= LOOP_LIMIT:
        return valid_pixels_loop(flat_valid)
    return np.flatnonzero(flat_valid).astype(np.uint32)


def metric_points(idepthmap, Kinv, pose=None, min_depth=0.0, max_depth=np.inf):
    """dict(depth (rows,cols) f32, depth_mm (rows,cols) u16, organized (rows,cols,3) f32, cloud (n,3) f32, cloud_pixel (n,) u32,
    n_points)."""
    x, y, z, valid = pixel_points(idepthmap, Kinv, min_depth, max_depth)
    rows, cols = z.shape
    depth = np.where(valid, z, QNAN).astype(F)
    with np.errstate(all="ignore"):
        mm = np.rint(z * F(1000.0)).astype(F)  # (ties to even)
        in_range = valid & (mm >= F(1)) & (mm <= F(65535))
    depth_mm = np.zeros((rows, cols), np.uint16)
    depth_mm[in_range] = mm[in_range].astype(np.uint16)
    if pose is not None:
        x, y, z = pose_points(pose, x, y, z)
    organized = np.empty((rows, cols, 3), F)
    for k, c in enumerate((x, y, z)):
        organized[..., k] = np.where(valid, c, QNAN)
    # the compaction: the valid pixels as a plain row-major walk meets them
    flat_valid, flat_points = valid.reshape(-1), organized.reshape(-1, 3)
    pixel = valid_pixels(flat_valid)
    cloud = flat_points[pixel.astype(np.int64)].copy()
    return dict(depth=depth, depth_mm=depth_mm, organized=organized, cloud=cloud, cloud_pixel=pixel, n_points=int(pixel.size))


def metric_mesh(pos, x, graph_scale, Kinv, normals, tris, tri_valid, pose=None):
    """dict(mesh_vertices (V,3), mesh_normals (V,3), mesh_triangles (n_valid,3) i32, n_valid): the vertices back-projected as
    flame_nltgv2_mesh_outputs does it (tests/mesh_ref.py: backproject), then posed; R * the vertex normals; the triangles with
    non-zero validity in ascending index."""
    K = np.asarray(Kinv, F).reshape(9)
    p = np.asarray(pos, F).reshape(-1, 2)
    one = F(1)
    with np.errstate(all="ignore"):
        idepth = (np.asarray(x, F) * F(graph_scale)).astype(F)
        h = [(K[3 * r] * p[:, 0] + K[3 * r + 1] * p[:, 1]) + K[3 * r + 2] * one for r in range(3)]
        P = [(c / idepth).astype(F) for c in h]
    n = np.asarray(normals, F).reshape(-1, 3)
    N = [n[:, 0], n[:, 1], n[:, 2]]
    if pose is not None:
        P = pose_points(pose, *P)
        N = pose_points(pose, *N, translate=False)
    tris = np.asarray(tris, np.int32).reshape(-1, 3)
    keep = [t for t in range(len(tris)) if tri_valid[t] != 0]
    return dict(mesh_vertices=np.stack(P, axis=1).astype(F), mesh_normals=np.stack(N, axis=1).astype(F),
                mesh_triangles=tris[keep].reshape(-1, 3), n_valid=len(keep))


def assert_same(got, ref, keys, what=""):
    """Every array of `keys` bit for bit, the counters of the lists among them exactly."""
    for k in keys:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape, f"{what}: {k} has shape {g.shape}, the checker {r.shape}"
        if r.dtype == np.float32:
            g, r = bits(g), bits(r)
        else:
            assert g.dtype == r.dtype, f"{what}: {k} is {g.dtype}, the checker {r.dtype}"
        bad = np.flatnonzero((g != r).reshape(-1))
        assert bad.size == 0, f"{what}: {k} differs at {bad[:8]} ({bad.size} of {r.size}): {g.reshape(-1)[bad[:4]]} vs {r.reshape(-1)[bad[:4]]}"
    for k, of in (("n_points", "cloud"), ("n_valid", "mesh_triangles")):  # (each counter travels with its list)
        if of in keys:
            assert got[k] == ref[k], f"{what}: {k} {got[k]} vs {ref[k]}"
