"""The checker of the volumetric map (include/flame_nltgv2.h, flame_nltgv2_volume_create): the rules stated there in numpy float32,
operation for operation, vectorised over voxels and pixels with a Python loop over the raycast's steps.  Nothing here has a counterpart
in the reference; the conventions are the library's own: every sum of three products left to right, no FMA, IEEE division.

    the store      voxel (i, j, k) is {tsdf, weight} at [k, j, i]; fresh or reset {1, 0}
    integrate      p = origin + index * voxel_size; P = T_cam_world p; front: P.z > near_depth; q = K P; u = q.x / q.z, v = q.y / q.z;
                   in image: -0.5 <= u < cols - 0.5, -0.5 <= v < rows - 0.5; the nearest pixel, clamped; d = map[row, col], zm = 1 / d;
                   valid: d > 0 and zm > min_depth and zm < max_depth; sdf = zm - P.z; behind: sdf < -trunc (left alone);
                   s = fmin(sdf / trunc, 1); W = w + weight; tsdf = ((tsdf * w) + (s * weight)) / W; w = fmin(W, max_weight)
    raycast        q = Kinv (col, row, 1); z_n = z_near + n * dz; p = T_world_cam (q * z_n); g = (p - origin) / voxel_size;
                   valid sample: every g in [0, n_axis - 1] and the eight weights > 0; i0 = min(floor(g), n_axis - 2), f = g - i0;
                   trilinear with a + t * (b - a) along x, y, z; the ray ends at the first valid sample <= 0: a hit iff the sample
                   before was valid and > 0, z* = z_prev + dz * (f_prev / (f_prev - f_cur)), pixel = 1 / (z* * q.z); else `back`;
                   a ray without any valid sample is `empty`; holes are the quiet NaN 0x7fc00000

Results are compared with the device's as bit patterns (`bits`, `.view(uint32)`): no tolerance.
"""
import numpy as np

F = np.float32
QNAN = np.uint32(0x7FC00000).view(np.float32)
INTEGRATE_COUNTERS = ("front", "in_image", "valid", "behind", "updated", "saturated")
RAYCAST_COUNTERS = ("hits", "back", "empty")


def bits(a):
    """The bit patterns of a float32 array, as they are."""
    return np.ascontiguousarray(a, F).view(np.uint32)


def pose_points(pose, x, y, z):
    """((r0 * x + r1 * y) + r2 * z) + t for the three rows of pose (12 floats, row-major [R | t]) -> three arrays."""
    T = np.asarray(pose, F).reshape(-1)[:12].reshape(3, 4)
    with np.errstate(all="ignore"):
        return [(((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(F) for r in range(3)]


class Volume:
    """The store: tsdf and weight, (nz, ny, nx) float32 each."""

    def __init__(self, nx, ny, nz, voxel_size, origin, trunc, max_weight):
        self.nx, self.ny, self.nz = int(nx), int(ny), int(nz)
        self.voxel_size, self.trunc, self.max_weight = F(voxel_size), F(trunc), F(max_weight)
        self.origin = np.asarray(origin, F).reshape(3)
        self.reset()

    def reset(self):
        self.tsdf = np.ones((self.nz, self.ny, self.nx), F)
        self.weight = np.zeros((self.nz, self.ny, self.nx), F)

    def copy(self):
        v = Volume(self.nx, self.ny, self.nz, self.voxel_size, self.origin, self.trunc, self.max_weight)
        v.tsdf, v.weight = self.tsdf.copy(), self.weight.copy()
        return v

    # -- rules 1 - 9 of the integration -------------------------------------------------------------------------------------------------
    def integrate(self, idepthmap, K, T_cam_world, weight=1.0, near_depth=0.0, min_depth=0.0, max_depth=np.inf):
        """Folds the (rows, cols) inverse-depth map into the volume -> dict of the six counters."""
        m = np.ascontiguousarray(idepthmap, F)
        rows, cols = m.shape
        K = np.asarray(K, F).reshape(9)
        wgt = F(weight)
        shape = (self.nz, self.ny, self.nx)
        with np.errstate(all="ignore"):
            idx = [np.arange(n, dtype=F) for n in (self.nx, self.ny, self.nz)]
            px = np.broadcast_to((self.origin[0] + idx[0] * self.voxel_size).astype(F)[None, None, :], shape)
            py = np.broadcast_to((self.origin[1] + idx[1] * self.voxel_size).astype(F)[None, :, None], shape)
            pz = np.broadcast_to((self.origin[2] + idx[2] * self.voxel_size).astype(F)[:, None, None], shape)
            Px, Py, Pz = pose_points(T_cam_world, px, py, pz)
            front = Pz > F(near_depth)
            q = [((K[3 * r] * Px + K[3 * r + 1] * Py) + K[3 * r + 2] * Pz).astype(F) for r in range(3)]
            u, v = (q[0] / q[2]).astype(F), (q[1] / q[2]).astype(F)
            half = F(0.5)
            in_image = front & (u >= -half) & (u < F(cols) - half) & (v >= -half) & (v < F(rows) - half)
            # (conversions only where the test passed: no NaN or huge value reaches them)
            col = np.zeros(shape, np.int64)
            row = np.zeros(shape, np.int64)
            col[in_image] = np.clip(np.floor((u[in_image] + half).astype(F)).astype(np.int64), 0, cols - 1)
            row[in_image] = np.clip(np.floor((v[in_image] + half).astype(F)).astype(np.int64), 0, rows - 1)
            d = m[row, col]
            zm = (F(1.0) / d).astype(F)
            valid = in_image & (d > F(0)) & (zm > F(min_depth)) & (zm < F(max_depth))
            sdf = (zm - Pz).astype(F)
            behind = valid & (sdf < -self.trunc)
            updated = valid & ~behind
            s = np.fmin((sdf / self.trunc).astype(F), F(1.0))
            W = (self.weight + wgt).astype(F)
            tsdf = (((self.tsdf * self.weight).astype(F) + (s * wgt).astype(F)).astype(F) / W).astype(F)
            w = np.fmin(W, self.max_weight)
            saturated = updated & (W > self.max_weight)
        self.tsdf = np.where(updated, tsdf, self.tsdf).astype(F)
        self.weight = np.where(updated, w, self.weight).astype(F)
        flags = (front, in_image, valid, behind, updated, saturated)
        self.flags = dict(zip(INTEGRATE_COUNTERS, flags))  # the last call's classes per voxel, (nz, ny, nx) bool: for tests that ask where
        return {k: int(np.count_nonzero(f)) for k, f in zip(INTEGRATE_COUNTERS, flags)}

    # -- the raycast --------------------------------------------------------------------------------------------------------------------
    def _sample(self, g):
        """-> (valid, value) of the samples at grid coordinates g = [gx, gy, gz]."""
        n_axis = (self.nx, self.ny, self.nz)
        shape = g[0].shape
        if min(n_axis) < 2:  # an axis of one voxel has no valid sample
            return np.zeros(shape, bool), np.zeros(shape, F)
        with np.errstate(all="ignore"):
            ok = np.ones(shape, bool)
            for a in range(3):
                ok &= (g[a] >= F(0)) & (g[a] <= F(n_axis[a] - 1))
            i0, f = [], []
            for a in range(3):
                ga = np.where(ok, g[a], F(0))
                i = np.minimum(np.floor(ga).astype(np.int64), n_axis[a] - 2)
                i0.append(i)
                f.append((ga - i.astype(F)).astype(F))
            ix, iy, iz = i0

            def tap(dx, dy, dz):
                return self.tsdf[iz + dz, iy + dy, ix + dx], self.weight[iz + dz, iy + dy, ix + dx]

            def lerp(a, b, t):
                return (a + (t * (b - a).astype(F)).astype(F)).astype(F)

            c = {}
            for dz in (0, 1):
                for dy in (0, 1):
                    (t0, w0), (t1, w1) = tap(0, dy, dz), tap(1, dy, dz)
                    ok &= (w0 > F(0)) & (w1 > F(0))
                    c[dy, dz] = lerp(t0, t1, f[0])
            val = lerp(lerp(c[0, 0], c[1, 0], f[1]), lerp(c[0, 1], c[1, 1], f[1]), f[2])
        return ok, val

    def raycast(self, Kinv, T_world_cam, rows, cols, z_near, dz, n_steps):
        """-> dict(map (rows, cols) f32 with the quiet NaN on holes, hits, back, empty)."""
        Ki = np.asarray(Kinv, F).reshape(9)
        z_near, dz = F(z_near), F(dz)
        shape = (rows, cols)
        col = np.broadcast_to(np.arange(cols, dtype=F)[None, :], shape)
        row = np.broadcast_to(np.arange(rows, dtype=F)[:, None], shape)
        one = F(1)
        with np.errstate(all="ignore"):
            q = [((Ki[3 * r] * col + Ki[3 * r + 1] * row) + Ki[3 * r + 2] * one).astype(F) for r in range(3)]
        out = np.full(shape, QNAN, F)
        ended = np.zeros(shape, bool)
        hit = np.zeros(shape, bool)
        back = np.zeros(shape, bool)
        any_valid = np.zeros(shape, bool)
        prev_ok = np.zeros(shape, bool)
        prev_val = np.zeros(shape, F)
        for n in range(int(n_steps)):
            if ended.all():
                break
            with np.errstate(all="ignore"):
                z = (z_near + F(n) * dz).astype(F)
                p = pose_points(T_world_cam, (q[0] * z).astype(F), (q[1] * z).astype(F), (q[2] * z).astype(F))
                g = [((p[a] - self.origin[a]).astype(F) / self.voxel_size).astype(F) for a in range(3)]
                ok, val = self._sample(g)
                ok &= ~ended
                any_valid |= ok
                ends = ok & (val <= F(0))
                is_hit = ends & prev_ok & (prev_val > F(0))
                z_prev = (z_near + F(n - 1) * dz).astype(F)
                zs = (z_prev + (dz * (prev_val / (prev_val - val).astype(F)).astype(F)).astype(F)).astype(F)
                pix = (F(1.0) / (zs * q[2]).astype(F)).astype(F)
            out = np.where(is_hit, pix, out).astype(F)
            hit |= is_hit
            back |= ends & ~is_hit
            ended |= ends
            prev_ok, prev_val = ok, val
        return dict(map=out, hits=int(np.count_nonzero(hit)), back=int(np.count_nonzero(back)), empty=int(np.count_nonzero(~any_valid)))


# ---- "the scene": what the GPU tests and the checker's own tests share ---------------------------------------------------------------------
SCENE = dict(nx=16, ny=12, nz=10, voxel_size=0.1, origin=(-0.8, -0.6, 0.5), trunc=0.3, max_weight=2.0)
SCENE_ROWS, SCENE_COLS = 24, 32
SCENE_K = np.array([20, 0, 16, 0, 20, 12, 0, 0, 1], F)
SCENE_KINV = np.array([0.05, 0, -0.8, 0, 0.05, -0.6, 0, 0, 1], F)
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F)
SCENE_RAYCAST = dict(z_near=0.3, dz=0.05, n_steps=30)


def scene_volume():
    return Volume(**SCENE)


def scene_map():
    """A wall at depth 1 with the columns from 20 on at depth 1.25, a NaN block, one zero and one negative pixel."""
    m = np.full((SCENE_ROWS, SCENE_COLS), 1.0, F)
    m[:, 20:] = F(0.8)
    m[3:7, 4:9] = np.nan
    m[15, 12] = F(0.0)
    m[16, 25] = F(-1.0)
    return m


def shifted_pose(dx):
    """T_world_cam of a camera shifted by dx along x."""
    T = IDENTITY.copy()
    T[3] = F(dx)
    return T


def assert_same_volume(got, ref, what=""):
    """got: dict(tsdf, weight) from the device; ref: a Volume.  Bit for bit."""
    for k, r in (("tsdf", ref.tsdf), ("weight", ref.weight)):
        g = np.asarray(got[k])
        assert g.shape == r.shape, f"{what}: {k} has shape {g.shape}, the checker {r.shape}"
        bad = np.flatnonzero((bits(g) != bits(r)).reshape(-1))
        assert bad.size == 0, f"{what}: {k} differs at {bad[:8]} ({bad.size} of {r.size}): {g.reshape(-1)[bad[:4]]} vs {r.reshape(-1)[bad[:4]]}"


def assert_same_counts(got, ref, keys, what=""):
    for k in keys:
        assert int(got[k]) == int(ref[k]), f"{what}: {k} {got[k]} vs the checker's {ref[k]}"


def assert_same_map(got, ref, what=""):
    g, r = np.asarray(got), np.asarray(ref)
    assert g.shape == r.shape, f"{what}: the map has shape {g.shape}, the checker {r.shape}"
    bad = np.flatnonzero((bits(g) != bits(r)).reshape(-1))
    assert bad.size == 0, f"{what}: the map differs at {bad[:8]} ({bad.size} of {r.size}): {g.reshape(-1)[bad[:4]]} vs {r.reshape(-1)[bad[:4]]}"
