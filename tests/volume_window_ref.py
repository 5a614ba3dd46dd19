"""The checker of the window that follows the camera (include/flame_nltgv2.h, THE WINDOW and flame_nltgv2_volume_shift_begin): the rules
stated there in numpy float32, operation for operation.  tests/volume_ref.py and tests/volume_mesh_ref.py stay the checkers of a volume
whose base is (0, 0, 0); what depends on the base is restated here:

    the window     local voxel (i, j, k) is global voxel base + (i, j, k); origin is the centre of GLOBAL voxel (0, 0, 0), for good
    shift          base' = base + s; destination (i, j, k) gets the record of source (i, j, k) + s where that lies in the window,
                   else {1, 0}; kept, kept_seen, lost_seen, entered
    integrate      rule 1 with p = origin + float(base + index) * voxel_size, the sum in integers; rules 2 - 9 as they were
    raycast        g = (p - origin) / voxel_size is global: valid iff base <= g <= base + n - 1 per axis (and the eight weights > 0);
                   ig = min(floor(g), base + n - 2), the local cell ig - base, f = g - float(ig)
    mesh           keys local; a vertex's position from the global indices of its edge's two voxels, as rule 1
    follow         c = t + focus_depth * R[:, 2]; g = (c - origin) / voxel_size; m = base + n // 2; q = trunc((g - m) / step);
                   shift = q * step; the kept box and the leaving slabs

Results are compared with the device's as bit patterns (`.view(uint32)`): no tolerance.
"""
import numpy as np

from tests import volume_mesh_ref as vmr
from tests import volume_ref as vr

F = np.float32
MAX_BASE = 1 << 22
SHIFT_COUNTERS = ("kept", "kept_seen", "lost_seen", "entered")


class Volume(vr.Volume):
    """vr.Volume with a base: the store is the window's, (nz, ny, nx), local indices."""

    def __init__(self, nx, ny, nz, voxel_size, origin, trunc, max_weight, base=(0, 0, 0)):
        super().__init__(nx, ny, nz, voxel_size, origin, trunc, max_weight)
        self.base = np.asarray(base, np.int64).reshape(3).copy()

    def copy(self):
        v = Volume(self.nx, self.ny, self.nz, self.voxel_size, self.origin, self.trunc, self.max_weight, self.base)
        v.tsdf, v.weight = self.tsdf.copy(), self.weight.copy()
        return v

    @property
    def dims(self):
        return (self.nx, self.ny, self.nz)

    # -- the shift ----------------------------------------------------------------------------------------------------------------------
    def shift(self, s):
        """Moves the window by s = (sx, sy, sz) voxels -> dict of the four counters; None (and nothing changes) past the base limit."""
        s = [int(v) for v in s]
        new_base = self.base + np.asarray(s, np.int64)
        if np.any(np.abs(new_base) > MAX_BASE):
            return None
        n = self.dims
        seen_before = int(np.count_nonzero(self.weight > F(0)))
        tsdf, weight = np.ones_like(self.tsdf), np.zeros_like(self.weight)
        kept = kept_seen = 0
        if all(abs(s[a]) < n[a] for a in range(3)):
            # destination [d0, d1) per axis receives source [d0 + s, d1 + s)
            dst = [slice(max(0, -s[a]), min(n[a], n[a] - s[a])) for a in range(3)]
            src = [slice(d.start + s[a], d.stop + s[a]) for a, d in enumerate(dst)]
            # (copied as bit patterns: NaN payloads and -0 survive)
            tsdf.view(np.uint32)[dst[2], dst[1], dst[0]] = self.tsdf.view(np.uint32)[src[2], src[1], src[0]]
            weight.view(np.uint32)[dst[2], dst[1], dst[0]] = self.weight.view(np.uint32)[src[2], src[1], src[0]]
            moved = self.weight[src[2], src[1], src[0]]
            kept, kept_seen = int(moved.size), int(np.count_nonzero(moved > F(0)))
        self.tsdf, self.weight = tsdf, weight
        self.base = new_base
        total = n[0] * n[1] * n[2]
        return dict(kept=kept, kept_seen=kept_seen, lost_seen=seen_before - kept_seen, entered=total - kept)

    # -- rule 1 of the integration with the base; rules 2 - 9 as in vr.Volume.integrate --------------------------------------------------
    def integrate(self, idepthmap, K, T_cam_world, weight=1.0, near_depth=0.0, min_depth=0.0, max_depth=np.inf):
        m = np.ascontiguousarray(idepthmap, F)
        rows, cols = m.shape
        K = np.asarray(K, F).reshape(9)
        wgt = F(weight)
        shape = (self.nz, self.ny, self.nx)
        with np.errstate(all="ignore"):
            # the sum in integers, then the conversion
            idx = [(self.base[a] + np.arange(n, dtype=np.int64)).astype(F) for a, n in enumerate(self.dims)]
            px = np.broadcast_to((self.origin[0] + (idx[0] * self.voxel_size).astype(F)).astype(F)[None, None, :], shape)
            py = np.broadcast_to((self.origin[1] + (idx[1] * self.voxel_size).astype(F)).astype(F)[None, :, None], shape)
            pz = np.broadcast_to((self.origin[2] + (idx[2] * self.voxel_size).astype(F)).astype(F)[:, None, None], shape)
            Px, Py, Pz = vr.pose_points(T_cam_world, px, py, pz)
            front = Pz > F(near_depth)
            q = [((K[3 * r] * Px + K[3 * r + 1] * Py) + K[3 * r + 2] * Pz).astype(F) for r in range(3)]
            u, v = (q[0] / q[2]).astype(F), (q[1] / q[2]).astype(F)
            half = F(0.5)
            in_image = front & (u >= -half) & (u < F(cols) - half) & (v >= -half) & (v < F(rows) - half)
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
        self.flags = dict(zip(vr.INTEGRATE_COUNTERS, flags))
        return {k: int(np.count_nonzero(f)) for k, f in zip(vr.INTEGRATE_COUNTERS, flags)}

    # -- the raycast's sample at GLOBAL coordinates g (vr.Volume.raycast computes them and calls this) -----------------------------------
    def _sample(self, g):
        n_axis = self.dims
        shape = g[0].shape
        if min(n_axis) < 2:
            return np.zeros(shape, bool), np.zeros(shape, F)
        with np.errstate(all="ignore"):
            ok = np.ones(shape, bool)
            for a in range(3):
                ok &= (g[a] >= F(self.base[a])) & (g[a] <= F(self.base[a] + n_axis[a] - 1))
            i0, f = [], []
            for a in range(3):
                ga = np.where(ok, g[a], F(self.base[a]))
                ig = np.minimum(np.floor(ga).astype(np.int64), self.base[a] + n_axis[a] - 2)
                i0.append(ig - self.base[a])
                f.append((ga - ig.astype(F)).astype(F))
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


def scene_volume():
    return Volume(**vr.SCENE)


def crop(big, small):
    """The part of `big` (a Volume on the same grid) under the window of `small` -> (tsdf, weight), the window's shape."""
    lo = [int(small.base[a] - big.base[a]) for a in range(3)]
    n = small.dims
    assert all(lo[a] >= 0 and lo[a] + n[a] <= big.dims[a] for a in range(3)), "the window leaves the larger volume"
    sl = (slice(lo[2], lo[2] + n[2]), slice(lo[1], lo[1] + n[1]), slice(lo[0], lo[0] + n[0]))
    return big.tsdf[sl], big.weight[sl]


# ---- the mesh: vmr.extract with the positions of the window ------------------------------------------------------------------------------
def extract(vol, lo=(0, 0, 0), hi=(0, 0, 0), want_normals=True, max_vertices=None, max_triangles=None):
    """vmr.extract of a window: keys, triangles, normals and counters are local and unchanged; the positions follow rule 1 with the base."""
    m = vmr.extract(vol, lo, hi, want_normals, max_vertices, max_triangles)
    keys = m["keys"]
    owner, e = keys // 7, keys % 7
    i0, j0, k0 = owner % vol.nx, (owner // vol.nx) % vol.ny, owner // (vol.nx * vol.ny)
    off = np.asarray(vmr.E, np.int64)[e] if keys.size else np.zeros((0, 3), np.int64)
    with np.errstate(all="ignore"):
        f0 = vol.tsdf[k0, j0, i0]
        f1 = vol.tsdf[k0 + off[:, 2], j0 + off[:, 1], i0 + off[:, 0]]
        t = (f0 / (f0 - f1).astype(F)).astype(F)
        verts = np.zeros((keys.size, 3), F)
        for ax, a0 in enumerate((i0, j0, k0)):
            g0 = (vol.base[ax] + a0).astype(F)
            g1 = (vol.base[ax] + a0 + off[:, ax]).astype(F)
            p0 = (vol.origin[ax] + (g0 * vol.voxel_size).astype(F)).astype(F)
            p1 = (vol.origin[ax] + (g1 * vol.voxel_size).astype(F)).astype(F)
            verts[:, ax] = (p0 + (t * (p1 - p0).astype(F)).astype(F)).astype(F)
    m["vertices"] = verts
    return m


def normals_untouched(vol, keys, shift):
    """For the vertices `keys` of the window AFTER a shift by `shift`: True where no voxel of the two gradients' stencils (the edge's two
    voxels' six neighbours each) was in the window before the shift and is outside it now -- there the normal is what it was."""
    n = np.asarray(vol.dims, np.int64)
    s = np.asarray(shift, np.int64)
    owner, e = keys // 7, keys % 7
    p0 = np.stack([owner % vol.nx, (owner // vol.nx) % vol.ny, owner // (vol.nx * vol.ny)], axis=1)
    p1 = p0 + (np.asarray(vmr.E, np.int64)[e] if keys.size else np.zeros((0, 3), np.int64))
    ok = np.ones(keys.size, bool)
    for p in (p0, p1):
        for ax in range(3):
            for d in (-1, 1):
                q = p.copy()
                q[:, ax] += d
                now_in = np.all((q >= 0) & (q < n), axis=1)
                before = q + s  # the same voxel's local index before the shift
                was_in = np.all((before >= 0) & (before < n), axis=1)
                ok &= ~(was_in & ~now_in)
    return ok


# ---- follow ------------------------------------------------------------------------------------------------------------------------------
def follow(vol, T_world_cam, focus_depth=0.0, step=8):
    """-> dict(shift [3], kept (lo, hi) or None, leaving [(lo, hi), ...]) in pre-shift local indices; None for an invalid argument."""
    T = np.asarray(T_world_cam, F).reshape(-1)[:12].reshape(3, 4)
    step = int(step)
    if step < 1 or not np.isfinite(F(focus_depth)):
        return None
    n = vol.dims
    shift = []
    with np.errstate(all="ignore"):
        for a in range(3):
            c = F(T[a, 3] + F(F(focus_depth) * T[a, 2]))
            if not np.isfinite(c):
                return None
            g = F(F(c - vol.origin[a]) / vol.voxel_size)
            m = int(vol.base[a]) + n[a] // 2
            q = np.trunc(F(F(g - F(m)) / F(step)))
            if not (-MAX_BASE <= q <= MAX_BASE):
                return None
            prod = int(q) * step
            if not (-(1 << 31) <= prod < (1 << 31)):
                return None
            shift.append(prod)
    return dict(shift=shift, **plan(n, shift))


def plan(n, shift):
    """The kept box and the leaving slabs of a shift of a window of n voxels."""
    if any(abs(shift[a]) >= n[a] for a in range(3)):
        return dict(kept=None, leaving=[([0, 0, 0], list(n))])
    kept_lo = [max(0, shift[a]) for a in range(3)]
    kept_hi = [min(n[a], n[a] + shift[a]) for a in range(3)]
    leaving = []
    for a in range(3):
        if shift[a] == 0:
            continue
        lo, hi = [0, 0, 0], list(n)
        for b in range(a):
            lo[b], hi[b] = kept_lo[b], kept_hi[b]
        if shift[a] > 0:
            lo[a], hi[a] = 0, shift[a] + 1  # one layer towards the kept side
        else:
            lo[a], hi[a] = n[a] + shift[a] - 1, n[a]
        leaving.append((lo, hi))
    return dict(kept=(kept_lo, kept_hi), leaving=leaving)


def box_cubes(n, lo, hi):
    """The cubes of a box (their lower corners' linear indices in the window): all eight corners inside it."""
    r = [np.arange(lo[a], hi[a] - 1) for a in range(3)]
    k, j, i = np.meshgrid(r[2], r[1], r[0], indexing="ij")
    return set(((k * n[1] + j) * n[0] + i).reshape(-1).tolist())


def assert_same_counts(got, ref, what=""):
    vr.assert_same_counts(got, ref, SHIFT_COUNTERS, what)
