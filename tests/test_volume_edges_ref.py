"""The volumetric map past one grid and off the axes, on the checker alone: the cases of tests/test_gpu_volume_edges.py and what each of
them must show before a device run means anything.  A: every round of the integration's grid-stride loop holds updated voxels, voxels
behind the surface and voxels in front of the camera but outside the image, and the partial last workgroup holds updated voxels.  B: the
raycast targets past sixteen workgroups have hits, `back` and `empty` rays.  C: with the general camera and pose the order of every sum of
three products shows in the bits (with the poses and cameras of tests/test_gpu_volume.py it does not).  D: the checker against the float64
restatement tests/volume_ref64.py, within propagated bounds; the raycast of an exact tilted plane against the ray-plane intersection.  No
GPU here."""
import functools

import numpy as np

from tests import test_gpu_volume as tv
from tests import volume_ref as vr
from tests import volume_ref64 as v64

F = np.float32
ROUND = 1024 * 256  # voxels per round of k_volume_integrate: kIntegrateGrid workgroups of 256


# ---- C: the general camera and pose ----------------------------------------------------------------------------------------------------------
def rotation(deg, axis=(1.0, 2.0, 3.0)):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    X = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.radians(deg)
    return np.eye(3) + np.sin(th) * X + (1 - np.cos(th)) * (X @ X)


def general_pose64(deg=17.0, t=(0.05, -0.02, 0.03)):
    return np.hstack([rotation(deg), np.asarray(t, np.float64)[:, None]])


def general_pose(deg=17.0, t=(0.05, -0.02, 0.03)):
    """T_cam_world, 12 floats: the rotation by `deg` about (1, 2, 3) and t, rounded from float64."""
    return general_pose64(deg, t).reshape(-1).astype(F)


def inverse_pose(deg=17.0, t=(0.05, -0.02, 0.03)):
    """T_world_cam of the same camera: the float64 inverse, rounded."""
    T = general_pose64(deg, t)
    return np.hstack([T[:, :3].T, -(T[:, :3].T @ T[:, 3])[:, None]]).reshape(-1).astype(F)


GENERAL_K64 = np.array([[20, 0.7, 16], [0.3, 19, 12], [0.01, -0.02, 1]], np.float64)  # a skew, and a bottom row other than 0 0 1
GENERAL_K = GENERAL_K64.reshape(-1).astype(F)
GENERAL_POSE, GENERAL_BACK = general_pose(), inverse_pose()
SECOND_POSE = general_pose(-11.0, (-0.04, 0.03, -0.02))
CAST = dict(z_near=0.3, dz=0.04, n_steps=40)


def general_kinv(rows, cols):
    """The float64 inverse of GENERAL_K scaled from the scene's 24 x 32 to the target, rounded."""
    return np.linalg.inv(np.diag([cols / 32.0, rows / 24.0, 1.0]) @ GENERAL_K64).reshape(-1).astype(F)


GENERAL_VOLUMES = ("16x12x10", "5x3x7", "70x9x5", "130x3x2")  # of tv.VOLUMES; the first is vr.SCENE


def general_calls():
    """The two integrations of C: (map, K, T_cam_world, keywords)."""
    m = vr.scene_map()
    return [(m, GENERAL_K, GENERAL_POSE, {}), ((m * F(0.97)).astype(F), GENERAL_K, SECOND_POSE, dict(weight=0.5))]


def centres(v):
    shape = (v.nz, v.ny, v.nx)
    idx = [np.arange(n, dtype=F) for n in (v.nx, v.ny, v.nz)]
    return (np.broadcast_to((v.origin[0] + idx[0] * v.voxel_size).astype(F)[None, None, :], shape),
            np.broadcast_to((v.origin[1] + idx[1] * v.voxel_size).astype(F)[None, :, None], shape),
            np.broadcast_to((v.origin[2] + idx[2] * v.voxel_size).astype(F)[:, None, None], shape))


def sum3(a, x, b, y, c, z, right):
    """a x + b y + c z in float32: left to right, as the header has it, or right to left."""
    return (a * x + (b * y + c * z)) if right else ((a * x + b * y) + c * z)


def pose_points_in_order(right):
    def pose_points(pose, x, y, z):
        T = np.asarray(pose, F).reshape(-1)[:12].reshape(3, 4)
        with np.errstate(all="ignore"):
            return [(sum3(T[r, 0], x, T[r, 1], y, T[r, 2], z, right) + T[r, 3]).astype(F) for r in range(3)]
    return pose_points


def product_in_order(M, x, y, z, right):
    M = np.asarray(M, F).reshape(9)
    return [sum3(M[3 * r], x, M[3 * r + 1], y, M[3 * r + 2], z, right).astype(F) for r in range(3)]


def pixel_rays(Kinv, rows, cols, right=False):
    """q = Kinv (col, row, 1) for every pixel of a rows x cols target, three float32 arrays."""
    col = np.broadcast_to(np.arange(cols, dtype=F)[None, :], (rows, cols))
    row = np.broadcast_to(np.arange(rows, dtype=F)[:, None], (rows, cols))
    return product_in_order(Kinv, col, row, F(1), right)


def changed(a, b):
    """How many elements differ in the bits of any of the arrays of a and b."""
    return int(np.count_nonzero(np.logical_or.reduce([vr.bits(x) != vr.bits(y) for x, y in zip(a, b)])))


def scene_through(calls, pose_points=None):
    """vr.SCENE through `calls` and one raycast from GENERAL_BACK -> (volume, map), with another pose_points in the checker if given."""
    saved = vr.pose_points
    try:
        if pose_points is not None:
            vr.pose_points = pose_points
        v = vr.scene_volume()
        for m, K, T, kw in calls:
            v.integrate(m, K, T, **kw)
        return v, v.raycast(general_kinv(24, 32), GENERAL_BACK, 24, 32, **CAST)["map"]
    finally:
        vr.pose_points = saved


def test_the_general_camera_shows_the_order_of_every_sum():
    v = vr.scene_volume()
    c = centres(v)
    left, right = pose_points_in_order(False), pose_points_in_order(True)
    assert changed(left(GENERAL_POSE, *c), vr.pose_points(GENERAL_POSE, *c)) == 0  # the local copy is the checker's arithmetic
    per_row = [changed([a], [b]) for a, b in zip(left(GENERAL_POSE, *c), right(GENERAL_POSE, *c))]
    P = left(GENERAL_POSE, *c)
    k_changed = changed(product_in_order(GENERAL_K, *P, False), product_in_order(GENERAL_K, *P, True))
    ki = general_kinv(24, 32)
    ki_changed = changed(pixel_rays(ki, 24, 32), pixel_rays(ki, 24, 32, True))
    print("right to left, voxels of the scene whose bits change: pose rows %s, K P %d of 1920; rays: Kinv %d of 768" % (per_row, k_changed, ki_changed))
    assert min(per_row) > 0 and k_changed > 0 and ki_changed > 0
    # ... and through to the outputs: the other order of pose_points alone changes the volume and the raycast's map
    (va, ma), (vb, mb) = scene_through(general_calls()), scene_through(general_calls(), right)
    out = changed([va.tsdf], [vb.tsdf]), changed([ma], [mb])
    print("right to left in pose_points: %d voxels' tsdf and %d pixels of the raycast change" % out)
    assert min(out) > 0
    # the poses and cameras of tests/test_gpu_volume.py hide all of it: zero everywhere
    tp = tv.turned_pose()
    old = [changed(left(tp, *c), right(tp, *c)), changed(left(vr.IDENTITY, *c), right(vr.IDENTITY, *c)),
           changed(product_in_order(vr.SCENE_K, *P, False), product_in_order(vr.SCENE_K, *P, True)),
           changed(pixel_rays(vr.SCENE_KINV, 24, 32), pixel_rays(vr.SCENE_KINV, 24, 32, True))]
    print("the same with turned_pose(), the identity, SCENE_K, SCENE_KINV:", old)
    assert old == [0, 0, 0, 0]


# ---- A: volumes past one grid ----------------------------------------------------------------------------------------------------------------
BIG = {
    # 1039 workgroups capped to 1024: 15 take a second round, the last with 195 voxels, three waves and three lanes
    "67x63x63": dict(nx=67, ny=63, nz=63, voxel_size=0.02, origin=(-0.66, -0.62, -0.1), trunc=0.1, max_weight=2.0),
    # three rounds; the third ends with a workgroup of 58 voxels, inside its first wave
    "131x65x62": dict(nx=131, ny=65, nz=62, voxel_size=0.01, origin=(-0.39, -0.54, 0.79), trunc=0.1, max_weight=2.0),
    # nx at the API's maximum, ny == 1; the second round is full workgroups only
    "1024x1x300": dict(nx=1024, ny=1, nz=300, voxel_size=0.004, origin=(-2.0, 0.0, 0.0), trunc=0.1, max_weight=2.0),
}
BIG_ROUNDS = {"67x63x63": 2, "131x65x62": 3, "1024x1x300": 2}
BIG_TAIL = {"67x63x63": 195, "131x65x62": 58, "1024x1x300": 0}
BIG_CALLS = [{}, dict(weight=1.5)]  # (1 + 1.5 passes max_weight = 2: the second call saturates)
BIG_TARGET = (24, 32)


@functools.lru_cache(maxsize=None)
def big_rounds(name):
    """The first integration of BIG[name] in the checker -> per round (updated, behind, in front but outside the image), and the updated
    voxels among the last n mod 256."""
    v = vr.Volume(**BIG[name])
    n = v.nx * v.ny * v.nz
    v.integrate(vr.scene_map(), GENERAL_K, GENERAL_POSE)
    fl = {k: f.reshape(-1) for k, f in v.flags.items()}
    classes = (fl["updated"], fl["behind"], fl["front"] & ~fl["in_image"])
    rounds = [tuple(int(np.count_nonzero(c[r * ROUND:(r + 1) * ROUND])) for c in classes) for r in range((n + ROUND - 1) // ROUND)]
    tail = n % 256
    return rounds, int(np.count_nonzero(fl["updated"][n - tail:])) if tail else 0


def check_big(name):
    p = BIG[name]
    n = p["nx"] * p["ny"] * p["nz"]
    blocks = (n + 255) // 256
    assert blocks > 1024 and (n + ROUND - 1) // ROUND == BIG_ROUNDS[name] and n % 256 == BIG_TAIL[name]
    rounds, tail_updated = big_rounds(name)
    print("%s: %d voxels, %d workgroups' worth; per round (updated, behind, in front and outside): %s; updated among the last %d: %d"
          % (name, n, blocks, rounds, BIG_TAIL[name], tail_updated))
    assert len(rounds) == BIG_ROUNDS[name] and all(min(r) > 0 for r in rounds), rounds
    assert tail_updated > 0 or BIG_TAIL[name] == 0


def test_every_round_of_the_volumes_past_one_grid_has_every_class():
    assert BIG_TAIL["67x63x63"] == 3 * 64 + 3 and 0 < BIG_TAIL["131x65x62"] < 64
    for name in BIG:
        check_big(name)
    # the second call saturates what the first one updated, and the raycast sees the result
    v = vr.Volume(**BIG["67x63x63"])
    counts = [v.integrate(vr.scene_map(), GENERAL_K, GENERAL_POSE, **kw) for kw in BIG_CALLS]
    assert counts[0]["saturated"] == 0 and counts[1]["saturated"] > 0
    r = v.raycast(general_kinv(*BIG_TARGET), GENERAL_BACK, *BIG_TARGET, **CAST)
    assert r["hits"] > 0


# ---- B: targets past sixteen workgroups ------------------------------------------------------------------------------------------------------
LARGE_TARGETS = [(96, 128), (97, 131)]  # 48 full workgroups: the 16 counter sets wrap three times; 12 707 pixels: the last workgroup is partial
LARGE_CAST = dict(z_near=0.3, dz=0.03, n_steps=45)


def integrated_scene():
    v = vr.scene_volume()
    for _ in range(2):
        v.integrate(vr.scene_map(), vr.SCENE_K, vr.IDENTITY)
    return v


def random_volume():
    """The random volume of test_gpu_raycast_on_uploaded_volumes: holes in its weights, values an integration would never produce."""
    rng = np.random.default_rng(5)
    v = vr.Volume(nx=9, ny=7, nz=11, voxel_size=0.1, origin=(-0.4, -0.3, 0.6), trunc=0.3, max_weight=8.0)
    v.tsdf = (rng.random((11, 7, 9)) * 6 - 3).astype(F)
    v.weight = np.where(rng.random((11, 7, 9)) < 0.1, 0, rng.random((11, 7, 9)) * 5).astype(F)
    return v


def large_views(rows, cols):
    """The two cameras of B: (Kinv, T_world_cam, name)."""
    return [(tv.target_kinv(rows, cols), vr.IDENTITY, "the identity"), (general_kinv(rows, cols), GENERAL_BACK, "the general pose")]


@functools.lru_cache(maxsize=None)
def large_counts(which):
    v = integrated_scene() if which == "scene" else random_volume()
    return [(rows, cols, what, {k: r[k] for k in vr.RAYCAST_COUNTERS})
            for rows, cols in LARGE_TARGETS for Kinv, T, what in large_views(rows, cols)
            for r in [v.raycast(Kinv, T, rows, cols, **LARGE_CAST)]]


def check_large(which):
    found = large_counts(which)
    for rows, cols, what, c in found:
        print("%s into %dx%d from %s: %s" % (which, rows, cols, what, c))
    assert any(min(c.values()) > 0 for _, _, _, c in found), found


def test_the_large_targets_have_hits_back_and_empty_rays():
    assert LARGE_TARGETS[0][0] * LARGE_TARGETS[0][1] == 48 * 256 and (97 * 131) % 256 == 163 and 163 % 64 != 0
    for which in ("scene", "random"):
        check_large(which)


# ---- D: against float64 ----------------------------------------------------------------------------------------------------------------------
DOUBT_CAP = 0.02  # of the voxels in front of the camera


def compare_integration(want, tsdf, weight, updated, what):
    """want: v64.integrate of one call; tsdf, weight: the float32 state after it; updated: the float32 decision per voxel.  Outside doubt
    the flag agrees exactly and tsdf and weight lie within the propagated bounds; the doubtful are few."""
    sure = ~want["doubt"]
    front = int(np.count_nonzero(want["front"]))
    doubtful = int(np.count_nonzero(want["doubt"]))
    flags = int(np.count_nonzero(sure & (np.asarray(updated, bool) != want["updated"])))
    dt = np.abs(np.asarray(tsdf, F).astype(np.float64) - want["tsdf"])
    dw = np.abs(np.asarray(weight, F).astype(np.float64) - want["weight"])
    worst = float(dt[sure].max()) if sure.any() else 0.0
    bound = float(want["e_tsdf"][sure].max()) if sure.any() else 0.0
    print("%s: doubtful %d of %d voxels (%d in front), flags that differ outside doubt %d, max |tsdf - float64| %.3g, largest bound %.3g"
          % (what, doubtful, want["doubt"].size, front, flags, worst, bound))
    assert doubtful <= DOUBT_CAP * front, (what, doubtful, front)
    assert flags == 0, what
    assert np.all(dt[sure] <= want["e_tsdf"][sure]) and np.all(dw[sure] <= want["e_weight"][sure]), what
    return doubtful, worst, bound


def test_the_checker_agrees_with_float64_on_the_general_camera():
    for name in GENERAL_VOLUMES:
        v = vr.Volume(**tv.VOLUMES[name])
        for call, (m, K, T, kw) in enumerate(general_calls()):
            want = v64.integrate(v.nx, v.ny, v.nz, v.voxel_size, v.origin, v.trunc, v.max_weight, v.tsdf, v.weight, m, K, T, **kw)
            c = v.integrate(m, K, T, **kw)
            assert c["updated"] > 0 and c["saturated"] == 0
            compare_integration(want, v.tsdf, v.weight, v.flags["updated"], "%s, call %d, the checker" % (name, call))


PLANE = dict(nx=19, ny=17, nz=13, voxel_size=0.1, origin=(-0.9, -0.8, 0.5), trunc=0.3)
PLANE_NORMAL, PLANE_POINT = (0.3, -0.2, -1.0), (0.05, 0.02, 1.1)
PLANE_TARGET = (97, 131)
PLANE_BACK = inverse_pose(7.0)
PLANE_CAST = dict(z_near=0.3, dz=0.04, n_steps=50)


def plane_volume():
    v = vr.Volume(max_weight=8.0, **PLANE)
    v.tsdf, v.weight = v64.plane_volume(normal=PLANE_NORMAL, point=PLANE_POINT, **PLANE)
    return v


@functools.lru_cache(maxsize=None)
def plane_case():
    """-> (the checker's raycast of the plane, the float64 intersections)."""
    rows, cols = PLANE_TARGET
    v = plane_volume()
    Kinv = general_kinv(rows, cols)
    r = v.raycast(Kinv, PLANE_BACK, rows, cols, **PLANE_CAST)
    plane = v64.ray_plane(pixel_rays(Kinv, rows, cols), PLANE_BACK, PLANE["voxel_size"], PLANE["origin"], PLANE["trunc"], PLANE_NORMAL,
                          PLANE_POINT, v.tsdf, PLANE_CAST["dz"])
    return r, plane


def compare_plane(depth_map, plane, what):
    """Every hit's z* = 1 / (map q.z) against the float64 intersection, in units of EPS M / slope + EPS z -> (the worst ratio, c)."""
    rows, cols = PLANE_TARGET
    hit = ~np.isnan(depth_map)
    q2 = pixel_rays(general_kinv(rows, cols), rows, cols)[2].astype(np.float64)
    zs = 1.0 / (np.asarray(depth_map, F).astype(np.float64)[hit] * q2[hit])
    z, slope = plane["z"][hit], plane["slope"][hit]
    unit = v64.EPS * plane["M"] / slope + v64.EPS * np.abs(z)
    ratio = float((np.abs(zs - z) / unit).max())
    c = float(v64.crossing_c(plane, hit))
    print("%s: %d hits, worst |z* - z| / (EPS M / slope + EPS z) = %.2f, derived c = %.1f (M %.3g, slope %.3g .. %.3g)"
          % (what, int(hit.sum()), ratio, c, plane["M"], slope.min(), slope.max()))
    assert ratio <= c, (what, ratio, c)
    return ratio, c


def test_the_checkers_raycast_of_a_tilted_plane_is_the_ray_plane_intersection():
    r, plane = plane_case()
    assert r["hits"] > 0.5 * PLANE_TARGET[0] * PLANE_TARGET[1] and r["hits"] == np.count_nonzero(~np.isnan(r["map"]))
    compare_plane(r["map"], plane, "the checker")
