"""The cases of tests/test_gpu_volume_window_edges.py and what each must show before a device run means anything: shifts of volumes past
one grid of k_volume_shift (volume_shift_kernels.hip), the extremes of a shift along one axis, and a second statement of the shift to hold
beside tests/volume_window_ref.py.  numpy only: no GPU, no torch.

THE WALK, as the kernel's header has it.  A lane owns one unit: one record (the 8-byte path) or two records side by side along x (the
16-byte path, taken where nx and delta = (s.z * ny + s.y) * nx + s.x are even, after each |s_a| was clamped to n_a).  A workgroup takes
256 consecutive units per round; the grid has min(ceil(n / 256), 1024) workgroups, so a round is `stride` = that times 256 units and unit
L of one round is unit L + stride of the next.  The lane divides once, L -> (i, j, k) with i in units along x, and from then on steps
(i, j, k) by the stride's own (di, dj, dk) with two carries: i past the row's end carries into j (the column carry), j past the slice's
end carries into k (the row carry).  rounds_and_carries() below walks that in numpy and says which carries a case exercises.

    131x65x62        52 864 units step without a carry, 5 408 with the column carry only, 186 558 with the row carry only, 20 956 with
                     both; for 403 of them the row carry fires only because the column carry did (j + dj == ny - 1)
    258x47x90        191 196 / 26 320 / 57 178 / 8 832, and 736                             (in pairs: nxu == 129)
    101x89x97        the row carry fires only because of the column carry for 3 283 units   (four rounds)
    1024x3x180, 1024x1x540    di == 0: the column carry never fires, as it must not

67x63x63, the smallest volume past one grid of the integration's tests, is deliberately absent: its second round has 3 779 units, which
all start in slice 0 at rows 0 .. 56: the column carry fires for 2 240 of them, the row carry for none, alone or with it, and k only ever
takes dk.  That is why check_big() asserts these classes instead of assuming them.
"""
import functools

import numpy as np

from tests import volume_ref as vr
from tests import volume_window_ref as wr

F = np.float32
BLOCK, MAX_GRID = 256, 1024  # kVolumeBlock, kIntegrateGrid
FRESH_TSDF, FRESH_WEIGHT = np.uint32(0x3F800000), np.uint32(0)  # {1.0f, 0.0f}
CARRY_CLASSES = ("none", "column", "row", "both")

# the bit patterns of test_gpu_special_values_survive_both_paths (an upload wants weight >= 0: -0 passes, no NaN, nothing negative)
SPECIAL_TSDF = np.array([0x7FC12345, 0xFFC00001, 0x7FFFFFFF, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000], np.uint32)
SPECIAL_WEIGHT = np.array([0x80000000, 0x00000001, 0x007FFFFF, 0x7F800000, 0x00000000], np.uint32)
N_SPECIAL = 400


def _volume(nx, ny, nz):
    return dict(vr.SCENE, nx=nx, ny=ny, nz=nz)  # (the geometry plays no part in a shift: any finite one)


def _big(nx, ny, nz, shift, record_bytes, units, rounds, tail):
    return dict(params=_volume(nx, ny, nz), shift=shift, record_bytes=record_bytes, units=units, rounds=rounds, tail=tail)


BIG_SHIFTS = {
    # all carries; the last workgroup has 58 units, inside its first wave
    "131x65x62": _big(131, 65, 62, (3, -2, 1), 8, 527930, 3, 58),
    # the counters add up over four rounds
    "101x89x97": _big(101, 89, 97, (-5, 7, -9), 8, 871933, 4, 253),
    # all carries on pairs
    "258x47x90": _big(258, 47, 90, (-2, 5, -7), 16, 545670, 3, 134),
    # the same bytes through the other path
    "258x47x90 odd": _big(258, 47, 90, (1, 0, 0), 8, 1091340, 5, 12),
    # nx at the maximum: nxu == 512 divides the stride, di == 0; dj == 2 of ny == 3
    "1024x3x180": _big(1024, 3, 180, (-4, 1, 2), 16, 276480, 2, 0),
    # ny == 1: di == dj == 0, dk == 512
    "1024x1x540": _big(1024, 1, 540, (6, 0, -3), 16, 276480, 2, 0),
    # kMove == false past one grid: the count alone, on pairs (delta == 0 is even)
    "258x47x90 zero": _big(258, 47, 90, (0, 0, 0), 0, 545670, 3, 134),
}
ALL_CLASSES = ("131x65x62", "258x47x90", "101x89x97")  # every class of step and the sub-class must occur
NO_COLUMN_CARRY = ("1024x3x180", "1024x1x540")

SMALL = {"16x12x10": dict(vr.SCENE), "15x7x5": dict(nx=15, ny=7, nz=5, voxel_size=0.1, origin=(-0.7, -0.3, 0.7), trunc=0.3, max_weight=2.0)}


def _extremes():
    out = []
    for name, p in SMALL.items():
        dims = (p["nx"], p["ny"], p["nz"])
        for a in range(3):
            for m in (dims[a] - 1, dims[a], dims[a] + 1, dims[a] + 1001):
                for sign in (1, -1):
                    for others in ((0, 0), (1, -2)):
                        s = [0, 0, 0]
                        s[a], s[(a + 1) % 3], s[(a + 2) % 3] = sign * m, others[0], others[1]
                        out.append((name, tuple(s)))
    # odd before the clamp and even after it; everything leaves through y, through z
    out += [("16x12x10", (17, 0, 0)), ("16x12x10", (-17, 1, 0)), ("16x12x10", (0, 12, 0)), ("16x12x10", (0, 0, -10))]
    return list(dict.fromkeys(out))  # (three of the four are among the above already: named here so that they stay)


EXTREMES = _extremes()


# ---- the path -------------------------------------------------------------------------------------------------------------------------------
def clamp(dims, s):
    """The shift as the kernel takes it (side_stage.hpp, clamped_shift): each component brought into [-n_a, n_a]."""
    return tuple(max(-n, min(n, int(v))) for n, v in zip(dims, s))


def record_bytes(dims, s):
    """What flame_nltgv2_shift_view.record_bytes must say: 0 for a zero shift; else 16 where nx and the linear displacement OF THE CLAMPED
    shift are even, 8 otherwise.  (17, 0, 0) on nx == 16 is clamped to (16, 0, 0): odd before, even after, so 16."""
    if not any(int(v) for v in s):
        return 0
    c = clamp(dims, s)
    delta = (c[2] * dims[1] + c[1]) * dims[0] + c[0]
    return 16 if dims[0] % 2 == 0 and delta % 2 == 0 else 8


def units_of(case):
    """-> (nxu, ny, nz, records per unit) of the kernel instance that runs the case; a zero shift has delta == 0: pairs where nx is even."""
    p = case["params"]
    dims = (p["nx"], p["ny"], p["nz"])
    pair = dims[0] % 2 == 0 and (record_bytes(dims, case["shift"]) in (0, 16))
    return (dims[0] // 2 if pair else dims[0]), dims[1], dims[2], (2 if pair else 1)


def stride_of(n):
    return min(-(-n // BLOCK), MAX_GRID) * BLOCK


# ---- the walk -------------------------------------------------------------------------------------------------------------------------------
def carried_step(i, j, k, step, nxu, ny):
    """One round forward by carries, never by a division: (i, j, k) of unit L -> of unit L + stride, and which carries fired."""
    di, dj, dk = step
    i = i + di
    column = i >= nxu
    i = i - nxu * column
    j = j + column  # the column carry
    j = j + dj
    row = j >= ny
    j = j - ny * row
    k = k + row  # the row carry
    k = k + dk
    return i, j, k, column, row


def decompose(L, nxu, ny):
    return L % nxu, (L // nxu) % ny, L // (nxu * ny)


def rounds_and_carries(case):
    """-> dict(rounds, tail, stride, step = (di, dj, dk), none, column, row, both, row_by_column): the steps of every unit that has a next
    round, by the carries they take.  Every lane starts from the decomposition of its first unit and is carried forward from there, as in
    the kernel; each round's carried (i, j, k) must equal the decomposition of its L -- the walk's own sanity check."""
    nxu, ny, nz, _ = units_of(case)
    n = nxu * ny * nz
    stride = stride_of(n)
    step = (stride % nxu, (stride // nxu) % ny, stride // (nxu * ny))
    L = np.arange(min(stride, n), dtype=np.int64)
    i, j, k = decompose(L, nxu, ny)
    counts = dict.fromkeys(CARRY_CLASSES + ("row_by_column",), 0)
    rounds = 1
    while True:
        live = L + stride < n
        if not live.any():
            break
        L, i, j, k = L[live], i[live], j[live], k[live]
        by_column = (j + step[1] == ny - 1)
        i, j, k, column, row = carried_step(i, j, k, step, nxu, ny)
        L = L + stride
        want = decompose(L, nxu, ny)
        assert np.array_equal(i, want[0]) and np.array_equal(j, want[1]) and np.array_equal(k, want[2]), \
            "round %d: the carried (i, j, k) is not L decomposed" % (rounds + 1)
        assert np.all((i < nxu) & (j < ny) & (k < nz))
        counts["none"] += int(np.count_nonzero(~column & ~row))
        counts["column"] += int(np.count_nonzero(column & ~row))
        counts["row"] += int(np.count_nonzero(~column & row))
        counts["both"] += int(np.count_nonzero(column & row))
        counts["row_by_column"] += int(np.count_nonzero(column & by_column))
        rounds += 1
    assert sum(counts[c] for c in CARRY_CLASSES) == max(0, n - stride)
    return dict(rounds=rounds, tail=n % BLOCK, stride=stride, step=step, units=n, **counts)


# ---- the content ----------------------------------------------------------------------------------------------------------------------------
def special_places(case):
    """Record indices that must hold special values: the last partial workgroup's, and the first units' of the second and third round."""
    nxu, ny, nz, per = units_of(case)
    n = nxu * ny * nz
    stride, tail = stride_of(n), (nxu * ny * nz) % BLOCK
    units = list(range(n - tail, n))[:16] + list(range(n - tail, n))[-16:]
    for r in (1, 2):
        units += [u for u in range(r * stride, r * stride + 16) if u < n]
    return np.unique(np.asarray([u * per + c for u in units for c in range(per)], np.int64))


def content_of(case, seed):
    """random_content for any dict(params, shift): a fresh pair of arrays."""
    p = case["params"]
    shape = (p["nz"], p["ny"], p["nx"])
    n = shape[0] * shape[1] * shape[2]
    rng = np.random.default_rng(seed)
    t = rng.uniform(-1, 1, shape).astype(F).view(np.uint32).reshape(-1)
    w = (F(2) - rng.uniform(0, 2, shape).astype(F)).astype(F)  # (0, 2]
    w = np.where(rng.random(shape) < 0.5, F(0), w).astype(F).view(np.uint32).reshape(-1)
    k = min(N_SPECIAL, n // 4)
    t[rng.choice(n, k, replace=False)] = np.resize(SPECIAL_TSDF, k)
    w[rng.choice(n, k, replace=False)] = np.resize(SPECIAL_WEIGHT, k)
    at = special_places(case)
    t[at] = np.resize(SPECIAL_TSDF, at.size)
    w[at] = np.resize(SPECIAL_WEIGHT, at.size)
    t, w = t.view(F).reshape(shape), w.view(F).reshape(shape)
    assert np.all(w >= 0)  # what an upload wants
    return t, w


@functools.lru_cache(maxsize=None)
def random_content(name, seed=11):
    """-> (tsdf, weight) of BIG_SHIFTS[name] or SMALL[name], float32 (nz, ny, nx), computed once, shared and read-only: tsdf uniform in
    [-1, 1], weight 0 for about half of the voxels and in (0, 2] for the rest, a few hundred special bit patterns scattered over both and
    placed in the last partial workgroup and in the first units of the second and third round."""
    t, w = content_of(BIG_SHIFTS[name] if name in BIG_SHIFTS else dict(params=SMALL[name], shift=(1, 0, 0)), seed)
    t.setflags(write=False), w.setflags(write=False)
    return t, w


def volume_of(params, content):
    v = wr.Volume(**params)
    v.tsdf, v.weight = content[0].copy(), content[1].copy()
    return v


# ---- the shift by hand ----------------------------------------------------------------------------------------------------------------------
def by_hand(before, s):
    """The shift stated without slices: for every destination index, gather the record of source (i, j, k) + s by integer index arrays where
    that lies in the volume, else write {1.0f, 0.0f}; on uint32 views; the counters by direct counts over the SOURCE records.
    before: a volume (tsdf, weight as (nz, ny, nx)); -> (tsdf, weight, counters)."""
    nz, ny, nx = before.tsdf.shape
    n = nx * ny * nz
    s = [int(v) for v in s]
    t, w = vr.bits(before.tsdf).reshape(-1), vr.bits(before.weight).reshape(-1)
    seen = np.ascontiguousarray(before.weight, F).reshape(-1) > F(0)
    L = np.arange(n, dtype=np.int64)
    i, j, k = L % nx, (L // nx) % ny, L // (nx * ny)

    def inside(a, b, c):
        return (a >= 0) & (a < nx) & (b >= 0) & (b < ny) & (c >= 0) & (c < nz)

    has_source = inside(i + s[0], j + s[1], k + s[2])  # destination L
    src = (((k + s[2]) * ny + (j + s[1])) * nx + (i + s[0]))[has_source]
    out_t, out_w = np.full(n, FRESH_TSDF, np.uint32), np.full(n, FRESH_WEIGHT, np.uint32)
    out_t[has_source], out_w[has_source] = t[src], w[src]
    stays = inside(i - s[0], j - s[1], k - s[2])  # source L
    counters = dict(kept=int(np.count_nonzero(stays)), kept_seen=int(np.count_nonzero(stays & seen)),
                    lost_seen=int(np.count_nonzero(~stays & seen)), entered=int(np.count_nonzero(~has_source)))
    return out_t.view(F).reshape(nz, ny, nx), out_w.view(F).reshape(nz, ny, nx), counters


def assert_same_as_by_hand(got, hand, what=""):
    """got: dict(tsdf, weight) or a Volume; hand: by_hand's result.  Bit for bit."""
    for key, want in (("tsdf", hand[0]), ("weight", hand[1])):
        g = got[key] if isinstance(got, dict) else getattr(got, key)
        bad = np.flatnonzero((vr.bits(g) != vr.bits(want)).reshape(-1))
        assert bad.size == 0, f"{what}: {key} differs from the shift by hand at {bad[:8]} ({bad.size} of {want.size})"


def kept_boxes(dims, s):
    """-> (destination slices, source slices) of the box a shift by s keeps, as [k, j, i] index tuples; None if nothing is kept."""
    if any(abs(int(s[a])) >= dims[a] for a in range(3)):
        return None
    dst = [slice(max(0, -int(s[a])), min(dims[a], dims[a] - int(s[a]))) for a in range(3)]
    src = [slice(d.start + int(s[a]), d.stop + int(s[a])) for a, d in enumerate(dst)]
    return (dst[2], dst[1], dst[0]), (src[2], src[1], src[0])


def assert_back_again(got, original, s, what=""):
    """After shift(s) and shift(-s): the box kept by the first shift holds its original bytes, the rest is fresh.
    got: dict(tsdf, weight) or a Volume; original: (tsdf, weight)."""
    shape = original[0].shape
    dims = (shape[2], shape[1], shape[0])
    want_t, want_w = np.full(shape, FRESH_TSDF, np.uint32), np.full(shape, FRESH_WEIGHT, np.uint32)
    boxes = kept_boxes(dims, s)
    if boxes is not None:
        _, src = boxes  # the sources of the first shift are back where they were
        want_t[src], want_w[src] = vr.bits(original[0])[src], vr.bits(original[1])[src]
    assert_same_as_by_hand(got, (want_t.view(F), want_w.view(F)), what)


# ---- the preconditions ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def content_rounds(name):
    """Per round of the walk over BIG_SHIFTS[name] with its random content, in records: (kept and seen, kept and unseen, lost and seen, lost
    and unseen, entered)."""
    case = BIG_SHIFTS[name]
    p = case["params"]
    nx, ny, nz = p["nx"], p["ny"], p["nz"]
    nxu, _, _, per = units_of(case)
    stride = stride_of(nxu * ny * nz) * per  # in records
    s = case["shift"]
    seen = random_content(name)[1].reshape(-1) > F(0)
    L = np.arange(nx * ny * nz, dtype=np.int64)
    i, j, k = L % nx, (L // nx) % ny, L // (nx * ny)
    stays = (i - s[0] >= 0) & (i - s[0] < nx) & (j - s[1] >= 0) & (j - s[1] < ny) & (k - s[2] >= 0) & (k - s[2] < nz)
    enters = ~((i + s[0] >= 0) & (i + s[0] < nx) & (j + s[1] >= 0) & (j + s[1] < ny) & (k + s[2] >= 0) & (k + s[2] < nz))
    out = []
    for lo in range(0, L.size, stride):
        r = slice(lo, lo + stride)
        out.append(tuple(int(np.count_nonzero(c[r])) for c in (stays & seen, stays & ~seen, ~stays & seen, ~stays & ~seen, enters)))
    return out


def check_big(name):
    """What BIG_SHIFTS[name] must show on the CPU before the device is asked: the rounds, the path and the tail of its table row, the
    carries it is there for, and content that makes every round change every counter."""
    case = BIG_SHIFTS[name]
    p = case["params"]
    dims = (p["nx"], p["ny"], p["nz"])
    nxu, ny, nz, per = units_of(case)
    walk = rounds_and_carries(case)
    print("%s shift %s: %d units of %d bytes, %d rounds of %d, tail %d, step %s; steps without a carry %d, column only %d, row only %d, "
          "both %d; row carry by the column carry alone %d"
          % (name, case["shift"], walk["units"], 8 * per, walk["rounds"], walk["stride"], walk["tail"], walk["step"], walk["none"],
             walk["column"], walk["row"], walk["both"], walk["row_by_column"]))
    assert record_bytes(dims, case["shift"]) == case["record_bytes"] and 8 * per == (case["record_bytes"] or 16)
    assert walk["units"] == case["units"] == nxu * ny * nz > MAX_GRID * BLOCK
    assert walk["rounds"] == case["rounds"] and walk["tail"] == case["tail"]
    if name in ALL_CLASSES:
        assert min(walk[c] for c in CARRY_CLASSES) > 0 and walk["row_by_column"] > 0, walk
    if name in NO_COLUMN_CARRY:
        assert walk["step"][0] == 0 and walk["column"] == walk["both"] == walk["row_by_column"] == 0, walk
        assert (walk["row"] > 0) == (ny > 1), walk  # (with ny == 1 and no column carry j stays 0)
    rounds = content_rounds(name)
    print("  per round (kept seen, kept unseen, lost seen, lost unseen, entered):", rounds)
    assert len(rounds) == case["rounds"]
    moves = any(case["shift"])
    for r in rounds:
        kept, lost = r[0] + r[1], r[2] + r[3]
        # (a round may lie wholly in the slices that leave: the last one of 258x47x90 does)
        assert (min(r[0], r[1]) > 0 or kept == 0) and (min(r[2], r[3]) > 0 or lost == 0), rounds
        assert (lost > 0 and r[4] > 0) if moves else (lost == 0 and r[4] == 0 and kept > 0), rounds
    assert sum(1 for r in rounds if r[0] + r[1] > 0 and r[2] + r[3] > 0) >= (2 if moves else 0), rounds
    # specials where a round begins and where the last workgroup ends
    at = special_places(case)
    t, w = random_content(name)
    assert at.size >= 16 * per and np.all(np.isin(vr.bits(t).reshape(-1)[at], SPECIAL_TSDF))
    assert np.all(np.isin(vr.bits(w).reshape(-1)[at], SPECIAL_WEIGHT))
    return walk
