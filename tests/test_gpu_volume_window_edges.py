"""flame_nltgv2_volume_shift* past one grid of k_volume_shift, at the extremes of a shift and around the swap of the volume's two buffers,
with the cases and preconditions of tests/volume_window_cases.py through the helpers of tests/test_gpu_volume_window.py.  Everything is
bit for bit against tests/volume_window_ref.py and against the shift stated by hand (volume_window_cases.by_hand): a shift moves bit
patterns and counts integers, so nothing here has a tolerance and every voxel of every case is compared."""
import numpy as np
import pytest

from tests import test_gpu_volume_window as tw
from tests import volume_mesh_ref as vmr
from tests import volume_ref as vr
from tests import volume_window_cases as wc
from tests import volume_window_ref as wr
from tests.metric_helpers import on_device

gpu, reg = tw.gpu, tw.reg  # the module-scoped fixtures of the window's tests


def dims_of(p):
    return (p["nx"], p["ny"], p["nz"])


def upload(reg, ref, content, what):
    ref.tsdf, ref.weight = content[0].copy(), content[1].copy()
    reg.volume_upload(ref.tsdf, ref.weight)
    vr.assert_same_volume(reg.volume_download(), ref, what + ", up and down")


def shift_both_ways(reg, ref, s, what, record_bytes=None):
    """tw.shift (the checker: counters, base, path, both arrays), then the same download and counters against the shift by hand."""
    hand = wc.by_hand(ref, s)
    dims = (ref.nx, ref.ny, ref.nz)
    got, want = tw.shift(reg, ref, s, what, record_bytes=wc.record_bytes(dims, s) if record_bytes is None else record_bytes)
    assert {k: got[k] for k in wr.SHIFT_COUNTERS} == hand[2], what
    wc.assert_same_as_by_hand(reg.volume_download(), hand, what)
    return got, want


def fresh_volume(reg, ref, what):
    ref.reset()
    vr.assert_same_volume(reg.volume_download(), ref, what)
    assert np.all(vr.bits(ref.tsdf) == wc.FRESH_TSDF) and not vr.bits(ref.weight).any()


# ---- A: past one grid -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(wc.BIG_SHIFTS))
def test_gpu_shifts_past_one_grid(gpu, reg, name):
    """Two to five rounds of the grid-stride loop on both paths and on the count-only instance: the carried (i, j, k) decides keep and
    enters from the second round on (a wrong carry leaves every record at the right linear place and wraps rows round the window's
    faces), the counters add up over the rounds with the lanes past n in the ballots, the counter slot is that of the capped grid.  Then
    back by -s: the mirror image, keep decided from the other side, the second swap of the buffers."""
    wc.check_big(name)  # the CPU alone first: rounds, path, tail, every class of carry, every counter changed by every round
    case = wc.BIG_SHIFTS[name]
    s, content = case["shift"], wc.random_content(name)
    ref = tw.create(gpu, reg, **case["params"])
    upload(reg, ref, content, name)
    got, want = shift_both_ways(reg, ref, s, name, record_bytes=case["record_bytes"])
    rounds = wc.content_rounds(name)
    assert got["kept_seen"] == sum(r[0] for r in rounds) and got["lost_seen"] == sum(r[2] for r in rounds)
    assert got["kept"] == sum(r[0] + r[1] for r in rounds) and got["entered"] == sum(r[4] for r in rounds)
    back = tuple(-c for c in s)
    got, _ = shift_both_ways(reg, ref, back, name + " and back")
    assert got["base"].tolist() == [0, 0, 0]
    wc.assert_back_again(reg.volume_download(), content, s, name + " and back")


# ---- B: the two paths -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_both_paths_give_the_same_bytes_past_one_grid(gpu, reg):
    case = wc.BIG_SHIFTS["258x47x90"]
    content = wc.random_content("258x47x90")
    ref = tw.create(gpu, reg, **case["params"])
    upload(reg, ref, content, "pairs")
    tw.shift(reg, ref, (2, 0, 0), "pairs", record_bytes=16)
    pairs = reg.volume_download()
    ref = tw.create(gpu, reg, **case["params"])
    upload(reg, ref, content, "single records")
    for n in range(2):
        tw.shift(reg, ref, (1, 0, 0), "single records, shift %d" % n, record_bytes=8)
    singles = reg.volume_download()
    nx = case["params"]["nx"]
    for k, fresh in (("tsdf", wc.FRESH_TSDF), ("weight", wc.FRESH_WEIGHT)):
        a, b, c = vr.bits(pairs[k]), vr.bits(singles[k]), vr.bits(content[0 if k == "tsdf" else 1])
        # the kept boxes of (2, 0, 0) and of (1, 0, 0) twice are the same columns; the two fresh columns
        assert np.array_equal(a[:, :, :nx - 2], b[:, :, :nx - 2]) and np.array_equal(a[:, :, :nx - 2], c[:, :, 2:]), k
        assert np.all(a[:, :, nx - 2:] == fresh) and np.all(b[:, :, nx - 2:] == fresh), k


# ---- C: the count alone -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_the_count_of_a_zero_shift_past_one_grid(gpu, reg):
    case = wc.BIG_SHIFTS["258x47x90 zero"]
    content = wc.random_content("258x47x90 zero")
    n = content[0].size
    tw.create(gpu, reg, **wc.SMALL["15x7x5"])  # another size first: the next create frees both buffers and takes one
    ref = tw.create(gpu, reg, **case["params"])
    upload(reg, ref, content, "before the count")
    assert reg.volume_info()["device_bytes"] == 8 * n
    got = reg.volume_shift((0, 0, 0))
    print("the count", got["counts"].tolist(), "device_ms %.3f" % got["device_ms"])
    assert got["kept"] == n and got["kept_seen"] == np.count_nonzero(content[1] > 0) and 0 < got["kept_seen"] < n
    assert got["lost_seen"] == got["entered"] == 0 and got["record_bytes"] == 0 and got["counts"][4:].tolist() == [0, 0, 0, 0]
    assert got["base"].tolist() == reg.volume_window().tolist() == [0, 0, 0]
    assert reg.volume_info()["device_bytes"] == 8 * n  # nothing allocated, nothing swapped
    vr.assert_same_volume(reg.volume_download(), ref, "after the count")
    # ... and with a second buffer in place the count still reads the live one
    tw.shift(reg, ref, (1, 0, 0), "a moving shift", record_bytes=8)
    assert reg.volume_info()["device_bytes"] == 2 * 8 * n
    got, want = tw.shift(reg, ref, (0, 0, 0), "the count after a swap", record_bytes=0)
    assert got["kept_seen"] == np.count_nonzero(ref.weight > 0) and reg.volume_info()["device_bytes"] == 2 * 8 * n


# ---- D: the extremes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,s", wc.EXTREMES, ids=["%s %d %d %d" % ((name,) + s) for name, s in wc.EXTREMES])
def test_gpu_extreme_shifts(gpu, reg, name, s):
    """One plane kept, nothing kept through each face, and shifts past the volume, which the kernel takes clamped to +-n (the parity of
    s.x and with it the path may change) and the base unclamped."""
    p = wc.SMALL[name]
    ref = tw.create(gpu, reg, **p)
    upload(reg, ref, wc.random_content(name), name)
    got, want = shift_both_ways(reg, ref, s, "%s %s" % (name, s))
    assert got["base"].tolist() == list(s)
    assert (got["kept"] == 0) == any(abs(s[a]) >= dims_of(p)[a] for a in range(3))
    assert got["kept_seen"] + got["lost_seen"] == np.count_nonzero(wc.random_content(name)[1] > 0)


# ---- E: the live buffer after a swap ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_reset_upload_and_create_after_a_shift(gpu, reg):
    """volume_release frees the shift's second buffer with the first (nltgv2_frame_capi.hip), so a create of another size starts from one
    buffer and the next moving shift takes a second of the new size; a create of the same byte size keeps both."""
    tw.create(gpu, reg, **wc.SMALL["15x7x5"])  # (so that the scene starts from one buffer, whatever ran before)
    ref = tw.create(gpu, reg, **vr.SCENE)
    content = wc.random_content("16x12x10")
    upload(reg, ref, content, "the scene")
    assert reg.volume_info()["device_bytes"] == 8 * 1920
    for swaps, s in ((1, (3, -2, 1)), (2, (2, 0, -1))):  # an odd and an even number of swaps
        shift_both_ways(reg, ref, s, "swap %d" % swaps)
        assert reg.volume_info()["device_bytes"] == 2 * 8 * 1920
        base = ref.base.tolist()
        reg.volume_reset()
        fresh_volume(reg, ref, "reset after %d swaps" % swaps)
        assert reg.volume_window().tolist() == base != [0, 0, 0]
        upload(reg, ref, content, "upload after %d swaps" % swaps)
        assert reg.volume_window().tolist() == base
    shift_both_ways(reg, ref, (-1, 1, 0), "a third swap")
    # the same byte size under other dimensions: both buffers stay
    other = dict(vr.SCENE, nx=10, ny=16, nz=12)
    ref = tw.create(gpu, reg, **other)
    assert reg.volume_info()["device_bytes"] == 2 * 8 * 1920 and reg.volume_window().tolist() == [0, 0, 0]
    assert dims_of(reg.volume_info()) == (10, 16, 12)
    fresh_volume(reg, ref, "created with the same bytes")
    upload(reg, ref, wc.content_of(dict(params=other, shift=(1, 0, 0)), 12), "10x16x12")
    shift_both_ways(reg, ref, (-3, 2, 1), "10x16x12", record_bytes=8)
    shift_both_ways(reg, ref, (2, -5, 3), "10x16x12 again", record_bytes=16)
    assert reg.volume_info()["device_bytes"] == 2 * 8 * 1920
    # another size, smaller and then larger than what the second buffer was: one buffer, then two of the new size
    for name, p, s in (("15x7x5", wc.SMALL["15x7x5"], (1, -1, 2)), ("67x9x5", dict(vr.SCENE, nx=67, ny=9, nz=5), (-2, 3, 1))):
        n = p["nx"] * p["ny"] * p["nz"]
        ref = tw.create(gpu, reg, **p)
        assert reg.volume_info()["device_bytes"] == 8 * n and reg.volume_window().tolist() == [0, 0, 0]
        fresh_volume(reg, ref, name + " created")
        upload(reg, ref, wc.content_of(dict(params=p, shift=s), 13), name)
        tw.shift(reg, ref, (0, 0, 0), name + ", a zero shift", record_bytes=0)
        assert reg.volume_info()["device_bytes"] == 8 * n
        shift_both_ways(reg, ref, s, name)
        assert reg.volume_info()["device_bytes"] == 2 * 8 * n
        shift_both_ways(reg, ref, tuple(-c for c in s), name + " and back")
        assert reg.volume_info()["device_bytes"] == 2 * 8 * n


# ---- F: stages queued around a shift ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_stages_queued_before_a_shift_answer_for_the_volume_before_it(gpu, reg):
    """A raycast and a mesh begun before a shift and ended after it (and after an integration into the shifted window) are those of the
    volume before the swap.  Every _begin waits for the side stream, so this is the bookkeeping across the swap, not a race."""
    s = (3, -2, 1)
    ref = tw.create(gpu, reg, **vr.SCENE)
    m = vr.scene_map()
    tw.integrate(gpu, reg, ref, m, vr.SCENE_K, vr.IDENTITY, "the scene")
    T = vr.shifted_pose(0.15)
    want_view = ref.raycast(vr.SCENE_KINV, T, vr.SCENE_ROWS, vr.SCENE_COLS, **vr.SCENE_RAYCAST)
    want_mesh = wr.extract(ref)
    assert want_view["hits"] > 0 and want_mesh["n_triangles"] > 0
    keep = on_device(m)
    reg.volume_raycast_begin(vr.SCENE_KINV, T, vr.SCENE_ROWS, vr.SCENE_COLS, gpu.RaycastParams(**vr.SCENE_RAYCAST))
    reg.volume_mesh_begin(gpu.VolumeMeshParams(max_vertices=want_mesh["n_vertices"], max_triangles=want_mesh["n_triangles"]))
    reg.volume_shift_begin(s)
    assert reg.volume_window().tolist() == list(s)
    kw = dict(weight=0.5)
    reg.volume_integrate_begin(vr.SCENE_K, vr.shifted_pose(0.3), *m.shape, gpu.IntegrateParams(map_device=keep.data_ptr(), **kw))
    got_integration = reg.volume_integrate_end()
    got_shift = reg.volume_shift_end()
    got_mesh = reg.volume_mesh_end()
    got_view = reg.volume_raycast_end()
    # the checker's sequence
    hand = wc.by_hand(ref, s)
    want_shift = ref.shift(s)
    with np.errstate(all="ignore"):
        want_integration = ref.integrate(m, vr.SCENE_K, vr.shifted_pose(0.3), **kw)
    vr.assert_same_counts(got_view, want_view, vr.RAYCAST_COUNTERS, "the raycast before the shift")
    vr.assert_same_map(got_view["map"], want_view["map"], "the raycast before the shift")
    vmr.assert_same_mesh(got_mesh, want_mesh, "the mesh before the shift")
    wr.assert_same_counts(got_shift, want_shift, "the shift between")
    assert hand[2] == want_shift and got_shift["shift"].tolist() == got_shift["base"].tolist() == list(s) and got_shift["record_bytes"] == 8
    vr.assert_same_counts(got_integration, want_integration, vr.INTEGRATE_COUNTERS, "the integration after the shift")
    assert want_integration["updated"] > 0 and want_shift["lost_seen"] > 0 and want_shift["kept_seen"] > 0
    vr.assert_same_volume(reg.volume_download(), ref, "after the sequence")
    # and the same two stages now answer for the shifted volume: not what they were
    after = reg.volume_mesh()
    vmr.assert_same_mesh(after, wr.extract(ref), "the mesh after the sequence")
    assert after["n_vertices"] != got_mesh["n_vertices"] or not np.array_equal(vr.bits(after["vertices"]), vr.bits(got_mesh["vertices"]))
