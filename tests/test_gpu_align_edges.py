"""The direct alignment past 2048 chunks and the pyramid's remaining sizes, against the checker (tests/align_ref.py) as bits: a frame whose
linearisation gives every workgroup but the last two chunks of 1024 pixels -- the loop over a workgroup's chunks, the reuse of its LDS
from one chunk to the next, the clamp of the last workgroup's range -- and pyramids of five levels, of the smallest legal source and of
many tiles in both directions.  The checker runs alone first and must show that nothing passes by being empty."""
import time

import numpy as np
import pytest

from tests import align_cases as ac
from tests import align_ref as ar
from tests.test_gpu_align import _assert_level, _reference, _tracker

pytestmark = pytest.mark.gpu
F = np.float32
MAX_GROUPS = 2048  # kAlignMaxGroups


def test_gpu_linearisation_of_more_than_2048_chunks(built):
    """1448 x 1449 = 2 098 152 pixels: 2049 chunks, the smallest frame at which a workgroup takes more than one: 1025 workgroups of two
    chunks, the last with one chunk of 1000 pixels; the partials are combined strided in three rounds, then pairwise."""
    import torch
    from flame_amd.stereo import AlignParams

    w, h, K = 1448, 1449, (1024.0, 1024.0, 724.0, 724.0)
    chunks = (w * h + 1023) // 1024
    per_group = (chunks + MAX_GROUPS - 1) // MAX_GROUPS
    groups = (chunks + per_group - 1) // per_group
    assert (chunks, per_group, groups) == (2049, 2, 1025) and chunks - (groups - 1) * per_group == 1 and w * h - (chunks - 1) * 1024 == 1000
    assert ((w - 1) * h + 1023) // 1024 <= MAX_GROUPS and (w * (h - 1) + 1023) // 1024 <= MAX_GROUPS  # no smaller frame of this shape reaches it
    r0, n0 = ac.driver_scene()[:2]
    ref, new = (np.ascontiguousarray(np.tile(a, (21, 16))[:h, :w]) for a in (r0, n0))
    assert ref.shape == (h, w)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    d = (0.5 + 0.2 * np.sin(xx / 97.0) * np.cos(yy / 61.0)).astype(F)
    q, t = ac.small_pose()
    t0 = time.perf_counter()
    want = _reference(ar.build_pyramid(ref, 1), ar.build_pyramid(new, 1), d, 0, K, 2, 10.0, q, t)
    print("the checker's linearisation of 2049 chunks: %.2f s" % (time.perf_counter() - t0), {n: want[n] for n in ar.COUNTS})
    assert want["n_used"] > 1800 * 1024 and want["n_outside"] > 0 and want["n_huber"] > 0 and np.count_nonzero(want["sums"]) == 28
    # the second chunk of a workgroup matters: the odd chunks alone hold used pixels
    odd = want["px"]["used"].reshape(-1)[:2048 * 1024].reshape(1024, 2, 1024)[:, 1]
    assert np.count_nonzero(odd) > 900 * 1024
    P = AlignParams(border=2, huber_k=10.0)
    with _tracker(w, h, K) as tr:
        tr.add_frame(1, ref)
        tr.add_frame(2, new)
        host = tr.align_linearize(P, 1, 2, 0, d, q, t)
        ar.assert_same_system(host, want, "2049 chunks, map from the host")
        dev = torch.from_numpy(d.copy()).cuda()
        torch.cuda.synchronize()
        first = tr.align_linearize(P, 1, 2, 0, int(dev.data_ptr()), q, t)
        again = tr.align_linearize(P, 1, 2, 0, int(dev.data_ptr()), q, t)
        ar.assert_same_system(first, want, "2049 chunks, map from a device buffer")
        assert first["sums"].tobytes() == again["sums"].tobytes() and all(first[n] == again[n] for n in ar.COUNTS)


@pytest.mark.parametrize("w,h,n_levels", [(64, 49, 5), (7, 7, 2), (641, 479, 4)])
def test_gpu_pyramids_of_the_remaining_sizes(built, w, h, n_levels):
    """64 x 49 over five levels, the most the API allows, ends at 4 x 4; 7 x 7 -> 4 x 4 is the smallest legal source: the 5 x 5 window
    reflects across the whole staged tile; 641 x 479 -> 321 x 240 -> 161 x 120 -> 81 x 60: many tiles in both directions, odd and even
    halvings."""
    assert ar.levels_valid(w, h, n_levels) and (n_levels == 4 or not ar.levels_valid(w, h, n_levels + 1))
    img = ac.random_image(w, h, 200 + w)
    want = ar.build_pyramid(img, n_levels)
    assert [p[0].shape for p in want] == [ar.level_size(w, h, l)[::-1] for l in range(n_levels)]
    assert all(np.ptp(p[0]) > 0 and np.abs(p[1]).max() > 0 and np.abs(p[2]).max() > 0 for p in want)  # nothing flat
    with _tracker(w, h, (64.0, 64.0, w / 2, h / 2)) as tr:
        tr.add_frame(7, img)
        tr.build_pyramid(7, n_levels)
        for l in range(n_levels):
            _assert_level(tr.download_pyramid_level(7, l), want[l], "%dx%d level %d" % (w, h, l))
