"""The raw-frame input stage inside the front of the per-frame chain (detect_features -> update_resident, 320x240, as
tests/test_feature_frontend.py drives it), run twice over the same three images: once through add_frame, once with every image
handed over as a BGRA8 frame with a padded stride in device memory, enqueue-only, through add_raw_frame with remap = 0.  Nothing is
distorted, grey(v, v, v) = v, so the resident feature records must be equal record for record."""
import numpy as np
import pytest

from tests import input_ref as ir
from tests.test_feature_frontend import HipSide, assert_records_equal, plane_scene

pytestmark = pytest.mark.gpu
PAD_BYTES = 5


class RawSide(HipSide):
    """Adds its frames from device memory; the buffers live until the side closes (the calls only enqueue)."""

    def __init__(self, sc, imgs):
        super().__init__(sc, imgs)
        self.tr.set_input(format=ir.BGRA8, remap=0, raw_width=sc.width, raw_height=sc.height)
        self.buffers = []

    def add_frame(self, k):
        img = self.imgs[k]
        h, w = img.shape
        rng = np.random.RandomState(k)
        raw = rng.randint(0, 256, size=(h, 4 * w + PAD_BYTES)).astype(np.uint8)  # alpha and the row padding: noise
        px = raw[:, :4 * w].reshape(h, w, 4)
        px[:, :, 0] = px[:, :, 1] = px[:, :, 2] = img
        dev = self.torch.from_numpy(raw).cuda()
        self.torch.cuda.synchronize()  # the producer's work is ordered before the call
        self.buffers.append(dev)
        assert self.tr.add_raw_frame(k, None, device_ptr=dev.data_ptr(), stride=4 * w + PAD_BYTES, want_stats=False) is None

    def close(self):
        super().close()  # (destroy waits for the stream)
        self.buffers = []


def test_gpu_chain_from_raw_device_frames_equals_the_chain_from_add_frame(built):
    sc = plane_scene(320, 240)
    imgs = {c: sc.render(c) for c in (9, 10, 11)}
    sides = [HipSide(sc, imgs), RawSide(sc, imgs)]
    try:
        for s in sides:
            for k in (9, 10):
                s.add_frame(k)
        counts = [s.detect(10, 9, None, False, 0) for s in sides]
        assert counts[0] == counts[1] > 100
        for s in sides:
            s.add_frame(11)
        stats = [s.update(11, 10, [10]) for s in sides]
        assert stats[0] == stats[1] and stats[0][0] > 0, stats
        a, b = sides[0].state(), sides[1].state()
        assert a[0].shape[0] == counts[0]
        assert_records_equal(b[0], a[0], "the resident set after the third frame")
        for k in (9, 10, 11):
            for x, y in zip(sides[0].tr.download_frame(k), sides[1].tr.download_frame(k)):
                assert x.tobytes() == y.tobytes(), "frame %d" % k
    finally:
        for s in sides:
            s.close()
