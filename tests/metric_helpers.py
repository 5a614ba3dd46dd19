"""What the tests of the metric outputs share (tests/test_metric_outputs.py, tests/test_gpu_metric_outputs*.py): cameras, poses, the
map of special values, and the way a GPU test gets an array into and out of device memory."""
import ctypes as C
import re

import numpy as np

F = np.float32
INF = float("inf")


def pinhole_kinv(fx=525.0, fy=520.0, cx=330.5, cy=230.25):
    """Kinv of a pinhole camera with an off-centre principal point, rounded to float32; its last row is (0, 0, 1)."""
    return np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]], np.float64).astype(F)


def kinv_for(cols, rows):
    return pinhole_kinv(fx=0.82 * cols, fy=0.81 * cols, cx=0.5 * cols + 10.5, cy=0.5 * rows - 9.75)


def rot_z(deg, t=(0.25, -1.5, 3.0)):
    """T_world_cam (3, 4): a rotation about the optical axis and a translation."""
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, 0, t[0]], [s, c, 0, t[1]], [0, 0, 1, t[2]]], np.float64).astype(F)


POSE = rot_z(30)


def special_map():
    """A NaN, 0, -1, +inf, the smallest denormal, a denormal whose reciprocal is finite, 1e-30 and ordinary values side by side.
    With a Kinv whose last row is (0, 0, 1), z = 1 / v: 0.5, 1 and 2 give z = 2, 1 and 0.5 exactly."""
    row = np.array([np.nan, 0.0, -1.0, INF, 1e-45, 6e-39, 1e-30, 0.5, -0.0, 2.0, -INF, 1.0], F)
    return np.stack([row, row[::-1], np.roll(row, 5)])


def on_device(a):
    """A torch tensor with the array's bytes in device memory (keep it alive while its address is in use)."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


_HIP = None


def hip_runtime():
    """The HIP runtime this process has ALREADY loaded (torch's: tests/conftest.py imports torch first so that one runtime serves the
    process), found in the process's own mappings and opened once more by its path, which hands back the loaded copy.  A second
    runtime would not know the library's allocations, so a process without exactly one is an error, not a fallback."""
    global _HIP
    if _HIP is None:
        with open("/proc/self/maps") as f:
            paths = sorted({line.split()[-1] for line in f if re.search(r"/libamdhip64\.so[.\d]*$", line.strip())})
        assert len(paths) == 1, f"expected exactly one HIP runtime loaded in this process, found {paths}"
        _HIP = C.CDLL(paths[0])
        _HIP.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _HIP.hipMemcpy.restype = C.c_int
    return _HIP


def fetch(ptr, shape, dtype):
    """The array at a device address (a view's *_device pointer), by a synchronous hipMemcpy."""
    out = np.empty(shape, dtype)
    if out.nbytes:
        rc = hip_runtime().hipMemcpy(out.ctypes.data, C.c_void_p(ptr), out.nbytes, 2)  # hipMemcpyDeviceToHost
        assert rc == 0, f"hipMemcpy from {ptr:#x} failed with {rc}"
    return out
