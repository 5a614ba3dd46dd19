"""ctypes mirror of include/flame_stereo.h: the per-feature epipolar inverse-depth update on MI355X.

Mirrors the reference interface of /root/reference/src/flame/flame.cc:1280-1752 (Flame::updateFeatureIDepths,
Flame::trackFeature), flame.cc:1754-1860 (Flame::projectFeatures), flame.cc:708-773 + 822-1278 (the detection loop
and Flame::detectFeatures), flame.cc:554-706 (Flame::prunePoseFrames), flame.cc:1954-1980 (the preprocessing of Flame::syncGraph) and src/flame/utils/frame.cc:33-71
(Frame::create, level 0; its further levels through build_pyramid).  The direct alignment (align_linearize, align_frame) has no
counterpart in the reference: include/flame_stereo.h is its definition.  There is no CPU path: every call fails with NLTGV2Error when the HIP library or a gfx950
device is missing.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .regularizer import NLTGV2Error, load_library, status_string

# == flame_stereo_feature == FeatureWithIDepth (flame.h:88-99)
FEATURE_DTYPE = np.dtype([("id", "<u4"), ("frame_id", "<u4"), ("x", "<f4"), ("y", "<f4"), ("idepth_mu", "<f4"),
                          ("idepth_var", "<f4"), ("valid", "u1"), ("reserved_", "u1", (3,)), ("num_updates", "<u4"),
                          ("num_dropouts", "<u4"), ("search_status", "<i4")])
assert FEATURE_DTYPE.itemsize == 40

_PARAM_FIELDS = [("min_baseline", C.c_float), ("do_letterbox", C.c_int32), ("rescale_factor_min", C.c_float),
                 ("rescale_factor_max", C.c_float), ("idepth_var_max", C.c_float), ("max_dropouts", C.c_int32),
                 ("outlier_sigma_thresh", C.c_float), ("do_meas_fusion", C.c_int32), ("win_size", C.c_int32),
                 ("search_sigma", C.c_float), ("min_grad_mag", C.c_float), ("idepth_min", C.c_float),
                 ("idepth_max", C.c_float), ("epilength_min", C.c_float), ("epilength_max", C.c_float),
                 ("process_var_factor", C.c_float), ("process_fail_var_factor", C.c_float), ("max_cost", C.c_float),
                 ("do_subpixel", C.c_int32), ("sample_dist", C.c_float), ("second_best_factor", C.c_float),
                 ("z_win_size", C.c_int32), ("pixel_var", C.c_float), ("epipolar_line_var", C.c_float)]


class StereoParams(C.Structure):
    """flame_stereo_params; defaults are the reference's (flame_stereo_default_params)."""
    _fields_ = _PARAM_FIELDS

    def __init__(self, **kw):
        super().__init__()
        _lib().flame_stereo_default_params(C.byref(self))
        for k, v in kw.items():
            if k not in dict(_PARAM_FIELDS):
                raise TypeError("unknown stereo parameter %r" % k)
            setattr(self, k, v)


class _Pose(C.Structure):
    _fields_ = [("frame_id", C.c_uint32), ("q_ref_to_new", C.c_float * 4), ("t_ref_to_new", C.c_float * 3),
                ("q_ref_to_pf", C.c_float * 4), ("t_ref_to_pf", C.c_float * 3)]


class DetectParams(C.Structure):
    """flame_stereo_detect_params: the members of flame::Params detection reads beyond StereoParams; defaults are the
    reference's (flame_stereo_default_detect_params)."""
    _fields_ = [("detection_win_size", C.c_int32), ("min_grad_mag", C.c_float), ("idepth_init", C.c_float),
                ("idepth_var_init", C.c_float)]

    def __init__(self, **kw):
        super().__init__()
        _lib().flame_stereo_default_detect_params(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("unknown detect parameter %r" % k)
            setattr(self, k, v)


FMT_GREY8, FMT_BGR8, FMT_RGB8, FMT_BGRA8, FMT_RGBA8 = range(5)  # FLAME_STEREO_FMT_*
FORMAT_BYTES = {FMT_GREY8: 1, FMT_BGR8: 3, FMT_RGB8: 3, FMT_BGRA8: 4, FMT_RGBA8: 4}


class InputParams(C.Structure):
    """flame_stereo_input_params: what the raw frames of add_raw_frame look like; defaults are
    flame_stereo_default_input_params' (GREY8, remap 0, sizes 0, K_raw = I, dist = 0).  K_raw: 9 floats, row-major; dist:
    up to 8 floats k1 k2 p1 p2 k3 k4 k5 k6 (the rest 0)."""
    _fields_ = [("format", C.c_int32), ("remap", C.c_int32), ("raw_width", C.c_int32), ("raw_height", C.c_int32),
                ("K_raw", C.c_float * 9), ("dist", C.c_float * 8)]

    def __init__(self, **kw):
        super().__init__()
        _lib().flame_stereo_default_input_params(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("unknown input parameter %r" % k)
            if k == "K_raw":
                v = (C.c_float * 9)(*[float(x) for x in _f32(v, 9)])
            elif k == "dist":
                d = np.zeros(8, np.float32)
                src = np.asarray(v, np.float32).reshape(-1)
                if src.size > 8:
                    raise ValueError("at most 8 distortion coefficients")
                d[:src.size] = src
                v = (C.c_float * 8)(*[float(x) for x in d])
            setattr(self, k, v)


class _InputStats(C.Structure):
    _fields_ = [("n_outside", C.c_int32)]


class _FeatureStats(C.Structure):
    _fields_ = [("num_features", C.c_int32), ("num_examined", C.c_int32), ("error_feature", C.c_int32)]


class _DetectionsStats(C.Structure):
    _fields_ = [("num_scored", C.c_int32), ("num_examined", C.c_int32), ("error_pixel", C.c_int32)]


class _PruneStats(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_examined", "num_moved", "num_invalidated", "num_removed", "num_features",
                                          "num_frames_dropped", "error_feature")]


class GraphParams(C.Structure):
    """flame_stereo_graph_params: the members of flame::Params that syncGraph's preprocessing reads; defaults are the
    reference's (flame_stereo_default_graph_params)."""
    _fields_ = [("idepth_var_max_graph", C.c_float), ("min_height", C.c_float), ("max_height", C.c_float),
                ("adaptive_data_weights", C.c_int32)]

    def __init__(self, **kw):
        super().__init__()
        _lib().flame_stereo_default_graph_params(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("unknown graph parameter %r" % k)
            setattr(self, k, v)


class _WorldPose(C.Structure):
    _fields_ = [("frame_id", C.c_uint32), ("q", C.c_float * 4), ("t", C.c_float * 3)]


_I32P = C.POINTER(C.c_int32)
GRAPH_COUNTERS = ("num_examined", "num_invalid", "num_fail_var", "num_fail_height", "error_feature")


class _GraphInputs(C.Structure):
    _fields_ = [("V", C.c_int32), ("feat_id", _I32P), ("pos", C.POINTER(C.c_float)), ("data_term", C.POINTER(C.c_float)),
                ("data_weight", C.POINTER(C.c_float)), ("feat_index", _I32P)] + [(n, C.c_int32) for n in GRAPH_COUNTERS]


class _Stats(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_idepth_updates", "num_fail_max_var", "num_fail_max_dropouts",
                                          "num_fail_ref_patch_grad", "num_fail_ambiguous_match", "num_fail_max_cost",
                                          "success", "error_feature")]


MATCH_KINDS = ("move_failed", "moved", "no_search_region", "no_gradient", "no_gradient_fresh", "ambiguous", "max_cost",
               "max_var_ring", "max_dropouts_ring")  # flame_stereo_matches_stats.kind_count, in order


class _MatchesStats(C.Structure):
    _fields_ = [("num_features", C.c_int32), ("kind_count", C.c_int32 * 9), ("lines_drawn", C.c_int32),
                ("lines_skipped", C.c_int32), ("rings_skipped", C.c_int32), ("refilled", C.c_int32), ("entries", C.c_int64)]


ALIGN_COUNTS = ("n_used", "n_no_depth", "n_behind", "n_outside", "n_huber")  # flame_stereo_align_system, in order
ALIGN_OK, ALIGN_TOO_FEW = 0, 1  # flame_stereo_align_result.status
ALIGN_FLAG_NOT_PD, ALIGN_FLAG_REJECTED, ALIGN_FLAG_MAX_ITERS = 1, 2, 4


class AlignParams(C.Structure):
    """flame_stereo_align_params; the defaults (flame_stereo_default_align_params) are this library's design choices."""
    _fields_ = [("border", C.c_int32), ("huber_k", C.c_float), ("coarsest_level", C.c_int32), ("finest_level", C.c_int32),
                ("max_iters_per_level", C.c_int32), ("min_pixels", C.c_int32), ("min_step", C.c_double),
                ("lm_lambda", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        _lib().flame_stereo_default_align_params(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("unknown align parameter %r" % k)
            setattr(self, k, v)


class _AlignSystem(C.Structure):
    _fields_ = [("H", C.c_double * 21), ("b", C.c_double * 6), ("cost", C.c_double)] + \
               [(n, C.c_int32) for n in ALIGN_COUNTS] + [("reserved_", C.c_int32)]


class _AlignTrace(C.Structure):
    _fields_ = [("level", C.c_int32), ("accepted", C.c_int32), ("q", C.c_double * 4), ("t", C.c_double * 3),
                ("delta", C.c_double * 6), ("sys", _AlignSystem)]


class _AlignResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("flags", C.c_int32), ("q", C.c_double * 4), ("t", C.c_double * 3),
                ("q_f32", C.c_float * 4), ("t_f32", C.c_float * 3), ("R_f32", C.c_float * 9),
                ("first_mean_cost", C.c_double), ("last_mean_cost", C.c_double), ("iters", C.c_int32 * 5),
                ("n_evals", C.c_int32)]


assert C.sizeof(AlignParams) == 40 and C.sizeof(_AlignSystem) == 248 and C.sizeof(_AlignTrace) == 360
assert C.sizeof(_AlignResult) == 168


def _system_dict(s):
    """An _AlignSystem as numpy copies: sums [28] float64 (H's upper triangle row-major, b, cost) and the five counts."""
    d = {"sums": np.array(list(s.H) + list(s.b) + [s.cost], np.float64)}
    d.update({n: int(getattr(s, n)) for n in ALIGN_COUNTS})
    return d


STEREO_ABI_SYMBOLS = (
    "flame_stereo_default_params", "flame_stereo_create", "flame_stereo_destroy", "flame_stereo_set_stream",
    "flame_stereo_set_camera", "flame_stereo_add_frame", "flame_stereo_drop_frame", "flame_stereo_frame_count",
    "flame_stereo_download_frame", "flame_stereo_update_feature_idepths", "flame_stereo_update_feature_idepths_device",
    "flame_stereo_last_kernel_ms", "flame_stereo_last_hip_error", "flame_stereo_set_features",
    "flame_stereo_update_resident", "flame_stereo_get_features", "flame_stereo_features_device", "flame_stereo_set_option",
    "flame_stereo_default_detect_params", "flame_stereo_project_features", "flame_stereo_get_projected",
    "flame_stereo_projected_device", "flame_stereo_detect_features", "flame_stereo_prune_pose_frames",
    "flame_stereo_prune_features", "flame_stereo_clear_features", "flame_stereo_default_graph_params",
    "flame_stereo_select_graph_features", "flame_stereo_select_graph_features_arrays",
    "flame_stereo_draw_features", "flame_stereo_frame_image_device", "flame_stereo_draw_matches",
    "flame_stereo_draw_detections", "flame_stereo_default_input_params", "flame_stereo_set_input",
    "flame_stereo_add_raw_frame", "flame_stereo_default_align_params", "flame_stereo_build_pyramid",
    "flame_stereo_download_pyramid_level", "flame_stereo_align_linearize", "flame_stereo_align_frame",
)
OPT_LANES_PER_FEATURE = 1
OPT_GRAPH_COPY = 2
OPT_RECORD_MATCHES = 3

_READY = False
_FP = C.POINTER(C.c_float)
_DP = C.POINTER(C.c_double)


def _lib():
    global _READY
    L = load_library()
    if not _READY:
        ctx = C.c_void_p
        PP = C.POINTER(StereoParams)
        sig = {
            "flame_stereo_default_params": (None, [PP]),
            "flame_stereo_create": (C.c_int, [C.POINTER(ctx), C.c_int]),
            "flame_stereo_destroy": (None, [ctx]),
            "flame_stereo_set_stream": (C.c_int, [ctx, C.c_void_p]),
            "flame_stereo_set_camera": (C.c_int, [ctx, _FP, _FP, C.c_int, C.c_int, C.c_int]),
            "flame_stereo_add_frame": (C.c_int, [ctx, C.c_uint32, C.c_void_p, C.c_int]),
            "flame_stereo_drop_frame": (C.c_int, [ctx, C.c_uint32]),
            "flame_stereo_frame_count": (C.c_int, [ctx]),
            "flame_stereo_download_frame": (C.c_int, [ctx, C.c_uint32, C.c_void_p, _FP, _FP]),
            "flame_stereo_update_feature_idepths": (C.c_int, [ctx, PP, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_Pose),
                                                              C.c_int, C.c_void_p, C.POINTER(_Stats)]),
            "flame_stereo_update_feature_idepths_device": (C.c_int, [ctx, PP, C.c_uint32, C.c_uint32, C.c_int,
                                                                     C.POINTER(_Pose), C.c_int, C.c_void_p,
                                                                     C.POINTER(_Stats)]),
            "flame_stereo_set_features": (C.c_int, [ctx, C.c_int, C.c_void_p]),
            "flame_stereo_update_resident": (C.c_int, [ctx, PP, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_Pose),
                                                       C.POINTER(_Stats)]),
            "flame_stereo_get_features": (C.c_int, [ctx, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
            "flame_stereo_features_device": (C.c_int, [ctx, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
            "flame_stereo_set_option": (C.c_int, [ctx, C.c_int, C.c_int]),
            "flame_stereo_last_kernel_ms": (C.c_float, [ctx]),
            "flame_stereo_last_hip_error": (C.c_int, [ctx]),
            "flame_stereo_default_detect_params": (None, [C.POINTER(DetectParams)]),
            "flame_stereo_project_features": (C.c_int, [ctx, PP, C.c_uint32, C.c_int, C.POINTER(_Pose),
                                                        C.POINTER(_FeatureStats)]),
            "flame_stereo_get_projected": (C.c_int, [ctx, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
            "flame_stereo_projected_device": (C.c_int, [ctx, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
            "flame_stereo_detect_features": (C.c_int, [ctx, PP, C.POINTER(DetectParams), C.c_uint32, _FP, _FP, _FP,
                                                       C.c_void_p, C.c_int, _FP, C.c_uint32, C.POINTER(_FeatureStats)]),
            "flame_stereo_prune_pose_frames": (C.c_int, [ctx, PP, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.c_int,
                                                         C.POINTER(_Pose), C.c_int, C.POINTER(_PruneStats)]),
            "flame_stereo_prune_features": (C.c_int, [ctx, PP, C.c_uint32, C.c_int, C.POINTER(C.c_uint32), C.c_int,
                                                      C.POINTER(_Pose), C.c_int, C.POINTER(C.c_int), C.c_void_p,
                                                      C.POINTER(_PruneStats)]),
            "flame_stereo_clear_features": (C.c_int, [ctx]),
            "flame_stereo_default_graph_params": (None, [C.POINTER(GraphParams)]),
            "flame_stereo_select_graph_features": (C.c_int, [ctx, C.POINTER(GraphParams), C.c_float, C.c_int,
                                                             C.POINTER(_WorldPose), C.POINTER(_GraphInputs)]),
            "flame_stereo_select_graph_features_arrays": (C.c_int, [ctx, C.POINTER(GraphParams), C.c_float, C.c_int,
                                                                    C.POINTER(_WorldPose), C.c_int, C.c_void_p, C.c_void_p,
                                                                    C.POINTER(_GraphInputs)]),
            "flame_stereo_draw_features": (C.c_int, [ctx, C.c_uint32, C.c_float, C.c_float, C.c_int, C.c_void_p,
                                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
            "flame_stereo_frame_image_device": (C.c_int, [ctx, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
            "flame_stereo_draw_matches": (C.c_int, [ctx, C.c_int, C.c_void_p, C.POINTER(_MatchesStats)]),
            "flame_stereo_draw_detections": (C.c_int, [ctx, PP, C.POINTER(DetectParams), C.c_uint32, _FP, _FP, C.c_float,
                                                       C.c_int, C.c_void_p, C.POINTER(_DetectionsStats)]),
            "flame_stereo_default_input_params": (None, [C.POINTER(InputParams)]),
            "flame_stereo_set_input": (C.c_int, [ctx, C.POINTER(InputParams)]),
            "flame_stereo_add_raw_frame": (C.c_int, [ctx, C.c_uint32, C.c_void_p, C.c_int, C.c_int,
                                                     C.POINTER(_InputStats)]),
            "flame_stereo_default_align_params": (None, [C.POINTER(AlignParams)]),
            "flame_stereo_build_pyramid": (C.c_int, [ctx, C.c_uint32, C.c_int]),
            "flame_stereo_download_pyramid_level": (C.c_int, [ctx, C.c_uint32, C.c_int, C.c_void_p, _FP, _FP]),
            "flame_stereo_align_linearize": (C.c_int, [ctx, C.POINTER(AlignParams), C.c_uint32, C.c_uint32, C.c_int, _FP,
                                                       C.c_void_p, _DP, _DP, C.POINTER(_AlignSystem)]),
            "flame_stereo_align_frame": (C.c_int, [ctx, C.POINTER(AlignParams), C.c_uint32, C.c_uint32, _FP, C.c_void_p, _DP,
                                                   _DP, C.POINTER(_AlignResult), C.POINTER(_AlignTrace), C.c_int,
                                                   C.POINTER(C.c_int)]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _READY = True
    return L


def _f32(a, n):
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    if a.size != n:
        raise ValueError("expected %d floats" % n)
    return a


class FeatureTracker:
    """Device-side counterpart of the state Flame::updateFeatureIDepths reads: the camera, the resident pose-frames
    (`pfs_`, flame.h:526) and the new frame."""

    def __init__(self, K, Kinv, width: int, height: int, border: int = 5, device: int = 0):
        self._L = _lib()
        self._ctx = C.c_void_p()
        self._chk(self._L.flame_stereo_create(C.byref(self._ctx), device), "create")
        self.width, self.height, self.border = width, height, border
        self._input = None  # (format, raw_width, raw_height) of the last set_input
        K, Kinv = _f32(K, 9), _f32(Kinv, 9)
        self._chk(self._L.flame_stereo_set_camera(self._ctx, K.ctypes.data_as(_FP), Kinv.ctypes.data_as(_FP), width, height,
                                                  border), "set_camera")

    def close(self):
        if self._ctx:
            self._L.flame_stereo_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc, what):
        if rc != 0:
            raise NLTGV2Error(rc, "%s: %s" % (what, status_string(rc)))

    def add_frame(self, frame_id: int, img: np.ndarray):
        """utils::Frame::create level 0 on the device (frame.cc:33-71)."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        if img.shape != (self.height, self.width):
            raise ValueError("image must be %dx%d" % (self.height, self.width))
        self._chk(self._L.flame_stereo_add_frame(self._ctx, frame_id, img.ctypes.data, img.strides[0]), "add_frame")

    def set_camera(self, K, Kinv, width: int, height: int, border: int = 5):
        """flame_stereo_set_camera: another working camera.  Drops all frames and forgets set_input."""
        K, Kinv = _f32(K, 9), _f32(Kinv, 9)
        self._chk(self._L.flame_stereo_set_camera(self._ctx, K.ctypes.data_as(_FP), Kinv.ctypes.data_as(_FP), width, height,
                                                  border), "set_camera")
        self.width, self.height, self.border = width, height, border
        self._input = None

    def set_input(self, params: InputParams = None, **kw):
        """flame_stereo_set_input: what the raw frames of add_raw_frame look like -- an InputParams, or its fields as
        keywords (format, remap, raw_width, raw_height, K_raw, dist)."""
        if params is None:
            params = InputParams(**kw)
        elif kw:
            raise TypeError("an InputParams or keywords, not both")
        self._chk(self._L.flame_stereo_set_input(self._ctx, C.byref(params)), "set_input")
        self._input = (int(params.format), int(params.raw_width), int(params.raw_height))

    def add_raw_frame(self, frame_id: int, raw, *, device_ptr=None, stride=None, want_stats=True):
        """flame_stereo_add_raw_frame: colour to grey, undistort / resize and Frame::create level 0 on the device, from a
        raw camera frame as set_input describes it.  `raw`: a uint8 numpy array of raw_height rows ((rows, cols) for GREY8,
        (rows, cols, channels) or (rows, bytes) otherwise; its row stride is taken from the array unless `stride` is
        given, its rows must be contiguous), or None together with `device_ptr`, the device address of such a frame with
        `stride` bytes per row (default: tight).  A device source with want_stats=False is enqueued only: the caller keeps
        the buffer alive and unchanged until the tracker's stream has passed it.  Returns the stats dict (n_outside), or
        None when want_stats is False."""
        if (raw is None) == (device_ptr is None):
            raise ValueError("raw or device_ptr, one of the two")
        if raw is not None:
            if raw.dtype != np.uint8 or raw.ndim not in (2, 3):
                raise ValueError("raw must be a uint8 array of 2 or 3 dimensions")
            if raw.strides[-1] != 1 or (raw.ndim == 3 and raw.strides[1] != raw.shape[2]):
                raw = np.ascontiguousarray(raw)
            row_bytes = raw.shape[1] * (raw.shape[2] if raw.ndim == 3 else 1)
            if stride is None:
                stride = raw.strides[0]
            inp = self._input
            if inp is not None:  # (without set_input the library answers; this keeps its reads inside the array)
                if raw.shape[0] != inp[2] or row_bytes < inp[1] * FORMAT_BYTES[inp[0]] or stride > raw.strides[0]:
                    raise ValueError("raw does not hold %d rows of %d pixels" % (inp[2], inp[1]))
            ptr = raw.ctypes.data
        else:
            ptr = int(device_ptr)
            if stride is None:
                inp = self._input
                if inp is None:
                    raise ValueError("stride is needed without set_input")
                stride = inp[1] * FORMAT_BYTES[inp[0]]
        st = _InputStats()
        rc = self._L.flame_stereo_add_raw_frame(self._ctx, frame_id, C.c_void_p(ptr), int(stride), int(raw is None),
                                                C.byref(st) if want_stats else None)
        self._chk(rc, "add_raw_frame")
        return {"n_outside": int(st.n_outside)} if want_stats else None

    def drop_frame(self, frame_id: int):
        self._chk(self._L.flame_stereo_drop_frame(self._ctx, frame_id), "drop_frame")

    def frame_count(self) -> int:
        return self._L.flame_stereo_frame_count(self._ctx)

    def download_frame(self, frame_id: int):
        shape = (self.height + 2 * self.border, self.width + 2 * self.border)
        pad = np.empty(shape, np.uint8)
        gx = np.empty(shape, np.float32)
        gy = np.empty(shape, np.float32)
        self._chk(self._L.flame_stereo_download_frame(self._ctx, frame_id, pad.ctypes.data, gx.ctypes.data_as(_FP),
                                                      gy.ctypes.data_as(_FP)), "download_frame")
        return pad, gx, gy

    @staticmethod
    def _poses(poses):
        arr = (_Pose * max(len(poses), 1))()
        for i, p in enumerate(poses):
            arr[i].frame_id = int(p["id"])
            for name, src, n in (("q_ref_to_new", "q_to_new", 4), ("t_ref_to_new", "t_to_new", 3),
                                 ("q_ref_to_pf", "q_to_pf", 4), ("t_ref_to_pf", "t_to_pf", 3)):
                v = _f32(p[src], n) if src in p else np.zeros(n, np.float32)  # (project_features reads *_to_new only)
                for k in range(n):
                    getattr(arr[i], name)[k] = float(v[k])
        return arr

    def update_feature_idepths(self, params: StereoParams, new_frame_id: int, curr_pf_id: int, poses, feats: np.ndarray,
                               raise_on_error: bool = True):
        """Flame::updateFeatureIDepths.  `poses`: list of dicts {id, q_to_new, t_to_new, q_to_pf, t_to_pf};
        `feats` (FEATURE_DTYPE) is updated in place.  Returns (status, stats dict)."""
        if feats.dtype != FEATURE_DTYPE or not feats.flags.c_contiguous:
            raise ValueError("feats must be a contiguous FEATURE_DTYPE array")
        st = _Stats()
        rc = self._L.flame_stereo_update_feature_idepths(self._ctx, C.byref(params), new_frame_id, curr_pf_id, len(poses),
                                                         self._poses(poses), feats.shape[0], feats.ctypes.data, C.byref(st))
        stats = {n: int(getattr(st, n)) for n, _ in _Stats._fields_}
        if rc != 0 and raise_on_error:
            raise NLTGV2Error(rc, "update_feature_idepths: %s (feature %d)" % (status_string(rc), stats["error_feature"]))
        return rc, stats

    def update_feature_idepths_device(self, params: StereoParams, new_frame_id: int, curr_pf_id: int, poses, n_feats: int,
                                      feats_device_ptr: int, wait: bool = True):
        st = _Stats()
        rc = self._L.flame_stereo_update_feature_idepths_device(self._ctx, C.byref(params), new_frame_id, curr_pf_id,
                                                                len(poses), self._poses(poses), n_feats,
                                                                C.c_void_p(feats_device_ptr), C.byref(st) if wait else None)
        self._chk(rc, "update_feature_idepths_device")
        return {n: int(getattr(st, n)) for n, _ in _Stats._fields_} if wait else None

    # ---- the resident feature set (the default way to run the path: features stay on the device between frames) ----
    def set_features(self, feats: np.ndarray):
        if feats.dtype != FEATURE_DTYPE or not feats.flags.c_contiguous:
            raise ValueError("feats must be a contiguous FEATURE_DTYPE array")
        self._chk(self._L.flame_stereo_set_features(self._ctx, feats.shape[0], feats.ctypes.data), "set_features")

    def update_resident(self, params: StereoParams, new_frame_id: int, curr_pf_id: int, poses, wait: bool = True,
                        raise_on_error: bool = True):
        """Flame::updateFeatureIDepths on the resident set, in place on the device.  Returns (status, stats dict)
        (wait=False: enqueued only, stats None)."""
        st = _Stats()
        rc = self._L.flame_stereo_update_resident(self._ctx, C.byref(params), new_frame_id, curr_pf_id, len(poses),
                                                  self._poses(poses), C.byref(st) if wait else None)
        if not wait:
            self._chk(rc, "update_resident")
            return rc, None
        stats = {n: int(getattr(st, n)) for n, _ in _Stats._fields_}
        if rc != 0 and raise_on_error:
            raise NLTGV2Error(rc, "update_resident: %s (feature %d)" % (status_string(rc), stats["error_feature"]))
        return rc, stats

    def get_features(self) -> np.ndarray:
        n = C.c_int(0)
        self._chk(self._L.flame_stereo_get_features(self._ctx, 0, None, C.byref(n)), "get_features")
        out = np.empty(n.value, FEATURE_DTYPE)
        self._chk(self._L.flame_stereo_get_features(self._ctx, n.value, out.ctypes.data, C.byref(n)), "get_features")
        return out

    def features_device(self):
        p, n = C.c_void_p(), C.c_int(0)
        self._chk(self._L.flame_stereo_features_device(self._ctx, C.byref(p), C.byref(n)), "features_device")
        return p.value or 0, n.value

    # ---- where the resident features come from and where they go ----
    def project_features(self, params: StereoParams, cur_frame_id: int, poses, raise_on_error: bool = True):
        """Flame::projectFeatures (flame.cc:1754-1860) on the resident set: drops the features that leave frame
        `cur_frame_id` and fills the projected set.  `poses`: list of dicts {id, q_to_new, t_to_new} with
        T_ref_to_cur = fcur.pose.inverse() * pf.pose (q_to_pf / t_to_pf are optional and not read).  Returns the kept
        count, or (status, stats dict) when raise_on_error is False."""
        st = _FeatureStats()
        rc = self._L.flame_stereo_project_features(self._ctx, C.byref(params), cur_frame_id, len(poses),
                                                   self._poses(poses), C.byref(st))
        stats = {n: int(getattr(st, n)) for n, _ in _FeatureStats._fields_}
        if not raise_on_error:
            return rc, stats
        if rc != 0:
            raise NLTGV2Error(rc, "project_features: %s (feature %d)" % (status_string(rc), stats["error_feature"]))
        return stats["num_features"]

    def get_projected(self) -> np.ndarray:
        """The projected set (Flame::feats_in_curr_) of the last project_features."""
        n = C.c_int(0)
        self._chk(self._L.flame_stereo_get_projected(self._ctx, 0, None, C.byref(n)), "get_projected")
        out = np.empty(n.value, FEATURE_DTYPE)
        self._chk(self._L.flame_stereo_get_projected(self._ctx, n.value, out.ctypes.data, C.byref(n)), "get_projected")
        return out

    def projected_device(self):
        p, n = C.c_void_p(), C.c_int(0)
        self._chk(self._L.flame_stereo_projected_device(self._ctx, C.byref(p), C.byref(n)), "projected_device")
        return p.value or 0, n.value

    def draw_features(self, cur_frame_id: int, idepth_var_max_graph: float, scene_color_scale: float = 1.0, flip: bool = False):
        """Flame::drawFeatures (flame.cc:2459-2510) on the projected set of the last project_features over resident frame
        `cur_frame_id`.  Returns (img (height, width, 3) u8, num_converged, num_unconverged)."""
        img = np.empty((self.height, self.width, 3), np.uint8)
        nc, nu = C.c_int32(0), C.c_int32(0)
        self._chk(self._L.flame_stereo_draw_features(self._ctx, cur_frame_id, C.c_float(idepth_var_max_graph),
                                                     C.c_float(scene_color_scale), int(bool(flip)), img.ctypes.data, C.byref(nc),
                                                     C.byref(nu)), "draw_features")
        return img, int(nc.value), int(nu.value)

    def set_record_matches(self, on):
        """FLAME_STEREO_OPT_RECORD_MATCHES: while on, every update also records what draw_matches paints (same feature
        records, statistics and return codes)."""
        self._chk(self._L.flame_stereo_set_option(self._ctx, OPT_RECORD_MATCHES, int(on)), "set_option")

    def draw_matches(self, flip: bool = False, raise_on_error: bool = True):
        """getDebugImageMatches (flame.cc:1293-1295 and the draws of updateFeatureIDepths / trackFeature) of the last update
        that ran with set_record_matches(True), over the image of the frame it named as new.  Returns a dict: img
        (height, width, 3) u8, num_features, kind_count (9 ints, MATCH_KINDS), lines_drawn, lines_skipped, rings_skipped,
        entries, refilled; (status, dict or None) when raise_on_error is False."""
        img = np.empty((self.height, self.width, 3), np.uint8)
        st = _MatchesStats()
        rc = self._L.flame_stereo_draw_matches(self._ctx, int(bool(flip)), img.ctypes.data, C.byref(st))
        res = None
        if rc == 0:
            res = {n: int(getattr(st, n)) for n in ("num_features", "lines_drawn", "lines_skipped", "rings_skipped", "entries",
                                                    "refilled")}
            res["kind_count"] = [int(v) for v in st.kind_count]
            res["img"] = img
        if not raise_on_error:
            return rc, res
        self._chk(rc, "draw_matches")
        return res

    def draw_detections(self, params: StereoParams, dparams: DetectParams, ref_frame_id: int, q_ref_to_prev, t_ref_to_prev,
                        max_score: float = 0.005, flip: bool = False, raise_on_error: bool = True):
        """getDebugImageDetections (flame.cc:1212-1251, 1272-1275, drawDetections :2363-2412): the epipolar-gradient score of
        the detect_features call with the same arguments, coloured with jet(score, 0, max_score) and blended over the image of
        resident frame `ref_frame_id` (0.005 is the reference's literal max_score).  Changes nothing but scratch.  Returns
        (img (height, width, 3) u8, stats dict: num_scored, num_examined, error_pixel), or (status, img, stats dict) when
        raise_on_error is False (img is unspecified unless status is 0)."""
        q, t = _f32(q_ref_to_prev, 4), _f32(t_ref_to_prev, 3)
        img = np.empty((self.height, self.width, 3), np.uint8)
        st = _DetectionsStats()
        rc = self._L.flame_stereo_draw_detections(self._ctx, C.byref(params), C.byref(dparams), ref_frame_id,
                                                  q.ctypes.data_as(_FP), t.ctypes.data_as(_FP), C.c_float(max_score),
                                                  int(bool(flip)), img.ctypes.data, C.byref(st))
        stats = {n: int(getattr(st, n)) for n, _ in _DetectionsStats._fields_}
        if not raise_on_error:
            return rc, img, stats
        if rc != 0:
            raise NLTGV2Error(rc, "draw_detections: %s (pixel %d)" % (status_string(rc), stats["error_pixel"]))
        return img, stats

    def frame_image_device(self, frame_id: int):
        """(device address, step_bytes) of the unpadded image of a resident frame: Regularizer.debug_images(None, ...,
        img_device=, step_bytes=).  Valid until the frame is dropped or replaced."""
        p, step = C.c_void_p(), C.c_int(0)
        self._chk(self._L.flame_stereo_frame_image_device(self._ctx, frame_id, C.byref(p), C.byref(step)), "frame_image_device")
        return p.value or 0, int(step.value)

    def detect_features(self, params: StereoParams, dparams: DetectParams, ref_frame_id: int, q_ref_to_prev,
                        t_ref_to_prev, idepthmap=None, mask_xy=None, first_id: int = 0, raise_on_error: bool = True):
        """Flame::detectFeatures + the detection loop's initialisation on resident frame `ref_frame_id`; the new
        features are appended to the resident set.  idepthmap: None (all NaN), a (height, width) float32 host array,
        or an int device address of such a map.  mask_xy: None, an (n, 2) host array of (x, y), or "projected" (the
        projected set of the last project_features).  Returns the number of new features, or (status, stats dict)
        when raise_on_error is False."""
        q, t = _f32(q_ref_to_prev, 4), _f32(t_ref_to_prev, 3)
        host_map, dev_map = None, None
        if isinstance(idepthmap, (int, np.integer)) and not isinstance(idepthmap, bool):
            dev_map = C.c_void_p(int(idepthmap))
        elif idepthmap is not None:
            host_map = np.ascontiguousarray(idepthmap, dtype=np.float32)
            if host_map.shape != (self.height, self.width):
                raise ValueError("idepthmap must be %dx%d" % (self.height, self.width))
        if isinstance(mask_xy, str):
            if mask_xy != "projected":
                raise ValueError("mask_xy must be None, an (n, 2) array or 'projected'")
            n_mask, mask = -1, None
        elif mask_xy is None:
            n_mask, mask = 0, None
        else:
            mask = np.ascontiguousarray(mask_xy, dtype=np.float32).reshape(-1, 2)
            n_mask = mask.shape[0]
        st = _FeatureStats()
        rc = self._L.flame_stereo_detect_features(
            self._ctx, C.byref(params), C.byref(dparams), ref_frame_id, q.ctypes.data_as(_FP), t.ctypes.data_as(_FP),
            host_map.ctypes.data_as(_FP) if host_map is not None else None, dev_map,
            n_mask, mask.ctypes.data_as(_FP) if mask is not None and n_mask > 0 else None, first_id, C.byref(st))
        stats = {n: int(getattr(st, n)) for n, _ in _FeatureStats._fields_}
        if not raise_on_error:
            return rc, stats
        if rc != 0:
            raise NLTGV2Error(rc, "detect_features: %s (pixel %d)" % (status_string(rc), stats["error_feature"]))
        return stats["num_features"]

    # ---- refining a frame's pose against a pose-frame's map ----
    def level_size(self, level: int):
        """(w_l, h_l) of pyramid level `level`: ((w + 1) // 2, (h + 1) // 2) per level."""
        w, h = self.width, self.height
        for _ in range(level):
            w, h = (w + 1) // 2, (h + 1) // 2
        return w, h

    def build_pyramid(self, frame_id: int, n_levels: int, raise_on_error: bool = True):
        """flame_stereo_build_pyramid: levels 1 .. n_levels - 1 of a resident frame (pyrDown in integers + central
        gradients), enqueue-only.  Returns the status."""
        rc = self._L.flame_stereo_build_pyramid(self._ctx, frame_id, int(n_levels))
        if raise_on_error:
            self._chk(rc, "build_pyramid")
        return rc

    def download_pyramid_level(self, frame_id: int, level: int, raise_on_error: bool = True):
        """(img u8, gradx f32, grady f32) of one level, each (h_l, w_l), unpadded; (status, None) on an error when
        raise_on_error is False."""
        w, h = self.level_size(level) if 0 <= level < 16 else (1, 1)
        img, gx, gy = np.empty((h, w), np.uint8), np.empty((h, w), np.float32), np.empty((h, w), np.float32)
        rc = self._L.flame_stereo_download_pyramid_level(self._ctx, frame_id, int(level), img.ctypes.data,
                                                         gx.ctypes.data_as(_FP), gy.ctypes.data_as(_FP))
        if not raise_on_error:
            return rc, ((img, gx, gy) if rc == 0 else None)
        self._chk(rc, "download_pyramid_level")
        return img, gx, gy

    def _map_args(self, idepthmap):
        """(keep-alive, host pointer, device pointer) of an inverse-depth map: a (height, width) float32 host array or an
        int device address."""
        if isinstance(idepthmap, (int, np.integer)) and not isinstance(idepthmap, bool):
            return None, None, C.c_void_p(int(idepthmap))
        if idepthmap is None:
            return None, None, None
        m = np.ascontiguousarray(idepthmap, dtype=np.float32)
        if m.shape != (self.height, self.width):
            raise ValueError("idepthmap must be %dx%d" % (self.height, self.width))
        return m, m.ctypes.data_as(_FP), None

    def align_linearize(self, params: AlignParams, ref_frame_id: int, new_frame_id: int, level: int, idepthmap, q, t,
                        raise_on_error: bool = True):
        """flame_stereo_align_linearize: the Gauss-Newton system of the direct alignment of `new_frame_id` against
        `ref_frame_id` and its map at the pose (q (w x y z), t) = T_ref_to_new, float64.  Returns a dict: sums [28] float64
        (H's upper triangle row-major, b, cost) and the counts ALIGN_COUNTS; (status, dict) when raise_on_error is False."""
        q = np.ascontiguousarray(q, np.float64).reshape(4)
        t = np.ascontiguousarray(t, np.float64).reshape(3)
        keep, hp, dp = self._map_args(idepthmap)
        out = _AlignSystem()
        rc = self._L.flame_stereo_align_linearize(self._ctx, C.byref(params), ref_frame_id, new_frame_id, int(level), hp, dp,
                                                  q.ctypes.data_as(_DP), t.ctypes.data_as(_DP), C.byref(out))
        del keep
        if not raise_on_error:
            return rc, _system_dict(out)
        self._chk(rc, "align_linearize")
        return _system_dict(out)

    def align_frame(self, params: AlignParams, ref_frame_id: int, new_frame_id: int, idepthmap, q_init, t_init,
                    max_trace: int = 256, raise_on_error: bool = True):
        """flame_stereo_align_frame: Gauss-Newton over the levels coarsest_level .. finest_level.  Returns a dict: status,
        flags, q [4] / t [3] float64, q_f32, t_f32, R_f32 [3, 3], first_mean_cost, last_mean_cost, iters [5], n_evals and
        trace: a list of dicts (level, accepted, q, t, delta, sums, counts), one per evaluation; (status code, dict) when
        raise_on_error is False."""
        q = np.ascontiguousarray(q_init, np.float64).reshape(4)
        t = np.ascontiguousarray(t_init, np.float64).reshape(3)
        keep, hp, dp = self._map_args(idepthmap)
        out = _AlignResult()
        trace = (_AlignTrace * max(max_trace, 1))()
        n = C.c_int(0)
        rc = self._L.flame_stereo_align_frame(self._ctx, C.byref(params), ref_frame_id, new_frame_id, hp, dp,
                                              q.ctypes.data_as(_DP), t.ctypes.data_as(_DP), C.byref(out), trace, int(max_trace),
                                              C.byref(n))
        del keep
        res = {"status": int(out.status), "flags": int(out.flags), "q": np.array(list(out.q), np.float64),
               "t": np.array(list(out.t), np.float64), "q_f32": np.array(list(out.q_f32), np.float32),
               "t_f32": np.array(list(out.t_f32), np.float32), "R_f32": np.array(list(out.R_f32), np.float32).reshape(3, 3),
               "first_mean_cost": float(out.first_mean_cost), "last_mean_cost": float(out.last_mean_cost),
               "iters": [int(v) for v in out.iters], "n_evals": int(out.n_evals), "trace": []}
        for k in range(min(int(n.value), max_trace)):
            e = trace[k]
            d = _system_dict(e.sys)
            d.update(level=int(e.level), accepted=int(e.accepted), q=np.array(list(e.q), np.float64),
                     t=np.array(list(e.t), np.float64), delta=np.array(list(e.delta), np.float64))
            res["trace"].append(d)
        if not raise_on_error:
            return rc, res
        self._chk(rc, "align_frame")
        return res

    # ---- letting a pose-frame go ----
    @staticmethod
    def _keep_ids(keep_ids):
        ids = [int(k) for k in keep_ids]
        return (C.c_uint32 * max(len(ids), 1))(*ids), len(ids)

    def prune_pose_frames(self, params: StereoParams, target_frame_id: int, keep_ids, dropped, first_new: int = None,
                          raise_on_error: bool = True):
        """Flame::prunePoseFrames (flame.cc:554-706) on the resident set: the features of the pose-frames in `dropped`
        are re-anchored in `target_frame_id` (the kept pose-frame with the largest id), then those frames are released.
        `keep_ids`: the ids that stay; `dropped`: list of dicts {id, q_to_new, t_to_new} with
        T = target.pose.inverse() * pf.pose.  Records [first_new, n) are new_feats_ (removed when the move fails, where
        older records are marked invalid); None = all are feats_.  Returns the stats dict, or (status, stats dict) when
        raise_on_error is False."""
        ids, n_keep = self._keep_ids(keep_ids)
        if first_new is None:
            first_new = self.features_device()[1]
        st = _PruneStats()
        rc = self._L.flame_stereo_prune_pose_frames(self._ctx, C.byref(params), target_frame_id, n_keep, ids, len(dropped),
                                                    self._poses(dropped), int(first_new), C.byref(st))
        stats = {n: int(getattr(st, n)) for n, _ in _PruneStats._fields_}
        if not raise_on_error:
            return rc, stats
        if rc != 0:
            raise NLTGV2Error(rc, "prune_pose_frames: %s (feature %d)" % (status_string(rc), stats["error_feature"]))
        return stats

    def prune_features(self, params: StereoParams, target_frame_id: int, keep_ids, dropped, feats: np.ndarray,
                       first_new: int = None, raise_on_error: bool = True):
        """The same on a host array: returns (the pruned array -- a view of `feats`, which is updated in place --,
        stats dict), or (status, array or None, stats dict) when raise_on_error is False."""
        if feats.dtype != FEATURE_DTYPE or not feats.flags.c_contiguous:
            raise ValueError("feats must be a contiguous FEATURE_DTYPE array")
        ids, n_keep = self._keep_ids(keep_ids)
        n = C.c_int(feats.shape[0])
        if first_new is None:
            first_new = feats.shape[0]
        st = _PruneStats()
        rc = self._L.flame_stereo_prune_features(self._ctx, C.byref(params), target_frame_id, n_keep, ids, len(dropped),
                                                 self._poses(dropped), int(first_new), C.byref(n), feats.ctypes.data,
                                                 C.byref(st))
        stats = {k: int(getattr(st, k)) for k, _ in _PruneStats._fields_}
        if not raise_on_error:
            return rc, (feats[:n.value] if rc == 0 else None), stats
        if rc != 0:
            raise NLTGV2Error(rc, "prune_features: %s (feature %d)" % (status_string(rc), stats["error_feature"]))
        return feats[:n.value], stats

    def clear_features(self):
        """The feature half of Flame::clear(): no resident features, no projected set; frames stay."""
        self._chk(self._L.flame_stereo_clear_features(self._ctx), "clear_features")

    # ---- which features become vertices of the graph ----
    @staticmethod
    def _world_poses(world_poses):
        arr = (_WorldPose * max(len(world_poses), 1))()
        for i, p in enumerate(world_poses):
            arr[i].frame_id = int(p["id"])
            q, t = _f32(p["q"], 4), _f32(p["t"], 3)
            for k in range(4):
                arr[i].q[k] = float(q[k])
            for k in range(3):
                arr[i].t[k] = float(t[k])
        return arr

    def select_graph_features(self, gparams: GraphParams, graph_scale: float, world_poses, feats: np.ndarray = None,
                              feats_in_curr: np.ndarray = None, raise_on_error: bool = True):
        """The preprocessing of Flame::syncGraph (flame.cc:1954-1980): which features become vertices of the graph and
        with which data term.  `world_poses`: list of dicts {id, q, t} with pf.pose (camera -> world) of every
        pose-frame.  Without the two arrays it runs on the resident and the projected set (index-aligned, i.e. right after
        project_features); with them (FEATURE_DTYPE, the same length) on those, touching neither resident set.  Returns a
        dict of numpy copies feat_id [V], pos [V, 2], data_term [V], data_weight [V], feat_index [V] -- what
        flame_nltgv2_sync_input takes -- plus V and the counters; (status, dict) when raise_on_error is False."""
        out = _GraphInputs()
        wp = self._world_poses(world_poses)
        if (feats is None) != (feats_in_curr is None):
            raise ValueError("feats and feats_in_curr go together")
        if feats is None:
            rc = self._L.flame_stereo_select_graph_features(self._ctx, C.byref(gparams), graph_scale, len(world_poses), wp,
                                                            C.byref(out))
        else:
            for a in (feats, feats_in_curr):
                if a.dtype != FEATURE_DTYPE or not a.flags.c_contiguous:
                    raise ValueError("feats must be a contiguous FEATURE_DTYPE array")
            if feats.shape != feats_in_curr.shape:
                raise ValueError("feats and feats_in_curr must be index-aligned")
            rc = self._L.flame_stereo_select_graph_features_arrays(self._ctx, C.byref(gparams), graph_scale, len(world_poses),
                                                                   wp, feats.shape[0], feats.ctypes.data,
                                                                   feats_in_curr.ctypes.data, C.byref(out))
        V = int(out.V)
        res = {n: int(getattr(out, n)) for n in GRAPH_COUNTERS}
        res["V"] = V

        def take(ptr, count, dtype):
            if count == 0 or not ptr:
                return np.zeros(count, dtype)
            return np.ctypeslib.as_array(ptr, shape=(count,)).astype(dtype, copy=True)

        res["feat_id"] = take(out.feat_id, V, np.int32)
        res["pos"] = take(out.pos, 2 * V, np.float32).reshape(V, 2)
        res["data_term"] = take(out.data_term, V, np.float32)
        res["data_weight"] = take(out.data_weight, V, np.float32)
        res["feat_index"] = take(out.feat_index, V, np.int32)
        if not raise_on_error:
            return rc, res
        if rc != 0:
            raise NLTGV2Error(rc, "select_graph_features: %s (feature %d)" % (status_string(rc), res["error_feature"]))
        return res

    def get_raw_idepths(self):
        """Flame::getRawIDepths (flame.h:255-273): (xy [n, 2], idepth_mu [n], idepth_var [n]) of the valid records of
        the projected set.  Host code over get_projected."""
        p = self.get_projected()
        p = p[p["valid"] != 0]
        return np.stack([p["x"], p["y"]], axis=1), p["idepth_mu"].copy(), p["idepth_var"].copy()

    def set_graph_copy(self, mode: int):
        """How select_graph_features copies its arrays down: 0 one block, 1 the counters first (same results)."""
        self._chk(self._L.flame_stereo_set_option(self._ctx, OPT_GRAPH_COPY, int(mode)), "set_option")

    def set_lanes_per_feature(self, lanes: int):
        self._chk(self._L.flame_stereo_set_option(self._ctx, OPT_LANES_PER_FEATURE, int(lanes)), "set_option")

    def set_stream(self, hip_stream_ptr):
        self._chk(self._L.flame_stereo_set_stream(self._ctx, C.c_void_p(hip_stream_ptr or 0)), "set_stream")

    def last_kernel_ms(self) -> float:
        return float(self._L.flame_stereo_last_kernel_ms(self._ctx))
