"""ctypes mirror of flame::optimizers::nltgv2_l1_graph_regularizer over the C-ABI
(include/flame_nltgv2.h -> libflame_nltgv2_hip.so).

Reference surface (/root/reference/src/flame/optimizers/nltgv2_l1_graph_regularizer.h):
  struct Params h:121-129            -> Params
  step(params, graph) h:134          -> Regularizer.step / .run(n)
  smoothnessCost / dataCost / cost   -> Regularizer.smoothness_cost / data_cost / cost  (h:139-151)
  internal::dualStep / primalStep / extraGradientStep h:158-168
                                     -> Regularizer.dual_step / primal_step / extragradient_step
Graph (h:107-112) is represented by a dict of flat numpy arrays (see flame_amd.synth.assemble_graph):
the order of `src/dst` is boost::edges() order and (src,dst) = (boost::source, boost::target).

This module never computes on the CPU: if the HIP library is missing or no GPU is present the calls
raise NLTGV2Error.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

_FP = C.POINTER(C.c_float)
_IP = C.POINTER(C.c_int32)

# stable options (include/flame_nltgv2.h) ...
OPT_SOLVER, OPT_USE_HIPGRAPH, OPT_PERSISTENT, OPT_PROBE, OPT_VERIFY_RECORDS, OPT_PLACEMENT, OPT_SYNC_PATH, OPT_COST_SUM, OPT_MESH_STATE = 1, 2, 5, 12, 14, 16, 17, 18, 19
# ... and the experimental range (tuning knobs / test hooks of the current kernels; tools/ and the tests use them)
OPT_BLOCK_WAVES, OPT_UNROLL, OPT_DUAL_PUBLISH, OPT_PRESLEEP, OPT_XCDS, OPT_FAULT_INJECT, OPT_POLL_GAP, OPT_PV_LEAN = 103, 104, 106, 108, 109, 110, 113, 114
RUN_PATHS = {0: "none", 1: "persistent (the lane-per-half-edge form, retired in round 3)", 2: "per-step hipGraph", 3: "per-step eager", 4: "canonical 4-sweep",
             5: "persistent-tv", 6: "persistent-pv", 7: "persistent-pv2"}
ERR_NAN = -5

VERTEX_STATE = ("x", "w1", "w2", "x_bar", "w1_bar", "w2_bar", "x_prev", "w1_prev", "w2_prev")
EDGE_STATE = ("q1", "q2", "q3")


def _rows_contiguous_u8(a) -> bool:
    """A 2-D u8 array whose rows are contiguous and lie at least a row's width apart, in order."""
    return a.dtype == np.uint8 and a.ndim == 2 and a.strides[1] == 1 and a.strides[0] >= max(a.shape[1], 1)


class NLTGV2Error(RuntimeError):
    def __init__(self, status: int, what: str):
        super().__init__(f"{what}: status {status} ({status_string(status)})")
        self.status = status


class Params(C.Structure):
    """== struct Params, nltgv2_l1_graph_regularizer.h:121-129 (same defaults)."""

    _fields_ = [(n, C.c_float) for n in ("data_factor", "step_x", "step_q", "theta", "x_min", "x_max")]

    def __init__(self, data_factor=0.1, step_x=0.001, step_q=125.0, theta=0.25, x_min=0.0, x_max=10.0):
        super().__init__(data_factor, step_x, step_q, theta, x_min, x_max)


class MeshFilterParams(C.Structure):
    """== the mesh filter fields of struct Params, params.h:69-85 (same defaults); flame_nltgv2_mesh_filter_params."""

    _fields_ = [("do_oblique_triangle_filter", C.c_int32), ("oblique_normal_thresh", C.c_float),
                ("oblique_idepth_diff_factor", C.c_float), ("oblique_idepth_diff_abs", C.c_float),
                ("do_edge_length_filter", C.c_int32), ("edge_length_thresh", C.c_float),
                ("do_idepth_triangle_filter", C.c_int32), ("min_triangle_idepth", C.c_float)]

    def __init__(self, do_oblique_triangle_filter=True, oblique_normal_thresh=1.39626, oblique_idepth_diff_factor=0.35,
                 oblique_idepth_diff_abs=0.1, do_edge_length_filter=True, edge_length_thresh=0.333,
                 do_idepth_triangle_filter=True, min_triangle_idepth=0.01):
        super().__init__(int(bool(do_oblique_triangle_filter)), oblique_normal_thresh, oblique_idepth_diff_factor,
                         oblique_idepth_diff_abs, int(bool(do_edge_length_filter)), edge_length_thresh,
                         int(bool(do_idepth_triangle_filter)), min_triangle_idepth)


class _MeshOutputsView(C.Structure):
    _fields_ = [("V", C.c_int32), ("T", C.c_int32), ("tri_valid", C.POINTER(C.c_uint8)), ("normals", _FP), ("vtx_idepth", _FP),
                ("n_valid", C.c_int32), ("rows", C.c_int32), ("cols", C.c_int32), ("filtered_map", _FP),
                ("filtered_coverage", C.c_int32), ("device_ms", C.c_float)]


class MetricParams(C.Structure):
    """== flame_nltgv2_metric_params (same defaults): the depth window (exclusive, metres), which map (the resident unfiltered one, the
    filtered one of mesh_outputs_begin(want_filtered_map=True), or map_device = the address of a caller's (rows, cols) f32 device
    map: its size is taken on trust, its writer must have completed before begin, and it must stay until _end), which outputs, and
    whether they travel to the host."""

    _fields_ = [("min_depth", C.c_float), ("max_depth", C.c_float), ("use_filtered_map", C.c_int32), ("want_depth", C.c_int32),
                ("want_depth_mm", C.c_int32), ("want_organized", C.c_int32), ("want_cloud", C.c_int32), ("want_mesh", C.c_int32),
                ("copy_out", C.c_int32), ("reserved", C.c_int32), ("map_device", C.c_void_p)]

    def __init__(self, min_depth=0.0, max_depth=float("inf"), use_filtered_map=False, want_depth=True, want_depth_mm=True,
                 want_organized=True, want_cloud=True, want_mesh=False, copy_out=True, map_device=None):
        super().__init__(min_depth, max_depth, int(bool(use_filtered_map)), int(bool(want_depth)), int(bool(want_depth_mm)),
                         int(bool(want_organized)), int(bool(want_cloud)), int(bool(want_mesh)), int(bool(copy_out)), 0,
                         int(map_device) if map_device else None)


_METRIC_ARRAYS = (("depth", _FP), ("depth_mm", C.POINTER(C.c_uint16)), ("organized", _FP), ("cloud", _FP),
                  ("cloud_pixel", C.POINTER(C.c_uint32)), ("mesh_vertices", _FP), ("mesh_normals", _FP), ("mesh_triangles", _IP))


class _MetricOutputsView(C.Structure):
    _fields_ = ([("rows", C.c_int32), ("cols", C.c_int32), ("V", C.c_int32), ("T", C.c_int32), ("n_points", C.c_int32), ("n_valid", C.c_int32)]
                + [f for name, typ in _METRIC_ARRAYS for f in ((name, typ), (name + "_device", C.c_void_p))]
                + [("device_ms", C.c_float)])


MAP_ERROR_PHOTO, MAP_ERROR_TRUTH = 0, 1


class MapErrorParams(C.Structure):
    """== flame_nltgv2_map_error_params (same defaults).  source: MAP_ERROR_PHOTO (KRKinv, Kt, border; the images of photo_set_images or
    ref_device / cmp_device with image_step_bytes) or MAP_ERROR_TRUTH (a true inverse-depth map: truth = a (rows, cols) f32 array,
    or truth_device = an address; relative).  win_size 0: the reference's choice; hist_scale 0: the source's default.  The arrays
    given here are kept alive by the object."""

    _fields_ = [("map_device", C.c_void_p), ("ref_device", C.c_void_p), ("cmp_device", C.c_void_p), ("truth_host", _FP),
                ("truth_device", C.c_void_p), ("gray_host", C.c_void_p), ("gray_device", C.c_void_p), ("KRKinv", C.c_float * 9),
                ("Kt", C.c_float * 3), ("source", C.c_int32), ("use_filtered_map", C.c_int32), ("image_step_bytes", C.c_int32),
                ("border", C.c_int32), ("relative", C.c_int32), ("win_size", C.c_int32), ("hist_scale", C.c_float),
                ("ptile_num", C.c_int32), ("ptile_den", C.c_int32), ("gray_step_bytes", C.c_int32), ("max_error", C.c_float),
                ("flip", C.c_int32), ("want_stats", C.c_int32), ("want_error_map", C.c_int32), ("want_image", C.c_int32),
                ("copy_out", C.c_int32)]

    def __init__(self, source=MAP_ERROR_PHOTO, KRKinv=None, Kt=None, border=3, ref_device=None, cmp_device=None, image_step_bytes=0,
                 truth=None, truth_device=None, relative=True, map_device=None, use_filtered_map=False, win_size=0, hist_scale=0.0,
                 ptile_num=99, ptile_den=100, gray=None, gray_device=None, gray_step_bytes=None, max_error=32.0, flip=False,
                 want_stats=True, want_error_map=True, want_image=False, copy_out=True):
        super().__init__()
        self.map_device = int(map_device) if map_device else None
        self.ref_device = int(ref_device) if ref_device else None
        self.cmp_device = int(cmp_device) if cmp_device else None
        self.image_step_bytes = int(image_step_bytes)
        self._keep = []
        if truth is not None:
            t = np.ascontiguousarray(truth, np.float32)
            self._keep.append(t)
            self.truth_host = t.ctypes.data_as(_FP)
        self.truth_device = int(truth_device) if truth_device else None
        if gray is not None:
            g = gray if isinstance(gray, np.ndarray) and _rows_contiguous_u8(gray) else np.ascontiguousarray(gray, np.uint8)
            self._keep.append(g)
            self.gray_host = g.ctypes.data
            self.gray_step_bytes = int(g.strides[0]) if gray_step_bytes is None else int(gray_step_bytes)
        else:
            self.gray_step_bytes = int(gray_step_bytes or 0)
        self.gray_device = int(gray_device) if gray_device else None
        k = np.eye(3, dtype=np.float32).reshape(9) if KRKinv is None else np.ascontiguousarray(KRKinv, np.float32).reshape(9)
        t3 = np.zeros(3, np.float32) if Kt is None else np.ascontiguousarray(Kt, np.float32).reshape(3)
        self.KRKinv = (C.c_float * 9)(*k.tolist())
        self.Kt = (C.c_float * 3)(*t3.tolist())
        self.source, self.use_filtered_map, self.border, self.relative = int(source), int(bool(use_filtered_map)), int(border), int(bool(relative))
        self.win_size, self.hist_scale, self.ptile_num, self.ptile_den = int(win_size), float(hist_scale), int(ptile_num), int(ptile_den)
        self.max_error, self.flip = float(max_error), int(bool(flip))
        self.want_stats, self.want_error_map, self.want_image, self.copy_out = (int(bool(v)) for v in (want_stats, want_error_map, want_image, copy_out))


class MapErrorStats(C.Structure):
    """== flame_nltgv2_map_error_stats."""

    _fields_ = [("hist", C.c_int32 * 256), ("n_valid", C.c_int32), ("median_bin", C.c_int32), ("ptile_bin", C.c_int32),
                ("mean", C.c_float), ("sum", C.c_double)]


class _MapErrorView(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("source", C.c_int32), ("win_size", C.c_int32), ("hist_scale", C.c_float),
                ("device_ms", C.c_float), ("stats", C.POINTER(MapErrorStats)), ("stats_device", C.c_void_p), ("error_map", _FP),
                ("error_map_device", C.c_void_p), ("image", C.POINTER(C.c_uint8)), ("image_device", C.c_void_p)]


class ViewParams(C.Structure):
    """== flame_nltgv2_view_params (same defaults): the camera the mesh is rendered into -- Kinv_src, K_dst, R (3x3 each) and t (3) with
    P_dst = R P_src + t --, near_depth, where the triangle validity comes from (0: all valid, 1: a host array, 2: what the last
    mesh_outputs_begin left on the device), which outputs, and whether they travel to the host."""

    _fields_ = [("Kinv_src", C.c_float * 9), ("K_dst", C.c_float * 9), ("R", C.c_float * 9), ("t", C.c_float * 3), ("near_depth", C.c_float),
                ("validity", C.c_int32), ("want_map", C.c_int32), ("want_tri_index", C.c_int32), ("copy_out", C.c_int32)]

    def __init__(self, Kinv_src=None, K_dst=None, R=None, t=None, near_depth=0.0, validity=0, want_map=True, want_tri_index=True, copy_out=True):
        super().__init__()
        eye = np.eye(3, dtype=np.float32)
        for name, m in (("Kinv_src", Kinv_src), ("K_dst", K_dst), ("R", R)):
            setattr(self, name, (C.c_float * 9)(*np.ascontiguousarray(eye if m is None else m, np.float32).reshape(9).tolist()))
        self.t = (C.c_float * 3)(*np.ascontiguousarray(np.zeros(3) if t is None else t, np.float32).reshape(3).tolist())
        self.near_depth, self.validity = float(near_depth), int(validity)
        self.want_map, self.want_tri_index, self.copy_out = (int(bool(v)) for v in (want_map, want_tri_index, copy_out))


class ViewCounts(C.Structure):
    """== flame_nltgv2_view_counts."""

    _fields_ = [("coverage", C.c_int32), ("tris_drawn", C.c_int32), ("tris_culled_vertex", C.c_int32), ("tris_culled_facing", C.c_int32)]


class _ViewOutputsView(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("T", C.c_int32), ("counts", ViewCounts), ("device_ms", C.c_float), ("map", _FP),
                ("map_device", C.c_void_p), ("tri_index", _IP), ("tri_index_device", C.c_void_p)]


KEPT_MESHES, FUSE_SOURCES = 16, 8


class FuseSource(C.Structure):
    """== flame_nltgv2_fuse_source (same defaults): slot = a kept slot or -1 for the live resident mesh (then validity 0 / 2 and
    graph_scale apply), its weight, and its camera into the target: Kinv_src, R (3x3) and t (3) with P_dst = R P_src + t."""

    _fields_ = [("slot", C.c_int32), ("validity", C.c_int32), ("graph_scale", C.c_float), ("weight", C.c_float), ("Kinv_src", C.c_float * 9),
                ("R", C.c_float * 9), ("t", C.c_float * 3)]

    def __init__(self, slot=-1, Kinv_src=None, R=None, t=None, weight=1.0, graph_scale=1.0, validity=0):
        super().__init__()
        eye = np.eye(3, dtype=np.float32)
        for name, m in (("Kinv_src", Kinv_src), ("R", R)):
            setattr(self, name, (C.c_float * 9)(*np.ascontiguousarray(eye if m is None else m, np.float32).reshape(9).tolist()))
        self.t = (C.c_float * 3)(*np.ascontiguousarray(np.zeros(3) if t is None else t, np.float32).reshape(3).tolist())
        self.slot, self.validity, self.graph_scale, self.weight = int(slot), int(validity), float(graph_scale), float(weight)


class FuseParams(C.Structure):
    """== flame_nltgv2_fuse_params (same defaults): up to FUSE_SOURCES sources, the target's K_dst and near_depth, the vote's rel_tol
    and min_support, which outputs, and whether they travel to the host."""

    _fields_ = [("n_sources", C.c_int32), ("sources", FuseSource * FUSE_SOURCES), ("K_dst", C.c_float * 9), ("near_depth", C.c_float),
                ("rel_tol", C.c_float), ("min_support", C.c_int32), ("want_fused", C.c_int32), ("want_masks", C.c_int32),
                ("want_spread", C.c_int32), ("want_layers", C.c_int32), ("copy_out", C.c_int32)]

    def __init__(self, sources=None, K_dst=None, near_depth=0.0, rel_tol=0.05, min_support=1, want_fused=True, want_masks=True,
                 want_spread=True, want_layers=False, copy_out=True, n_sources=None):
        super().__init__()
        sources = list(sources) if sources is not None else [FuseSource()]
        for i in range(FUSE_SOURCES):
            C.memmove(C.byref(self.sources[i]), C.byref(sources[i] if i < len(sources) else FuseSource()), C.sizeof(FuseSource))
        self.n_sources = len(sources) if n_sources is None else int(n_sources)
        self.K_dst = (C.c_float * 9)(*np.ascontiguousarray(np.eye(3) if K_dst is None else K_dst, np.float32).reshape(9).tolist())
        self.near_depth, self.rel_tol, self.min_support = float(near_depth), float(rel_tol), int(min_support)
        self.want_fused, self.want_masks, self.want_spread, self.want_layers, self.copy_out = (
            int(bool(v)) for v in (want_fused, want_masks, want_spread, want_layers, copy_out))


class FuseCounts(C.Structure):
    """== flame_nltgv2_fuse_counts: 32 words."""

    _fields_ = [("coverage", C.c_int32), ("support_hist", C.c_int32 * (FUSE_SOURCES + 1)), ("present", C.c_int32 * FUSE_SOURCES),
                ("inlier", C.c_int32 * FUSE_SOURCES), ("tris_drawn", C.c_int32), ("reserved", C.c_int32 * 5)]


_FUSE_ARRAYS = (("fused", _FP), ("present_mask", C.POINTER(C.c_uint8)), ("inlier_mask", C.POINTER(C.c_uint8)), ("spread", _FP), ("layers", _FP))


class _FuseOutputsView(C.Structure):
    _fields_ = ([("rows", C.c_int32), ("cols", C.c_int32), ("n_sources", C.c_int32), ("device_ms", C.c_float), ("counts", FuseCounts)]
                + [f for name, typ in _FUSE_ARRAYS for f in ((name, typ), (name + "_device", C.c_void_p))])


class VolumeParams(C.Structure):
    """== flame_nltgv2_volume_params (same defaults): nx, ny, nz voxels of voxel_size metres, origin = the world position of the centre
    of voxel (0, 0, 0), the truncation distance and the weight at which a voxel saturates."""

    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("voxel_size", C.c_float), ("origin", C.c_float * 3),
                ("trunc", C.c_float), ("max_weight", C.c_float)]

    def __init__(self, nx=64, ny=64, nz=64, voxel_size=0.05, origin=(0.0, 0.0, 0.0), trunc=0.15, max_weight=64.0):
        super().__init__(int(nx), int(ny), int(nz), float(voxel_size),
                         (C.c_float * 3)(*np.asarray(origin, np.float32).reshape(3).tolist()), float(trunc), float(max_weight))


class IntegrateParams(C.Structure):
    """== flame_nltgv2_integrate_params (same defaults): the call's weight, the near plane, the depth window (exclusive, metres) and
    which map, under the rules of MetricParams: the resident unfiltered one, the filtered one, or map_device."""

    _fields_ = [("weight", C.c_float), ("near_depth", C.c_float), ("min_depth", C.c_float), ("max_depth", C.c_float),
                ("use_filtered_map", C.c_int32), ("reserved", C.c_int32), ("map_device", C.c_void_p)]

    def __init__(self, weight=1.0, near_depth=0.0, min_depth=0.0, max_depth=float("inf"), use_filtered_map=False, map_device=None):
        super().__init__(weight, near_depth, min_depth, max_depth, int(bool(use_filtered_map)), 0, int(map_device) if map_device else None)


class IntegrateCounts(C.Structure):
    """== flame_nltgv2_integrate_counts: 8 words."""

    _fields_ = [("front", C.c_int32), ("in_image", C.c_int32), ("valid", C.c_int32), ("behind", C.c_int32), ("updated", C.c_int32),
                ("saturated", C.c_int32), ("reserved", C.c_int32 * 2)]


class _IntegrateView(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("device_ms", C.c_float), ("reserved", C.c_int32), ("counts", IntegrateCounts)]


class RaycastParams(C.Structure):
    """== flame_nltgv2_raycast_params (same defaults): the first sample's depth, the step, the number of steps, and whether the map
    travels to the host."""

    _fields_ = [("z_near", C.c_float), ("dz", C.c_float), ("n_steps", C.c_int32), ("copy_out", C.c_int32)]

    def __init__(self, z_near=0.1, dz=0.05, n_steps=64, copy_out=True):
        super().__init__(z_near, dz, int(n_steps), int(bool(copy_out)))


class RaycastCounts(C.Structure):
    """== flame_nltgv2_raycast_counts."""

    _fields_ = [("hits", C.c_int32), ("back", C.c_int32), ("empty", C.c_int32), ("reserved", C.c_int32)]


class _RaycastView(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("device_ms", C.c_float), ("reserved", C.c_int32), ("counts", RaycastCounts),
                ("map", _FP), ("map_device", C.c_void_p)]


class VolumeMeshParams(C.Structure):
    """== flame_nltgv2_volume_mesh_params (same defaults): the box lo <= index < hi (all-zero hi: the whole volume), the capacities, and
    whether normals are made and the arrays travel to the host."""

    _fields_ = [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3), ("max_vertices", C.c_int32), ("max_triangles", C.c_int32),
                ("want_normals", C.c_int32), ("copy_out", C.c_int32)]

    def __init__(self, lo=(0, 0, 0), hi=(0, 0, 0), max_vertices=0, max_triangles=0, want_normals=True, copy_out=True):
        super().__init__((C.c_int32 * 3)(*[int(v) for v in lo]), (C.c_int32 * 3)(*[int(v) for v in hi]), int(max_vertices), int(max_triangles),
                         int(bool(want_normals)), int(bool(copy_out)))


class VolumeMeshCounts(C.Structure):
    """== flame_nltgv2_volume_mesh_counts: 8 words."""

    _fields_ = [("n_vertices", C.c_int32), ("n_triangles", C.c_int32), ("live_cubes", C.c_int32), ("surface_cubes", C.c_int32),
                ("overflow", C.c_int32), ("reserved", C.c_int32 * 3)]


class _VolumeMeshView(C.Structure):
    _fields_ = [("counts", VolumeMeshCounts), ("device_ms", C.c_float), ("pass_ms", C.c_float * 4), ("reserved", C.c_int32 * 3),
                ("vertices", _FP), ("vertices_device", C.c_void_p), ("normals", _FP), ("normals_device", C.c_void_p),
                ("triangles", C.POINTER(C.c_int32)), ("triangles_device", C.c_void_p)]


class ShiftCounts(C.Structure):
    """== flame_nltgv2_shift_counts: 8 words."""

    _fields_ = [("kept", C.c_int32), ("kept_seen", C.c_int32), ("lost_seen", C.c_int32), ("entered", C.c_int32), ("reserved", C.c_int32 * 4)]


class _ShiftView(C.Structure):
    _fields_ = [("shift", C.c_int32 * 3), ("device_ms", C.c_float), ("base", C.c_int32 * 3), ("record_bytes", C.c_int32), ("counts", ShiftCounts)]


class FollowParams(C.Structure):
    """== flame_nltgv2_follow_params (same defaults): the point the window follows lies focus_depth along the optical axis (0: the camera
    centre); the window moves in whole steps of `step` voxels."""

    _fields_ = [("focus_depth", C.c_float), ("step", C.c_int32)]

    def __init__(self, focus_depth=0.0, step=8):
        super().__init__(focus_depth, int(step))


class FollowPlan(C.Structure):
    """== flame_nltgv2_follow_plan: 32 words; boxes as VolumeMeshParams takes them, pre-shift local indices."""

    _fields_ = [("shift", C.c_int32 * 3), ("n_leaving", C.c_int32), ("has_kept", C.c_int32), ("kept_lo", C.c_int32 * 3), ("kept_hi", C.c_int32 * 3),
                ("leaving_lo", (C.c_int32 * 3) * 3), ("leaving_hi", (C.c_int32 * 3) * 3), ("reserved", C.c_int32 * 3)]


class DebugImageParams(C.Structure):
    """== flame_nltgv2_debug_image_params (same defaults): scene_color_scale params.h:109, debug_flip_images, and which of
    drawInverseDepthMap / drawNormals are wanted."""

    _fields_ = [("scene_color_scale", C.c_float), ("flip", C.c_int32), ("want_idepthmap", C.c_int32), ("want_normals", C.c_int32)]

    def __init__(self, scene_color_scale=1.0, flip=False, want_idepthmap=True, want_normals=True):
        super().__init__(scene_color_scale, int(bool(flip)), int(bool(want_idepthmap)), int(bool(want_normals)))


class _DebugImagesView(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("idepthmap_img", C.POINTER(C.c_uint8)), ("normals_img", C.POINTER(C.c_uint8)),
                ("w1_map", _FP), ("w2_map", _FP), ("device_ms", C.c_float)]


class WireframeParams(C.Structure):
    """== flame_nltgv2_wireframe_params (same defaults): scene_color_scale params.h:109, debug_flip_images, and where the triangle
    validity comes from (0: all valid, 1: a host array, 2: what the last mesh_outputs_begin left on the device)."""

    _fields_ = [("scene_color_scale", C.c_float), ("flip", C.c_int32), ("validity", C.c_int32)]

    def __init__(self, scene_color_scale=1.0, flip=False, validity=0):
        super().__init__(scene_color_scale, int(bool(flip)), int(validity))


class _WireframeView(C.Structure):
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("wireframe_img", C.POINTER(C.c_uint8)), ("lines_drawn", C.c_int32),
                ("lines_skipped", C.c_int32), ("entries", C.c_int64), ("refilled", C.c_int32), ("device_ms", C.c_float)]


class _Graph(C.Structure):
    _fields_ = (
        [("V", C.c_int32), ("E", C.c_int32), ("pos", _FP)]
        + [(n, _FP) for n in VERTEX_STATE + ("data_term", "data_weight")]
        + [("src", _IP), ("dst", _IP)]
        + [(n, _FP) for n in ("alpha", "beta") + EDGE_STATE]
    )


class _SyncInput(C.Structure):
    _fields_ = [("V", C.c_int32), ("feat_id", _IP), ("pos", _FP), ("data_term", _FP), ("data_weight", _FP),
                ("init_x", _FP), ("E", C.c_int32), ("edges", _IP), ("check_sticky_obstacles", C.c_int32),
                ("sticky_threshold", C.c_float), ("init_graph_scale", C.c_float), ("edges_unique", C.c_int32),
                ("init_from_map", C.c_int32)]


class _Projection(C.Structure):
    _fields_ = [("K", C.c_float * 9), ("Kinv", C.c_float * 9), ("KRKinv", C.c_float * 9), ("q_ref_to_cmp", C.c_float * 4),
                ("t_ref_to_cmp", C.c_float * 3), ("region_x", C.c_float), ("region_y", C.c_float), ("region_w", C.c_float),
                ("region_h", C.c_float)]


class _Info(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("device", C.c_int32), ("V", C.c_int32), ("E", C.c_int32),
        ("n_slices", C.c_int32), ("max_degree", C.c_int32), ("padded_half_edges", C.c_int64),
        ("device_bytes", C.c_int64), ("algorithmic_bytes_per_iter", C.c_int64), ("compute_units", C.c_int32),
        ("device_name", C.c_char * 64), ("gcn_arch", C.c_char * 32), ("last_run_path", C.c_int32), ("he_waves", C.c_int32), ("tv_waves", C.c_int32),
        ("tv_wave_capacity", C.c_int32), ("last_run_groups", C.c_int32), ("timeouts_recovered", C.c_int32),
        ("patches", C.c_int32), ("torn_records_detected", C.c_int32), ("last_sync_path", C.c_int32),
        ("last_run_waves_per_cu", C.c_int32), ("reserved0", C.c_int32), ("reserved1", C.c_int32), ("replays_per_step", C.c_int32),
    ]


def library_path() -> str:
    # (FLAME_AMD_LIBRARY: another build of the same library -- same-box A/B of two builds, tools/ab.py)
    return os.environ.get("FLAME_AMD_LIBRARY") or os.path.join(_HERE, "libflame_nltgv2_hip.so")


# every symbol include/flame_nltgv2.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = (
    "flame_nltgv2_default_params", "flame_nltgv2_create", "flame_nltgv2_destroy", "flame_nltgv2_set_stream", "flame_nltgv2_stream_wait_run", "flame_nltgv2_runs_in_flight", "flame_nltgv2_run_open", "flame_nltgv2_iterations",
    "flame_nltgv2_upload_graph", "flame_nltgv2_update_data", "flame_nltgv2_upload_state", "flame_nltgv2_run",
    "flame_nltgv2_run_async", "flame_nltgv2_sync", "flame_nltgv2_run_timed", "flame_nltgv2_save_prev",
    "flame_nltgv2_dual_step", "flame_nltgv2_primal_step", "flame_nltgv2_extragradient_step", "flame_nltgv2_step",
    "flame_nltgv2_costs", "flame_nltgv2_download_state", "flame_nltgv2_export_idepth_device",
    "flame_nltgv2_export_idepth_device_async", "flame_nltgv2_set_export_target",
    "flame_nltgv2_set_option", "flame_nltgv2_get_info", "flame_nltgv2_last_error", "flame_nltgv2_last_hip_error",
    "flame_nltgv2_status_string", "flame_nltgv2_abi_version", "flame_nltgv2_pack_probe", "flame_nltgv2_read_probe", "flame_nltgv2_layout_selftest", "flame_nltgv2_placement_info",
    "flame_nltgv2_photo_set_images", "flame_nltgv2_photo_residual", "flame_nltgv2_photo_fuse",
    "flame_nltgv2_photo_residual_last", "flame_nltgv2_sync_graph", "flame_nltgv2_sync_prepare", "flame_nltgv2_sync_commit",
    "flame_nltgv2_get_topology", "flame_nltgv2_graph_size", "flame_nltgv2_set_feature_ids", "flame_nltgv2_interpolate_mesh",
    "flame_nltgv2_interpolate_mesh_begin", "flame_nltgv2_interpolate_mesh_end",
    "flame_nltgv2_interpolate_mesh_arrays", "flame_nltgv2_project_graph", "flame_nltgv2_rescale_data",
    "flame_delaunay_triangulate",
    "flame_nltgv2_default_mesh_filter_params", "flame_nltgv2_oblique_cos_bound", "flame_nltgv2_mesh_outputs_begin",
    "flame_nltgv2_mesh_outputs_end", "flame_nltgv2_mesh_outputs",
    "flame_nltgv2_default_metric_params", "flame_nltgv2_metric_outputs_begin", "flame_nltgv2_metric_outputs_end",
    "flame_nltgv2_metric_outputs",
    "flame_nltgv2_default_map_error_params", "flame_nltgv2_map_error_begin", "flame_nltgv2_map_error_end", "flame_nltgv2_map_error",
    "flame_nltgv2_default_view_params", "flame_nltgv2_render_view_begin", "flame_nltgv2_render_view_end", "flame_nltgv2_render_view",
    "flame_nltgv2_render_view_arrays",
    "flame_nltgv2_keep_mesh", "flame_nltgv2_keep_mesh_arrays", "flame_nltgv2_drop_mesh", "flame_nltgv2_kept_mesh_info", "flame_nltgv2_get_kept_mesh",
    "flame_nltgv2_default_fuse_params", "flame_nltgv2_fuse_views_begin", "flame_nltgv2_fuse_views_end", "flame_nltgv2_fuse_views",
    "flame_nltgv2_default_volume_params", "flame_nltgv2_default_integrate_params", "flame_nltgv2_default_raycast_params",
    "flame_nltgv2_volume_create", "flame_nltgv2_volume_reset", "flame_nltgv2_volume_destroy", "flame_nltgv2_volume_info",
    "flame_nltgv2_volume_download", "flame_nltgv2_volume_upload", "flame_nltgv2_volume_integrate_begin", "flame_nltgv2_volume_integrate_end",
    "flame_nltgv2_volume_integrate", "flame_nltgv2_volume_raycast_begin", "flame_nltgv2_volume_raycast_end", "flame_nltgv2_volume_raycast",
    "flame_nltgv2_default_volume_mesh_params", "flame_nltgv2_volume_mesh_begin", "flame_nltgv2_volume_mesh_end", "flame_nltgv2_volume_mesh",
    "flame_nltgv2_default_follow_params", "flame_nltgv2_volume_window", "flame_nltgv2_volume_shift_begin", "flame_nltgv2_volume_shift_end",
    "flame_nltgv2_volume_shift", "flame_nltgv2_volume_follow",
    "flame_nltgv2_default_debug_image_params", "flame_nltgv2_debug_images_begin", "flame_nltgv2_debug_images_end",
    "flame_nltgv2_debug_images",
    "flame_nltgv2_default_wireframe_params", "flame_nltgv2_debug_wireframe_begin", "flame_nltgv2_debug_wireframe_end",
    "flame_nltgv2_debug_wireframe",
)


def load_library():
    """Loads libflame_nltgv2_hip.so (built in-tree by __graft_entry__.build()).  Raises if absent:
    there is no fallback implementation."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise NLTGV2Error(-2, f"HIP library not built: {path} (run __graft_entry__.build())")
    L = C.CDLL(path)
    ctx = C.c_void_p
    PP, GP = C.POINTER(Params), C.POINTER(_Graph)
    sig = {
        "flame_nltgv2_default_params": (None, [PP]),
        "flame_nltgv2_create": (C.c_int, [C.POINTER(ctx), C.c_int]),
        "flame_nltgv2_destroy": (C.c_int, [ctx]),
        "flame_nltgv2_set_stream": (C.c_int, [ctx, C.c_void_p]),
        "flame_nltgv2_stream_wait_run": (C.c_int, [ctx, C.c_void_p]),
        "flame_nltgv2_runs_in_flight": (C.c_int, [ctx, C.POINTER(C.c_int32)]),
        "flame_nltgv2_run_open": (C.c_int, [ctx, C.POINTER(Params), C.c_int, C.POINTER(C.c_int32)]),
        "flame_nltgv2_iterations": (C.c_int, [ctx, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
        "flame_nltgv2_upload_graph": (C.c_int, [ctx, GP]),
        "flame_nltgv2_update_data": (C.c_int, [ctx, _FP, _FP]),
        "flame_nltgv2_upload_state": (C.c_int, [ctx, GP]),
        "flame_nltgv2_run": (C.c_int, [ctx, PP, C.c_int]),
        "flame_nltgv2_run_async": (C.c_int, [ctx, PP, C.c_int]),
        "flame_nltgv2_sync": (C.c_int, [ctx]),
        "flame_nltgv2_run_timed": (C.c_int, [ctx, PP, C.c_int, _FP]),
        "flame_nltgv2_save_prev": (C.c_int, [ctx]),
        "flame_nltgv2_dual_step": (C.c_int, [ctx, PP]),
        "flame_nltgv2_primal_step": (C.c_int, [ctx, PP]),
        "flame_nltgv2_extragradient_step": (C.c_int, [ctx, PP]),
        "flame_nltgv2_step": (C.c_int, [ctx, PP]),
        "flame_nltgv2_costs": (C.c_int, [ctx, PP, _FP, _FP]),
        "flame_nltgv2_download_state": (C.c_int, [ctx, GP]),
        "flame_nltgv2_export_idepth_device": (C.c_int, [ctx, C.c_void_p, C.c_float]),
        "flame_nltgv2_export_idepth_device_async": (C.c_int, [ctx, C.c_void_p, C.c_float]),
        "flame_nltgv2_set_export_target": (C.c_int, [ctx, C.c_void_p, C.c_float]),
        "flame_nltgv2_set_option": (C.c_int, [ctx, C.c_int, C.c_int]),
        "flame_nltgv2_get_info": (C.c_int, [ctx, C.POINTER(_Info)]),
        "flame_nltgv2_last_error": (C.c_int, [ctx]),
        "flame_nltgv2_last_hip_error": (C.c_int, [ctx]),
        "flame_nltgv2_status_string": (C.c_char_p, [C.c_int]),
        "flame_nltgv2_abi_version": (C.c_int, []),
        "flame_nltgv2_layout_selftest": (C.c_int, [ctx, C.POINTER(C.c_int64)]),
        "flame_nltgv2_placement_info": (C.c_int, [ctx, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_float)]),
        "flame_nltgv2_pack_probe": (C.c_int, [GP, _IP, _IP, _IP, _IP, C.c_int64, C.POINTER(C.c_int64)]),
        "flame_nltgv2_read_probe": (C.c_int, [ctx, C.POINTER(C.c_uint32), C.c_int64, C.POINTER(C.c_int64)]),
        "flame_nltgv2_photo_set_images": (C.c_int, [ctx, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int]),
        "flame_nltgv2_photo_residual": (C.c_int, [ctx, _FP, _FP, C.c_float, C.c_int, _FP]),
        "flame_nltgv2_photo_fuse": (C.c_int, [ctx, _FP, _FP, C.c_float, C.c_int, C.c_int]),
        "flame_nltgv2_photo_residual_last": (C.c_int, [ctx, _FP]),
        "flame_nltgv2_sync_graph": (C.c_int, [ctx, C.POINTER(_SyncInput)]),
        "flame_nltgv2_sync_prepare": (C.c_int, [ctx, C.POINTER(_SyncInput)]),
        "flame_nltgv2_sync_commit": (C.c_int, [ctx]),
        "flame_nltgv2_get_topology": (C.c_int, [ctx, _IP, _IP, _IP]),
        "flame_nltgv2_graph_size": (C.c_int, [ctx, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "flame_nltgv2_set_feature_ids": (C.c_int, [ctx, _IP]),
        "flame_delaunay_triangulate": (C.c_int, [_FP, C.c_int32, _IP, C.c_int32, _IP, _IP, C.c_int32, _IP]),
        "flame_nltgv2_project_graph": (C.c_int, [ctx, C.POINTER(_Projection), C.c_float, C.POINTER(C.c_uint8), _FP]),
        "flame_nltgv2_rescale_data": (C.c_int, [ctx, C.c_float, _FP, PP]),
        "flame_nltgv2_interpolate_mesh": (C.c_int, [ctx, _IP, C.c_int32, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_float,
                                                    _FP, _IP]),
        "flame_nltgv2_interpolate_mesh_begin": (C.c_int, [ctx, _IP, C.c_int32, C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_float]),
        "flame_nltgv2_interpolate_mesh_end": (C.c_int, [ctx, C.POINTER(_FP), _IP]),
        "flame_nltgv2_interpolate_mesh_arrays": (C.c_int, [ctx, _IP, C.c_int32, _FP, _FP, C.c_int32, C.POINTER(C.c_uint8),
                                                           C.POINTER(C.c_uint8), C.c_int, C.c_int, _FP, _IP]),
        "flame_nltgv2_default_mesh_filter_params": (None, [C.POINTER(MeshFilterParams)]),
        "flame_nltgv2_oblique_cos_bound": (C.c_float, [C.c_float]),
        "flame_nltgv2_mesh_outputs_begin": (C.c_int, [ctx, _IP, C.c_int32, _FP, C.POINTER(MeshFilterParams), C.c_int, C.c_int,
                                                      C.c_float, C.c_int]),
        "flame_nltgv2_mesh_outputs_end": (C.c_int, [ctx, C.POINTER(_MeshOutputsView)]),
        "flame_nltgv2_mesh_outputs": (C.c_int, [ctx, _IP, C.c_int32, _FP, C.POINTER(MeshFilterParams), C.c_int, C.c_int, C.c_float,
                                                C.POINTER(C.c_uint8), _FP, _FP, _IP, _FP, _IP]),
        "flame_nltgv2_default_metric_params": (None, [C.POINTER(MetricParams)]),
        "flame_nltgv2_metric_outputs_begin": (C.c_int, [ctx, _FP, _FP, C.POINTER(MetricParams), C.c_int, C.c_int]),
        "flame_nltgv2_metric_outputs_end": (C.c_int, [ctx, C.POINTER(_MetricOutputsView)]),
        "flame_nltgv2_metric_outputs": (C.c_int, [ctx, _FP, _FP, C.POINTER(MetricParams), C.c_int, C.c_int, _FP, C.POINTER(C.c_uint16), _FP,
                                                  _FP, C.POINTER(C.c_uint32), _IP, _FP, _FP, _IP, _IP]),
        "flame_nltgv2_default_map_error_params": (None, [C.POINTER(MapErrorParams)]),
        "flame_nltgv2_map_error_begin": (C.c_int, [ctx, C.POINTER(MapErrorParams), C.c_int, C.c_int]),
        "flame_nltgv2_map_error_end": (C.c_int, [ctx, C.POINTER(_MapErrorView)]),
        "flame_nltgv2_map_error": (C.c_int, [ctx, C.POINTER(MapErrorParams), C.c_int, C.c_int, _FP, C.POINTER(C.c_uint8),
                                             C.POINTER(MapErrorStats)]),
        "flame_nltgv2_default_view_params": (None, [C.POINTER(ViewParams)]),
        "flame_nltgv2_render_view_begin": (C.c_int, [ctx, C.POINTER(ViewParams), C.c_void_p, C.c_int, C.c_int, C.c_float]),
        "flame_nltgv2_render_view_end": (C.c_int, [ctx, C.POINTER(_ViewOutputsView)]),
        "flame_nltgv2_render_view": (C.c_int, [ctx, C.POINTER(ViewParams), C.c_void_p, C.c_int, C.c_int, C.c_float, _FP, _IP,
                                               C.POINTER(ViewCounts)]),
        "flame_nltgv2_render_view_arrays": (C.c_int, [ctx, C.POINTER(ViewParams), _IP, C.c_int32, _FP, _FP, C.c_int32, C.c_void_p, C.c_int,
                                                      C.c_int, _FP, _IP, C.POINTER(ViewCounts)]),
        "flame_nltgv2_keep_mesh": (C.c_int, [ctx, C.c_int32, C.c_float, C.c_int32]),
        "flame_nltgv2_keep_mesh_arrays": (C.c_int, [ctx, C.c_int32, _IP, C.c_int32, _FP, _FP, C.c_int32, C.c_void_p]),
        "flame_nltgv2_drop_mesh": (C.c_int, [ctx, C.c_int32]),
        "flame_nltgv2_kept_mesh_info": (C.c_int, [ctx, C.c_int32, _IP, _IP, _IP]),
        "flame_nltgv2_get_kept_mesh": (C.c_int, [ctx, C.c_int32, _FP, _FP, _IP, C.c_void_p]),
        "flame_nltgv2_default_fuse_params": (None, [C.POINTER(FuseParams)]),
        "flame_nltgv2_fuse_views_begin": (C.c_int, [ctx, C.POINTER(FuseParams), C.c_int, C.c_int]),
        "flame_nltgv2_fuse_views_end": (C.c_int, [ctx, C.POINTER(_FuseOutputsView)]),
        "flame_nltgv2_fuse_views": (C.c_int, [ctx, C.POINTER(FuseParams), C.c_int, C.c_int, _FP, C.c_void_p, C.c_void_p, _FP, _FP,
                                              C.POINTER(FuseCounts)]),
        "flame_nltgv2_default_volume_params": (None, [C.POINTER(VolumeParams)]),
        "flame_nltgv2_default_integrate_params": (None, [C.POINTER(IntegrateParams)]),
        "flame_nltgv2_default_raycast_params": (None, [C.POINTER(RaycastParams)]),
        "flame_nltgv2_volume_create": (C.c_int, [ctx, C.POINTER(VolumeParams)]),
        "flame_nltgv2_volume_reset": (C.c_int, [ctx]),
        "flame_nltgv2_volume_destroy": (C.c_int, [ctx]),
        "flame_nltgv2_volume_info": (C.c_int, [ctx, C.POINTER(VolumeParams), C.POINTER(C.c_int64)]),
        "flame_nltgv2_volume_download": (C.c_int, [ctx, _FP, _FP]),
        "flame_nltgv2_volume_upload": (C.c_int, [ctx, _FP, _FP]),
        "flame_nltgv2_volume_integrate_begin": (C.c_int, [ctx, _FP, _FP, C.POINTER(IntegrateParams), C.c_int, C.c_int]),
        "flame_nltgv2_volume_integrate_end": (C.c_int, [ctx, C.POINTER(_IntegrateView)]),
        "flame_nltgv2_volume_integrate": (C.c_int, [ctx, _FP, _FP, C.POINTER(IntegrateParams), C.c_int, C.c_int, C.POINTER(IntegrateCounts)]),
        "flame_nltgv2_volume_raycast_begin": (C.c_int, [ctx, _FP, _FP, C.POINTER(RaycastParams), C.c_int, C.c_int]),
        "flame_nltgv2_volume_raycast_end": (C.c_int, [ctx, C.POINTER(_RaycastView)]),
        "flame_nltgv2_volume_raycast": (C.c_int, [ctx, _FP, _FP, C.POINTER(RaycastParams), C.c_int, C.c_int, _FP, C.POINTER(RaycastCounts)]),
        "flame_nltgv2_default_follow_params": (None, [C.POINTER(FollowParams)]),
        "flame_nltgv2_volume_window": (C.c_int, [ctx, C.POINTER(C.c_int32)]),
        "flame_nltgv2_volume_shift_begin": (C.c_int, [ctx, C.POINTER(C.c_int32)]),
        "flame_nltgv2_volume_shift_end": (C.c_int, [ctx, C.POINTER(_ShiftView)]),
        "flame_nltgv2_volume_shift": (C.c_int, [ctx, C.POINTER(C.c_int32), C.POINTER(ShiftCounts)]),
        "flame_nltgv2_volume_follow": (C.c_int, [ctx, _FP, C.POINTER(FollowParams), C.POINTER(FollowPlan)]),
        "flame_nltgv2_default_volume_mesh_params": (None, [C.POINTER(VolumeMeshParams)]),
        "flame_nltgv2_volume_mesh_begin": (C.c_int, [ctx, C.POINTER(VolumeMeshParams)]),
        "flame_nltgv2_volume_mesh_end": (C.c_int, [ctx, C.POINTER(_VolumeMeshView)]),
        "flame_nltgv2_volume_mesh": (C.c_int, [ctx, C.POINTER(VolumeMeshParams), _FP, _FP, C.POINTER(C.c_int32), C.POINTER(VolumeMeshCounts)]),
        "flame_nltgv2_default_debug_image_params": (None, [C.POINTER(DebugImageParams)]),
        "flame_nltgv2_debug_images_begin": (C.c_int, [ctx, C.c_void_p, C.c_void_p, C.c_int, _FP, C.POINTER(DebugImageParams), C.c_int,
                                                      C.c_int]),
        "flame_nltgv2_debug_images_end": (C.c_int, [ctx, C.POINTER(_DebugImagesView)]),
        "flame_nltgv2_debug_images": (C.c_int, [ctx, C.c_void_p, C.c_void_p, C.c_int, _FP, C.POINTER(DebugImageParams), C.c_int, C.c_int,
                                                C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), _FP, _FP]),
        "flame_nltgv2_default_wireframe_params": (None, [C.POINTER(WireframeParams)]),
        "flame_nltgv2_debug_wireframe_begin": (C.c_int, [ctx, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(WireframeParams),
                                                         C.c_int, C.c_int, C.c_float]),
        "flame_nltgv2_debug_wireframe_end": (C.c_int, [ctx, C.POINTER(_WireframeView)]),
        "flame_nltgv2_debug_wireframe": (C.c_int, [ctx, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(WireframeParams), C.c_int,
                                                   C.c_int, C.c_float, C.POINTER(C.c_uint8), _IP, _IP]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _LIB = L
    return L


def status_string(status: int) -> str:
    try:
        return load_library().flame_nltgv2_status_string(int(status)).decode()
    except Exception:  # library missing
        return "?"


def _as(arr, dtype, n, name):
    a = np.ascontiguousarray(arr, dtype=dtype)
    if a.size != n:
        raise ValueError(f"{name}: expected {n} elements, got {a.size}")
    return a


def _graph_view(g: dict, keep: list, need_all=True) -> _Graph:
    V, E = int(g["V"]), int(g["E"])
    cg = _Graph()
    cg.V, cg.E = V, E
    sizes = {"pos": 2 * V, "data_term": V, "data_weight": V, "src": E, "dst": E, "alpha": E, "beta": E}
    sizes.update({k: V for k in VERTEX_STATE})
    sizes.update({k: E for k in EDGE_STATE})
    for name, ctype in _Graph._fields_[2:]:
        if name not in g or g[name] is None:
            if need_all and not name.endswith("_prev"):
                raise KeyError(name)
            continue
        dt = np.int32 if ctype is _IP else np.float32
        a = _as(g[name], dt, sizes[name], name)
        keep.append(a)
        setattr(cg, name, a.ctypes.data_as(ctype))
    return cg


def delaunay(pos, out=None):
    """Delaunay triangulation of float32 points with the library's own triangulator (host code, exact
    predicates).  Returns (triangles (T,3) int32 counter-clockwise, edges (E,2) int32).  `out` = (triangles, edges) arrays of at least
    (2 n, 3) and (3 n, 2) int32 to write into -- what a frame loop keeps between frames, as the C++ facade's vectors do (fresh arrays
    of this size are fresh pages: the library's writers fault them in)."""
    L = load_library()
    p = np.ascontiguousarray(pos, np.float32).reshape(-1, 2)
    n = p.shape[0]
    nt, ne = C.c_int32(0), C.c_int32(0)
    if out is not None and out[0].shape[0] >= 2 * n and out[1].shape[0] >= 3 * n and out[0].dtype == np.int32 and out[1].dtype == np.int32:
        tri, edg = out
    else:
        tri = np.empty((max(2 * n, 1), 3), np.int32)
        edg = np.empty((max(3 * n, 1), 2), np.int32)
    rc = L.flame_delaunay_triangulate(p.ctypes.data_as(_FP), n, tri.ctypes.data_as(_IP), tri.shape[0], C.byref(nt),
                                      edg.ctypes.data_as(_IP), edg.shape[0], C.byref(ne))
    if rc != 0:
        raise NLTGV2Error(rc, "flame_delaunay_triangulate")
    return tri[: nt.value], edg[: ne.value]  # (views of the over-allocated arrays: no second copy)


def pack_probe(g: dict):
    """Host-only view of the SELL-64 layout the fused sweep uses (no GPU needed)."""
    L = load_library()
    keep = []
    cg = _graph_view(g, keep, need_all=False)
    rows = C.c_int64(0)
    n_slices = L.flame_nltgv2_pack_probe(C.byref(cg), None, None, None, None, 0, C.byref(rows))
    if n_slices < 0:
        raise NLTGV2Error(n_slices, "pack_probe")
    perm = np.empty(n_slices * 64, np.int32)
    slice_row = np.empty(n_slices + 1, np.int32)
    rec_nbr = np.empty(rows.value * 64, np.int32)
    rec_edge = np.empty(rows.value * 64, np.int32)
    rc = L.flame_nltgv2_pack_probe(C.byref(cg), perm.ctypes.data_as(_IP), slice_row.ctypes.data_as(_IP),
                                   rec_nbr.ctypes.data_as(_IP), rec_edge.ctypes.data_as(_IP), rows.value,
                                   C.byref(rows))
    if rc < 0:
        raise NLTGV2Error(rc, "pack_probe")
    return dict(n_slices=n_slices, rows=rows.value, perm=perm, slice_row=slice_row,
                rec_nbr=rec_nbr.view(np.uint32), rec_edge=rec_edge)


class Regularizer:
    """One solver context on one GPU; holds the device image of one Graph."""

    def __init__(self, device: int = 0):
        self._L = load_library()
        self._ctx = C.c_void_p()
        self._mesh_T = -1  # triangles the last interpolate_mesh[_begin] / mesh_outputs_begin of this object sent down
        rc = self._L.flame_nltgv2_create(C.byref(self._ctx), int(device))
        if rc != 0:
            self._ctx = None
            raise NLTGV2Error(rc, "flame_nltgv2_create")
        self.V = self.E = 0

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.flame_nltgv2_destroy(self._ctx)
            self._ctx = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc, what):
        if rc != 0:
            raise NLTGV2Error(rc, what)

    # ---- graph in / out -------------------------------------------------------------------------
    def upload_graph(self, g: dict):
        keep = []
        cg = _graph_view(g, keep)
        self._chk(self._L.flame_nltgv2_upload_graph(self._ctx, C.byref(cg)), "upload_graph")
        self.V, self.E = int(g["V"]), int(g["E"])

    def sync_prepare(self, *args, **kw):
        """First half of sync_graph (same arguments): checks, one staged copy, the new topology's construction enqueued on a side
        stream -- the solver may keep iterating (run_async) until sync_commit()."""
        self._sync(self._L.flame_nltgv2_sync_prepare, "sync_prepare", *args, **kw)

    def sync_commit(self):
        """Second half: waits for the construction, settles the runs, swaps the new topology in, moves the state."""
        self._chk(self._L.flame_nltgv2_sync_commit(self._ctx), "sync_commit")
        self._refresh_size()

    def _refresh_size(self):
        nv, ne = C.c_int32(0), C.c_int32(0)
        self._chk(self._L.flame_nltgv2_graph_size(self._ctx, C.byref(nv), C.byref(ne)), "graph_size")
        self.V, self.E = int(nv.value), int(ne.value)

    def sync_graph(self, *args, **kw):
        """Per-frame warm-start synchronisation (Flame::syncGraph's graph edits, flame.cc:1985-2121).

        init_graph_scale > 0: new vertices whose init_x is NaN start at their neighbours' mean
        (init_with_prediction's fallback, flame.cc:2133-2158)."""
        self._sync(self._L.flame_nltgv2_sync_graph, "sync_graph", *args, **kw)
        self._refresh_size()

    def _sync(self, fn, what, feat_id, pos, data_term, data_weight, edges, init_x=None, check_sticky_obstacles=False,
              sticky_threshold=0.25, init_graph_scale=0.0, edges_unique=False, init_from_map=False):
        V = int(len(feat_id))
        fid = _as(feat_id, np.int32, V, "feat_id")
        p = _as(pos, np.float32, 2 * V, "pos")
        d = _as(data_term, np.float32, V, "data_term")
        w = _as(data_weight, np.float32, V, "data_weight")
        ed = np.ascontiguousarray(edges, np.int32).reshape(-1, 2)
        si = _SyncInput()
        si.V, si.E = V, int(ed.shape[0])
        si.feat_id, si.pos = fid.ctypes.data_as(_IP), p.ctypes.data_as(_FP)
        si.data_term, si.data_weight = d.ctypes.data_as(_FP), w.ctypes.data_as(_FP)
        ix = None
        if init_x is not None:
            ix = _as(init_x, np.float32, V, "init_x")
            si.init_x = ix.ctypes.data_as(_FP)
        si.edges = ed.ctypes.data_as(_IP)
        si.check_sticky_obstacles = 1 if check_sticky_obstacles else 0
        si.sticky_threshold = sticky_threshold
        si.init_graph_scale = float(init_graph_scale)
        si.edges_unique = 1 if edges_unique else 0  # (the caller vouches: e.g. the edges of flame_amd.delaunay)
        si.init_from_map = 1 if init_from_map else 0  # new vertices start at the device-resident dense map's prediction (flame.cc:2131)
        self._chk(fn(self._ctx, C.byref(si)), what)

    def placement_info(self) -> dict:
        """Record placement of the patch-per-wave form (FLAME_NLTGV2_OPT_PLACEMENT): state (1 in use, 0 not yet, -1
        unavailable), records placed for the current topology, one-way hand-off (us) on the best / mean / worst page."""
        st, n = C.c_int32(0), C.c_int32(0)
        us = (C.c_float * 3)()
        self._chk(self._L.flame_nltgv2_placement_info(self._ctx, C.byref(st), C.byref(n), us), "placement_info")
        return {"state": int(st.value), "placed_records": int(n.value), "best_us": float(us[0]), "mean_us": float(us[1]),
                "worst_us": float(us[2])}

    def layout_selftest(self) -> int:
        """Words of the device-expanded layout arrays that differ from the host builders' (0 = identical)."""
        n = C.c_int64(-1)
        self._chk(self._L.flame_nltgv2_layout_selftest(self._ctx, C.byref(n)), "layout_selftest")
        return int(n.value)

    def set_feature_ids(self, feat_id):
        fid = _as(feat_id, np.int32, self.V, "feat_id")
        self._chk(self._L.flame_nltgv2_set_feature_ids(self._ctx, fid.ctypes.data_as(_IP)), "set_feature_ids")

    def topology(self):
        src = np.empty(self.E, np.int32)
        dst = np.empty(self.E, np.int32)
        fid = np.empty(self.V, np.int32)
        self._chk(self._L.flame_nltgv2_get_topology(self._ctx, src.ctypes.data_as(_IP), dst.ctypes.data_as(_IP),
                                                     fid.ctypes.data_as(_IP)), "get_topology")
        return src, dst, fid

    def project_graph(self, K, Kinv, KRKinv, q, t, region, graph_scale=1.0):
        """Flame::projectGraph on the device state; returns (keep mask, new positions)."""
        pr = _Projection()
        for name, a, n in (("K", K, 9), ("Kinv", Kinv, 9), ("KRKinv", KRKinv, 9), ("q_ref_to_cmp", q, 4), ("t_ref_to_cmp", t, 3)):
            arr = np.ascontiguousarray(a, np.float32).reshape(n)
            setattr(pr, name, (C.c_float * n)(*arr.tolist()))
        pr.region_x, pr.region_y, pr.region_w, pr.region_h = [float(r) for r in region]
        keep = np.zeros(self.V, np.uint8)
        pos = np.empty((self.V, 2), np.float32)
        self._chk(self._L.flame_nltgv2_project_graph(self._ctx, C.byref(pr), C.c_float(graph_scale),
                                                     keep.ctypes.data_as(C.POINTER(C.c_uint8)), pos.ctypes.data_as(_FP)),
                  "project_graph")
        return keep, pos

    def rescale_data(self, graph_scale, params: Params):
        """The rescale_data block (flame.cc:328-351); updates params.data_factor; returns the new graph scale."""
        ns = C.c_float(0)
        self._chk(self._L.flame_nltgv2_rescale_data(self._ctx, C.c_float(graph_scale), C.byref(ns), C.byref(params)),
                  "rescale_data")
        return float(ns.value)

    def update_data(self, data_term, data_weight):
        d = _as(data_term, np.float32, self.V, "data_term")
        w = _as(data_weight, np.float32, self.V, "data_weight")
        self._chk(self._L.flame_nltgv2_update_data(self._ctx, d.ctypes.data_as(_FP), w.ctypes.data_as(_FP)),
                  "update_data")

    def upload_state(self, state: dict):
        keep = []
        s = dict(state)
        s.setdefault("V", self.V)
        s.setdefault("E", self.E)
        cg = _graph_view(s, keep, need_all=False)
        self._chk(self._L.flame_nltgv2_upload_state(self._ctx, C.byref(cg)), "upload_state")

    def download_state(self, keys=VERTEX_STATE + EDGE_STATE) -> dict:
        out = {}
        cg = _Graph()
        for k in keys:
            n = self.V if k in VERTEX_STATE else self.E
            out[k] = np.empty(n, np.float32)
            setattr(cg, k, out[k].ctypes.data_as(_FP))
        self._chk(self._L.flame_nltgv2_download_state(self._ctx, C.byref(cg)), "download_state")
        return out

    # ---- the reference call surface -------------------------------------------------------------
    def run(self, params: Params, n_iters: int):
        """n_iters x step(params, graph), nltgv2...cc:33-49."""
        self._chk(self._L.flame_nltgv2_run(self._ctx, C.byref(params), int(n_iters)), "run")

    def step(self, params: Params):
        self._chk(self._L.flame_nltgv2_step(self._ctx, C.byref(params)), "step")

    def run_async(self, params: Params, n_iters: int):
        self._chk(self._L.flame_nltgv2_run_async(self._ctx, C.byref(params), int(n_iters)), "run_async")

    def sync(self):
        self._chk(self._L.flame_nltgv2_sync(self._ctx), "sync")

    def run_timed(self, params: Params, n_iters: int) -> float:
        """Returns device milliseconds (HIP events on the solver's stream)."""
        ms = C.c_float(0)
        self._chk(self._L.flame_nltgv2_run_timed(self._ctx, C.byref(params), int(n_iters), C.byref(ms)), "run_timed")
        return float(ms.value)

    def save_prev(self):
        self._chk(self._L.flame_nltgv2_save_prev(self._ctx), "save_prev")

    def dual_step(self, params: Params):
        self._chk(self._L.flame_nltgv2_dual_step(self._ctx, C.byref(params)), "dual_step")

    def primal_step(self, params: Params):
        self._chk(self._L.flame_nltgv2_primal_step(self._ctx, C.byref(params)), "primal_step")

    def extragradient_step(self, params: Params):
        self._chk(self._L.flame_nltgv2_extragradient_step(self._ctx, C.byref(params)), "extragradient_step")

    def costs(self, params: Params):
        s, d = C.c_float(0), C.c_float(0)
        self._chk(self._L.flame_nltgv2_costs(self._ctx, C.byref(params), C.byref(s), C.byref(d)), "costs")
        return float(s.value), float(d.value)

    def smoothness_cost(self, params: Params) -> float:
        return self.costs(params)[0]

    def data_cost(self, params: Params) -> float:
        return self.costs(params)[1]

    def cost(self, params: Params) -> float:
        s, d = self.costs(params)
        return float(np.float32(s) + np.float32(d))

    # ---- mesh -> dense inverse-depth map (utils::interpolateMesh) -----------------------------------
    def interpolate_mesh(self, triangles, rows, cols, graph_scale=1.0, tri_valid=None):
        """Rasterises the solver's current x*graph_scale over `triangles`; returns (idepthmap, coverage)."""
        tr = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
        img = np.empty((rows, cols), np.float32)
        cov = C.c_int32(0)
        U8 = C.POINTER(C.c_uint8)
        tv = None if tri_valid is None else np.ascontiguousarray(tri_valid, np.uint8)
        self._chk(self._L.flame_nltgv2_interpolate_mesh(self._ctx, tr.ctypes.data_as(_IP), tr.shape[0],
                                                        None if tv is None else tv.ctypes.data_as(U8), rows, cols,
                                                        C.c_float(graph_scale), img.ctypes.data_as(_FP), C.byref(cov)),
                  "interpolate_mesh")
        self._mesh_T = tr.shape[0]
        return img, int(cov.value)

    def interpolate_mesh_begin(self, triangles, rows, cols, graph_scale=1.0, tri_valid=None):
        """interpolate_mesh in two halves: settles the runs, enqueues rasteriser + copy-out on a side stream and returns; the
        solver may iterate (run_async) until interpolate_mesh_end() fetches the map."""
        tr = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
        U8 = C.POINTER(C.c_uint8)
        tv = None if tri_valid is None else np.ascontiguousarray(tri_valid, np.uint8)
        self._chk(self._L.flame_nltgv2_interpolate_mesh_begin(self._ctx, tr.ctypes.data_as(_IP), tr.shape[0],
                                                              None if tv is None else tv.ctypes.data_as(U8), rows, cols,
                                                              C.c_float(graph_scale)), "interpolate_mesh_begin")
        self._map_shape = (rows, cols)
        self._mesh_T = tr.shape[0]

    def interpolate_mesh_end(self, copy=True):
        """-> (idepthmap, coverage); copy=False: a view of the context's pinned buffer, valid until the next begin."""
        p, cov = _FP(), C.c_int32(0)
        self._chk(self._L.flame_nltgv2_interpolate_mesh_end(self._ctx, C.byref(p), C.byref(cov)), "interpolate_mesh_end")
        rows, cols = self._map_shape
        img = np.ctypeslib.as_array(p, shape=(rows, cols))
        return (img.copy() if copy else img), int(cov.value)

    # -- the mesh outputs of Flame::update(), flame.cc:372-407 (flame_nltgv2_mesh_outputs*) -------------------------------------
    def mesh_outputs_begin(self, triangles, Kinv, rows, cols, graph_scale=1.0, filter=None, want_filtered_map=False):
        """Enqueues vtx_idepths / vertex normals / triangle validity (and the filtered dense map) of the resident state on the side
        stream and returns.  triangles=None: the triangles the last interpolate_mesh[_begin] of this object left on the device (an
        int instead: that many of them -- the library refuses a count that is not the resident one)."""
        if triangles is None or isinstance(triangles, (int, np.integer)):
            T = self._mesh_T if triangles is None else int(triangles)
            tp = None
        else:
            tr = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
            T, tp = tr.shape[0], tr.ctypes.data_as(_IP)
        k = np.ascontiguousarray(Kinv, np.float32).reshape(9)
        f = filter if filter is not None else MeshFilterParams()
        self._chk(self._L.flame_nltgv2_mesh_outputs_begin(self._ctx, tp, T, k.ctypes.data_as(_FP), C.byref(f), rows, cols,
                                                          C.c_float(graph_scale), int(bool(want_filtered_map))), "mesh_outputs_begin")
        if tp is not None:
            self._mesh_T = T

    def mesh_outputs_end(self, copy=True) -> dict:
        """Waits for the side stream; dict(tri_valid (T,) u8, normals (V,3), vtx_idepth (V,), n_valid, device_ms and, if asked for,
        filtered_map (rows,cols), filtered_coverage).  copy=False: views of the context's pinned memory, valid until the next begin."""
        v = _MeshOutputsView()
        self._chk(self._L.flame_nltgv2_mesh_outputs_end(self._ctx, C.byref(v)), "mesh_outputs_end")
        take = (lambda a: a.copy()) if copy else (lambda a: a)
        out = dict(
            tri_valid=take(np.ctypeslib.as_array(v.tri_valid, shape=(v.T,))) if v.T > 0 else np.zeros(0, np.uint8),
            normals=take(np.ctypeslib.as_array(v.normals, shape=(v.V, 3))),
            vtx_idepth=take(np.ctypeslib.as_array(v.vtx_idepth, shape=(v.V,))),
            n_valid=int(v.n_valid), device_ms=float(v.device_ms))
        if v.rows > 0:
            out["filtered_map"] = take(np.ctypeslib.as_array(v.filtered_map, shape=(v.rows, v.cols)))
            out["filtered_coverage"] = int(v.filtered_coverage)
        return out

    def mesh_outputs(self, triangles, Kinv, rows, cols, graph_scale=1.0, filter=None, want_filtered_map=False) -> dict:
        """mesh_outputs_begin; mesh_outputs_end."""
        self.mesh_outputs_begin(triangles, Kinv, rows, cols, graph_scale, filter, want_filtered_map)
        return self.mesh_outputs_end()

    # -- the metric outputs: depth image, point clouds, 3-D mesh (flame_nltgv2_metric_outputs*) -----------------------------------------
    def metric_outputs_begin(self, Kinv, rows, cols, pose=None, params=None):
        """Enqueues the depth image / millimetre image / organised and dense cloud (and, params.want_mesh, the posed mesh with its
        surviving triangles) on the side stream and returns.  pose: T_world_cam as 12 floats, row-major [R | t] (a (3, 4) array or
        the top of a (4, 4) one); None: the camera frame.  The map and the mesh buffers are the ones the earlier
        interpolate_mesh[_begin] / mesh_outputs_begin left on the device (params.use_filtered_map, params.map_device)."""
        k = np.ascontiguousarray(Kinv, np.float32).reshape(9)
        p = params if params is not None else MetricParams()
        t = None if pose is None else np.ascontiguousarray(np.asarray(pose, np.float32).reshape(-1)[:12])
        if t is not None and t.size != 12:
            raise ValueError("pose: expected 12 floats, row-major [R | t]")
        self._chk(self._L.flame_nltgv2_metric_outputs_begin(self._ctx, k.ctypes.data_as(_FP), None if t is None else t.ctypes.data_as(_FP),
                                                            C.byref(p), rows, cols), "metric_outputs_begin")

    def metric_outputs_end(self, copy=True) -> dict:
        """Waits for the side stream; dict(n_points, n_valid, device_ms, device = {name: address} and, as asked for, depth (rows,cols)
        f32, depth_mm (rows,cols) u16, organized (rows,cols,3), cloud (n_points,3), cloud_pixel (n_points,) u32, mesh_vertices (V,3),
        mesh_normals (V,3), mesh_triangles (n_valid,3) i32).  copy=False: views of the context's pinned memory, valid until the
        next begin.  With MetricParams(copy_out=False) only the counters and the device addresses are there."""
        v = _MetricOutputsView()
        self._chk(self._L.flame_nltgv2_metric_outputs_end(self._ctx, C.byref(v)), "metric_outputs_end")
        take = (lambda a: a.copy()) if copy else (lambda a: a)
        shapes = dict(depth=(v.rows, v.cols), depth_mm=(v.rows, v.cols), organized=(v.rows, v.cols, 3), cloud=(v.n_points, 3),
                      cloud_pixel=(v.n_points,), mesh_vertices=(v.V, 3), mesh_normals=(v.V, 3), mesh_triangles=(v.n_valid, 3))
        out = dict(n_points=int(v.n_points), n_valid=int(v.n_valid), device_ms=float(v.device_ms), rows=int(v.rows), cols=int(v.cols),
                   V=int(v.V), T=int(v.T), device={})
        for name, typ in _METRIC_ARRAYS:
            dev = getattr(v, name + "_device")
            if dev:
                out["device"][name] = int(dev)
            ptr = getattr(v, name)
            if ptr:
                shape = shapes[name]
                out[name] = take(np.ctypeslib.as_array(ptr, shape=shape)) if shape[0] > 0 else np.zeros(shape, typ._type_)
        return out

    def metric_outputs(self, Kinv, rows, cols, pose=None, params=None) -> dict:
        """metric_outputs_begin; metric_outputs_end."""
        self.metric_outputs_begin(Kinv, rows, cols, pose, params)
        return self.metric_outputs_end()

    # -- the map error: photometric or against a true map (flame_nltgv2_map_error*; the dead block flame.cc:854-984) ------------------
    def map_error_begin(self, params: MapErrorParams, rows, cols):
        """Enqueues the error image of the chosen map (params.map_device, params.use_filtered_map, else the resident map of the last
        interpolate_mesh[_begin]), its box mean, the statistics and the picture on the side stream and returns."""
        self._chk(self._L.flame_nltgv2_map_error_begin(self._ctx, C.byref(params), rows, cols), "map_error_begin")

    def map_error_end(self, copy=True) -> dict:
        """Waits for the side stream; dict(rows, cols, source, win_size, hist_scale, device_ms, device = {name: address} and, as asked
        for, n_valid, hist (256,) i32, median_bin, ptile_bin, sum (a Python float: the double), mean (np.float32), error_map
        (rows, cols) f32 with NaN where no error is defined, image (rows, cols, 3) u8).  copy=False: views of the context's pinned
        memory, valid until the next begin.  With MapErrorParams(copy_out=False) only the statistics and the addresses are there."""
        v = _MapErrorView()
        self._chk(self._L.flame_nltgv2_map_error_end(self._ctx, C.byref(v)), "map_error_end")
        take = (lambda a: a.copy()) if copy else (lambda a: a)
        out = dict(rows=int(v.rows), cols=int(v.cols), source=int(v.source), win_size=int(v.win_size), hist_scale=float(v.hist_scale),
                   device_ms=float(v.device_ms), device={})
        for name in ("stats", "error_map", "image"):
            dev = getattr(v, name + "_device")
            if dev:
                out["device"][name] = int(dev)
        if v.stats:
            s = v.stats.contents
            out.update(hist=np.ctypeslib.as_array(s.hist).copy(), n_valid=int(s.n_valid), median_bin=int(s.median_bin),
                       ptile_bin=int(s.ptile_bin), mean=np.float32(s.mean), sum=float(s.sum))
        if v.error_map:
            out["error_map"] = take(np.ctypeslib.as_array(v.error_map, shape=(v.rows, v.cols)))
        if v.image:
            out["image"] = take(np.ctypeslib.as_array(v.image, shape=(v.rows, v.cols, 3)))
        return out

    def map_error(self, params: MapErrorParams, rows, cols) -> dict:
        """map_error_begin; map_error_end."""
        self.map_error_begin(params, rows, cols)
        return self.map_error_end()

    # -- the mesh rendered into another camera (flame_nltgv2_render_view*) --------------------------------------------------------------
    def render_view_begin(self, params: ViewParams, rows, cols, graph_scale=1.0, tri_valid=None):
        """Enqueues the resident triangles over the state's pos / x, seen from the camera of `params`, on the side stream and returns.
        rows x cols is the target's size.  tri_valid: a (T,) u8 array, for params.validity == 1."""
        tv = None if tri_valid is None else np.ascontiguousarray(tri_valid, np.uint8)
        self._chk(self._L.flame_nltgv2_render_view_begin(self._ctx, C.byref(params), None if tv is None else C.c_void_p(tv.ctypes.data), rows, cols,
                                                         C.c_float(graph_scale)), "render_view_begin")

    def render_view_end(self, copy=True) -> dict:
        """Waits for the side stream; dict(rows, cols, T, coverage, tris_drawn, tris_culled_vertex, tris_culled_facing, device_ms,
        device = {name: address} and, as asked for, map (rows, cols) f32 with NaN on holes, tri_index (rows, cols) i32 with -1 on
        holes).  copy=False: views of the context's pinned memory, valid until the next begin.  With ViewParams(copy_out=False) only
        the counters and the addresses are there."""
        v = _ViewOutputsView()
        self._chk(self._L.flame_nltgv2_render_view_end(self._ctx, C.byref(v)), "render_view_end")
        take = (lambda a: a.copy()) if copy else (lambda a: a)
        out = dict(rows=int(v.rows), cols=int(v.cols), T=int(v.T), device_ms=float(v.device_ms), device={})
        out.update({k: int(getattr(v.counts, k)) for k, _ in ViewCounts._fields_})
        for name in ("map", "tri_index"):
            dev = getattr(v, name + "_device")
            if dev:
                out["device"][name] = int(dev)
            if getattr(v, name):
                out[name] = take(np.ctypeslib.as_array(getattr(v, name), shape=(v.rows, v.cols)))
        return out

    def render_view(self, params: ViewParams, rows, cols, graph_scale=1.0, tri_valid=None) -> dict:
        """render_view_begin; render_view_end."""
        self.render_view_begin(params, rows, cols, graph_scale, tri_valid)
        return self.render_view_end()

    def render_view_arrays(self, params: ViewParams, triangles, vertices, idepths, rows, cols, tri_valid=None) -> dict:
        """The same for a mesh of the caller's (a pose-frame's stored triangles, vertices and idepths), synchronously; the resident
        triangles and maps stay as they are.  -> dict(map, tri_index, coverage, tris_drawn, tris_culled_vertex, tris_culled_facing)."""
        tr = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
        xy = np.ascontiguousarray(vertices, np.float32).reshape(-1, 2)
        val = _as(idepths, np.float32, xy.shape[0], "idepths")
        tv = None if tri_valid is None else np.ascontiguousarray(tri_valid, np.uint8)
        img, idx, cnt = np.empty((rows, cols), np.float32), np.empty((rows, cols), np.int32), ViewCounts()
        self._chk(self._L.flame_nltgv2_render_view_arrays(
            self._ctx, C.byref(params), tr.ctypes.data_as(_IP), tr.shape[0], xy.ctypes.data_as(_FP), val.ctypes.data_as(_FP), xy.shape[0],
            None if tv is None else C.c_void_p(tv.ctypes.data), rows, cols, img.ctypes.data_as(_FP), idx.ctypes.data_as(_IP), C.byref(cnt)),
            "render_view_arrays")
        out = dict(map=img, tri_index=idx)
        out.update({k: int(getattr(cnt, k)) for k, _ in ViewCounts._fields_})
        return out

    # -- the meshes pose-frames keep, and their fusion in one view (flame_nltgv2_keep_mesh*, flame_nltgv2_fuse_views*) ------------------------
    def keep_mesh(self, slot, graph_scale=1.0, validity=0):
        """Snapshots the resident mesh (triangles, pos, x * graph_scale; validity 2: with the filters' validity) into the slot, device
        to device on the side stream."""
        self._chk(self._L.flame_nltgv2_keep_mesh(self._ctx, int(slot), C.c_float(graph_scale), int(validity)), "keep_mesh")

    def keep_mesh_arrays(self, slot, triangles, vertices, idepths, tri_valid=None):
        """Uploads a mesh of the caller's into the slot (a pose-frame's stored triangles, vertices and idepths)."""
        tr = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
        xy = np.ascontiguousarray(vertices, np.float32).reshape(-1, 2)
        val = _as(idepths, np.float32, xy.shape[0], "idepths")
        tv = None if tri_valid is None else _as(tri_valid, np.uint8, tr.shape[0], "tri_valid")
        self._chk(self._L.flame_nltgv2_keep_mesh_arrays(self._ctx, int(slot), tr.ctypes.data_as(_IP), tr.shape[0], xy.ctypes.data_as(_FP),
                                                        val.ctypes.data_as(_FP), xy.shape[0], None if tv is None else C.c_void_p(tv.ctypes.data)),
                  "keep_mesh_arrays")

    def drop_mesh(self, slot):
        self._chk(self._L.flame_nltgv2_drop_mesh(self._ctx, int(slot)), "drop_mesh")

    def kept_mesh_info(self, slot):
        """-> (V, T, has_validity); (-1, -1, False) for an empty slot."""
        V, T, hv = C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self._L.flame_nltgv2_kept_mesh_info(self._ctx, int(slot), C.byref(V), C.byref(T), C.byref(hv)), "kept_mesh_info")
        return int(V.value), int(T.value), bool(hv.value)

    def get_kept_mesh(self, slot) -> dict:
        """Downloads a slot -> dict(vertices (V,2) f32, idepths (V,) f32, triangles (T,3) i32, tri_valid (T,) u8 or None)."""
        V, T, hv = self.kept_mesh_info(slot)
        if V < 0:
            raise NLTGV2Error(-1, "get_kept_mesh: the slot is empty")
        xy, val, tr = np.empty((V, 2), np.float32), np.empty(V, np.float32), np.empty((T, 3), np.int32)
        tv = np.empty(T, np.uint8) if hv else None
        self._chk(self._L.flame_nltgv2_get_kept_mesh(self._ctx, int(slot), xy.ctypes.data_as(_FP), val.ctypes.data_as(_FP), tr.ctypes.data_as(_IP),
                                                     None if tv is None else C.c_void_p(tv.ctypes.data)), "get_kept_mesh")
        return dict(vertices=xy, idepths=val, triangles=tr, tri_valid=tv)

    def fuse_views_begin(self, params: FuseParams, rows, cols):
        """Enqueues the sources of `params` (kept slots, at most one live mesh) rendered into the target camera and the vote per pixel on
        the side stream and returns.  rows x cols is the target's size."""
        self._chk(self._L.flame_nltgv2_fuse_views_begin(self._ctx, None if params is None else C.byref(params), rows, cols), "fuse_views_begin")

    def fuse_views_end(self, copy=True) -> dict:
        """Waits for the side stream; dict(rows, cols, n_sources, device_ms, counts (32 i32, as they lie on the device), coverage,
        support_hist (9), present (8), inlier (8), tris_drawn, device = {name: address} and, as asked for, fused (rows, cols) f32 with
        NaN on holes, present_mask / inlier_mask (rows, cols) u8, spread (rows, cols) f32, layers (n_sources, rows, cols) f32).
        copy=False: views of the context's pinned memory, valid until the next begin."""
        v = _FuseOutputsView()
        self._chk(self._L.flame_nltgv2_fuse_views_end(self._ctx, C.byref(v)), "fuse_views_end")
        take = (lambda a: a.copy()) if copy else (lambda a: a)
        c = v.counts
        out = dict(rows=int(v.rows), cols=int(v.cols), n_sources=int(v.n_sources), device_ms=float(v.device_ms), device={},
                   counts=np.frombuffer(bytes(c), np.int32).copy(), coverage=int(c.coverage), support_hist=list(c.support_hist),
                   present=list(c.present), inlier=list(c.inlier), tris_drawn=int(c.tris_drawn))
        for name, _ in _FUSE_ARRAYS:
            dev = getattr(v, name + "_device")
            if dev:
                out["device"][name] = int(dev)
            if getattr(v, name):
                shape = (v.n_sources, v.rows, v.cols) if name == "layers" else (v.rows, v.cols)
                out[name] = take(np.ctypeslib.as_array(getattr(v, name), shape=shape))
        return out

    def fuse_views(self, params: FuseParams, rows, cols) -> dict:
        """fuse_views_begin; fuse_views_end."""
        self.fuse_views_begin(params, rows, cols)
        return self.fuse_views_end()

    # -- the volumetric map: integrate depth maps, raycast a view (flame_nltgv2_volume_*) ---------------------------------------------------
    def volume_create(self, params: VolumeParams = None):
        """Makes the context's truncated-signed-distance volume, every voxel {tsdf 1, weight 0}; replaces an existing one."""
        p = params if params is not None else VolumeParams()
        self._chk(self._L.flame_nltgv2_volume_create(self._ctx, C.byref(p)), "volume_create")

    def volume_reset(self):
        self._chk(self._L.flame_nltgv2_volume_reset(self._ctx), "volume_reset")

    def volume_destroy(self):
        self._chk(self._L.flame_nltgv2_volume_destroy(self._ctx), "volume_destroy")

    def volume_info(self) -> dict:
        """-> dict(nx, ny, nz, voxel_size, origin (3,), trunc, max_weight, device_bytes)."""
        p, b = VolumeParams(), C.c_int64()
        self._chk(self._L.flame_nltgv2_volume_info(self._ctx, C.byref(p), C.byref(b)), "volume_info")
        return dict(nx=int(p.nx), ny=int(p.ny), nz=int(p.nz), voxel_size=float(p.voxel_size), origin=np.array(list(p.origin), np.float32),
                    trunc=float(p.trunc), max_weight=float(p.max_weight), device_bytes=int(b.value))

    def volume_download(self) -> dict:
        """-> dict(tsdf, weight), each (nz, ny, nx) f32: voxel (i, j, k) is [k, j, i]."""
        i = self.volume_info()
        shape = (i["nz"], i["ny"], i["nx"])
        tsdf, weight = np.empty(shape, np.float32), np.empty(shape, np.float32)
        self._chk(self._L.flame_nltgv2_volume_download(self._ctx, tsdf.ctypes.data_as(_FP), weight.ctypes.data_as(_FP)), "volume_download")
        return dict(tsdf=tsdf, weight=weight)

    def volume_upload(self, tsdf, weight):
        """Replaces every voxel (for tests of the raycast); both arrays hold nx * ny * nz floats, voxel (i, j, k) at [k, j, i]."""
        i = self.volume_info()
        n = i["nx"] * i["ny"] * i["nz"]
        t, w = _as(tsdf, np.float32, n, "tsdf"), _as(weight, np.float32, n, "weight")
        self._chk(self._L.flame_nltgv2_volume_upload(self._ctx, t.ctypes.data_as(_FP), w.ctypes.data_as(_FP)), "volume_upload")

    @staticmethod
    def _pose12(pose, name):
        t = np.ascontiguousarray(np.asarray(pose, np.float32).reshape(-1)[:12])
        if t.size != 12:
            raise ValueError(f"{name}: expected 12 floats, row-major [R | t]")
        return t

    def volume_integrate_begin(self, K, T_cam_world, rows, cols, params: IntegrateParams = None):
        """Enqueues the integration of one (rows, cols) inverse-depth map seen from T_cam_world (12 floats, row-major [R | t]) on the
        side stream and returns.  The map is the resident one, the filtered one or params.map_device."""
        k = np.ascontiguousarray(K, np.float32).reshape(9)
        t = self._pose12(T_cam_world, "T_cam_world")
        p = params if params is not None else IntegrateParams()
        self._chk(self._L.flame_nltgv2_volume_integrate_begin(self._ctx, k.ctypes.data_as(_FP), t.ctypes.data_as(_FP), C.byref(p), rows, cols),
                  "volume_integrate_begin")

    def volume_integrate_end(self) -> dict:
        """Waits for the side stream; dict(rows, cols, device_ms, counts (8 i32, as they lie on the device), front, in_image, valid,
        behind, updated, saturated)."""
        v = _IntegrateView()
        self._chk(self._L.flame_nltgv2_volume_integrate_end(self._ctx, C.byref(v)), "volume_integrate_end")
        out = dict(rows=int(v.rows), cols=int(v.cols), device_ms=float(v.device_ms), counts=np.frombuffer(bytes(v.counts), np.int32).copy())
        out.update({k: int(getattr(v.counts, k)) for k, _ in IntegrateCounts._fields_ if k != "reserved"})
        return out

    def volume_integrate(self, K, T_cam_world, rows, cols, params: IntegrateParams = None) -> dict:
        """volume_integrate_begin; volume_integrate_end."""
        self.volume_integrate_begin(K, T_cam_world, rows, cols, params)
        return self.volume_integrate_end()

    def volume_raycast_begin(self, Kinv, T_world_cam, rows, cols, params: RaycastParams = None):
        """Enqueues the volume seen from T_world_cam (12 floats, row-major [R | t]) through Kinv as a (rows, cols) inverse-depth map on
        the side stream and returns."""
        k = np.ascontiguousarray(Kinv, np.float32).reshape(9)
        t = self._pose12(T_world_cam, "T_world_cam")
        p = params if params is not None else RaycastParams()
        self._chk(self._L.flame_nltgv2_volume_raycast_begin(self._ctx, k.ctypes.data_as(_FP), t.ctypes.data_as(_FP), C.byref(p), rows, cols),
                  "volume_raycast_begin")

    def volume_raycast_end(self, copy=True) -> dict:
        """Waits for the side stream; dict(rows, cols, device_ms, counts (4 i32), hits, back, empty, device = {"map": address} and,
        with copy_out, map (rows, cols) f32 with NaN on holes).  copy=False: a view of the context's pinned memory, valid until the
        next begin."""
        v = _RaycastView()
        self._chk(self._L.flame_nltgv2_volume_raycast_end(self._ctx, C.byref(v)), "volume_raycast_end")
        out = dict(rows=int(v.rows), cols=int(v.cols), device_ms=float(v.device_ms), counts=np.frombuffer(bytes(v.counts), np.int32).copy(),
                   hits=int(v.counts.hits), back=int(v.counts.back), empty=int(v.counts.empty), device={})
        if v.map_device:
            out["device"]["map"] = int(v.map_device)
        if v.map:
            a = np.ctypeslib.as_array(v.map, shape=(v.rows, v.cols))
            out["map"] = a.copy() if copy else a
        return out

    def volume_raycast(self, Kinv, T_world_cam, rows, cols, params: RaycastParams = None) -> dict:
        """volume_raycast_begin; volume_raycast_end."""
        self.volume_raycast_begin(Kinv, T_world_cam, rows, cols, params)
        return self.volume_raycast_end()

    def volume_mesh_begin(self, params: VolumeMeshParams = None):
        """Enqueues the surface extraction of a box of the volume (marching tetrahedra, flame_nltgv2.h) on the side stream and returns."""
        p = params if params is not None else VolumeMeshParams()
        self._chk(self._L.flame_nltgv2_volume_mesh_begin(self._ctx, C.byref(p)), "volume_mesh_begin")

    def volume_mesh_end(self, copy=True) -> dict:
        """Waits for the side stream; dict(counts (8 i32), n_vertices, n_triangles, live_cubes, surface_cubes, overflow, device_ms,
        pass_ms (4 f32: classify, count, scan, emit), device = {"vertices", "normals", "triangles": addresses} and, with copy_out and no
        overflow, vertices (n, 3) f32, normals (n, 3) f32 (if wanted), triangles (m, 3) i32).  copy=False: views of the context's pinned
        memory, valid until the next begin."""
        v = _VolumeMeshView()
        self._chk(self._L.flame_nltgv2_volume_mesh_end(self._ctx, C.byref(v)), "volume_mesh_end")
        c = v.counts
        out = dict(counts=np.frombuffer(bytes(c), np.int32).copy(), n_vertices=int(c.n_vertices), n_triangles=int(c.n_triangles),
                   live_cubes=int(c.live_cubes), surface_cubes=int(c.surface_cubes), overflow=int(c.overflow), device_ms=float(v.device_ms),
                   pass_ms=np.array(list(v.pass_ms), np.float32), device={})
        for name, dev in (("vertices", v.vertices_device), ("normals", v.normals_device), ("triangles", v.triangles_device)):
            if dev:
                out["device"][name] = int(dev)
        for name, ptr, n, dt in (("vertices", v.vertices, c.n_vertices, np.float32), ("normals", v.normals, c.n_vertices, np.float32),
                                 ("triangles", v.triangles, c.n_triangles, np.int32)):
            if ptr:
                a = np.ctypeslib.as_array(ptr, shape=(n, 3)) if n > 0 else np.zeros((0, 3), dt)
                out[name] = a.copy() if copy else a
        return out

    def volume_mesh(self, params: VolumeMeshParams = None, lo=(0, 0, 0), hi=(0, 0, 0), want_normals=True) -> dict:
        """volume_mesh_begin; volume_mesh_end.  Without params: a count query (max_* = 0, nothing but the counters travels), then the call
        with exactly the counts it gave."""
        if params is None:
            self.volume_mesh_begin(VolumeMeshParams(lo, hi, 0, 0, False, False))
            q = self.volume_mesh_end()
            params = VolumeMeshParams(lo, hi, q["n_vertices"], q["n_triangles"], want_normals, True)
        self.volume_mesh_begin(params)
        return self.volume_mesh_end()

    # -- the window that follows the camera (flame_nltgv2_volume_shift*, flame_nltgv2_volume_window, flame_nltgv2_volume_follow) --------
    def volume_window(self) -> np.ndarray:
        """-> base (3,) i32: local voxel (i, j, k) is global voxel base + (i, j, k)."""
        b = (C.c_int32 * 3)()
        self._chk(self._L.flame_nltgv2_volume_window(self._ctx, b), "volume_window")
        return np.array(list(b), np.int32)

    def volume_shift_begin(self, shift):
        """Enqueues the move of the window by shift (3 ints, voxels) on the side stream and returns: destination voxel (i, j, k) gets the
        record of (i, j, k) + shift where that lies in the window, else a fresh one."""
        s = (C.c_int32 * 3)(*[int(v) for v in shift])
        self._chk(self._L.flame_nltgv2_volume_shift_begin(self._ctx, s), "volume_shift_begin")

    def volume_shift_end(self) -> dict:
        """Waits for the side stream; dict(shift (3,), base (3,), device_ms, record_bytes (16, 8 or 0), counts (8 i32), kept, kept_seen,
        lost_seen, entered)."""
        v = _ShiftView()
        self._chk(self._L.flame_nltgv2_volume_shift_end(self._ctx, C.byref(v)), "volume_shift_end")
        out = dict(shift=np.array(list(v.shift), np.int32), base=np.array(list(v.base), np.int32), device_ms=float(v.device_ms),
                   record_bytes=int(v.record_bytes), counts=np.frombuffer(bytes(v.counts), np.int32).copy())
        out.update({k: int(getattr(v.counts, k)) for k, _ in ShiftCounts._fields_ if k != "reserved"})
        return out

    def volume_shift(self, shift) -> dict:
        """volume_shift_begin; volume_shift_end."""
        self.volume_shift_begin(shift)
        return self.volume_shift_end()

    def volume_follow(self, T_world_cam, params: FollowParams = None) -> dict:
        """Where the window should move for a camera at T_world_cam (12 floats, row-major [R | t]); host arithmetic, nothing shifts.
        -> dict(shift (3,) i32, kept: (lo, hi) or None, leaving: [(lo, hi), ...] in pre-shift local indices, plan: the FollowPlan)."""
        t = self._pose12(T_world_cam, "T_world_cam")
        p = params if params is not None else FollowParams()
        plan = FollowPlan()
        self._chk(self._L.flame_nltgv2_volume_follow(self._ctx, t.ctypes.data_as(_FP), C.byref(p), C.byref(plan)), "volume_follow")
        kept = (list(plan.kept_lo), list(plan.kept_hi)) if plan.has_kept else None
        leaving = [(list(plan.leaving_lo[b]), list(plan.leaving_hi[b])) for b in range(plan.n_leaving)]
        return dict(shift=np.array(list(plan.shift), np.int32), kept=kept, leaving=leaving, plan=plan)

    # -- the debug images of Flame::update()'s "Draw stuff", flame.cc:490-511 (flame_nltgv2_debug_images*) ----------------------------
    def debug_images_begin(self, img, K, rows, cols, params=None, img_device=None, step_bytes=None):
        """Enqueues drawInverseDepthMap / the w1, w2 maps / drawNormals over the resident map of the last interpolate_mesh[_begin] on
        the side stream and returns.  The grey image: `img`, a (rows, cols) u8 array whose rows are contiguous (a view with a larger
        row stride is passed as it is), or img=None and img_device = a device address with step_bytes (e.g.
        FeatureTracker.frame_image_device)."""
        k = np.ascontiguousarray(K, np.float32).reshape(9)
        p = params if params is not None else DebugImageParams()
        if img is not None:
            if not (isinstance(img, np.ndarray) and _rows_contiguous_u8(img) and img.shape == (rows, cols)):
                img = np.ascontiguousarray(img, np.uint8).reshape(rows, cols)
            host, dev, step = C.c_void_p(img.ctypes.data), None, int(img.strides[0]) if step_bytes is None else int(step_bytes)
        else:
            host, dev, step = None, (C.c_void_p(int(img_device)) if img_device else None), int(step_bytes if step_bytes is not None else cols)
        self._chk(self._L.flame_nltgv2_debug_images_begin(self._ctx, host, dev, step, k.ctypes.data_as(_FP), C.byref(p), rows, cols),
                  "debug_images_begin")

    def debug_images_end(self, copy=True) -> dict:
        """Waits for the side stream; dict(device_ms and, as asked for, idepthmap_img (rows,cols,3) u8, normals_img (rows,cols,3) u8,
        w1_map, w2_map (rows,cols) f32).  copy=False: views of the context's pinned memory, valid until the next begin."""
        v = _DebugImagesView()
        self._chk(self._L.flame_nltgv2_debug_images_end(self._ctx, C.byref(v)), "debug_images_end")
        take = (lambda a: a.copy()) if copy else (lambda a: a)
        out = dict(device_ms=float(v.device_ms))
        if v.idepthmap_img:
            out["idepthmap_img"] = take(np.ctypeslib.as_array(v.idepthmap_img, shape=(v.rows, v.cols, 3)))
        if v.normals_img:
            out["normals_img"] = take(np.ctypeslib.as_array(v.normals_img, shape=(v.rows, v.cols, 3)))
            out["w1_map"] = take(np.ctypeslib.as_array(v.w1_map, shape=(v.rows, v.cols)))
            out["w2_map"] = take(np.ctypeslib.as_array(v.w2_map, shape=(v.rows, v.cols)))
        return out

    def debug_images(self, img, K, rows, cols, params=None, img_device=None, step_bytes=None) -> dict:
        """debug_images_begin; debug_images_end."""
        self.debug_images_begin(img, K, rows, cols, params, img_device, step_bytes)
        return self.debug_images_end()

    # -- getDebugImageWireframe, drawWireframe flame.cc:2414-2457 (flame_nltgv2_debug_wireframe*) -------------------------------------
    def debug_wireframe_begin(self, img, rows, cols, graph_scale=1.0, params=None, tri_valid=None, img_device=None, step_bytes=None):
        """Enqueues drawWireframe over the resident triangles and the state's pos / x on the side stream and returns.  The grey image
        as in debug_images_begin.  tri_valid: a (T,) u8 array, for params.validity == 1 (given without params, it selects that)."""
        if params is None:
            params = WireframeParams(validity=0 if tri_valid is None else 1)
        tv = None if tri_valid is None else np.ascontiguousarray(tri_valid, np.uint8)
        if img is not None:
            if not (isinstance(img, np.ndarray) and _rows_contiguous_u8(img) and img.shape == (rows, cols)):
                img = np.ascontiguousarray(img, np.uint8).reshape(rows, cols)
            host, dev, step = C.c_void_p(img.ctypes.data), None, int(img.strides[0]) if step_bytes is None else int(step_bytes)
        else:
            host, dev, step = None, (C.c_void_p(int(img_device)) if img_device else None), int(step_bytes if step_bytes is not None else cols)
        self._chk(self._L.flame_nltgv2_debug_wireframe_begin(self._ctx, host, dev, step, None if tv is None else C.c_void_p(tv.ctypes.data),
                                                             C.byref(params), rows, cols, C.c_float(graph_scale)), "debug_wireframe_begin")

    def debug_wireframe_end(self, copy=True) -> dict:
        """Waits for the side stream; dict(wireframe_img (rows,cols,3) u8, lines_drawn, lines_skipped, entries, refilled, device_ms).
        copy=False: a view of the context's pinned memory, valid until the next begin."""
        v = _WireframeView()
        self._chk(self._L.flame_nltgv2_debug_wireframe_end(self._ctx, C.byref(v)), "debug_wireframe_end")
        img = np.ctypeslib.as_array(v.wireframe_img, shape=(v.rows, v.cols, 3))
        return dict(wireframe_img=img.copy() if copy else img, lines_drawn=int(v.lines_drawn), lines_skipped=int(v.lines_skipped),
                    entries=int(v.entries), refilled=int(v.refilled), device_ms=float(v.device_ms))

    def debug_wireframe(self, img, rows, cols, graph_scale=1.0, params=None, tri_valid=None, img_device=None, step_bytes=None) -> dict:
        """debug_wireframe_begin; debug_wireframe_end."""
        self.debug_wireframe_begin(img, rows, cols, graph_scale, params, tri_valid, img_device, step_bytes)
        return self.debug_wireframe_end()

    def interpolate_mesh_arrays(self, triangles, vertices, values, rows, cols, vtx_valid=None, tri_valid=None):
        tr = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
        xy = np.ascontiguousarray(vertices, np.float32).reshape(-1, 2)
        val = _as(values, np.float32, xy.shape[0], "values")
        img = np.empty((rows, cols), np.float32)
        cov = C.c_int32(0)
        U8 = C.POINTER(C.c_uint8)
        tv = None if tri_valid is None else np.ascontiguousarray(tri_valid, np.uint8)
        vv = None if vtx_valid is None else np.ascontiguousarray(vtx_valid, np.uint8)
        self._chk(self._L.flame_nltgv2_interpolate_mesh_arrays(
            self._ctx, tr.ctypes.data_as(_IP), tr.shape[0], xy.ctypes.data_as(_FP), val.ctypes.data_as(_FP), xy.shape[0],
            None if vv is None else vv.ctypes.data_as(U8), None if tv is None else tv.ctypes.data_as(U8), rows, cols,
            img.ctypes.data_as(_FP), C.byref(cov)), "interpolate_mesh_arrays")
        return img, int(cov.value)

    # ---- config-5 epilogue ----------------------------------------------------------------------
    def photo_set_images(self, ref, cmp):
        """Row-strided u8 views with contiguous rows (e.g. img[:, :cols] of a padded buffer) go as they are, strides[0] as the
        row step; anything else is copied into contiguous rows first."""
        ref, cmp = np.asarray(ref), np.asarray(cmp)
        if ref.shape != cmp.shape or ref.ndim != 2:
            raise ValueError("two equally sized single-channel u8 images expected")
        if not (_rows_contiguous_u8(ref) and _rows_contiguous_u8(cmp) and ref.strides[0] == cmp.strides[0]):
            ref, cmp = np.ascontiguousarray(ref, np.uint8), np.ascontiguousarray(cmp, np.uint8)
        U8 = C.POINTER(C.c_uint8)
        self._chk(self._L.flame_nltgv2_photo_set_images(self._ctx, ref.ctypes.data_as(U8), cmp.ctypes.data_as(U8),
                                                         ref.shape[0], ref.shape[1], ref.strides[0]), "photo_set_images")

    def photo_residual(self, KRKinv, Kt, graph_scale=1.0, border=3):
        k = np.ascontiguousarray(KRKinv, np.float32).reshape(9)
        t = np.ascontiguousarray(Kt, np.float32).reshape(3)
        err = np.empty(self.V, np.float32)
        self._chk(self._L.flame_nltgv2_photo_residual(self._ctx, k.ctypes.data_as(_FP), t.ctypes.data_as(_FP),
                                                       C.c_float(graph_scale), int(border), err.ctypes.data_as(_FP)),
                  "photo_residual")
        return err

    # ---- plumbing -------------------------------------------------------------------------------
    def photo_fuse(self, KRKinv=None, Kt=None, graph_scale=1.0, border=3, enable=True):
        """While enabled, every run also leaves the photometric residual of its final x on the device (config 5)."""
        if not enable:
            self._chk(self._L.flame_nltgv2_photo_fuse(self._ctx, None, None, C.c_float(1.0), 3, 0), "photo_fuse")
            return
        k = np.ascontiguousarray(KRKinv, np.float32).reshape(9)
        t = np.ascontiguousarray(Kt, np.float32).reshape(3)
        self._chk(self._L.flame_nltgv2_photo_fuse(self._ctx, k.ctypes.data_as(_FP), t.ctypes.data_as(_FP),
                                                  C.c_float(graph_scale), int(border), 1), "photo_fuse")

    def photo_residual_last(self) -> np.ndarray:
        err = np.empty(self.V, np.float32)
        self._chk(self._L.flame_nltgv2_photo_residual_last(self._ctx, err.ctypes.data_as(_FP)), "photo_residual_last")
        return err

    def set_stream(self, hip_stream_ptr: int | None):
        self._chk(self._L.flame_nltgv2_set_stream(self._ctx, C.c_void_p(hip_stream_ptr or 0)), "set_stream")

    def runs_in_flight(self) -> int:
        """How many of the last two run_async() runs the device has not finished yet (non-blocking)."""
        n = C.c_int32(0)
        self._chk(self._L.flame_nltgv2_runs_in_flight(self._ctx, C.byref(n)), "runs_in_flight")
        return int(n.value)

    def run_open(self, params: Params, max_iters: int) -> bool:
        """A run that goes on (at most max_iters, even) until the next call that needs the solver settled asks it to stop.  False: not
        applicable to this graph / configuration -- nothing was enqueued, use run_async."""
        opened = C.c_int32(0)
        self._chk(self._L.flame_nltgv2_run_open(self._ctx, C.byref(params), int(max_iters), C.byref(opened)), "run_open")
        return bool(opened.value)

    def iterations(self):
        """(iterations applied by all runs so far, whether an open run is in flight and not yet counted); never waits."""
        total, open_ = C.c_int64(0), C.c_int32(0)
        self._chk(self._L.flame_nltgv2_iterations(self._ctx, C.byref(total), C.byref(open_)), "iterations")
        return int(total.value), bool(open_.value)

    def stream_wait_run(self, hip_stream_ptr: int):
        """Another stream of the caller waits for everything enqueued on the solver's stream so far (right behind run_async: at no cost to
        the solver's stream -- the launch carries the event)."""
        self._chk(self._L.flame_nltgv2_stream_wait_run(self._ctx, C.c_void_p(hip_stream_ptr)), "stream_wait_run")

    def set_option(self, option: int, value: int):
        self._chk(self._L.flame_nltgv2_set_option(self._ctx, int(option), int(value)), "set_option")

    def export_idepth_device(self, device_ptr: int, scale: float = 1.0, wait: bool = True):
        fn = self._L.flame_nltgv2_export_idepth_device if wait else self._L.flame_nltgv2_export_idepth_device_async
        self._chk(fn(self._ctx, C.c_void_p(device_ptr), C.c_float(scale)), "export_idepth_device")

    def set_export_target(self, device_ptr: int | None, scale: float = 1.0):
        """While set, every run also leaves scale * x (original vertex order) in this device buffer."""
        self._chk(self._L.flame_nltgv2_set_export_target(self._ctx, C.c_void_p(device_ptr or 0), C.c_float(scale)),
                  "set_export_target")

    def read_probe(self) -> np.ndarray:
        """Cycle probe of the last patch-per-wave run (OPT_PROBE): uint32 [patches, steps, 8] flattened."""
        n = C.c_int64(0)
        self._chk(self._L.flame_nltgv2_read_probe(self._ctx, None, 0, C.byref(n)), "read_probe")
        out = np.zeros(int(n.value), dtype=np.uint32)
        if out.size:
            self._chk(self._L.flame_nltgv2_read_probe(self._ctx, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size,
                                                      C.byref(n)), "read_probe")
        return out

    def info(self) -> dict:
        i = _Info()
        self._chk(self._L.flame_nltgv2_get_info(self._ctx, C.byref(i)), "get_info")
        d = {n: getattr(i, n) for n, _ in _Info._fields_}
        d["device_name"] = d["device_name"].decode(errors="replace")
        d["gcn_arch"] = d["gcn_arch"].decode(errors="replace")
        return d

    def last_error(self) -> int:
        return int(self._L.flame_nltgv2_last_error(self._ctx))
