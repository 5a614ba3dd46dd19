"""The wireframe image on the device, GPU part (the CPU part and the cases: tests/test_wireframe.py).  Every byte is compared with the
sequential restatement tests/wireframe_ref.py; no tolerance, no excluded pixel.  The state is set with upload_graph so that x is
chosen, not solved for."""
import ctypes as C

import numpy as np
import pytest

from flame_amd import synth
from tests import mesh_ref as mr
from tests import test_wireframe as tw
from tests import wireframe_ref as wr
from tests.test_debug_images import COLOR_SCALE, COLS, GRAPH_SCALE, ROWS, F, assert_image
from tests.test_debug_images import scene  # noqa: F401  (the module-scoped scene, as a fixture)


@pytest.fixture(scope="module")
def gpu(built):
    import torch  # noqa: F401

    import flame_amd

    return flame_amd


def check_lists(gpu, case, rows, cols, names=None):
    """Every triangle list of a case over one uploaded graph: picture and counters against the checker."""
    with gpu.Regularizer(0) as reg:
        reg.upload_graph(case["g"])
        for name, tris in case["tris"].items():
            if names is not None and name not in names:
                continue
            reg.interpolate_mesh(tris, rows, cols)
            got = reg.debug_wireframe(case["img"], rows, cols)
            ref, nd, ns = wr.draw_wireframe(case["img"], tris, case["pos"], case["x"])
            assert (got["lines_drawn"], got["lines_skipped"]) == (nd, ns), name
            assert_image(got["wireframe_img"], ref, name)


@pytest.mark.gpu
def test_gpu_single_triangles_every_kind_of_line_both_vertex_orders(gpu):
    check_lists(gpu, tw.single_case(), tw.SINGLE_ROWS, tw.SINGLE_COLS)


@pytest.mark.gpu
def test_gpu_two_triangles_in_both_list_orders(gpu):
    check_lists(gpu, tw.pair_case(), tw.SINGLE_ROWS, tw.SINGLE_COLS)


@pytest.mark.gpu
def test_gpu_fan_overflows_a_fresh_buffer_and_is_refilled_once(gpu):
    c = tw.fan_case()
    rows, cols = tw.FAN_ROWS, tw.FAN_COLS
    ref, nd, ns, counts = wr.draw_wireframe(c["img"], c["tris"], c["pos"], c["x"], want_counts=True)
    with gpu.Regularizer(0) as reg:  # a fresh context: its entry buffer holds 2 * rows * cols
        reg.upload_graph(c["g"])
        reg.interpolate_mesh(c["tris"], rows, cols)
        first = reg.debug_wireframe(c["img"], rows, cols)
        assert first["entries"] == counts.sum() > 2 * rows * cols and first["refilled"] == 1
        assert (first["lines_drawn"], first["lines_skipped"]) == (nd, ns)
        assert_image(first["wireframe_img"], ref, "fan, refilled")
        again = reg.debug_wireframe(c["img"], rows, cols)
        assert again["refilled"] == 0 and again["entries"] == first["entries"]
        assert_image(again["wireframe_img"], ref, "fan, second call")
        # the same triangles in reversed order: another picture, still the checker's
        reg.interpolate_mesh(c["tris"][::-1], rows, cols)
        rev = reg.debug_wireframe(c["img"], rows, cols)
        assert rev["refilled"] == 0
        assert_image(rev["wireframe_img"], wr.draw_wireframe(c["img"], c["tris"][::-1], c["pos"], c["x"])[0], "fan, reversed list")


@pytest.mark.gpu
def test_gpu_scene_host_and_device_image_flip_scales_and_the_c_form(gpu, scene):
    import torch

    s = scene
    dev_buf = torch.from_numpy(s["buf"]).cuda()
    with gpu.Regularizer(0) as reg:
        reg.upload_graph(s["g"])
        reg.interpolate_mesh(s["tris"], ROWS, COLS, graph_scale=GRAPH_SCALE)
        for flip in (False, True):
            for scale in (COLOR_SCALE, 0.75):
                ref, nd, ns = tw.scene_wireframe(s, scale=scale, flip=flip)
                p = gpu.WireframeParams(scene_color_scale=scale, flip=flip)
                host = reg.debug_wireframe(s["img"], ROWS, COLS, GRAPH_SCALE, p)  # a view: step_bytes 96
                assert (host["lines_drawn"], host["lines_skipped"], host["refilled"]) == (nd, ns, 0)
                assert_image(host["wireframe_img"], ref, f"host image, flip {flip}, scale {scale}")
                dev = reg.debug_wireframe(None, ROWS, COLS, GRAPH_SCALE, p, img_device=dev_buf.data_ptr() + 7, step_bytes=96)
                assert_image(dev["wireframe_img"], ref, f"device image, flip {flip}, scale {scale}")
                tight = reg.debug_wireframe(np.ascontiguousarray(s["img"]), ROWS, COLS, GRAPH_SCALE, p)  # step_bytes == cols
                assert_image(tight["wireframe_img"], ref, f"packed host image, flip {flip}, scale {scale}")
        # the synchronous C form into the caller's array; another image size than the resident map's is no error (the map is not read)
        out = np.zeros((ROWS, COLS, 3), np.uint8)
        nd_c, ns_c = C.c_int32(-1), C.c_int32(-1)
        p = gpu.WireframeParams(scene_color_scale=0.75)
        rc = gpu.load_library().flame_nltgv2_debug_wireframe(reg._ctx, s["img"].ctypes.data, None, 96, None, C.byref(p), ROWS, COLS,
                                                             C.c_float(GRAPH_SCALE), out.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                             C.byref(nd_c), C.byref(ns_c))
        assert rc == 0 and (nd_c.value, ns_c.value) == (3 * len(s["tris"]), 0)
        assert_image(out, tw.scene_wireframe(s, scale=0.75)[0], "synchronous form")
        wide = np.zeros((ROWS + 3, COLS + 5), np.uint8)
        wide[:ROWS, :COLS] = s["img"]
        got = reg.debug_wireframe(wide, ROWS + 3, COLS + 5, GRAPH_SCALE, gpu.WireframeParams(scene_color_scale=COLOR_SCALE))
        idepth = mr.vertex_idepths(s["g"]["x"], GRAPH_SCALE)
        assert_image(got["wireframe_img"], wr.draw_wireframe(wide, s["tris"], s["pos"], idepth, None, COLOR_SCALE)[0], "a larger image")
    del dev_buf


@pytest.mark.gpu
def test_gpu_validity_none_host_array_and_the_filters_on_the_device(gpu, scene):
    s = scene
    lib = gpu.load_library()
    T = len(s["tris"])
    third = np.ones(T, np.uint8)
    third[::3] = 0
    g2 = tw.filter_state(s)
    Kinv, valid = tw.scene_filter_validity(s, g2)
    img = np.ascontiguousarray(s["img"])

    def raw(reg, validity, tri_valid=None):
        p = gpu.WireframeParams(scene_color_scale=COLOR_SCALE, validity=validity)
        return lib.flame_nltgv2_debug_wireframe_begin(reg._ctx, img.ctypes.data, None, COLS, tri_valid, C.byref(p), ROWS, COLS, C.c_float(GRAPH_SCALE))

    with gpu.Regularizer(0) as reg:
        reg.upload_graph(s["g"])
        reg.interpolate_mesh(s["tris"], ROWS, COLS, graph_scale=GRAPH_SCALE)
        got = reg.debug_wireframe(img, ROWS, COLS, GRAPH_SCALE, gpu.WireframeParams(scene_color_scale=COLOR_SCALE))
        assert_image(got["wireframe_img"], tw.scene_wireframe(s)[0], "validity 0")
        got = reg.debug_wireframe(img, ROWS, COLS, GRAPH_SCALE, gpu.WireframeParams(scene_color_scale=COLOR_SCALE, validity=1), tri_valid=third)
        ref, nd, ns = tw.scene_wireframe(s, tri_valid=third)
        assert (got["lines_drawn"], got["lines_skipped"]) == (nd, ns) == (3 * int(third.sum()), 0)
        assert_image(got["wireframe_img"], ref, "validity 1, every third triangle off")
        assert raw(reg, 2) == -1  # no mesh_outputs_begin yet
        # the filters' validity, from the device
        reg.upload_graph(g2)
        reg.interpolate_mesh_begin(s["tris"], ROWS, COLS, graph_scale=GRAPH_SCALE)
        assert raw(reg, 2) == -1  # (the mesh_outputs_begin above belongs to no topology at all; still none for this one)
        reg.mesh_outputs_begin(None, Kinv, ROWS, COLS, graph_scale=GRAPH_SCALE)
        reg.debug_wireframe_begin(img, ROWS, COLS, GRAPH_SCALE, gpu.WireframeParams(scene_color_scale=COLOR_SCALE, validity=2))
        mesh = reg.mesh_outputs_end()
        got = reg.debug_wireframe_end()
        reg.interpolate_mesh_end()
        assert np.array_equal(mesh["tri_valid"], valid)
        ref, nd, ns = tw.scene_wireframe(s, tri_valid=valid, g=g2)
        assert (got["lines_drawn"], got["lines_skipped"]) == (nd, ns) == (3 * int(valid.sum()), 0)
        assert_image(got["wireframe_img"], ref, "validity 2")
        # new triangles were handed in: the validity on the device speaks of the old ones
        reg.interpolate_mesh(s["tris"][::-1], ROWS, COLS, graph_scale=GRAPH_SCALE)
        assert raw(reg, 2) == -1
        reg.mesh_outputs_begin(None, Kinv, ROWS, COLS, graph_scale=GRAPH_SCALE)
        got = reg.debug_wireframe(img, ROWS, COLS, GRAPH_SCALE, gpu.WireframeParams(scene_color_scale=COLOR_SCALE, validity=2))
        assert_image(got["wireframe_img"], tw.scene_wireframe(s, tri_valid=valid[::-1], g=g2, tris=s["tris"][::-1])[0], "validity 2, reversed list")
        # ... and a new topology
        reg.upload_graph(s["g"])
        assert raw(reg, 2) == -1 and raw(reg, 0) == -1


@pytest.mark.gpu
def test_gpu_lines_that_leave_the_image_are_skipped_and_counted(gpu):
    c = tw.outside_case()
    rows, cols = tw.SINGLE_ROWS, tw.SINGLE_COLS
    tris = c["tris"]
    valid = np.ones(len(tris), np.uint8)
    valid[2] = 0
    with gpu.Regularizer(0) as reg:
        reg.upload_graph(c["g"])
        reg.interpolate_mesh(tris, rows, cols)
        for tv in (None, valid):
            got = reg.debug_wireframe(c["img"], rows, cols, tri_valid=tv)
            ref, nd, ns = wr.draw_wireframe(c["img"], tris, c["pos"], c["x"], tv)
            assert (got["lines_drawn"], got["lines_skipped"]) == (nd, ns) and ns > 0
            assert nd + ns == 3 * (len(tris) if tv is None else int(tv.sum()))
            assert_image(got["wireframe_img"], ref, "outside")


@pytest.mark.gpu
def test_gpu_every_error_is_reported_before_anything_is_enqueued(gpu, scene):
    s = scene
    lib = gpu.load_library()
    img = np.ascontiguousarray(s["img"])
    T = len(s["tris"])
    ones = np.ones(T, np.uint8)
    K = s["K"]

    def raw(reg, host=img.ctypes.data, dev=None, step=COLS, tri_valid=None, validity=0, params=True, rows=ROWS, cols=COLS):
        p = gpu.WireframeParams(scene_color_scale=COLOR_SCALE, validity=validity)
        return lib.flame_nltgv2_debug_wireframe_begin(reg._ctx, host, dev, step, tri_valid, C.byref(p) if params else None, rows, cols,
                                                      C.c_float(GRAPH_SCALE))

    with gpu.Regularizer(0) as reg:
        assert raw(reg) == -4  # no graph
        reg.upload_graph(s["g"])
        assert raw(reg) == -1  # no resident triangles
        reg.interpolate_mesh(s["tris"], ROWS, COLS, graph_scale=GRAPH_SCALE)
        p = gpu.WireframeParams(scene_color_scale=COLOR_SCALE)
        first = reg.debug_wireframe(img, ROWS, COLS, GRAPH_SCALE, p)
        dbg_first = reg.debug_images(img, K, ROWS, COLS, gpu.DebugImageParams(scene_color_scale=COLOR_SCALE))
        reg.debug_images_begin(img, K, ROWS, COLS, gpu.DebugImageParams(scene_color_scale=COLOR_SCALE))  # pending across what follows
        reg.debug_wireframe_begin(img, ROWS, COLS, GRAPH_SCALE, p)  # pending: its _end must survive every error below
        assert raw(reg, dev=C.c_void_p(img.ctypes.data)) == -1  # both image pointers
        assert raw(reg, host=None) == -1                        # neither
        assert raw(reg, step=COLS - 1) == -1
        assert raw(reg, tri_valid=ones.ctypes.data, validity=0) == -1 and raw(reg, tri_valid=ones.ctypes.data, validity=2) == -1
        assert raw(reg, validity=1) == -1 and raw(reg, validity=3) == -1 and raw(reg, validity=-1) == -1
        assert raw(reg, params=False) == -1 and raw(reg, rows=0) == -1 and raw(reg, cols=-2) == -1 and raw(reg, rows=40000) == -1
        assert lib.flame_nltgv2_debug_wireframe_end(reg._ctx, None) == -1
        kept = reg.debug_wireframe_end()
        assert np.array_equal(kept["wireframe_img"], first["wireframe_img"])
        assert (kept["lines_drawn"], kept["lines_skipped"], kept["entries"]) == (first["lines_drawn"], first["lines_skipped"], first["entries"])
        # a whole wireframe begin / end inside a pending debug_images: that stage's outputs are its own
        again = reg.debug_wireframe(img, ROWS, COLS, GRAPH_SCALE, gpu.WireframeParams(scene_color_scale=0.6, flip=True))
        assert not np.array_equal(again["wireframe_img"], first["wireframe_img"])
        dbg = reg.debug_images_end()
        for k in ("idepthmap_img", "normals_img", "w1_map", "w2_map"):
            assert np.array_equal(dbg[k], dbg_first[k], equal_nan=True), k
        # ... and the reverse: a debug_images call inside a pending wireframe
        reg.debug_wireframe_begin(img, ROWS, COLS, GRAPH_SCALE, p)
        reg.debug_images(img, K, ROWS, COLS, gpu.DebugImageParams(scene_color_scale=0.6))
        Kinv = np.linalg.inv(K.astype(np.float64)).astype(F)
        reg.mesh_outputs(None, Kinv, ROWS, COLS, graph_scale=GRAPH_SCALE, want_filtered_map=True)
        kept = reg.debug_wireframe_end()
        assert np.array_equal(kept["wireframe_img"], first["wireframe_img"])
        # triangles of other arrays (interpolate_mesh_arrays): no resident triangles any more
        reg.debug_wireframe_begin(img, ROWS, COLS, GRAPH_SCALE, p)
        reg.interpolate_mesh_arrays(s["tris"], s["pos"], s["g"]["x"], ROWS, COLS)
        assert raw(reg) == -1
        # a new topology: the resident triangles belong to the old one
        reg.interpolate_mesh(s["tris"], ROWS, COLS, graph_scale=GRAPH_SCALE)
        reg.debug_wireframe_begin(img, ROWS, COLS, GRAPH_SCALE, p)
        reg.upload_graph(synth.copy_graph(s["g"]))
        assert raw(reg) == -1
        kept = reg.debug_wireframe_end()
        assert np.array_equal(kept["wireframe_img"], first["wireframe_img"])
    with gpu.Regularizer(0) as fresh:
        assert lib.flame_nltgv2_debug_wireframe_end(fresh._ctx, C.byref(gpu.regularizer._WireframeView())) == -1  # nothing begun


@pytest.mark.gpu
def test_gpu_pending_outputs_survive_the_other_stages_regrowing_their_pinned_buffers(gpu, scene):
    """Every stage's pinned buffer grows with half as much again; twice the rows and twice the columns is four times the bytes of every
    region but the per-vertex and per-triangle ones (a few hundred bytes here), so a call at 100 x 140 after one at 50 x 70 replaces
    the buffer of every stage it goes through.  A replaced buffer must be that stage's alone: what another stage's begin left
    pending comes out of its _end as it went in.  (A begin of the SAME stage does supersede its own pending _end.)"""
    from oracle import capi as oracle
    from tests import debug_ref as dr

    s = scene
    R2, C2 = 2 * ROWS, 2 * COLS
    img = np.ascontiguousarray(s["img"])
    big = tw.grey(R2, C2, 45)
    K = s["K"]
    Kinv = np.linalg.inv(K.astype(np.float64)).astype(F)
    wp, dp = gpu.WireframeParams(scene_color_scale=COLOR_SCALE), gpu.DebugImageParams(scene_color_scale=COLOR_SCALE)
    idepth = mr.vertex_idepths(s["g"]["x"], GRAPH_SCALE)
    small = dict(wireframe_img=tw.scene_wireframe(s)[0], idepthmap_img=dr.draw_inverse_depth_map(img, s["dense"], COLOR_SCALE),
                 normals_img=dr.draw_normals(img, K, s["dense"], s["w1m"], s["w2m"]), w1_map=s["w1m"], w2_map=s["w2m"])
    dense2, w1m2, w2m2 = (oracle.raster_interpolate_mesh(s["tris"], s["pos"], v, R2, C2) for v in (idepth, s["g"]["w1"], s["g"]["w2"]))
    large = dict(wireframe_img=wr.draw_wireframe(big, s["tris"], s["pos"], idepth, None, COLOR_SCALE)[0],
                 idepthmap_img=dr.draw_inverse_depth_map(big, dense2, COLOR_SCALE), normals_img=dr.draw_normals(big, K, dense2, w1m2, w2m2),
                 w1_map=w1m2, w2_map=w2m2)

    def same(got, ref, what):
        assert got.keys() & ref.keys(), what
        for k in got.keys() & ref.keys():
            assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k], equal_nan=True), (what, k)

    # the larger calls right behind two pending small ones: every stage they use replaces its buffer, and their results are right
    with gpu.Regularizer(0) as reg:
        reg.upload_graph(s["g"])
        reg.interpolate_mesh(s["tris"], ROWS, COLS, graph_scale=GRAPH_SCALE)
        reg.debug_wireframe_begin(img, ROWS, COLS, GRAPH_SCALE, wp)
        reg.debug_images_begin(img, K, ROWS, COLS, dp)
        dense, _ = reg.interpolate_mesh(s["tris"], R2, C2, graph_scale=GRAPH_SCALE)
        mesh = reg.mesh_outputs(None, Kinv, R2, C2, graph_scale=GRAPH_SCALE, want_filtered_map=True)
        dbg = reg.debug_images(big, K, R2, C2, dp)
        wire = reg.debug_wireframe(big, R2, C2, GRAPH_SCALE, wp)
        assert np.array_equal(dense, dense2, equal_nan=True) and mesh["filtered_map"].shape == (R2, C2)
        same(dbg, large, "debug images at 100 x 140")
        same(wire, large, "wireframe at 100 x 140")
    # two pending small begins, then the OTHER stages replace their buffers: the two small _ends return the first pictures
    with gpu.Regularizer(0) as reg:
        reg.upload_graph(s["g"])
        reg.interpolate_mesh_begin(s["tris"], ROWS, COLS, graph_scale=GRAPH_SCALE)  # (small buffers for the map and the mesh outputs first)
        reg.interpolate_mesh_end()
        reg.mesh_outputs(None, Kinv, ROWS, COLS, graph_scale=GRAPH_SCALE, want_filtered_map=True)
        reg.debug_wireframe_begin(img, ROWS, COLS, GRAPH_SCALE, wp)
        reg.debug_images_begin(img, K, ROWS, COLS, dp)
        reg.interpolate_mesh_begin(s["tris"], R2, C2, graph_scale=GRAPH_SCALE)
        mesh = reg.mesh_outputs(None, Kinv, R2, C2, graph_scale=GRAPH_SCALE, want_filtered_map=True)
        dense, _ = reg.interpolate_mesh_end()
        assert np.array_equal(dense, dense2, equal_nan=True) and mesh["filtered_map"].shape == (R2, C2)
        same(reg.debug_wireframe_end(), small, "pending wireframe, map and mesh outputs regrown")
        same(reg.debug_images_end(), small, "pending debug images, map and mesh outputs regrown")
        # ... and the two debug stages against each other (the resident map is the large one now)
        reg.debug_wireframe_begin(img, ROWS, COLS, GRAPH_SCALE, wp)
        same(reg.debug_images(big, K, R2, C2, dp), large, "debug images at 100 x 140 inside a pending wireframe")
        same(reg.debug_wireframe_end(), small, "pending wireframe, debug images regrown")
        reg.interpolate_mesh(s["tris"], ROWS, COLS, graph_scale=GRAPH_SCALE)
        reg.debug_images_begin(img, K, ROWS, COLS, dp)
        same(reg.debug_wireframe(big, R2, C2, GRAPH_SCALE, wp), large, "wireframe at 100 x 140 inside pending debug images")
        same(reg.debug_images_end(), small, "pending debug images, wireframe regrown")
