"""The debug images on the device, GPU part (the CPU part, the scene and why the two are separate files: tests/test_debug_images.py).
Every byte is compared with the numpy restatement tests/debug_ref.py and, for the w maps, with the raster checker; no tolerance.
The state is set with upload_graph so that x, w1 and w2 are chosen, not solved for."""
import ctypes as C

import numpy as np
import pytest

from flame_amd import synth
from oracle import capi as oracle
from tests import debug_ref as dr
from tests import mesh_ref as mr
from tests.test_debug_images import COLOR_SCALE, COLS, GRAPH_SCALE, ROWS, F, assert_image, feature_set
from tests.test_debug_images import scene  # noqa: F401  (the module-scoped scene, as a fixture)
from tests.test_mesh_outputs import bits


@pytest.fixture(scope="module")
def gpu(built):
    import torch  # noqa: F401

    import flame_amd

    return flame_amd


@pytest.mark.gpu
def test_gpu_idepth_image_host_and_device_path_flipped_or_not(gpu, scene):
    import torch

    s = scene
    dev_buf = torch.from_numpy(s["buf"]).cuda()
    with gpu.Regularizer(0) as reg:
        reg.upload_graph(s["g"])
        dense, _ = reg.interpolate_mesh(s["tris"], ROWS, COLS, graph_scale=GRAPH_SCALE)
        assert np.array_equal(bits(dense), bits(s["dense"]))
        for flip in (False, True):
            ref = dr.draw_inverse_depth_map(s["img"], s["dense"], COLOR_SCALE, flip)
            p = gpu.DebugImageParams(scene_color_scale=COLOR_SCALE, flip=flip, want_normals=False)
            host = reg.debug_images(s["img"], s["K"], ROWS, COLS, p)  # a view: step_bytes 96
            assert set(host) == {"idepthmap_img", "device_ms"}
            assert_image(host["idepthmap_img"], ref, f"host image, flip {flip}")
            dev = reg.debug_images(None, s["K"], ROWS, COLS, p, img_device=dev_buf.data_ptr() + 7, step_bytes=96)
            assert_image(dev["idepthmap_img"], ref, f"device image, flip {flip}")
            tight = reg.debug_images(np.ascontiguousarray(s["img"]), s["K"], ROWS, COLS, p)  # step_bytes == cols
            assert_image(tight["idepthmap_img"], ref, f"packed host image, flip {flip}")
        # the synchronous C form into the caller's arrays
        out = np.zeros((ROWS, COLS, 3), np.uint8)
        p = gpu.DebugImageParams(scene_color_scale=0.75)
        k = np.ascontiguousarray(s["K"], F).reshape(9)
        rc = gpu.load_library().flame_nltgv2_debug_images(reg._ctx, s["img"].ctypes.data, None, 96, k.ctypes.data_as(C.POINTER(C.c_float)),
                                                          C.byref(p), ROWS, COLS, out.ctypes.data_as(C.POINTER(C.c_uint8)), None, None, None)
        assert rc == 0
        assert_image(out, dr.draw_inverse_depth_map(s["img"], s["dense"], 0.75), "synchronous form")
    del dev_buf


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
def test_gpu_w_maps_and_normals_image(gpu, scene, masked):
    """masked: the resident map was rasterised with a validity mask, so its key image does not name the winners of the all-valid
    rasterisation and the stage rasterises w1 and w2 itself; the maps are the all-valid ones either way."""
    s = scene
    tri_valid = None
    dense_ref = s["dense"]
    if masked:
        tri_valid = np.ones(len(s["tris"]), np.uint8)
        tri_valid[::3] = 0
        dense_ref = oracle.raster_interpolate_mesh(s["tris"], s["pos"], mr.vertex_idepths(s["g"]["x"], GRAPH_SCALE), ROWS, COLS, tri_valid=tri_valid)
        assert np.isnan(dense_ref).sum() > np.isnan(s["dense"]).sum()
    with gpu.Regularizer(0) as reg:
        reg.upload_graph(s["g"])
        reg.interpolate_mesh_begin(s["tris"], ROWS, COLS, graph_scale=GRAPH_SCALE, tri_valid=tri_valid)
        for flip in (False, True):
            got = reg.debug_images(s["img"], s["K"], ROWS, COLS, gpu.DebugImageParams(scene_color_scale=COLOR_SCALE, flip=flip))
            assert np.array_equal(bits(got["w1_map"]), bits(s["w1m"])), "w1_map"
            assert np.array_equal(bits(got["w2_map"]), bits(s["w2m"])), "w2_map"
            assert_image(got["normals_img"], dr.draw_normals(s["img"], s["K"], dense_ref, s["w1m"], s["w2m"], flip), f"normals, flip {flip}")
            assert_image(got["idepthmap_img"], dr.draw_inverse_depth_map(s["img"], dense_ref, COLOR_SCALE, flip), f"idepth, flip {flip}")
        dense, _ = reg.interpolate_mesh_end()
        assert np.array_equal(bits(dense), bits(dense_ref))
        only_n = reg.debug_images(s["img"], s["K"], ROWS, COLS, gpu.DebugImageParams(want_idepthmap=False))
        assert "idepthmap_img" not in only_n
        assert_image(only_n["normals_img"], dr.draw_normals(s["img"], s["K"], dense_ref, s["w1m"], s["w2m"]), "normals alone")


@pytest.mark.gpu
def test_gpu_features_image_and_counters(gpu, scene):
    from flame_amd.stereo import FeatureTracker, StereoParams

    s = scene
    K = s["K"]
    Kinv = np.linalg.inv(K.astype(np.float64)).astype(F)
    feats = feature_set()
    img = np.ascontiguousarray(s["img"])
    with FeatureTracker(K, Kinv, COLS, ROWS, border=3) as tr:
        tr.add_frame(11, img)
        tr.set_features(feats)
        sp = StereoParams(win_size=1, rescale_factor_max=0.5)  # the valid region of projectFeatures: one pixel off the border
        tr.project_features(sp, 11, [dict(id=10, q_to_new=[1, 0, 0, 0], t_to_new=[0, 0, 0])])
        proj = tr.get_projected()
        # conditions on the projected set, which is what is drawn
        assert len(proj) >= 40
        var = proj["idepth_var"]
        run = np.unique(var[np.isin(proj["id"], np.arange(108, 124))])
        at = [v for v in run if np.nextafter(v, F(1)) in run and np.nextafter(v, F(0)) in run]
        assert at, run
        thr = F(at[0])  # a variance equal to the threshold, and one an ulp either side of it
        assert (var == thr).any() and (var == np.nextafter(thr, F(1))).any() and (var == np.nextafter(thr, F(0))).any() and np.isnan(var).any()
        xi, yi = (proj["x"] + F(0.5)).astype(int), (proj["y"] + F(0.5)).astype(int)
        drawn = var < thr
        assert (xi[drawn] - 2 < 0).any() and (xi[drawn] + 2 >= COLS).any() and (yi[drawn] - 2 < 0).any() and (yi[drawn] + 2 >= ROWS).any()
        d = np.flatnonzero(drawn)
        close = [(a, b) for a in d for b in d if a < b and abs(xi[a] - xi[b]) <= 4 and abs(yi[a] - yi[b]) <= 4]
        assert len(close) >= 3  # overlapping rectangles
        assert not np.isnan(proj["idepth_mu"]).any()
        for flip in (False, True):
            for scale in (1.0, 0.6):
                ref, nc, nu = dr.draw_features(img, proj, thr, scale, flip)
                got, gc, gu = tr.draw_features(11, float(thr), scale, flip)
                assert (gc, gu) == (nc, nu) and nc + nu == len(proj) and 0 < nu
                assert_image(got, ref, f"features, flip {flip}, scale {scale}")
        # the accessor: the unpadded image inside the padded one
        ptr, step = tr.frame_image_device(11)
        assert ptr != 0 and step == COLS + 6
        with gpu.Regularizer(0) as reg:
            reg.upload_graph(s["g"])
            reg.interpolate_mesh(s["tris"], ROWS, COLS, graph_scale=GRAPH_SCALE)
            got = reg.debug_images(None, K, ROWS, COLS, gpu.DebugImageParams(scene_color_scale=COLOR_SCALE), img_device=ptr, step_bytes=step)
            assert_image(got["idepthmap_img"], dr.draw_inverse_depth_map(img, s["dense"], COLOR_SCALE), "over the resident frame's image")
        # an empty projected set: the grey image
        tr.set_features(feats[:0])
        tr.project_features(sp, 11, [dict(id=10, q_to_new=[1, 0, 0, 0], t_to_new=[0, 0, 0])])
        got, gc, gu = tr.draw_features(11, 1.0)
        assert (gc, gu) == (0, 0) and np.array_equal(got, np.repeat(img[:, :, None], 3, axis=2))
        with pytest.raises(gpu.NLTGV2Error):
            tr.draw_features(99, 1.0)  # no such frame


@pytest.mark.gpu
def test_gpu_beside_a_running_solver_nothing_else_is_disturbed(gpu, scene):
    """interpolate_mesh_begin, debug_images_begin, run_async, the two _ends: the images describe the map's state, and the resident
    map (through init_from_map of a following sync), the pinned map, mesh_outputs(triangles = NULL) and the solver's state are
    bit-equal to a run without the debug call."""
    s = scene
    g, tris = s["g"], s["tris"]
    Kinv = np.linalg.inv(s["K"].astype(np.float64)).astype(F)
    params = gpu.Params()
    rng = np.random.default_rng(5)
    V = g["V"]
    keep = np.sort(rng.permutation(V)[: V - 6])
    new_pos = (rng.random((8, 2)) * [50, 34] + [9, 7]).astype(F)
    feat_id = np.concatenate([keep, np.arange(V, V + 8)]).astype(np.int32)
    pos2 = np.concatenate([g["pos"][keep], new_pos]).astype(F)
    data2 = np.concatenate([g["data_term"][keep], np.full(8, 0.6, F)]).astype(F)
    _, edges2 = gpu.delaunay(pos2)
    runs = []
    for with_debug in (False, True):
        with gpu.Regularizer(0) as reg:
            reg.upload_graph(g)
            reg.run(params, 40)
            at40 = reg.download_state()
            reg.interpolate_mesh_begin(tris, ROWS, COLS, graph_scale=GRAPH_SCALE)
            if with_debug:
                reg.debug_images_begin(s["img"], s["K"], ROWS, COLS, gpu.DebugImageParams(scene_color_scale=COLOR_SCALE))
            reg.run_async(params, 2000)
            dense_view, cov = reg.interpolate_mesh_end(copy=False)
            dense = dense_view.copy()
            if with_debug:
                got = reg.debug_images_end()
                idepth = mr.vertex_idepths(at40["x"], GRAPH_SCALE)
                dense_ref = oracle.raster_interpolate_mesh(tris, g["pos"], idepth, ROWS, COLS)
                w1m = oracle.raster_interpolate_mesh(tris, g["pos"], at40["w1"], ROWS, COLS)
                w2m = oracle.raster_interpolate_mesh(tris, g["pos"], at40["w2"], ROWS, COLS)
                assert np.array_equal(bits(dense), bits(dense_ref))
                assert np.array_equal(bits(got["w1_map"]), bits(w1m)) and np.array_equal(bits(got["w2_map"]), bits(w2m))
                assert_image(got["idepthmap_img"], dr.draw_inverse_depth_map(s["img"], dense_ref, COLOR_SCALE), "idepth image of the map's state")
                assert_image(got["normals_img"], dr.draw_normals(s["img"], s["K"], dense_ref, w1m, w2m), "normals image of the map's state")
                assert np.array_equal(dense_view, dense, equal_nan=True), "interpolate_mesh_end's pinned map changed"
            mesh = reg.mesh_outputs(None, Kinv, ROWS, COLS, graph_scale=GRAPH_SCALE, want_filtered_map=True)
            state = reg.download_state()
            assert not np.array_equal(state["x"], at40["x"])
            reg.sync_graph(feat_id, pos2, data2, np.ones(len(feat_id), F), edges2, init_graph_scale=GRAPH_SCALE, init_from_map=True)
            runs.append(dict(dense=dense, cov=cov, mesh=mesh, state=state, synced=reg.download_state()))
    a, b = runs
    assert np.array_equal(bits(a["dense"]), bits(b["dense"])) and a["cov"] == b["cov"]
    for k in ("tri_valid", "normals", "vtx_idepth", "filtered_map"):
        assert np.array_equal(a["mesh"][k], b["mesh"][k], equal_nan=True), k
    for which in ("state", "synced"):
        for k in a[which]:
            assert np.array_equal(bits(a[which][k]), bits(b[which][k])), (which, k)
    assert not np.array_equal(a["synced"]["x"][-8:], data2[-8:])  # (the new vertices did start at the map's prediction)


@pytest.mark.gpu
def test_gpu_every_error_is_reported_before_anything_is_enqueued(gpu, scene):
    s = scene
    lib = gpu.load_library()
    K9 = np.ascontiguousarray(s["K"], F).reshape(9)
    FP = C.POINTER(C.c_float)
    img = np.ascontiguousarray(s["img"])
    p = gpu.DebugImageParams(scene_color_scale=COLOR_SCALE)

    def raw(reg, host=img.ctypes.data, dev=None, step=COLS, K=K9.ctypes.data_as(FP), params=C.byref(p), rows=ROWS, cols=COLS):
        return lib.flame_nltgv2_debug_images_begin(reg._ctx, host, dev, step, K, params, rows, cols)

    with gpu.Regularizer(0) as reg:
        assert raw(reg) == -4  # no graph
        reg.upload_graph(s["g"])
        assert raw(reg) == -1  # no resident map
        reg.interpolate_mesh(s["tris"], ROWS, COLS, graph_scale=GRAPH_SCALE)
        first = reg.debug_images(img, s["K"], ROWS, COLS, p)
        reg.debug_images_begin(img, s["K"], ROWS, COLS, p)  # pending: its _end must survive every error below
        assert raw(reg, rows=ROWS + 1) == -1 and raw(reg, cols=COLS - 1) == -1 and raw(reg, rows=0) == -1  # a map of another size
        assert raw(reg, dev=C.c_void_p(img.ctypes.data)) == -1  # both image pointers
        assert raw(reg, host=None) == -1                        # neither
        assert raw(reg, step=COLS - 1) == -1
        assert raw(reg, K=None) == -1 and raw(reg, params=None) == -1
        assert lib.flame_nltgv2_debug_images_end(reg._ctx, None) == -1
        kept = reg.debug_images_end()
        for k in ("idepthmap_img", "normals_img", "w1_map", "w2_map"):
            assert np.array_equal(kept[k], first[k], equal_nan=True), k
        # another image in the resident buffers (interpolate_mesh_arrays): no resident map any more
        reg.debug_images_begin(img, s["K"], ROWS, COLS, p)
        reg.interpolate_mesh_arrays(s["tris"], s["pos"], s["g"]["x"], ROWS, COLS)
        assert raw(reg) == -1
        # a new topology: the resident triangles belong to the old one
        reg.interpolate_mesh(s["tris"], ROWS, COLS, graph_scale=GRAPH_SCALE)
        reg.debug_images_begin(img, s["K"], ROWS, COLS, p)
        g2 = synth.copy_graph(s["g"])
        reg.upload_graph(g2)
        assert raw(reg) == -1
        kept = reg.debug_images_end()
        for k in ("idepthmap_img", "normals_img", "w1_map", "w2_map"):
            assert np.array_equal(kept[k], first[k], equal_nan=True), k
    with gpu.Regularizer(0) as fresh:
        assert lib.flame_nltgv2_debug_images_end(fresh._ctx, C.byref(gpu.regularizer._DebugImagesView())) == -1  # nothing begun


@pytest.mark.gpu
def test_gpu_key_image_is_not_read_after_mesh_outputs_hands_in_a_new_triangle_list(gpu, scene):
    """interpolate_mesh_begin(tris) leaves a key image that names winners of `tris`; mesh_outputs(tris reversed) replaces the resident
    triangles and rasterises nothing.  The key image's indices now name other triangles, so the stage has to rasterise w1 / w2 itself,
    over the reversed list."""
    s = scene
    rev = np.ascontiguousarray(s["tris"][::-1])
    Kinv = np.linalg.inv(s["K"].astype(np.float64)).astype(F)
    w1m = oracle.raster_interpolate_mesh(rev, s["pos"], s["g"]["w1"], ROWS, COLS)
    w2m = oracle.raster_interpolate_mesh(rev, s["pos"], s["g"]["w2"], ROWS, COLS)
    with gpu.Regularizer(0) as reg:
        reg.upload_graph(s["g"])
        reg.interpolate_mesh_begin(s["tris"], ROWS, COLS, graph_scale=GRAPH_SCALE)
        reg.mesh_outputs(rev, Kinv, ROWS, COLS, graph_scale=GRAPH_SCALE)
        got = reg.debug_images(s["img"], s["K"], ROWS, COLS, gpu.DebugImageParams(scene_color_scale=COLOR_SCALE))
        assert np.array_equal(bits(got["w1_map"]), bits(w1m)), "w1_map"
        assert np.array_equal(bits(got["w2_map"]), bits(w2m)), "w2_map"
        dense, _ = reg.interpolate_mesh_end()
        assert np.array_equal(bits(dense), bits(s["dense"]))  # (the map itself is the first list's)
        assert_image(got["normals_img"], dr.draw_normals(s["img"], s["K"], s["dense"], w1m, w2m), "normals over the reversed list's maps")
