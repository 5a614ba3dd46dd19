"""Sequential restatement of the reference's matches image (getDebugImageMatches), the checker of flame_stereo_draw_matches:

  Flame::updateFeatureIDepths   flame.cc:1286-1534 (the loop :1307-1496 and its three copies of the ring block)
  Flame::trackFeature           flame.cc:1536-1752
  utils::applyColorMapLine      utils/visualization.h:236-260

Feature by feature, in index order, drawing into a numpy image pixel by pixel; the rule is the one include/flame_stereo.h states
(rules 1-6 there).  Only the CONTROL FLOW around the stereo routines is restated here: predict, getSearchRegion, search, the
measurement model, the fusion and project are the oracle's (oracle/stereo_oracle.c through oracle.stereo_capi.lib()).  The
self-check (tests/test_matches.py) is that the feature records this walk ends with equal those of the oracle's own
stereo_update_feature_idepths on the same input, record for record.

NOT pinned to the reference binary, like the rest of the front-end.  What the reference leaves to OpenCV, which is not part of
this tree, is restated and UNPINNED: cv::rectangle's fill rule, the line walk (tests/wireframe_ref.py), the ring's pixel set
(ring_points), the rule for a segment whose rounded endpoint leaves the image (not drawn and counted) and the conversion of a
coordinate that does not fit an int (saturates; a NaN gives 0).  One deliberate deviation: a ring whose projection would
FLAME_ASSERT is not drawn and is counted."""
import ctypes as C

import numpy as np

from oracle import stereo_capi as so
from tests.debug_ref import _flip, _gray3
from tests.wireframe_ref import blend, endpoint, walk

F = np.float32
_FP = C.POINTER(C.c_float)

# kind_count order (flame_stereo_matches_stats): seven rectangles, then the two rings
MOVE_FAILED, MOVED, NO_REGION, NO_GRADIENT, NO_GRADIENT_FRESH, AMBIGUOUS, MAX_COST, GREEN, BLUE = range(9)
COLORS = {MOVE_FAILED: (0, 51, 102), MOVED: (255, 0, 255), NO_REGION: (0, 0, 0), NO_GRADIENT: (255, 255, 0),
          NO_GRADIENT_FRESH: (255, 255, 255), AMBIGUOUS: (0, 0, 255), MAX_COST: (0, 255, 255), GREEN: (0, 255, 0),
          BLUE: (255, 0, 0)}

_READY = False


def _lib():
    """The oracle's library with the signatures of the three routines oracle/stereo_capi.py does not bind."""
    global _READY
    L = so.lib()
    if not _READY:
        GP, PP, f, i = C.POINTER(so.Geometry), C.POINTER(so.Params), C.c_float, C.c_int
        L.stereo_predict.argtypes = [GP, f, f, f, f, f, _FP, _FP, _FP, _FP]
        L.stereo_predict.restype = i
        L.stereo_search.argtypes = [PP, GP, f, C.c_void_p, C.c_void_p, i, i, i, f, f, f, f, f, f, _FP, _FP]
        L.stereo_search.restype = i
        L.stereo_meas_idepth.argtypes = [PP, GP, _FP, _FP, i, i, i, f, f, f, f, _FP, _FP]
        L.stereo_meas_idepth.restype = i
        _READY = True
    return L


def c_int(v):
    """(int)v of a float: C truncation; saturates where C leaves it undefined, a NaN gives 0 (UNPINNED)."""
    v = float(v)
    if v != v:
        return 0
    return int(max(-2.0 ** 31, min(2.0 ** 31 - 1, np.trunc(v))))


def center(x, y):
    """cv::Point2i(x + 0.5f, y + 0.5f)"""
    with np.errstate(all="ignore"):
        return c_int(F(F(x) + F(0.5))), c_int(F(F(y) + F(0.5)))


def ring_points(cx, cy, r):
    """The pixels of cv::circle(centre, r, colour) with thickness 1, LINE_8 (UNPINNED), each once, unclipped."""
    out = []

    def plot4(a, b):
        out.append((cx + a, cy + b))
        if a:
            out.append((cx - a, cy + b))
        if b:
            out.append((cx + a, cy - b))
        if a and b:
            out.append((cx - a, cy - b))

    err, dx, dy, plus, minus = 0, r, 0, 1, 2 * r - 1
    while dx >= dy:
        plot4(dx, dy)
        if dx != dy:
            plot4(dy, dx)
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return out


def fill_rect(out, cx, cy, r, color):
    """cv::rectangle(centre - (r, r), centre + (r, r), colour, -1): both corners inclusive, clipped.  -> pixels written."""
    rows, cols = out.shape[:2]
    x0, x1 = max(cx - r, 0), min(cx + r, cols - 1)
    y0, y1 = max(cy - r, 0), min(cy + r, rows - 1)
    if x0 > x1 or y0 > y1:
        return 0
    out[y0:y1 + 1, x0:x1 + 1] = color
    return (x1 - x0 + 1) * (y1 - y0 + 1)


def draw_ring(out, cx, cy, r, color):
    rows, cols = out.shape[:2]
    n = 0
    for x, y in ring_points(cx, cy, r):
        if 0 <= x < cols and 0 <= y < rows:
            out[y, x] = color
            n += 1
    return n


def blend_line(out, p1, p2, color):
    """applyColorMapLine with a constant colour and alpha 0.5 between two rounded endpoints inside the image."""
    px = walk(p1, p2)
    for x, y in px:
        out[y, x] = blend(out[y, x], color)
    return len(px)


def _rect_contains(rx, ry, rw, rh, px, py):
    if not (np.isfinite(px) and np.isfinite(py)):
        return False
    ix, iy = int(np.rint(F(px))), int(np.rint(F(py)))
    return rx <= ix < rx + rw and ry <= iy < ry + rh


def update_and_draw(params, K, Kinv, width, height, pad, frames, new_frame, new_img, curr_pf_id, feats, flip=False, draw=True, trace=None):
    """updateFeatureIDepths with debug_draw_matches on.  `frames`: list of dicts {id, img_pad, q_to_new, t_to_new, q_to_pf,
    t_to_pf}; new_frame = (img_pad, gradx_pad, grady_pad); new_img: the unpadded grey image; `feats` (oracle FEATURE_DTYPE) is
    updated in place.  Returns a dict: rc and stats[7] as oracle.stereo_capi.update_feature_idepths gives them, img,
    kind_count[9], lines_drawn, lines_skipped, rings_skipped (and its split green_skipped / blue_skipped), entries.
    `trace`: None, or a list that receives one (draw id, kind, "rect" | "line" | "ring", geometry) per draw: the centre of a
    rectangle or ring, the two rounded endpoints of a segment."""
    L = _lib()
    P = params
    out = _gray3(new_img).astype(np.int32)
    rows, cols = height + 2 * pad, width + 2 * pad
    r1, r2 = width // 320, 4 * width // 320
    geos = {}
    for fr in frames:
        fid = int(fr["id"])
        if fid not in geos:
            geos[fid] = (so.load_geometry(K, Kinv, fr["q_to_new"], fr["t_to_new"]),
                         so.load_geometry(K, Kinv, fr["q_to_pf"], fr["t_to_pf"]),
                         np.ascontiguousarray(fr["img_pad"], np.uint8), np.asarray(fr["t_to_new"], F))
    new_pad = np.ascontiguousarray(new_frame[0], np.uint8)
    new_gx, new_gy = np.ascontiguousarray(new_frame[1], F), np.ascontiguousarray(new_frame[2], F)
    stats = np.zeros(7, np.int32)
    res = dict(rc=0, stats=stats, kind_count=[0] * 9, lines_drawn=0, lines_skipped=0, rings_skipped=0, green_skipped=0,
               blue_skipped=0, entries=0)
    kc = res["kind_count"]
    off = F(pad)
    with np.errstate(all="ignore"):
        border = int(F(F(F(P.rescale_factor_max) * F(P.win_size)) / F(2)) + F(1))
    row_offset = height // 3 if P.do_letterbox else 0
    region = (border, border + row_offset, width - 2 * border, height - 2 * border - 2 * row_offset)
    fl = [C.c_float() for _ in range(4)]
    ref = [C.byref(v) for v in fl]

    cur = [0]  # the feature being walked

    def note(k, kind, what, geometry):
        if trace is not None:
            trace.append((4 * cur[0] + k, kind, what, geometry))

    def rect(kind, ucx, ucy):
        kc[kind] += 1
        cx, cy = center(ucx, ucy)
        note(0, kind, "rect", (cx, cy))
        if draw:
            res["entries"] += fill_rect(out, cx, cy, r1, COLORS[kind])

    def fail(f, g):
        with np.errstate(all="ignore"):
            f["idepth_var"] = F(F(f["idepth_var"]) * F(P.process_fail_var_factor))
            over = bool(F(f["idepth_var"]) > F(P.idepth_var_max))
        rings = []
        if over:
            f["valid"] = 0
            stats[1] += 1
            rings.append((GREEN, "green_skipped"))
        f["num_dropouts"] += 1
        if int(f["num_dropouts"]) > int(np.uint32(P.max_dropouts)):
            f["valid"] = 0
            stats[2] += 1
            rings.append((BLUE, "blue_skipped"))
        for kind, skipped in rings:
            a, b, c = C.c_float(), C.c_float(), C.c_float()
            if L.stereo_project_idepth(C.byref(g), F(f["x"]), F(f["y"]), F(f["idepth_mu"]), C.byref(a), C.byref(b), C.byref(c)):
                res["rings_skipped"] += 1  # the reference would assert here; the library leaves the ring out
                res[skipped] += 1
                continue
            kc[kind] += 1
            cx, cy = center(a.value, b.value)
            note(2 if kind == GREEN else 3, kind, "ring", (cx, cy))
            if draw:
                res["entries"] += draw_ring(out, cx, cy, r2, COLORS[kind])

    for i in range(feats.shape[0]):
        f = feats[i]
        cur[0] = i
        if int(f["frame_id"]) not in geos:
            res["rc"] = 1 + i
            break
        g, gpf, ref_pad, t = geos[int(f["frame_id"])]
        with np.errstate(all="ignore"):
            baseline = np.sqrt(F(F(F(t[0] * t[0]) + F(t[1] * t[1])) + F(t[2] * t[2])))
        if baseline < F(P.min_baseline):
            continue
        # ---- trackFeature ----
        tracked, asserted = False, False
        flow = None
        while True:
            pr = L.stereo_predict(C.byref(g), P.process_var_factor, f["x"], f["y"], f["idepth_mu"], f["idepth_var"], *ref)
            if pr < 0:
                asserted = True
            if pr != 0:
                break
            ucx, ucy, idepth_cmp = F(fl[0].value), F(fl[1].value), F(fl[2].value)
            rescale = F(1.0)
            with np.errstate(all="ignore"):
                if F(f["idepth_mu"]) > 0 and idepth_cmp > 0:
                    rescale = F(idepth_cmp / F(f["idepth_mu"]))
            if np.isnan(rescale) or not rescale > 0:
                asserted = True
                break
            if rescale <= F(P.rescale_factor_min) or rescale >= F(P.rescale_factor_max):
                mr = L.stereo_predict(C.byref(gpf), P.process_var_factor, f["x"], f["y"], f["idepth_mu"], f["idepth_var"], *ref)
                if mr < 0:
                    asserted = True
                    break
                upx, upy, idepth_pf = F(fl[0].value), F(fl[1].value), F(fl[2].value)
                if mr != 0 or not _rect_contains(*region, upx, upy):
                    f["valid"] = 0
                    rect(MOVE_FAILED, ucx, ucy)
                    break
                old = F(f["idepth_mu"])
                f["frame_id"] = curr_pf_id
                f["x"], f["y"] = upx, upy
                f["idepth_mu"] = idepth_pf
                with np.errstate(all="ignore"):
                    v4 = F(idepth_pf / old)
                    v4 = F(v4 * v4)
                    v4 = F(v4 * v4)
                    if float(idepth_pf) < 1e-6:
                        v4 = F(1)
                    f["idepth_var"] = F(F(f["idepth_var"]) * v4)
                rect(MOVED, ucx, ucy)
                break
            sr = so.search_region(P, g, width, height, f["x"], f["y"], f["idepth_mu"], f["idepth_var"])
            if sr[0] < 0:
                asserted = True
                break
            if sr[0] == 0:
                rect(NO_REGION, ucx, ucy)
                break
            sx, sy, ex, ey = sr[1:5]
            if not _rect_contains(*region, f["x"], f["y"]):
                break
            fl[0].value, fl[1].value = ucx, ucy
            st = L.stereo_search(C.byref(P), C.byref(g), rescale, ref_pad.ctypes.data, new_pad.ctypes.data, rows, cols, cols,
                                 F(F(f["x"]) + off), F(F(f["y"]) + off), F(sx + off), F(sy + off), F(ex + off), F(ey + off),
                                 ref[0], ref[1])
            if st < 0:
                asserted = True
                break
            f["search_status"] = st
            if st != 0:
                kind = {1: NO_GRADIENT_FRESH if int(f["num_updates"]) == 0 else NO_GRADIENT, 2: AMBIGUOUS, 3: MAX_COST}[st]
                rect(kind, ucx, ucy)
                p1, p2 = endpoint((sx, sy), height, width), endpoint((ex, ey), height, width)
                if p1 is None or p2 is None:
                    res["lines_skipped"] += 1
                else:
                    res["lines_drawn"] += 1
                    note(1, kind, "line", (p1, p2))
                    if draw:
                        res["entries"] += blend_line(out, p1, p2, COLORS[kind])
                break
            flow = (F(F(fl[0].value) - off), F(F(fl[1].value) - off))
            tracked = True
            break
        if asserted:
            res["rc"] = -(1 + i)
            break
        status = int(f["search_status"])
        if status in (1, 2, 3):
            stats[2 + status] += 1
        if not tracked:
            fail(f, g)
            continue
        sr = L.stereo_meas_idepth(C.byref(P), C.byref(g), new_gx.ctypes.data_as(_FP), new_gy.ctypes.data_as(_FP), rows, cols, cols,
                                  f["x"], f["y"], flow[0], flow[1], ref[0], ref[1])
        if sr < 0:
            res["rc"] = -(1 + i)
            break
        if sr == 0:
            fail(f, g)
            continue
        mu_meas, var_meas = F(fl[0].value), F(fl[1].value)
        if not L.stereo_fuse(f["idepth_mu"], f["idepth_var"], mu_meas, var_meas, ref[2], ref[3], P.outlier_sigma_thresh):
            fail(f, g)
            continue
        mu_post, var_post = F(fl[2].value), F(fl[3].value)
        if np.isnan(mu_post) or np.isnan(var_post) or not var_post >= 0:
            res["rc"] = -(1 + i)
            break
        if P.do_meas_fusion:
            f["idepth_mu"], f["idepth_var"] = mu_post, var_post
        else:
            f["idepth_mu"], f["idepth_var"] = mu_meas, var_meas
        f["valid"] = 1
        f["num_updates"] += 1
        f["num_dropouts"] = 0
        stats[0] += 1
        stats[6] = 1
    res["img"] = _flip(out.astype(np.uint8), flip)
    return res
