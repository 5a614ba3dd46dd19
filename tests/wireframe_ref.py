"""Sequential restatement of the reference's wireframe image, the checker of flame_nltgv2_debug_wireframe:

  Flame::drawWireframe                flame.cc:2414-2457
  utils::drawColorMappedWireframe     utils/image_utils.h:693-719
  utils::applyColorMapLine            utils/visualization.h:235-260

Triangle by triangle, three lines each (v0 -> v1, v1 -> v2, v0 -> v2), pixel by pixel, in the reference's order; the rule is the one
include/flame_nltgv2.h states (rules 1-7 there).  What the reference leaves to OpenCV, which is not part of this tree, is restated and
UNPINNED: the line walk (cv::LineIterator, OpenCV 3.2, connectivity 8), the rule for lines that leave the image (not drawn and counted,
where the reference clips) and the colour of a NaN (tests/debug_ref.py)."""
import numpy as np

from tests.debug_ref import _flip, _gray3, jet

F = np.float32


def cv_round(v):
    """cvRound: round half to even."""
    return int(np.rint(F(v)))


def walk(p1, p2):
    """The pixels cv::LineIterator(img, p1, p2) visits, starting at p1; count = max(|dx|, |dy|) + 1 of them."""
    x, y = int(p1[0]), int(p1[1])
    dx, dy = int(p2[0]) - x, int(p2[1]) - y
    sx, sy = (-1 if dx < 0 else 1), (-1 if dy < 0 else 1)
    dx, dy = abs(dx), abs(dy)
    if dy > dx:
        major, minor = (0, sy), (sx, 0)
        dx, dy = dy, dx
    else:
        major, minor = (sx, 0), (0, sy)
    err = dx - 2 * dy
    out = []
    for _ in range(dx + 1):
        out.append((x, y))
        m = err < 0
        err += -2 * dy + (2 * dx if m else 0)
        x += major[0] + (minor[0] if m else 0)
        y += major[1] + (minor[1] if m else 0)
    return out


def line_values(a_val, b_val, count):
    """val_ii = A_val + ii * slope0 with slope0 = (B_val - A_val) / count, in float without FMA."""
    with np.errstate(all="ignore"):
        slope0 = F(F(F(b_val) - F(a_val)) / F(count))
        return [F(F(a_val) + F(F(ii) * slope0)) for ii in range(count)]


def blend(old, color):
    """color * 0.5f + old * 0.5f stored into a uchar: exact in float, truncated."""
    return (np.asarray(color, np.int32) + np.asarray(old, np.int32)) >> 1


def endpoint(p, rows, cols):
    """The rounded endpoint, or None where it is not finite or rounds outside the image."""
    if not (np.isfinite(p[0]) and np.isfinite(p[1])):
        return None
    x, y = cv_round(p[0]), cv_round(p[1])
    return (x, y) if 0 <= x <= cols - 1 and 0 <= y <= rows - 1 else None


def draw_wireframe(img, tris, pos, idepth, tri_valid=None, scene_color_scale=1.0, flip=False, want_counts=False):
    """-> (image, lines_drawn, lines_skipped); with want_counts also the number of draws per pixel.  idepth: vtx_idepths_ =
    x * graph_scale (tests/mesh_ref.vertex_idepths)."""
    out = _gray3(img).astype(np.int32)
    rows, cols = out.shape[:2]
    pos, idepth = np.asarray(pos, F), np.asarray(idepth, F)
    counts = np.zeros((rows, cols), np.int64)
    drawn = skipped = 0
    for t, tri in enumerate(np.asarray(tris).reshape(-1, 3)):
        if tri_valid is not None and not tri_valid[t]:
            continue
        for a, b in ((tri[0], tri[1]), (tri[1], tri[2]), (tri[0], tri[2])):
            p1, p2 = endpoint(pos[a], rows, cols), endpoint(pos[b], rows, cols)
            if p1 is None or p2 is None:
                skipped += 1
                continue
            drawn += 1
            px = walk(p1, p2)
            vals = np.array(line_values(idepth[a], idepth[b], len(px)), F)
            with np.errstate(all="ignore"):
                colors = jet((vals * F(scene_color_scale)).astype(F))
            for (x, y), c in zip(px, colors):
                out[y, x] = blend(out[y, x], c)
                counts[y, x] += 1
    res = (_flip(out.astype(np.uint8), flip), drawn, skipped)
    return res + (counts,) if want_counts else res
