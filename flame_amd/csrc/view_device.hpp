// view_device.hpp -- the device functions of the view renderer's rules 1 - 5 (include/flame_nltgv2.h, flame_nltgv2_render_view_begin),
// one copy for view_kernels.hip (one mesh into one key image) and fuse_kernels.hip (up to eight meshes into eight key layers).  Both
// translation units are built with -ffp-contract=off: every expression here is float32 without FMA, every sum of three products left
// to right; division and the int64 -> float conversions are correctly rounded.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "view_kernels.h"

namespace flame_hip {
namespace view_device {

__device__ __forceinline__ float dot3(const float* m, float x, float y, float z) { return (m[0] * x + m[1] * y) + m[2] * z; }

// Rule 1 for the vertex at p (source pixels) with inverse depth id.
__device__ __forceinline__ ViewVertex view_vertex(float2 p, float id, const ViewCamera& cam) {
  const float qx = dot3(cam.Kinv_src, p.x, p.y, 1.0f), qy = dot3(cam.Kinv_src + 3, p.x, p.y, 1.0f), qz = dot3(cam.Kinv_src + 6, p.x, p.y, 1.0f);
  const float Px = qx / id, Py = qy / id, Pz = qz / id;
  const float Dx = dot3(cam.R, Px, Py, Pz) + cam.t[0], Dy = dot3(cam.R + 3, Px, Py, Pz) + cam.t[1], Dz = dot3(cam.R + 6, Px, Py, Pz) + cam.t[2];
  const float hx = dot3(cam.K_dst, Dx, Dy, Dz), hy = dot3(cam.K_dst + 3, Dx, Dy, Dz), hz = dot3(cam.K_dst + 6, Dx, Dy, Dz);
  const float sx = (hx / hz) * 16.0f, sy = (hy / hz) * 16.0f;
  const float ssx = p.x * 16.0f, ssy = p.y * 16.0f;
  // (every comparison with a NaN is false: a NaN anywhere makes the vertex unusable)
  const bool usable = id > 0.0f && Dz > cam.near_depth && __builtin_fabsf(sx) <= kViewCoordBound && __builtin_fabsf(sy) <= kViewCoordBound &&
                      __builtin_fabsf(ssx) <= kViewCoordBound && __builtin_fabsf(ssy) <= kViewCoordBound;
  ViewVertex o{0, 0, 0, 0, 0.0f, 0};
  if (usable) {
    o.X = __float2int_rn(sx), o.Y = __float2int_rn(sy), o.Xs = __float2int_rn(ssx), o.Ys = __float2int_rn(ssy);
    o.idepth = 1.0f / Dz;
    o.usable = 1;
  }
  return o;
}

__device__ __forceinline__ long long area2(int ax, int ay, int bx, int by, int cx, int cy) {
  return (long long)(bx - ax) * (long long)(cy - ay) - (long long)(by - ay) * (long long)(cx - ax);
}

// Rule 2.  What becomes of triangle t: kDraw, or why not.  *A: the doubled signed area in the target view.
enum { kDraw = 0, kInvalid = 1, kCulledVertex = 2, kCulledFacing = 3 };
__device__ __forceinline__ int classify(int t, const uint8_t* __restrict__ tri_valid, const ViewVertex& a, const ViewVertex& b, const ViewVertex& c,
                                        long long* A) {
  if (tri_valid && !tri_valid[t]) return kInvalid;
  if (!(a.usable && b.usable && c.usable)) return kCulledVertex;
  *A = area2(a.X, a.Y, b.X, b.Y, c.X, c.Y);
  const long long As = area2(a.Xs, a.Ys, b.Xs, b.Ys, c.Xs, c.Ys);
  if (*A == 0 || As == 0 || (*A > 0) != (As > 0)) return kCulledFacing;
  return kDraw;
}

// The pixel columns and rows whose centres (multiples of 16) lie in the triangle's bounding box, clipped to the image (>> floors).
struct ViewBox {
  int c0, r0;
  unsigned w, n;  // columns, pixels (0: none; rows, cols <= 32767: n < 2^30)
};
__device__ __forceinline__ ViewBox bounding_box(const ViewVertex& a, const ViewVertex& b, const ViewVertex& c, int rows, int cols) {
  const int c0 = max((min(a.X, min(b.X, c.X)) + 15) >> 4, 0), c1 = min(max(a.X, max(b.X, c.X)) >> 4, cols - 1);
  const int r0 = max((min(a.Y, min(b.Y, c.Y)) + 15) >> 4, 0), r1 = min(max(a.Y, max(b.Y, c.Y)) >> 4, rows - 1);
  ViewBox box{c0, r0, 0u, 0u};
  if (c1 >= c0 && r1 >= r0) box.w = (unsigned)(c1 - c0 + 1), box.n = box.w * (unsigned)(r1 - r0 + 1);
  return box;
}

// s * E(i, j) at pixel (col, row) = e0 + row * dy + col * dx.
struct ViewEdge {
  long long e0;
  int dx, dy;
};
__device__ __forceinline__ ViewEdge make_edge(int s, const ViewVertex& i, const ViewVertex& j) {
  const int ex = j.X - i.X, ey = j.Y - i.Y;  // (|.| <= 2^21; times 16: 2^25)
  ViewEdge e;
  e.e0 = (long long)s * ((long long)ey * (long long)i.X - (long long)ex * (long long)i.Y);
  e.dx = -s * 16 * ey, e.dy = s * 16 * ex;
  return e;
}
__device__ __forceinline__ long long edge_at(const ViewEdge& e, int col, int row) {
  return e.e0 + (long long)row * (long long)e.dy + (long long)col * (long long)e.dx;
}

// Rules 3 - 5 for the pixels first, first + stride, ... of the drawn triangle t's box, into the key image `keys` of rows x cols.
__device__ __forceinline__ void raster_pixels(int t, long long A, const ViewVertex& a, const ViewVertex& b, const ViewVertex& c, const ViewBox& box,
                                              unsigned first, unsigned stride, unsigned long long* __restrict__ keys, int cols) {
  const int s = A > 0 ? 1 : -1;
  const float norm = (float)(A > 0 ? A : -A);
  const ViewEdge ea = make_edge(s, b, c), eb = make_edge(s, c, a), ec = make_edge(s, a, b);
  const unsigned long long lo = (unsigned long long)(t + 1);
  for (unsigned i = first; i < box.n; i += stride) {
    const unsigned dr = i / box.w;
    const int row = box.r0 + (int)dr, col = box.c0 + (int)(i - dr * box.w);
    const long long wa = edge_at(ea, col, row), wb = edge_at(eb, col, row), wc = edge_at(ec, col, row);
    if ((wa | wb | wc) < 0) continue;  // (a sign bit set in any of the three)
    const float val = (a.idepth * (float)wa + (b.idepth * (float)wb + c.idepth * (float)wc)) / norm;
    if (val > 0.0f && val < __builtin_inff())
      atomicMax(&keys[(size_t)row * (size_t)cols + (size_t)col], ((unsigned long long)__float_as_uint(val) << 32) | lo);
  }
}

}  // namespace view_device
}  // namespace flame_hip
