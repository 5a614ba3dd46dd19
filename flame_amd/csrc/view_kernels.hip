// view_kernels.hip -- the mesh rendered into another camera (include/flame_nltgv2.h, flame_nltgv2_render_view_begin, states every rule;
// tests/view_ref.py restates them in numpy float32 and Python integers and is the checker, bit for bit):
//   clear       the key image and the counters
//   vertices    one lane per vertex: back-projection with its inverse depth, R P + t, projection, 1/16-pixel snapping in both views,
//               1 / z' -- float32, every sum of three products left to right
//   triangles   one lane per triangle counts what rule 2 makes of it (one atomic per workgroup and counter); one wavefront per drawn
//               triangle walks its pixel bounding box clipped to the image -- but a triangle stretched across a depth edge can hold a
//               thousand times the pixels of its neighbours, and one wave walking it alone was the whole kernel's time
//               (profiles/render_view.txt): boxes of more than kViewWavePixels pixels are listed and shared by kViewBigWaves waves each.  The edge functions are affine in (col, row) with integer
//               coefficients: w = e0 + row * dy + col * dx in int64 is the rule's value exactly (|X|, |Y| <= 2^20: |w| < 2^44).  The
//               nearest surface wins through a 64-bit atomicMax on {bits(val), t + 1}: val > 0, so its bits order as the floats do
//   resolve     keys -> map, owner index, coverage (one atomic per workgroup: the lesson of k_raster_resolve)
// No floating-point atomics: the key image does not depend on scheduling.  Built with -ffp-contract=off (no FMA); division and the
// int64 -> float conversions are correctly rounded.
#include <hip/hip_runtime.h>

#include "view_kernels.h"

namespace flame_hip {
namespace {

constexpr int kPerThread = kViewResolveTile / 256;

__global__ void __launch_bounds__(256)
k_view_clear(long n, unsigned long long* __restrict__ keys, ViewCounts* __restrict__ counts, int* __restrict__ big) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *counts = ViewCounts{0, 0, 0, 0}, big[0] = 0;
  const long base = (long)blockIdx.x * kViewResolveTile + threadIdx.x;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const long i = base + (long)j * 256;
    if (i < n) keys[i] = 0ull;
  }
}

__device__ __forceinline__ float dot3(const float* m, float x, float y, float z) { return (m[0] * x + m[1] * y) + m[2] * z; }

__global__ void __launch_bounds__(256)
k_view_vertices(int V, const float2* __restrict__ pos, const float* __restrict__ values, float value_scale, ViewCamera cam,
                ViewVertex* __restrict__ out) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const float2 p = pos[v];
  const float id = values[v] * value_scale;
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
  out[v] = o;
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

// One lane per triangle: what rule 2 makes of it, counted with one atomic per workgroup and counter; a drawn triangle whose box holds
// more than kViewWavePixels pixels goes on the list big[1 ..], big[0] counting them (few: a triangle stretched across a depth edge).
__global__ void __launch_bounds__(256)
k_view_count(int T, const int32_t* __restrict__ tris, const uint8_t* __restrict__ tri_valid, const ViewVertex* __restrict__ vtx,
             ViewCounts* __restrict__ counts, int* __restrict__ big, int rows, int cols) {
  __shared__ int s_n[4];
  if (threadIdx.x < 4) s_n[threadIdx.x] = 0;
  __syncthreads();
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  int cls = kInvalid;
  if (t < T) {
    long long A = 0;
    const ViewVertex a = vtx[tris[3 * t]], b = vtx[tris[3 * t + 1]], c = vtx[tris[3 * t + 2]];
    cls = classify(t, tri_valid, a, b, c, &A);
    if (cls == kDraw && bounding_box(a, b, c, rows, cols).n > (unsigned)kViewWavePixels) big[1 + atomicAdd(&big[0], 1)] = t;
  }
  for (int k = kDraw; k <= kCulledFacing; ++k) {
    if (k == kInvalid) continue;
    const int n = __popcll(__ballot(cls == k));
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(&s_n[k], n);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_n[kDraw]) atomicAdd(&counts->tris_drawn, s_n[kDraw]);
    if (s_n[kCulledVertex]) atomicAdd(&counts->tris_culled_vertex, s_n[kCulledVertex]);
    if (s_n[kCulledFacing]) atomicAdd(&counts->tris_culled_facing, s_n[kCulledFacing]);
  }
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

// Rules 3 - 5 for the pixels first, first + stride, ... of the drawn triangle t's box.
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

// One wavefront per triangle whose box holds at most kViewWavePixels pixels: the others are k_view_raster_big's.
__global__ void __launch_bounds__(64)
k_view_raster(int T, const int32_t* __restrict__ tris, const uint8_t* __restrict__ tri_valid, const ViewVertex* __restrict__ vtx,
              unsigned long long* __restrict__ keys, int rows, int cols) {
  const int t = blockIdx.x;
  if (t >= T) return;
  const ViewVertex a = vtx[tris[3 * t]], b = vtx[tris[3 * t + 1]], c = vtx[tris[3 * t + 2]];
  long long A = 0;
  if (classify(t, tri_valid, a, b, c, &A) != kDraw) return;
  const ViewBox box = bounding_box(a, b, c, rows, cols);
  if (box.n > (unsigned)kViewWavePixels) return;
  raster_pixels(t, A, a, b, c, box, threadIdx.x, 64u, keys, cols);
}

// The listed triangles: kViewBigWaves wavefronts share one triangle's box (blockIdx.x: which of them), blockIdx.y walks the list.
__global__ void __launch_bounds__(64)
k_view_raster_big(const int32_t* __restrict__ tris, const ViewVertex* __restrict__ vtx, const int* __restrict__ big,
                  unsigned long long* __restrict__ keys, int rows, int cols) {
  const int n_big = big[0];
  for (int item = blockIdx.y; item < n_big; item += gridDim.y) {
    const int t = big[1 + item];
    const ViewVertex a = vtx[tris[3 * t]], b = vtx[tris[3 * t + 1]], c = vtx[tris[3 * t + 2]];
    long long A = 0;
    (void)classify(t, nullptr, a, b, c, &A);  // (listed: drawn)
    raster_pixels(t, A, a, b, c, bounding_box(a, b, c, rows, cols), blockIdx.x * 64u + threadIdx.x, 64u * kViewBigWaves, keys, cols);
  }
}

__global__ void __launch_bounds__(256)
k_view_resolve(long n, const unsigned long long* __restrict__ keys, float* __restrict__ map, int32_t* __restrict__ tri_index,
               ViewCounts* __restrict__ counts) {
  __shared__ int s_count;
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  int count = 0;
  const long base = (long)blockIdx.x * kViewResolveTile + threadIdx.x;
#pragma unroll
  for (int j = 0; j < kPerThread; ++j) {
    const long i = base + (long)j * 256;
    bool covered = false;
    if (i < n) {
      const unsigned long long k = keys[i];
      const int owner = (int)(unsigned)k;  // t + 1; 0: nobody
      covered = owner != 0;
      if (map) map[i] = covered ? __uint_as_float((unsigned)(k >> 32)) : __uint_as_float(0x7fc00000u);
      if (tri_index) tri_index[i] = owner - 1;
    }
    count += __popcll(__ballot(covered));
  }
  if ((threadIdx.x & 63) == 0 && count) atomicAdd(&s_count, count);
  __syncthreads();
  if (threadIdx.x == 0 && s_count) atomicAdd(&counts->coverage, s_count);
}

inline dim3 tiles(long n) { return dim3((unsigned)((n + kViewResolveTile - 1) / kViewResolveTile)); }

}  // namespace

int launch_view_clear(long n, unsigned long long* keys, ViewCounts* counts, int* big, hipStream_t s) {
  hipLaunchKernelGGL(k_view_clear, tiles(n > 0 ? n : 1), dim3(256), 0, s, n, keys, counts, big);
  return (int)hipGetLastError();
}

int launch_view_vertices(int V, const float2* pos, const float* values, float value_scale, const ViewCamera& cam, ViewVertex* out, hipStream_t s) {
  if (V <= 0) return 0;
  hipLaunchKernelGGL(k_view_vertices, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, s, V, pos, values, value_scale, cam, out);
  return (int)hipGetLastError();
}

int launch_view_raster(int T, const int32_t* tris, const uint8_t* tri_valid, const ViewVertex* vtx, unsigned long long* keys, ViewCounts* counts,
                       int* big, int rows, int cols, hipStream_t s) {
  if (T <= 0) return 0;
  hipLaunchKernelGGL(k_view_count, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, T, tris, tri_valid, vtx, counts, big, rows, cols);
  hipLaunchKernelGGL(k_view_raster, dim3((unsigned)T), dim3(64), 0, s, T, tris, tri_valid, vtx, keys, rows, cols);
  hipLaunchKernelGGL(k_view_raster_big, dim3(kViewBigWaves, kViewBigRows), dim3(64), 0, s, tris, vtx, big, keys, rows, cols);
  return (int)hipGetLastError();
}

int launch_view_resolve(long n, const unsigned long long* keys, float* map, int32_t* tri_index, ViewCounts* counts, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_view_resolve, tiles(n), dim3(256), 0, s, n, keys, map, tri_index, counts);
  return (int)hipGetLastError();
}

}  // namespace flame_hip
