// debug_kernels.hip -- the debug images of the reference, from what the pipeline leaves on the device:
//   drawInverseDepthMap                                  flame.cc:2699-2719
//   w1_map_ / w2_map_ + drawNormals, planeParamToNormal  flame.cc:497-506, 2643-2697
//   drawFeatures                                         flame.cc:2459-2510
//   utils::jet, utils::normalMap                         utils/visualization.h:119-167
// Every picture is a pure function of its pixel (or, for the features, a fill where the last writer wins), and every byte is
// meant to equal the reference's: the arithmetic is its scalar code with C++'s promotions as written there (float where it is
// float, double where a double literal or variable pulls the expression up), built with -ffp-contract=off like the rest of the
// library; division and square root are the correctly rounded ones, in both precisions.  tests/debug_ref.py restates the same.
//
// drawWireframe is wireframe_kernels.hip, the matches picture matches_kernels.hip, drawDetections detections_kernels.hip; the
// colour map and the pixel stores these files share are debug_pixel.hpp.
// Not here (include/flame_nltgv2.h says why): cv::putText (debug_draw_text_overlay is taken as false).  debug_draw_photo_error is
// map_error_kernels.hip.
//
// Streaming kernels: a thread owns four consecutive OUTPUT pixels, 12 bytes, and stores them as three dwords.
#include <hip/hip_runtime.h>

#include "debug_kernels.h"
#include "debug_pixel.hpp"

namespace flame_hip {
namespace {

// utils::normalMap, visualization.h:119-130: (blue, green, red), float arithmetic; `255 * (n + 1) / 2` is (255 * (n + 1)) / 2
__device__ __forceinline__ void normal_map(float nx, float ny, float nz, uint8_t c[3]) {
  c[2] = to_u8((255.0f * (nx + 1.0f)) / 2.0f);
  c[1] = to_u8((255.0f * (ny + 1.0f)) / 2.0f);
  c[0] = to_u8(127.0f * nz + 127.0f);
}

// planeParamToNormal (flame.cc:2643-2663) at u = (col, row), as written: K(0,0) and K(1,1) stand where one would expect the
// principal point.  The float subexpressions stay float; a, b, d and nx..nz are double; the normal is cast to float, normalised
// the way mesh_kernels.hip does it (a no-op unless the squared norm is > 0) and negated.  Returns whether normal(2) > 0.
__device__ __forceinline__ bool plane_normal(float k00, float k11, float ux, float uy, float idepth, float w1, float w2,
                                             float n[3]) {
  const float af = ((w1 * ux + w2 * uy) - w1 * k00) - w2 * k11;
  const double a = (double)af;
  const float bf = ((k00 * k00) * w1) * w1 + ((k11 * k11) * w2) * w2;
  const double e = (double)idepth - a;
  const double b = (double)bf + e * e;
  const double d = 1.0 / sqrt(b);
  float nx = (float)((double)(k00 * w1) * d);
  float ny = (float)((double)(k11 * w2) * d);
  float nz = (float)(e * d);
  const float z = (nx * nx + ny * ny) + nz * nz;
  if (z > 0.0f) {
    const float len = sqrtf(z);
    nx = nx / len, ny = ny / len, nz = nz / len;
  }
  n[0] = -nx, n[1] = -ny, n[2] = -nz;
  return n[2] > 0.0f;
}

__device__ __forceinline__ float edge_eval(int v0x, int v0y, int v1x, int v1y, int px, int py) {
  const float A = (float)(v1y - v0y);
  const float B = (float)(v0x - v1x);
  const float C = (float)(v1x * v0y - v0x * v1y);
  return (A * (float)px + B * (float)py) + C;
}

// One pixel per lane: the triangle that won the pixel (k_raster_triangles' key: index + 1 in the high word) and its three edge
// functions once more, with k_raster_triangles' expressions, for w1 and w2 instead of the inverse depth.
__global__ void __launch_bounds__(256)
k_debug_wmaps(long n, int cols, const unsigned long long* __restrict__ keys, const int32_t* __restrict__ tris,
              const float2* __restrict__ vtx, const float* __restrict__ w1v, const float* __restrict__ w2v,
              float* __restrict__ w1_map, float* __restrict__ w2_map) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned hi = (unsigned)(keys[i] >> 32);
  float o1 = __builtin_nanf(""), o2 = __builtin_nanf("");
  if (hi != 0u) {
    const long t = (long)hi - 1;
    const int a = tris[3 * t], b = tris[3 * t + 1], c = tris[3 * t + 2];
    const float2 f1 = vtx[c], f2 = vtx[b], f3 = vtx[a];
    const int p1x = __float2int_rn(f1.x), p1y = __float2int_rn(f1.y);
    const int p2x = __float2int_rn(f2.x), p2y = __float2int_rn(f2.y);
    const int p3x = __float2int_rn(f3.x), p3y = __float2int_rn(f3.y);
    const int x = (int)(i % cols), y = (int)(i / cols);
    const float e1 = edge_eval(p2x, p2y, p3x, p3y, x, y);
    const float e2 = edge_eval(p3x, p3y, p1x, p1y, x, y);
    const float e3 = edge_eval(p1x, p1y, p2x, p2y, x, y);
    const float norm = e1 + (e2 + e3);
    o1 = (w1v[c] * e1 + (w1v[b] * e2 + w1v[a] * e3)) / norm;
    o2 = (w2v[c] * e1 + (w2v[b] * e2 + w2v[a] * e3)) / norm;
  }
  w1_map[i] = o1, w2_map[i] = o2;
}

template <bool kIdepth, bool kNormals>
__global__ void __launch_bounds__(256)
k_debug_images(DebugImageArgs a, const float* __restrict__ idepthmap, const float* __restrict__ w1_map,
               const float* __restrict__ w2_map, uint8_t* __restrict__ idepth_img, uint8_t* __restrict__ normals_img) {
  const long n = (long)a.rows * a.cols;
  const long o0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * kPixelsPerThread;
  if (o0 >= n) return;
  uint32_t pi[4] = {0u, 0u, 0u, 0u}, pn[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < kPixelsPerThread; ++k) {
    const long o = o0 + k;
    if (o >= n) continue;
    const long i = a.flip ? n - 1 - o : o;  // the source pixel of output pixel o
    const int row = (int)(i / a.cols), col = (int)(i % a.cols);
    const uint8_t g = a.gray[(long)row * a.gray_step + col];  // cvtColor(GRAY2RGB): three equal bytes
    const float v = idepthmap[i];
    if (kIdepth) {
      uint8_t c[3] = {g, g, g};
      if (!(v != v)) jet02(v * a.scene_color_scale, c);
      pi[k] = pack3(c);
    }
    if (kNormals) {
      uint8_t c[3] = {g, g, g};
      float nrm[3];
      if (plane_normal(a.k00, a.k11, (float)col, (float)row, v, w1_map[i], w2_map[i], nrm)) normal_map(nrm[0], nrm[1], nrm[2], c);
      pn[k] = pack3(c);
    }
  }
  if (kIdepth) store_pixels(idepth_img, o0, n, pi);
  if (kNormals) store_pixels(normals_img, o0, n, pn);
}

// drawFeatures, pass 1: one lane per feature.  A feature with idepth_var < idepth_var_max_graph (strict; a NaN is not drawn)
// claims the pixels of [xi - 2, xi + 2] x [yi - 2, yi + 2], both corners inclusive, clipped to the image (cv::rectangle with
// thickness -1: restated, UNPINNED), xi = (int)(x + 0.5f), yi = (int)(y + 0.5f).  The sequential loop leaves the feature with
// the highest index on top: atomicMax of index + 1.
__global__ void __launch_bounds__(256)
k_draw_features_claim(int n, const char* __restrict__ feats, int stride, float var_max, int rows, int cols,
                      uint32_t* __restrict__ owner, int* __restrict__ counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool drawn = false;
  if (i < n) {
    const float* f = (const float*)(feats + (size_t)i * stride);
    const float x = f[0], y = f[1], var = f[3];
    drawn = var < var_max;
    if (drawn) {
      const long xi = (long)(int)(x + 0.5f), yi = (long)(int)(y + 0.5f);
      const long x0 = xi - 2 > 0 ? xi - 2 : 0, x1 = xi + 2 < cols - 1 ? xi + 2 : cols - 1;
      const long y0 = yi - 2 > 0 ? yi - 2 : 0, y1 = yi + 2 < rows - 1 ? yi + 2 : rows - 1;
      for (long yy = y0; yy <= y1; ++yy)
        for (long xx = x0; xx <= x1; ++xx) atomicMax(&owner[yy * cols + xx], (uint32_t)i + 1u);
    }
  }
  const int n_drawn = __popcll(__ballot(drawn)), n_rest = __popcll(__ballot(i < n && !drawn));
  if ((threadIdx.x & 63) == 0) {
    if (n_drawn) atomicAdd(&counts[0], n_drawn);
    if (n_rest) atomicAdd(&counts[1], n_rest);
  }
}

// ... pass 2: per output pixel, the grey value or its owner's jet(idepth_mu * scene_color_scale, 0, 2)
__global__ void __launch_bounds__(256)
k_draw_features_paint(DebugImageArgs a, const char* __restrict__ feats, int stride, const uint32_t* __restrict__ owner,
                      uint8_t* __restrict__ img) {
  const long n = (long)a.rows * a.cols;
  const long o0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * kPixelsPerThread;
  if (o0 >= n) return;
  uint32_t px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < kPixelsPerThread; ++k) {
    const long o = o0 + k;
    if (o >= n) continue;
    const long i = a.flip ? n - 1 - o : o;
    const int row = (int)(i / a.cols), col = (int)(i % a.cols);
    const uint8_t g = a.gray[(long)row * a.gray_step + col];
    uint8_t c[3] = {g, g, g};
    const uint32_t own = owner[i];
    if (own != 0u) {
      const float* f = (const float*)(feats + (size_t)(own - 1u) * stride);
      jet02(f[2] * a.scene_color_scale, c);
    }
    px[k] = pack3(c);
  }
  store_pixels(img, o0, n, px);
}

}  // namespace

int launch_debug_wmaps(const unsigned long long* keys, const int32_t* tris, const float2* vtx, const float* w1, const float* w2,
                       float* w1_map, float* w2_map, int rows, int cols, hipStream_t s) {
  const long n = (long)rows * cols;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_debug_wmaps, grid1d(n), dim3(256), 0, s, n, cols, keys, tris, vtx, w1, w2, w1_map, w2_map);
  return (int)hipGetLastError();
}

int launch_debug_images(const DebugImageArgs& a, const float* idepthmap, const float* w1_map, const float* w2_map,
                        uint8_t* idepth_img, uint8_t* normals_img, hipStream_t s) {
  const long n = (long)a.rows * a.cols;
  if (n <= 0 || (!idepth_img && !normals_img)) return 0;
  const dim3 grid = grid1d((n + kPixelsPerThread - 1) / kPixelsPerThread);
  if (idepth_img && normals_img)
    hipLaunchKernelGGL((k_debug_images<true, true>), grid, dim3(256), 0, s, a, idepthmap, w1_map, w2_map, idepth_img, normals_img);
  else if (idepth_img)
    hipLaunchKernelGGL((k_debug_images<true, false>), grid, dim3(256), 0, s, a, idepthmap, w1_map, w2_map, idepth_img, normals_img);
  else
    hipLaunchKernelGGL((k_debug_images<false, true>), grid, dim3(256), 0, s, a, idepthmap, w1_map, w2_map, idepth_img, normals_img);
  return (int)hipGetLastError();
}

int launch_draw_features(const DebugImageArgs& a, int n, const void* xy_mu_var, int stride_bytes, float idepth_var_max_graph,
                         uint32_t* owner, int* counts, uint8_t* img, hipStream_t s) {
  const long px = (long)a.rows * a.cols;
  if (px <= 0) return 0;
  (void)hipMemsetAsync(owner, 0, sizeof(uint32_t) * (size_t)px, s);
  (void)hipMemsetAsync(counts, 0, 2 * sizeof(int), s);
  if (n > 0)
    hipLaunchKernelGGL(k_draw_features_claim, grid1d(n), dim3(256), 0, s, n, (const char*)xy_mu_var, stride_bytes,
                       idepth_var_max_graph, a.rows, a.cols, owner, counts);
  hipLaunchKernelGGL(k_draw_features_paint, grid1d((px + kPixelsPerThread - 1) / kPixelsPerThread), dim3(256), 0, s, a,
                     (const char*)xy_mu_var, stride_bytes, owner, img);
  return (int)hipGetLastError();
}

}  // namespace flame_hip
