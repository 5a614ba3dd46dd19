// map_error_kernels.hip -- the error of a dense inverse-depth map (include/flame_nltgv2.h, flame_nltgv2_map_error_begin, states every
// rule; tests/map_error_ref.py restates them in numpy float32 and is the checker, bit for bit):
//   error image   PHOTO: photo_residual_at (nltgv2_device.hpp, unchanged) at every pixel (col, row) with the map's value there;
//                 TRUTH: |v - t| or |v - t| / t where !(v != v) && t > 0; NaN where no error is defined
//   box mean      sum / (float)count over the non-NaN errors of the window; the sum separably in float32: per row left to right from
//                 +0.0f, then those row sums top to bottom from +0.0f.  One workgroup makes a tile of 64 x 16 outputs from the errors
//                 around it in LDS; its halo rows' sums are taken the same way, so the tiling does not show
//   statistics    a 256-bin histogram, privatised per workgroup in LDS (a wave whose lanes all hit one bin adds once) and merged with
//                 one integer atomic per non-zero bin; the sum in double: every 1024 consecutive pixels pairwise, p[t] += p[t + s] for
//                 s = 512 .. 1, then the partials as k_block_sum (nltgv2_kernels.hip) adds them.  No floating-point atomics: the
//                 result does not depend on the launch geometry
//   picture       grey, or jet(err, 0, max_error) (debug_pixel.hpp) where the error is not NaN
// Built with -ffp-contract=off (no FMA); division and the conversions are correctly rounded.
#include <hip/hip_runtime.h>

#include "debug_pixel.hpp"
#include "map_error_kernels.h"
#include "nltgv2_device.hpp"
#include "pairwise_sum.hpp"

namespace flame_hip {
namespace {

constexpr int kHistGroups = 256;  // workgroups of the histogram pass at most (one per CU): each takes consecutive chunks

// (rows * cols < 2^31, flame_nltgv2_map_error_begin: 32-bit divisions)
__global__ void __launch_bounds__(256)
k_map_error_photo(int rows, int cols, MapErrorPhoto p, const float* __restrict__ map, float* __restrict__ err) {
  const long n = (long)rows * cols;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t row = (uint32_t)i / (uint32_t)cols, col = (uint32_t)i - row * (uint32_t)cols;
  err[i] = photo_residual_at(make_float2((float)col, (float)row), map[i], p.geo, p.ref, p.cmp, rows, cols, p.step, p.border);
}

__global__ void __launch_bounds__(256)
k_map_error_truth(long n, const float* __restrict__ map, const float* __restrict__ truth, int relative, float* __restrict__ err) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v = map[i], t = truth[i];
  float e = __builtin_nanf("");
  if (!(v != v) && t > 0.0f) {
    e = __builtin_fabsf(v - t);
    if (relative) e = e / t;
    if (e != e) e = __builtin_nanf("");  // (inf - inf, inf / inf: a hole like any other, with the bits of one)
  }
  err[i] = e;
}

// Dynamic LDS: [H][W] errors (NaN outside the image) | [H][kMapErrorTileW] row sums | [H][kMapErrorTileW] row counts, with
// H = kMapErrorTileH + 2h, W = kMapErrorTileW + 2h.
__global__ void __launch_bounds__(256)
k_map_error_box(int rows, int cols, int h, const float* __restrict__ err, float* __restrict__ out) {
  extern __shared__ float lds[];
  const int W = kMapErrorTileW + 2 * h, H = kMapErrorTileH + 2 * h;
  float* s_val = lds;
  float* s_sum = s_val + H * W;
  int* s_cnt = (int*)(s_sum + H * kMapErrorTileW);
  const int row0 = blockIdx.y * kMapErrorTileH, col0 = blockIdx.x * kMapErrorTileW;
  const int t = threadIdx.x;
  for (int idx = t; idx < H * W; idx += 256) {
    const int r = idx / W, c = idx - r * W;
    const int gr = row0 - h + r, gc = col0 - h + c;
    float v = __builtin_nanf("");
    if (gr >= 0 && gr < rows && gc >= 0 && gc < cols) v = err[(long)gr * cols + gc];
    s_val[idx] = v;
  }
  __syncthreads();
  for (int idx = t; idx < H * kMapErrorTileW; idx += 256) {
    const int r = idx / kMapErrorTileW, c = idx % kMapErrorTileW;
    float sum = 0.0f;
    int cnt = 0;
    for (int k = 0; k <= 2 * h; ++k) {
      const float v = s_val[r * W + c + k];
      if (!(v != v)) sum += v, ++cnt;
    }
    s_sum[idx] = sum, s_cnt[idx] = cnt;
  }
  __syncthreads();
  for (int idx = t; idx < kMapErrorTileH * kMapErrorTileW; idx += 256) {
    const int r = idx / kMapErrorTileW, c = idx % kMapErrorTileW;
    const int gr = row0 + r, gc = col0 + c;
    if (gr >= rows || gc >= cols) continue;
    const float own = s_val[(r + h) * W + c + h];
    float o = own;
    if (!(own != own)) {
      float sum = 0.0f;
      int cnt = 0;
      for (int k = 0; k <= 2 * h; ++k) sum += s_sum[(r + k) * kMapErrorTileW + c], cnt += s_cnt[(r + k) * kMapErrorTileW + c];
      o = sum / (float)cnt;  // (cnt >= 1: the pixel itself)
    }
    out[(long)gr * cols + gc] = o;
  }
}

// Workgroup b takes the chunks [b * per_group, (b + 1) * per_group): partials[c] is a function of chunk c alone, the histogram is
// integers.  hist must be zero before the launch.
__global__ void __launch_bounds__(kMapErrorChunk)
k_map_error_hist(long n, int chunks, int per_group, const float* __restrict__ err, float scale, double* __restrict__ partials,
                 int32_t* __restrict__ hist) {
  __shared__ double p[kMapErrorChunk];
  __shared__ int s_hist[kMapErrorBins];
  const int t = threadIdx.x;
  if (t < kMapErrorBins) s_hist[t] = 0;
  __syncthreads();
  const int c0 = blockIdx.x * per_group;
  const int c1 = c0 + per_group < chunks ? c0 + per_group : chunks;
  for (int c = c0; c < c1; ++c) {
    const long i = (long)c * kMapErrorChunk + t;
    float e = __builtin_nanf("");
    if (i < n) e = err[i];
    const bool valid = !(e != e);
    int bin = 0;
    if (valid) {
      const float sc = e * scale;
      bin = sc >= 255.0f ? 255 : (int)(sc + 0.5f);  // (the clamp first: +inf is never converted; an error is never below -0)
    }
    const unsigned long long vm = __ballot(valid);
    if (vm != 0ull) {  // (uniform over the wave)
      const int first = __ffsll((long long)vm) - 1;
      const int lead = __shfl(bin, first);
      if (__ballot(valid && bin == lead) == vm) {  // one bin for the whole wave: one add, not 64 queueing on a word
        if ((t & 63) == first) atomicAdd(&s_hist[lead], __popcll(vm));
      } else if (valid) {
        atomicAdd(&s_hist[bin], 1);
      }
    }
    p[t] = valid ? (double)e : 0.0;
    const double sum = pairwise_sum(p, t);
    if (t == 0) partials[c] = sum;
  }
  __syncthreads();
  if (t < kMapErrorBins && s_hist[t] != 0) atomicAdd(&hist[t], s_hist[t]);
}

// One workgroup: the partials as k_block_sum adds them (thread t: t, t + 1024, ... in turn; then pairwise), the ranks, the mean.  The
// ranks: an inclusive scan of the 256 bins in LDS; cum is monotone, so each rule holds from one bin on and the lane of that bin alone
// sees it begin.
__global__ void __launch_bounds__(kMapErrorChunk)
k_map_error_finish(int chunks, const double* __restrict__ partials, int ptile_num, int ptile_den, MapErrorStats* __restrict__ st) {
  __shared__ double p[kMapErrorChunk];
  __shared__ long long cum[kMapErrorBins];
  const int t = threadIdx.x;
  double sum = 0.0;
  for (int i = t; i < chunks; i += kMapErrorChunk) sum += partials[i];
  p[t] = sum;
  if (t < kMapErrorBins) cum[t] = st->hist[t];
  sum = pairwise_sum(p, t);  // (its first barrier also publishes cum)
  for (int d = 1; d < kMapErrorBins; d <<= 1) {
    const long long add = (t < kMapErrorBins && t >= d) ? cum[t - d] : 0;
    __syncthreads();
    if (t < kMapErrorBins) cum[t] += add;
    __syncthreads();
  }
  const long long nv = cum[kMapErrorBins - 1];
  if (t < kMapErrorBins && nv > 0) {
    const long long here = cum[t], before = t > 0 ? cum[t - 1] : 0;
    if (2 * here > nv && !(t > 0 && 2 * before > nv)) st->median_bin = t;
    const long long den = ptile_den, num = ptile_num;
    if (den * here > num * nv && !(t > 0 && den * before > num * nv)) st->ptile_bin = t;
  }
  if (t != 0) return;
  if (nv == 0) st->median_bin = -1;
  if (nv == 0 || !((long long)ptile_den * nv > (long long)ptile_num * nv)) st->ptile_bin = -1;  // (no bin: none at all, or ptile_num == ptile_den)
  st->n_valid = (int32_t)nv;
  st->sum = sum;
  st->mean = nv > 0 ? (float)(sum / (double)nv) : 0.0f;
}

__global__ void __launch_bounds__(256)
k_map_error_picture(int rows, int cols, const uint8_t* __restrict__ gray, int gray_step, const float* __restrict__ err, float max_error,
                    int flip, uint8_t* __restrict__ img) {
  const long n = (long)rows * cols;
  const long o0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * kPixelsPerThread;
  if (o0 >= n) return;
  uint32_t px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < kPixelsPerThread; ++k) {
    const long o = o0 + k;
    if (o >= n) continue;
    const long i = flip ? n - 1 - o : o;  // the source pixel of output pixel o
    const int row = (int)(i / cols), col = (int)(i % cols);
    const uint8_t g = gray[(long)row * gray_step + col];
    uint8_t c[3] = {g, g, g};
    const float e = err[i];
    if (!(e != e)) jet(e, 0.0f, max_error, c);
    px[k] = pack3(c);
  }
  store_pixels(img, o0, n, px);
}

}  // namespace

int launch_map_error_photo(int rows, int cols, const MapErrorPhoto& p, const float* map, float* err, hipStream_t s) {
  const long n = (long)rows * cols;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_map_error_photo, grid1d(n), dim3(256), 0, s, rows, cols, p, map, err);
  return (int)hipGetLastError();
}

int launch_map_error_truth(int rows, int cols, const float* map, const float* truth, int relative, float* err, hipStream_t s) {
  const long n = (long)rows * cols;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_map_error_truth, grid1d(n), dim3(256), 0, s, n, map, truth, relative, err);
  return (int)hipGetLastError();
}

int launch_map_error_box(int rows, int cols, int win, const float* err, float* out, hipStream_t s) {
  if (rows <= 0 || cols <= 0) return 0;
  if (win < 3 || win > kMapErrorMaxWin || win % 2 == 0) return (int)hipErrorInvalidValue;
  const int h = win / 2;
  const int W = kMapErrorTileW + 2 * h, H = kMapErrorTileH + 2 * h;
  const size_t lds = sizeof(float) * ((size_t)H * W + 2 * (size_t)H * kMapErrorTileW);  // (h = 15: 41 KB of the 64 a workgroup may have)
  const dim3 grid((unsigned)((cols + kMapErrorTileW - 1) / kMapErrorTileW), (unsigned)((rows + kMapErrorTileH - 1) / kMapErrorTileH));
  hipLaunchKernelGGL(k_map_error_box, grid, dim3(256), lds, s, rows, cols, h, err, out);
  return (int)hipGetLastError();
}

int launch_map_error_stats(long n, const float* err, float hist_scale, int ptile_num, int ptile_den, double* partials, MapErrorStats* stats,
                           hipStream_t s) {
  if (n <= 0) return 0;
  const int chunks = (int)map_error_chunks(n);
  const int per_group = (chunks + kHistGroups - 1) / kHistGroups;
  const int groups = (chunks + per_group - 1) / per_group;
  hipError_t e = hipMemsetAsync(stats, 0, sizeof(MapErrorStats), s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_map_error_hist, dim3((unsigned)groups), dim3(kMapErrorChunk), 0, s, n, chunks, per_group, err, hist_scale, partials,
                     (int32_t*)stats);  // (hist is the struct's first member)
  hipLaunchKernelGGL(k_map_error_finish, dim3(1), dim3(kMapErrorChunk), 0, s, chunks, partials, ptile_num, ptile_den, stats);
  return (int)hipGetLastError();
}

int launch_map_error_picture(int rows, int cols, const uint8_t* gray, int gray_step, const float* err, float max_error, int flip, uint8_t* img,
                             hipStream_t s) {
  const long n = (long)rows * cols;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_map_error_picture, grid1d((n + kPixelsPerThread - 1) / kPixelsPerThread), dim3(256), 0, s, rows, cols, gray, gray_step, err,
                     max_error, flip, img);
  return (int)hipGetLastError();
}

}  // namespace flame_hip
