// align_kernels.hip -- the pyramid levels of a resident frame and the Gauss-Newton system of a direct image alignment
// (include/flame_stereo.h, flame_stereo_build_pyramid / flame_stereo_align_linearize, states every rule; tests/align_ref.py restates them
// in numpy and is the checker, bit for bit):
//   pyrDown       out(y, x) = (sum_{i,j} k_i k_j src(r(2y + i), r(2x + j)) + 128) >> 8, k = 1 4 6 4 1, r = BORDER_REFLECT_101 repeated; in
//                 integers.  A workgroup makes a tile of 32 x 8 outputs and the ring of outputs around it from a source tile staged in LDS,
//                 then the level's central gradients from those outputs: image and both gradients in one pass
//   linearisation one lane per level pixel; the warp, the bilinear taps, the residual, the 1 x 6 Jacobian and the Huber weight in float32
//                 (one rounding per operation: -ffp-contract=off), the 28 products in double; every 1024 consecutive pixels pairwise
//                 (pairwise_sum.hpp), 7 sums per round through 56 KB of LDS, then the chunk partials as flame_nltgv2_map_error's `sum` adds
//                 them.  The counts by ballot and popcount per wave, one integer atomic per workgroup and count.  No floating-point
//                 atomics: the result does not depend on the launch geometry
#include <hip/hip_runtime.h>

#include "align_kernels.h"

namespace flame_hip {
namespace {

constexpr int kPyrTileW = 32, kPyrTileH = 8;                                    // outputs per workgroup (256 threads)
constexpr int kPyrOutW = kPyrTileW + 2, kPyrOutH = kPyrTileH + 2;               // with the ring the gradients read
constexpr int kPyrSrcW = 2 * kPyrOutW + 3, kPyrSrcH = 2 * kPyrOutH + 3;         // 71 x 23 source pixels

// cv::borderInterpolate(BORDER_REFLECT_101), repeated until inside: the closed form (even, period 2 (len - 1)); len >= 2.
__device__ __forceinline__ int reflect_101(int p, int len) {
  if ((unsigned)p < (unsigned)len) return p;
  const int period = 2 * (len - 1);
  const int m = (p < 0 ? -p : p) % period;
  return m < len ? m : period - m;
}

__global__ void __launch_bounds__(256)
k_pyr_down(const uint8_t* __restrict__ src, int sw, int sh, int src_pitch, int dw, int dh, uint8_t* __restrict__ dst,
           float* __restrict__ gx, float* __restrict__ gy) {
  __shared__ uint8_t s_src[kPyrSrcH * kPyrSrcW];
  __shared__ int s_out[kPyrOutH * kPyrOutW];
  const int t = threadIdx.x;
  const int ox0 = blockIdx.x * kPyrTileW - 1, oy0 = blockIdx.y * kPyrTileH - 1;  // output coordinates of s_out[0]
  const int sx0 = 2 * ox0 - 2, sy0 = 2 * oy0 - 2;                                // source coordinates of s_src[0]
  for (int idx = t; idx < kPyrSrcH * kPyrSrcW; idx += 256) {
    const int r = idx / kPyrSrcW, c = idx - r * kPyrSrcW;
    s_src[idx] = src[(size_t)reflect_101(sy0 + r, sh) * src_pitch + reflect_101(sx0 + c, sw)];
  }
  __syncthreads();
  for (int idx = t; idx < kPyrOutH * kPyrOutW; idx += 256) {
    const int r = idx / kPyrOutW, c = idx - r * kPyrOutW;
    const uint8_t* p = s_src + (2 * r) * kPyrSrcW + 2 * c;  // the window's corner: source (2 y - 2, 2 x - 2)
    int sum = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int ki = i == 0 || i == 4 ? 1 : (i == 2 ? 6 : 4);
      const uint8_t* q = p + i * kPyrSrcW;
      sum += ki * ((q[0] + q[4]) + 4 * (q[1] + q[3]) + 6 * q[2]);
    }
    s_out[idx] = (sum + 128) >> 8;
  }
  __syncthreads();
  const int r = t / kPyrTileW + 1, c = t % kPyrTileW + 1;
  const int x = ox0 + c, y = oy0 + r;
  if (x >= dw || y >= dh) return;
  const int* o = s_out + r * kPyrOutW + c;
  const float v = (float)o[0];
  float vx, vy;  // getCentralGradient: central inside, forward / backward in the first / last column and row
  if (x == 0) vx = (float)o[1] - v;
  else if (x == dw - 1) vx = v - (float)o[-1];
  else vx = 0.5f * ((float)o[1] - (float)o[-1]);
  if (y == 0) vy = (float)o[kPyrOutW] - v;
  else if (y == dh - 1) vy = v - (float)o[-kPyrOutW];
  else vy = 0.5f * ((float)o[kPyrOutW] - (float)o[-kPyrOutW]);
  const size_t i = (size_t)y * dw + x;
  dst[i] = (uint8_t)o[0];
  gx[i] = vx;
  gy[i] = vy;
}

__device__ __forceinline__ float bilinear_u8(const uint8_t* p, int pitch, float w00, float w01, float w10, float w11) {
  const float g00 = (float)p[0], g01 = (float)p[1], g10 = (float)p[pitch], g11 = (float)p[pitch + 1];
  return ((w00 * g00 + w01 * g01) + w10 * g10) + w11 * g11;
}
__device__ __forceinline__ float bilinear_f32(const float* p, int pitch, float w00, float w01, float w10, float w11) {
  const float g00 = p[0], g01 = p[1], g10 = p[pitch], g11 = p[pitch + 1];
  return ((w00 * g00 + w01 * g01) + w10 * g10) + w11 * g11;
}

// (i, j) of the s-th sum of H: the upper triangle, row-major.
__host__ __device__ constexpr int h_row(int s) { return s < 6 ? 0 : s < 11 ? 1 : s < 15 ? 2 : s < 18 ? 3 : s < 20 ? 4 : 5; }
__host__ __device__ constexpr int h_col(int s) { return h_row(s) + (s - (h_row(s) * 6 - h_row(s) * (h_row(s) - 1) / 2)); }

enum { kClassNone = 0, kClassUsed = 1, kClassNoDepth = 2, kClassBehind = 3, kClassOutside = 4 };

// Workgroup g takes the chunks [g * per_group, (g + 1) * per_group): partials[q * chunks + c] is a function of chunk c alone.  out->counts
// must be zero before the launch.
__global__ void __launch_bounds__(kPairwiseChunk)
k_align_linearize(AlignArgs a, int chunks, int per_group, double* __restrict__ partials, AlignSystem* __restrict__ out) {
  __shared__ double p[kAlignGroupSums * kPairwiseChunk];
  __shared__ int s_cnt[kAlignCounts];
  const int t = threadIdx.x;
  if (t < kAlignCounts) s_cnt[t] = 0;
  __syncthreads();
  const int w = a.ref.w, h = a.ref.h;
  const long n = (long)w * h;
  const float fb = (float)a.border;
  const float umax = (float)(w - 1 - a.border), vmax = (float)(h - 1 - a.border);
  const int c0 = blockIdx.x * per_group;
  const int c1 = c0 + per_group < chunks ? c0 + per_group : chunks;
  for (int c = c0; c < c1; ++c) {
    const long i = (long)c * kPairwiseChunk + t;
    int cls = kClassNone;
    bool huber = false;
    float wgt = 0.0f, r = 0.0f, J[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (i < n) {
      const int y = (int)((uint32_t)i / (uint32_t)w), x = (int)i - y * w;  // (w * h < 2^31: the planes exist)
      if (x >= a.border && x < w - a.border && y >= a.border && y < h - a.border) {
        const float d = a.map[((size_t)y << a.shift) * a.map_w + ((size_t)x << a.shift)];
        if (!(d == d && d > 0.0f && d < __builtin_inff())) {
          cls = kClassNoDepth;
        } else {
          const float pa = ((float)x - a.cx) / a.fx, pb = ((float)y - a.cy) / a.fy;
          const float Xx = ((a.R[0] * pa + a.R[1] * pb) + a.R[2]) + a.t[0] * d;
          const float Xy = ((a.R[3] * pa + a.R[4] * pb) + a.R[5]) + a.t[1] * d;
          const float Xz = ((a.R[6] * pa + a.R[7] * pb) + a.R[8]) + a.t[2] * d;
          if (!(Xz > 0.0f)) {
            cls = kClassBehind;
          } else {
            const float xn = Xx / Xz, yn = Xy / Xz, rho = d / Xz;
            const float u = a.fx * xn + a.cx, v = a.fy * yn + a.cy;
            // decided on the floats, before any conversion to an integer and before any address is formed; a NaN fails it
            if (!(u >= fb && v >= fb && u < umax && v < vmax)) {
              cls = kClassOutside;
            } else {
              cls = kClassUsed;
              const int x0 = (int)u, y0 = (int)v;  // border >= 1: 1 <= x0 <= w - 3, the four taps lie inside the level
              const float dx = u - (float)x0, dy = v - (float)y0;
              const float w11 = dx * dy, w01 = dx - w11, w10 = dy - w11, w00 = ((1.0f - dx) - dy) + w11;
              const size_t o = (size_t)y0 * a.cur.pitch + x0;
              const float inew = bilinear_u8(a.cur.img + o, a.cur.pitch, w00, w01, w10, w11);
              const float gx = bilinear_f32(a.cur.gx + o, a.cur.pitch, w00, w01, w10, w11);
              const float gy = bilinear_f32(a.cur.gy + o, a.cur.pitch, w00, w01, w10, w11);
              r = inew - (float)a.ref.img[(size_t)y * a.ref.pitch + x];
              const float Gx = a.fx * gx, Gy = a.fy * gy, xy = xn * yn;
              J[0] = Gx * rho;
              J[1] = Gy * rho;
              J[2] = -((Gx * xn + Gy * yn) * rho);
              J[3] = -(Gx * xy + Gy * (1.0f + yn * yn));
              J[4] = Gx * (1.0f + xn * xn) + Gy * xy;
              J[5] = Gy * xn - Gx * yn;
              const float ar = __builtin_fabsf(r);
              huber = !(ar <= a.huber_k);
              wgt = huber ? a.huber_k / ar : 1.0f;
            }
          }
        }
      }
    }
    // counts: one add per wave and class into LDS
#pragma unroll
    for (int k = 1; k <= 4; ++k) {
      const unsigned long long m = __ballot(cls == k);
      if (m != 0ull && (t & 63) == 0) atomicAdd(&s_cnt[k - 1], __popcll(m));
    }
    {
      const unsigned long long m = __ballot(huber);
      if (m != 0ull && (t & 63) == 0) atomicAdd(&s_cnt[4], __popcll(m));
    }
    // the 28 terms, ((double)wgt * (double)J_i) * (double)J_j and so on; +0.0 from a pixel that contributes nothing
    double wj[7];
#pragma unroll
    for (int k = 0; k < 6; ++k) wj[k] = (double)wgt * (double)J[k];
    wj[6] = (double)wgt * (double)r;
    const bool used = cls == kClassUsed;
    double sums[kAlignGroupSums];
    // round 0: H00..H05, H11 | 1: H12..H15, H22..H24 | 2: H25, H33..H35, H44, H45, H55 | 3: b0..b5, cost
    int q = 0;
#pragma unroll
    for (int round = 0; round < 4; ++round) {
#pragma unroll
      for (int k = 0; k < kAlignGroupSums; ++k) {
        const int s = round * kAlignGroupSums + k;  // index among the 28
        double term;
        if (s < 21) {
          term = wj[h_row(s)] * (double)J[h_col(s)];
        } else if (s < 27) {
          term = wj[s - 21] * (double)r;
        } else {
          term = wj[6] * (double)r;
        }
        p[k * kPairwiseChunk + t] = used ? term : 0.0;
      }
      pairwise_sum_n<kAlignGroupSums>(p, t, sums);
      if (t == 0) {
#pragma unroll
        for (int k = 0; k < kAlignGroupSums; ++k) partials[(size_t)(q + k) * chunks + c] = sums[k];
      }
      q += kAlignGroupSums;
    }
  }
  __syncthreads();
  if (t < kAlignCounts && s_cnt[t] != 0) atomicAdd(&out->counts[t], s_cnt[t]);
}

// One workgroup: each sum's partials as k_map_error_finish adds them (thread t: t, t + 1024, ... in turn from +0.0; then pairwise).
__global__ void __launch_bounds__(kPairwiseChunk)
k_align_finish(int chunks, const double* __restrict__ partials, AlignSystem* __restrict__ out) {
  __shared__ double p[kAlignGroupSums * kPairwiseChunk];
  const int t = threadIdx.x;
  double sums[kAlignGroupSums];
  for (int q = 0; q < kAlignSums; q += kAlignGroupSums) {
#pragma unroll
    for (int k = 0; k < kAlignGroupSums; ++k) {
      const double* b = partials + (size_t)(q + k) * chunks;
      double sum = 0.0;
      for (int i = t; i < chunks; i += kPairwiseChunk) sum += b[i];
      p[k * kPairwiseChunk + t] = sum;
    }
    pairwise_sum_n<kAlignGroupSums>(p, t, sums);
    if (t == 0) {
#pragma unroll
      for (int k = 0; k < kAlignGroupSums; ++k) out->sums[q + k] = sums[k];
    }
  }
}

}  // namespace

int launch_pyr_down(const uint8_t* src, int sw, int sh, int src_pitch, uint8_t* dst, float* gx, float* gy, hipStream_t s) {
  if (sw < 2 || sh < 2) return (int)hipErrorInvalidValue;
  const int dw = (sw + 1) / 2, dh = (sh + 1) / 2;
  const dim3 grid((unsigned)((dw + kPyrTileW - 1) / kPyrTileW), (unsigned)((dh + kPyrTileH - 1) / kPyrTileH));
  hipLaunchKernelGGL(k_pyr_down, grid, dim3(256), 0, s, src, sw, sh, src_pitch, dw, dh, dst, gx, gy);
  return (int)hipGetLastError();
}

int launch_align_linearize(const AlignArgs& a, double* partials, AlignSystem* out, hipStream_t s) {
  const long n = (long)a.ref.w * a.ref.h;
  if (n <= 0) return (int)hipErrorInvalidValue;
  const int chunks = (int)align_chunks(n);
  const int per_group = (chunks + kAlignMaxGroups - 1) / kAlignMaxGroups;
  const int groups = (chunks + per_group - 1) / per_group;
  hipError_t e = hipMemsetAsync(out, 0, sizeof(AlignSystem), s);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(k_align_linearize, dim3((unsigned)groups), dim3(kPairwiseChunk), 0, s, a, chunks, per_group, partials, out);
  hipLaunchKernelGGL(k_align_finish, dim3(1), dim3(kPairwiseChunk), 0, s, chunks, partials, out);
  return (int)hipGetLastError();
}

}  // namespace flame_hip
