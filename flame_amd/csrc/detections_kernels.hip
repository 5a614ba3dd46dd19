// detections_kernels.hip -- the detections debug image of the reference (getDebugImageDetections), from what
// flame_stereo_add_frame leaves on the device:
//   the score of detectFeatures' scan loop   flame.cc:1212-1251 (its `score`, written at :1249)
//   drawDetections                           flame.cc:2363-2412
//   utils::applyColorMap, utils::jet         utils/visualization.h:272-287, 142-167
// The picture is a pure function of its pixel: the score is recomputed from the two gradients with k_detect_cells' expressions
// (stereo_geometry.hpp's reference_epiline, (row, col) passed as (x, y)), so nothing is recorded at detection time and the
// detection launches what it always launched.  include/flame_stereo.h (flame_stereo_draw_detections) states the rule, the
// blend's rounding included (UNPINNED); tests/detections_ref.py restates it.  Built with -ffp-contract=off like the rest.
//
// A streaming kernel of k_debug_images' form: a thread owns four consecutive OUTPUT pixels, 12 bytes, and stores them as three
// dwords.  Consecutive lanes read consecutive groups of four floats of a gradient row; the padded pitch lets a thread's four
// pixels cross a row end, so row and column are formed per pixel.  The scored pixels are counted per wave (ballot + popcount)
// and added with one atomic per wave into one of kDetSlots copies of the counter (detections_kernels.h says why).
#include <hip/hip_runtime.h>

#include <climits>

#include "detections_kernels.h"
#include "debug_pixel.hpp"
#include "stereo_geometry.hpp"

namespace flame_hip {
namespace {

// `0.7 * debug_img + 0.3 * img_rgb` on 8-bit data (flame.cc:2388) as cv::addWeighted(A, 0.7, B, 0.3, 0): both weights cast to
// float, two rounded products, one rounded sum, then saturate_cast<uchar>: round to nearest, ties to even, clamped.  UNPINNED.
__device__ __forceinline__ uint8_t blend(uint8_t c, uint8_t g) {
  const float t = (float)c * 0.7f + (float)g * 0.3f;
  const int r = __float2int_rn(t);
  return (uint8_t)(r < 0 ? 0 : r > 255 ? 255 : r);
}

__global__ void __launch_bounds__(256)
k_draw_detections(const DebugImageArgs a, const DetectGrid scan, const Geo geo, const StereoCamera cam,
                  const float* __restrict__ gx_pad, const float* __restrict__ gy_pad, const float max_score,
                  int* __restrict__ stats, uint8_t* __restrict__ img) {
  const long n = (long)a.rows * a.cols;
  const long o0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * kPixelsPerThread;
  const int pw = cam.width + 2 * cam.border;
  uint32_t px[4] = {0u, 0u, 0u, 0u};
  int n_scored = 0;
#pragma unroll
  for (int k = 0; k < kPixelsPerThread; ++k) {
    const long o = o0 + k;
    bool scored = false;
    if (o < n) {
      const long i = a.flip ? n - 1 - o : o;  // the source pixel of output pixel o
      const int ii = (int)(i / a.cols), jj = (int)(i % a.cols);
      const uint8_t g = a.gray[(long)ii * a.gray_step + jj];  // cvtColor(GRAY2RGB): three equal bytes
      uint8_t c[3] = {0, 0, 0};                               // debug_img->setTo(0): what an unscored pixel keeps
      if (ii >= scan.r_lo && ii < scan.r_hi && jj >= scan.c_lo && jj < scan.c_hi) {
        const size_t at = (size_t)(ii + cam.border) * pw + (jj + cam.border);
        const float gx = gx_pad[at], gy = gy_pad[at];
        const float gmag2 = gx * gx + gy * gy;
        if (!(gmag2 < scan.g2)) {
          V2 epi;
          if (!reference_epiline(geo, cam, V2{(float)ii, (float)jj}, &epi)) {  // (row, col) as (x, y), as flame.cc:1228
            atomicMax(&stats[kDetAssert], INT_MAX - (ii * cam.width + jj));
          } else {
            const float epigrad = gx * epi.x + gy * epi.y;
            const float epigrad2 = epigrad * epigrad;
            const float score = fabsf(epigrad);
            if (!(epigrad2 < scan.g2) && !(score != score)) {  // a NaN score is an unscored pixel (applyColorMap's isnan)
              scored = true;
              jet(score, 0.0f, max_score, c);
            }
          }
        }
      }
      c[0] = blend(c[0], g), c[1] = blend(c[1], g), c[2] = blend(c[2], g);
      px[k] = pack3(c);
    }
    n_scored += __popcll(__ballot(scored));  // (every lane of the wave is here: nothing returned early)
  }
  if (o0 < n) store_pixels(img, o0, n, px);
  if ((threadIdx.x & 63) == 0 && n_scored) atomicAdd(&stats[kDetCount + (blockIdx.x % kDetSlots) * kDetSlotStride], n_scored);
}

}  // namespace

int launch_draw_detections(const DebugImageArgs& a, const DetectGrid& scan, const Geo& geo, const StereoCamera& cam,
                           const float* gx_pad, const float* gy_pad, float max_score, int* stats, uint8_t* img, hipStream_t s) {
  const long n = (long)a.rows * a.cols;
  (void)hipMemsetAsync(stats, 0, kDetWords * sizeof(int), s);
  if (n <= 0) return (int)hipGetLastError();
  hipLaunchKernelGGL(k_draw_detections, grid1d((n + kPixelsPerThread - 1) / kPixelsPerThread), dim3(256), 0, s, a, scan, geo, cam,
                     gx_pad, gy_pad, max_score, stats, img);
  return (int)hipGetLastError();
}

}  // namespace flame_hip
