// map_error_kernels.h -- launch wrappers of map_error_kernels.hip: how good a dense inverse-depth map is -- the per-pixel photometric
// error against another frame, or the error against a true map, its NaN-aware box mean, a 256-bin histogram with two ranks, the sum and
// the mean, and a picture (include/flame_nltgv2.h, flame_nltgv2_map_error_begin, states every rule).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nltgv2_kernels.h"
#include "pairwise_sum.hpp"

namespace flame_hip {

constexpr int kMapErrorBins = 256;
constexpr int kMapErrorChunk = kPairwiseChunk;  // 1024 consecutive linear pixel indices per partial of the sum: part of the sum's definition
constexpr int kMapErrorMaxWin = 31;   // the widest box the tile's LDS holds
constexpr int kMapErrorTileW = 64, kMapErrorTileH = 16;  // output pixels per workgroup of the box mean

// == flame_nltgv2_map_error_stats, as the kernels leave it on the device.
struct MapErrorStats {
  int32_t hist[kMapErrorBins];
  int32_t n_valid, median_bin, ptile_bin;
  float mean;
  double sum;
};

inline long map_error_chunks(long n) { return (n + kMapErrorChunk - 1) / kMapErrorChunk; }

struct MapErrorPhoto {
  PhotoGeometry geo;
  const uint8_t* ref;
  const uint8_t* cmp;
  int step, border;
};

// err[row * cols + col] = photo_residual_at((col, row), map[..], ...): one lane per pixel.
int launch_map_error_photo(int rows, int cols, const MapErrorPhoto& p, const float* map, float* err, hipStream_t s);
// err = |v - t| (relative: / t) where !(v != v) && t > 0, NaN elsewhere.
int launch_map_error_truth(int rows, int cols, const float* map, const float* truth, int relative, float* err, hipStream_t s);
// The box mean of win x win (odd, 3 .. kMapErrorMaxWin) over the non-NaN errors; out != err.
int launch_map_error_box(int rows, int cols, int win, const float* err, float* out, hipStream_t s);
// Histogram, ranks, sum and mean of the n errors into *stats; partials: [map_error_chunks(n)] doubles of scratch.
int launch_map_error_stats(long n, const float* err, float hist_scale, int ptile_num, int ptile_den, double* partials, MapErrorStats* stats,
                           hipStream_t s);
// The grey image with every non-NaN error pixel replaced by jet(err, 0, max_error); flip: reversed linear pixel order.
int launch_map_error_picture(int rows, int cols, const uint8_t* gray, int gray_step, const float* err, float max_error, int flip, uint8_t* img,
                             hipStream_t s);

}  // namespace flame_hip
