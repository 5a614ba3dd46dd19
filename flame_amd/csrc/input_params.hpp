// input_params.hpp -- the pure host part of the raw-frame input stage (flame_stereo_set_input / flame_stereo_add_raw_frame,
// include/flame_stereo.h): bytes per pixel of a format, the validation both entry points share, and the grid arithmetic of
// k_input_rectify.  No HIP in here: tests/cpp/input_params_test.cc runs it under the sanitizers (make sanitize).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "flame_stereo.h"

namespace flame_hip {

constexpr int kInputPixelsPerThread = 4;  // one dword of output per lane
constexpr int kInputBlock = 256;
constexpr int kInputMaxDim = 16384;  // set_camera's bound on the working camera, applied to the raw one too

// 0 for an unknown format
inline int input_bytes_per_pixel(int format) {
  switch (format) {
    case FLAME_STEREO_FMT_GREY8: return 1;
    case FLAME_STEREO_FMT_BGR8:
    case FLAME_STEREO_FMT_RGB8: return 3;
    case FLAME_STEREO_FMT_BGRA8:
    case FLAME_STEREO_FMT_RGBA8: return 4;
    default: return 0;
  }
}

// What flame_stereo_set_input accepts for a working camera of cam_width x cam_height.
inline bool input_params_valid(const flame_stereo_input_params* p, int cam_width, int cam_height) {
  if (!p || input_bytes_per_pixel(p->format) == 0) return false;
  if (p->remap != 0 && p->remap != 1) return false;
  if (p->raw_width < 2 || p->raw_height < 2 || p->raw_width > kInputMaxDim || p->raw_height > kInputMaxDim) return false;
  if (p->remap == 0 && (p->raw_width != cam_width || p->raw_height != cam_height)) return false;
  return true;
}

// What flame_stereo_add_raw_frame accepts on top of that.
inline bool input_frame_valid(const flame_stereo_input_params& p, const void* raw, int row_stride_bytes) {
  const int bpp = input_bytes_per_pixel(p.format);
  return raw != nullptr && bpp != 0 && (long)row_stride_bytes >= (long)p.raw_width * bpp;
}

// Bytes of the raw frame from its first to its last pixel byte (the last row ends with its pixels, not with its stride).
inline size_t input_frame_bytes(const flame_stereo_input_params& p, int row_stride_bytes) {
  return (size_t)(p.raw_height - 1) * (size_t)row_stride_bytes + (size_t)p.raw_width * (size_t)input_bytes_per_pixel(p.format);
}

// Threads and workgroups of k_input_rectify for n output pixels: kInputPixelsPerThread pixels per thread, the last thread
// may own fewer.
inline long input_threads(long n_pixels) { return (n_pixels + kInputPixelsPerThread - 1) / kInputPixelsPerThread; }
inline unsigned input_blocks(long n_pixels) { return (unsigned)((input_threads(n_pixels) + kInputBlock - 1) / kInputBlock); }

}  // namespace flame_hip
