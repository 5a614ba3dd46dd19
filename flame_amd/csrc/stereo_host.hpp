// stereo_host.hpp -- the pure part of the stereo front end's host code (stereo_capi.hip, stereo_front_capi.hip,
// stereo_debug_align_capi.hip), no HIP and no context: how far a buffer grows, the scan rectangle of projectFeatures / detectFeatures /
// prunePoseFrames, the cell grid of detectFeatures, the decode of a stage's stats words and the interior of a padded plane.
// tests/cpp/stereo_host_test.cc walks all of it.
#ifndef FLAME_AMD_STEREO_HOST_HPP_
#define FLAME_AMD_STEREO_HOST_HPP_

#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>

namespace flame_hip {
namespace host {

// Elements a device array gets when `count` no longer fit, and a pinned one (it is reallocated less often: hipHostFree waits too).
inline size_t grown(size_t count) { return count + count / 2 + 16; }
inline size_t grown_pinned(size_t count) { return count * 2 + 16; }
// Entries of the matches picture's fold: two per pixel, or a quarter above what the last picture needed.
inline size_t entry_capacity(size_t px, size_t last_total) { return std::max(2 * px, last_total + last_total / 4); }

// `int border = params.rescale_factor_max * params.fparams.win_size / 2 + 1;` (flame.cc:847, 1771): float arithmetic
inline int front_border(float rescale_factor_max, int win_size) { return (int)(rescale_factor_max * win_size / 2 + 1); }

// cols [c_lo, c_hi), rows [r_lo, r_hi): the image without `border` on every side and, letterboxed, without height / 3 rows at the
// top and at the bottom.  w() = width - 2 border, h() = height - 2 border - 2 row_offset: cv::Rect's width and height.
struct ScanRect {
  int c_lo, r_lo, c_hi, r_hi;
  int w() const { return c_hi - c_lo; }
  int h() const { return r_hi - r_lo; }
};
inline ScanRect scan_rect(int width, int height, int border, bool letterbox) {
  const int row_offset = letterbox ? height / 3 : 0;
  return ScanRect{border, border + row_offset, width - border, height - border - row_offset};
}

// utils::fast_ceil(static_cast<float>(size) / win) (image_utils.h:82-85)
inline int ceil_cells(int size, int win) {
  const float f = (float)size / win;
  return (int)f < f ? (int)f + 1 : (int)f;
}
// A host mask point lies in the image and in a cell of the wc x hc grid (the reference indexes its cell mask with it unchecked).
inline bool mask_point_valid(float x, float y, int width, int height, int win, int wc, int hc) {
  if (!(x >= 0.0f && y >= 0.0f && x < (float)width && y < (float)height)) return false;
  return (uint32_t)(x / (float)win) < (uint32_t)wc && (uint32_t)(y / (float)win) < (uint32_t)hc;
}

// A stage's kernels leave the lowest index of a record that tripped an assert and of one that names an unknown frame, INT_MAX for
// none.  Which of the two the reference meets first depends on its loop:
enum class ErrorRule {
  kBadFrameFirst,  // pfs.at() / pfs_[id] of every record comes before any assert (update, projectFeatures, prunePoseFrames)
  kLowerIndex,     // one loop stops at the first record that fails either; within a record the assert comes first (syncGraph)
  kAssertOnly,     // no record names a frame (detectFeatures)
};
enum class ErrorKind { kNone, kAssert, kBadFrame };
struct FirstError { ErrorKind kind; int index; };  // index: the record; -1 with kNone
inline FirstError first_error(int assert_idx, int bad_frame_idx, ErrorRule rule) {
  const bool a = assert_idx != INT_MAX, b = rule != ErrorRule::kAssertOnly && bad_frame_idx != INT_MAX;
  if (!a && !b) return FirstError{ErrorKind::kNone, -1};
  const bool is_assert = !b || (a && rule == ErrorRule::kLowerIndex && assert_idx <= bad_frame_idx);
  return is_assert ? FirstError{ErrorKind::kAssert, assert_idx} : FirstError{ErrorKind::kBadFrame, bad_frame_idx};
}

// Counters accumulated in `slots` copies `stride` words apart, from words[first]: sums[c] = the sum of counter c over the copies.
inline void sum_slots(const int* words, int first, int slots, int stride, int n_counters, int* sums) {
  for (int c = 0; c < n_counters; ++c) {
    int sum = 0;
    for (int k = 0; k < slots; ++k) sum += words[first + k * stride + c];
    sums[c] = sum;
  }
}

// Elements from the start of a plane padded by `border` on every side (`pitch` = width + 2 border) to its pixel (0, 0).
inline size_t interior_offset(int border, int pitch) { return (size_t)border * pitch + border; }

}  // namespace host
}  // namespace flame_hip

#endif  // FLAME_AMD_STEREO_HOST_HPP_
