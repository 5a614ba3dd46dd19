// draw_lists.hpp -- device functions the pictures drawn as per-pixel folds share (wireframe_kernels.hip, matches_kernels.hip; the
// update kernel of stereo_kernels.hip rounds its segment's endpoints with them): the rounding of a line's endpoints and the line walk.
// The kernel that gives every touched pixel its range of the entry buffer is draw_offsets.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace flame_hip {
namespace {

// cvRound of an endpoint coordinate and whether it lies in [0, hi]: a NaN, an infinity and anything that rounds outside fail.
__device__ __forceinline__ bool round_inside(float v, int hi, int* out) {
  const float r = rintf(v);  // round half to even, as __float2int_rn; compared as a float first: no cast of a huge value
  if (!(r >= 0.0f && r <= (float)hi)) return false;
  *out = (int)r;
  return true;
}

// cv::LineIterator (OpenCV 3.2, connectivity 8) from (x1, y1) to (x2, y2), restated (UNPINNED): f(ii, count, x, y) for each of
// its count = max(|dx|, |dy|) + 1 pixels.  Every pixel lies in the endpoints' bounding box.
template <class F>
__device__ __forceinline__ void walk_line(int x1, int y1, int x2, int y2, F f) {
  int x = x1, y = y1;
  int dx = x2 - x1, dy = y2 - y1;
  const int sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1;
  dx = dx < 0 ? -dx : dx, dy = dy < 0 ? -dy : dy;
  int major_x = sx, major_y = 0, minor_x = 0, minor_y = sy;
  if (dy > dx) {  // y is the major axis
    const int t = dx;
    dx = dy, dy = t;
    major_x = 0, major_y = sy, minor_x = sx, minor_y = 0;
  }
  int err = dx - 2 * dy;
  const int count = dx + 1;
  for (int ii = 0; ii < count; ++ii) {
    f(ii, count, x, y);
    const bool m = err < 0;
    err += -2 * dy + (m ? 2 * dx : 0);
    x += major_x + (m ? minor_x : 0), y += major_y + (m ? minor_y : 0);
  }
}

}  // namespace
}  // namespace flame_hip
