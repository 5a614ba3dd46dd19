// input_kernels.h -- launch wrapper of input_kernels.hip: a raw camera frame (grey or colour, any stride, with lens
// distortion, of any size) to the unpadded grey image launch_frame_pad_gradient reads (include/flame_stereo.h,
// flame_stereo_add_raw_frame states the rule).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flame_stereo.h"

namespace flame_hip {

// What the map of a rectified pixel reads: the first two rows of the working camera's Kinv, the raw camera, the distortion.
struct InputMap {
  float kinv[6];
  float fx, skew, cx, fy, cy;               // K_raw[0] [1] [2] [4] [5]
  float k1, k2, p1, p2, k3, k4, k5, k6;     // flame_stereo_input_params::dist, in its order
  int raw_width, raw_height;
};

// The count of the outside pixels is accumulated in kInputSlots copies, kInputSlotStride ints apart (one 128-byte line each),
// chosen by workgroup, and summed by the host, like the counters of the update kernel (stereo_kernels.h) and of the
// detections picture (detections_kernels.h: one counter word for every wave's atomic took 85 of that kernel's 106 us).
constexpr int kInputSlots = 64, kInputSlotStride = 32;
constexpr int kInputWords = kInputSlots * kInputSlotStride;

// Zeroes the kInputWords stats words, then writes the width x height grey image `out` (tight rows, 4-byte aligned base).
// `raw`: map.raw_height rows of `row_stride_bytes`, no alignment assumed; with remap false the map is not read and the raw
// frame has the output's size.  `format` is one of FLAME_STEREO_FMT_*, validated by the caller (input_params.hpp).
int launch_input_rectify(const InputMap& map, int format, bool remap, const uint8_t* raw, int row_stride_bytes, int width,
                         int height, int* stats, uint8_t* out, hipStream_t s);

}  // namespace flame_hip
