// detections_kernels.h -- launch wrapper of detections_kernels.hip: getDebugImageDetections (flame.cc:1212-1251, 1272-1275,
// 2363-2412) from the frame's resident gradients and grey image (include/flame_stereo.h, flame_stereo_draw_detections states
// the rule).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "debug_kernels.h"
#include "feature_kernels.h"

namespace flame_hip {

// stats words of the picture.  [kDetAssert]: INT_MAX - p for the lowest p = row * width + col whose referenceEpiline asserted, 0
// when none did (kept as a maximum, so that the whole block starts as zeros: one memset).  The count of the pixels with a
// non-NaN score is accumulated in kDetSlots copies behind it, kDetSlotStride ints apart (one 128-byte line each), chosen by
// workgroup, and summed by the host, like the counters of the update kernel (stereo_kernels.h): one counter word for every
// wave's atomic took 85 of the kernel's 106 us at 1920x1080 (profiles/detections.txt).
constexpr int kDetAssert = 0, kDetCount = 32, kDetSlots = 64, kDetSlotStride = 32;
constexpr int kDetWords = kDetCount + kDetSlots * kDetSlotStride;

// Zeroes the kDetWords stats words, then paints.  `a`: rows, cols, gray, gray_step and flip are read; `scan`: the rectangle and g2 of
// detectFeatures (win, hc, wc are not read); gx_pad / gy_pad: the frame's padded gradients, cam.border pixels on every side.
// img: rows * cols * 3 bytes, 4-byte aligned.
int launch_draw_detections(const DebugImageArgs& a, const DetectGrid& scan, const Geo& geo, const StereoCamera& cam,
                           const float* gx_pad, const float* gy_pad, float max_score, int* stats, uint8_t* img, hipStream_t s);

}  // namespace flame_hip
