// align_kernels.h -- launch wrappers of align_kernels.hip: the pyramid levels of a resident frame and the Gauss-Newton system of a direct
// image alignment against a dense inverse-depth map (include/flame_stereo.h, flame_stereo_build_pyramid / flame_stereo_align_linearize,
// states every rule; tests/align_ref.py restates them in numpy and is the checker, bit for bit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pairwise_sum.hpp"

namespace flame_hip {

constexpr int kAlignSums = 28;        // 21 of H, 6 of b, the cost
constexpr int kAlignCounts = 5;       // n_used, n_no_depth, n_behind, n_outside, n_huber
constexpr int kAlignGroupSums = 7;    // sums reduced together: 7 x 1024 doubles = 56 KB of LDS, 4 rounds
constexpr int kAlignMaxGroups = 2048; // workgroups of the linearisation at most; beyond, each takes consecutive chunks

// What the two kernels leave on the device: == the head of flame_stereo_align_system.
struct AlignSystem {
  double sums[kAlignSums];
  int32_t counts[kAlignCounts];
  int32_t reserved_;
};

// One pyramid level of a frame.  Level 0 lives inside the padded planes (pitch = width + 2 border, the pointers at pixel (0, 0));
// levels >= 1 are unpadded (pitch = w).
struct AlignLevel {
  const uint8_t* img;
  const float* gx;
  const float* gy;
  int w, h, pitch;
};

struct AlignArgs {
  AlignLevel ref, cur;   // the same w, h
  const float* map;      // level-0 resolution, map_w floats per row
  int map_w, shift;      // the level: d = map[(y << shift) * map_w + (x << shift)]
  int border;
  float huber_k;
  float fx, fy, cx, cy;  // of the level
  float R[9], t[3];
};

inline long align_chunks(long n) { return (n + kPairwiseChunk - 1) / kPairwiseChunk; }

// dst (dw x dh = ((sw + 1) / 2, (sh + 1) / 2), unpadded) = pyrDown of src (sw x sh, src_pitch bytes per row), with its central gradients.
int launch_pyr_down(const uint8_t* src, int sw, int sh, int src_pitch, uint8_t* dst, float* gx, float* gy, hipStream_t s);
// The 28 sums and 5 counts of one linearisation into *out; partials: [28][align_chunks(w * h)] doubles of scratch.
int launch_align_linearize(const AlignArgs& a, double* partials, AlignSystem* out, hipStream_t s);

}  // namespace flame_hip
