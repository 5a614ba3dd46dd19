// wireframe_kernels.h -- launch wrappers of wireframe_kernels.hip: drawWireframe (flame.cc:2414-2457, utils/image_utils.h:693-719,
// utils/visualization.h:235-260) from what already stands on the device (include/flame_nltgv2.h, flame_nltgv2_debug_wireframe_begin).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace flame_hip {

// One line of one triangle, draw id = 3 * triangle + k (k = 0: v0 -> v1, 1: v1 -> v2, 2: v0 -> v2): the rounded endpoints and the
// values at them.  Everything behind the setup kernel reads these records alone.  A line that is not walked (its triangle is not
// valid, or an endpoint lies outside the image) has x1 = -1; a walked one has coordinates inside the image, which are >= 0.
struct WireDraw {
  int16_t x1, y1, x2, y2;
  float a_val, b_val;
};
static_assert(sizeof(WireDraw) == 16, "a draw record is 16 bytes");

// counts: {lines_drawn, lines_skipped, total entries (the cursor of the offsets kernel), -}
enum { kWireDrawn = 0, kWireSkipped = 1, kWireTotal = 2, kWireCounts = 4 };

struct WireBuffers {
  WireDraw* draws;     // [3 T]
  uint32_t* cnt;       // [rows * cols] draws that touch the pixel
  uint32_t* offset;    // [rows * cols] where the pixel's entries begin
  uint32_t* fill;      // [rows * cols] entries stored so far
  uint64_t* entries;   // [capacity] id << 32 | c[0] | c[1] << 8 | c[2] << 16
  uint32_t capacity;
  int* counts;         // [kWireCounts]
};

struct WireImageArgs {
  int rows, cols;
  const uint8_t* gray;  // rows of cols bytes, gray_step bytes apart (device memory)
  int gray_step;
  float scene_color_scale;
  int flip;
};

// Setup (the only reader of vtx / x / tri_valid), count and offsets.  3 T draws; tri_valid may be NULL (every triangle valid).
// Zeroes cnt, fill and counts first.  `after_setup`, if not NULL, is recorded right behind the setup kernel.
int launch_wireframe_lists(int T, const int32_t* tris, const float2* vtx, const float* x, float value_scale, const uint8_t* tri_valid,
                           const WireBuffers& b, int rows, int cols, hipEvent_t after_setup, hipStream_t s);

// Fill, fold and paint: needs the draw records, cnt and offset of launch_wireframe_lists; zeroes fill first, so it can be repeated
// with a larger entry buffer.  img: rows * cols * 3 bytes, 4-byte aligned.
int launch_wireframe_paint(int T, const WireBuffers& b, const WireImageArgs& a, uint8_t* img, hipStream_t s);

}  // namespace flame_hip
