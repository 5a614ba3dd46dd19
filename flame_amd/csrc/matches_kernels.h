// matches_kernels.h -- launch wrappers of matches_kernels.hip: getDebugImageMatches (flame.cc:1293-1295, 1350-1372, 1626-1725) from
// the draw records the recording instances of the update kernel leave (stereo_kernels.h, MatchRecord; include/flame_stereo.h,
// flame_stereo_draw_matches states the rule).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stereo_kernels.h"

namespace flame_hip {

// counts: [0, kMatchKinds) the draws by kind (flame_stereo_matches_stats.kind_count), then the words below
enum { kMatchLinesDrawn = kMatchKinds, kMatchLinesSkipped, kMatchRingsSkippedCount, kMatchTotal, kMatchCounts = 16 };

struct MatchBuffers {
  uint32_t* cnt;      // [rows * cols] draws that touch the pixel
  uint32_t* offset;   // [rows * cols] where the pixel's entries begin
  uint32_t* fill;     // [rows * cols] entries stored so far
  uint64_t* entries;  // [capacity] id << 32 | opaque << 24 | c[0] | c[1] << 8 | c[2] << 16, id = 4 * feature + k
  uint32_t capacity;
  int* counts;        // [kMatchCounts]
};

struct MatchImageArgs {
  int rows, cols;
  const uint8_t* gray;  // rows of cols bytes, gray_step bytes apart (device memory)
  int gray_step;
  int flip;
};

// Count and offsets over n records.  Zeroes cnt and counts first.
int launch_matches_lists(int n, const MatchRecord* records, const MatchBuffers& b, int rows, int cols, hipStream_t s);

// Fill, fold and paint: needs cnt and offset of launch_matches_lists; zeroes fill first, so it can be repeated with a larger
// entry buffer.  img: rows * cols * 3 bytes, 4-byte aligned.
int launch_matches_paint(int n, const MatchRecord* records, const MatchBuffers& b, const MatchImageArgs& a, uint8_t* img,
                         hipStream_t s);

}  // namespace flame_hip
