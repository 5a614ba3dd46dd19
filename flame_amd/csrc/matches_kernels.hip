// matches_kernels.hip -- getDebugImageMatches from the draw records of the update (stereo_kernels.h, MatchRecord):
//   updateFeatureIDepths   flame.cc:1293-1295 (the base image), 1350-1357 / 1365-1372 (the rings, three call sites each)
//   trackFeature           flame.cc:1626-1631, 1651-1656, 1668-1673, 1699-1725 (the rectangles and the searched segment)
//   applyColorMapLine      utils/visualization.h:236-260
// The reference draws sequentially, feature by feature; rectangles and rings overwrite, the segment blends.  A pixel's final value
// is a fold over the draws that touched it, in draw order (draw id = 4 * feature + k; k = 0 rectangle, 1 segment, 2 green ring,
// 3 blue ring).  The wireframe's scheme (wireframe_kernels.hip), with one more bit per entry that says "overwrite":
//   count     one lane per feature walks its draws: cnt[pixel] += 1
//   offsets   draw_offsets.hpp
//   fill      one lane per feature walks again: (id << 32 | opaque << 24 | colour) into the pixel's range
//   fold      per OUTPUT pixel, four per thread: the grey value, then the entries in increasing id
// Every pixel of every draw is tested against the image on its own; include/flame_stereo.h states the rule,
// tests/matches_ref.py restates it.
#include <hip/hip_runtime.h>

#include "debug_pixel.hpp"
#include "draw_lists.hpp"
#include "draw_offsets.hpp"
#include "matches_kernels.h"

namespace flame_hip {
namespace {

constexpr uint32_t kOpaque = 1u << 24;

// colours of the nine kinds, c[0] | c[1] << 8 | c[2] << 16 (flame.cc:1630, 1655, 1672, 1704-1710, 1351, 1366)
__device__ __forceinline__ uint32_t kind_colour(int kind) {
  switch (kind) {
    case kMatchMoveFailed: return 0u | (51u << 8) | (102u << 16);
    case kMatchMoved: return 255u | (0u << 8) | (255u << 16);
    case kMatchNoRegion: return 0u;
    case kMatchNoGradient: return 255u | (255u << 8);
    case kMatchNoGradientFresh: return 255u | (255u << 8) | (255u << 16);
    case kMatchAmbiguous: return 255u << 16;
    case kMatchMaxCost: return (255u << 8) | (255u << 16);
    case kMatchGreen: return 255u << 8;
    default: return 255u;  // kMatchBlue
  }
}

// cv::circle(centre, r, colour), thickness 1, LINE_8, restated (UNPINNED; include/flame_stereo.h has the walk): f(x, y) once per
// pixel of the outline, inside the image or not.
template <class F>
__device__ __forceinline__ void walk_ring(long cx, long cy, int r, F f) {
  auto plot4 = [&](int a, int b) {
    f(cx + a, cy + b);
    if (a) f(cx - a, cy + b);
    if (b) f(cx + a, cy - b);
    if (a && b) f(cx - a, cy - b);
  };
  int err = 0, dx = r, dy = 0, plus = 1, minus = 2 * r - 1;
  while (dx >= dy) {
    plot4(dx, dy);
    if (dx != dy) plot4(dy, dx);
    dy += 1, err += plus, plus += 2;
    if (err > 0) err -= minus, dx -= 1, minus -= 2;
  }
}

// The draws of one record, in draw order: f(k, colour word, x, y) for every pixel of every draw that lies inside the image.
template <class F>
__device__ __forceinline__ void walk_record(const MatchRecord& d, int rows, int cols, F f) {
  const int r1 = cols / 320, r2 = 4 * cols / 320;  // debug_feature_radius of trackFeature (:1547) and of updateFeatureIDepths (:1291)
  const uint32_t kind1 = d.flags & kMatchKindMask;
  const uint32_t colour = kind1 ? kind_colour((int)kind1 - 1) : 0u;
  if (kind1) {
    const long x0 = (long)d.rect_x - r1 > 0 ? (long)d.rect_x - r1 : 0, x1 = (long)d.rect_x + r1 < cols - 1 ? (long)d.rect_x + r1 : cols - 1;
    const long y0 = (long)d.rect_y - r1 > 0 ? (long)d.rect_y - r1 : 0, y1 = (long)d.rect_y + r1 < rows - 1 ? (long)d.rect_y + r1 : rows - 1;
    for (long y = y0; y <= y1; ++y)
      for (long x = x0; x <= x1; ++x) f(0, colour | kOpaque, x, y);
  }
  if (d.flags & kMatchLine)
    walk_line(d.x1, d.y1, d.x2, d.y2, [&](int, int, int x, int y) {
      if ((unsigned)x < (unsigned)cols && (unsigned)y < (unsigned)rows) f(1, colour, (long)x, (long)y);
    });
  if ((d.flags & (kMatchRingGreen | kMatchRingBlue)) && !(d.flags & kMatchRingsSkipped)) {
    const long cx = d.ring_x, cy = d.ring_y;
    if (cx + r2 < 0 || cx - r2 >= cols || cy + r2 < 0 || cy - r2 >= rows) return;  // no pixel of either ring is inside
    for (int k = 2; k < 4; ++k) {
      if (!(d.flags & (k == 2 ? kMatchRingGreen : kMatchRingBlue))) continue;
      const uint32_t c = kind_colour(k == 2 ? kMatchGreen : kMatchBlue) | kOpaque;
      walk_ring(cx, cy, r2, [&](long x, long y) {
        if (x >= 0 && x < cols && y >= 0 && y < rows) f(k, c, x, y);
      });
    }
  }
}

__global__ void __launch_bounds__(256)
k_match_count(int n, const MatchRecord* __restrict__ records, int rows, int cols, uint32_t* __restrict__ cnt,
              int* __restrict__ counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t flags = 0u;
  if (i < n) {
    const MatchRecord d = records[i];
    flags = d.flags;
    if (flags) walk_record(d, rows, cols, [&](int, uint32_t, long x, long y) { atomicAdd(&cnt[y * cols + x], 1u); });
  }
  // the counters, summed over the wave (no lane left before this point)
  const uint32_t kind1 = flags & kMatchKindMask;
  const bool skipped = (flags & kMatchRingsSkipped) != 0u;
  const int rings = ((flags & kMatchRingGreen) ? 1 : 0) + ((flags & kMatchRingBlue) ? 1 : 0);
  const bool lead = (threadIdx.x & 63) == 0;
#pragma unroll
  for (int k = 0; k < kMatchKinds - 2; ++k) {
    const int m = __popcll(__ballot(kind1 == (uint32_t)k + 1u));
    if (lead && m) atomicAdd(&counts[k], m);
  }
  const int green = __popcll(__ballot((flags & kMatchRingGreen) && !skipped));
  const int blue = __popcll(__ballot((flags & kMatchRingBlue) && !skipped));
  const int lines = __popcll(__ballot((flags & kMatchLine) != 0u)), lines_out = __popcll(__ballot((flags & kMatchLineSkipped) != 0u));
  const int one = __popcll(__ballot(skipped && rings == 1)), two = __popcll(__ballot(skipped && rings == 2));
  if (lead) {
    if (green) atomicAdd(&counts[kMatchGreen], green);
    if (blue) atomicAdd(&counts[kMatchBlue], blue);
    if (lines) atomicAdd(&counts[kMatchLinesDrawn], lines);
    if (lines_out) atomicAdd(&counts[kMatchLinesSkipped], lines_out);
    if (one + two) atomicAdd(&counts[kMatchRingsSkippedCount], one + 2 * two);
  }
}

__global__ void __launch_bounds__(256)
k_match_fill(int n, const MatchRecord* __restrict__ records, int rows, int cols, const uint32_t* __restrict__ offset,
             uint32_t* __restrict__ fill, uint64_t* __restrict__ entries, uint32_t capacity) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const MatchRecord d = records[i];
  if (!d.flags) return;
  walk_record(d, rows, cols, [&](int k, uint32_t colour, long x, long y) {
    const long p = y * cols + x;
    const uint32_t at = offset[p] + atomicAdd(&fill[p], 1u);
    if (at < capacity) entries[at] = ((uint64_t)(4u * (uint32_t)i + (uint32_t)k) << 32) | (uint64_t)colour;
  });
}

__global__ void __launch_bounds__(256)
k_match_fold(MatchImageArgs a, const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ offset,
             const uint64_t* __restrict__ entries, uint32_t capacity, uint8_t* __restrict__ img) {
  const long n = (long)a.rows * a.cols;
  const long o0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * kPixelsPerThread;
  if (o0 >= n) return;
  uint32_t px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int k = 0; k < kPixelsPerThread; ++k) {
    const long o = o0 + k;
    if (o >= n) continue;
    const long i = a.flip ? n - 1 - o : o;  // the source pixel of output pixel o
    const int row = (int)(i / a.cols), col = (int)(i % a.cols);
    const uint32_t g = a.gray[(long)row * a.gray_step + col];  // cvtColor(GRAY2RGB): three equal bytes
    uint32_t c0 = g, c1 = g, c2 = g;
    const uint32_t c = cnt[i], off = offset[i];
    // (a list that does not fit the entry buffer is left alone: the total says so and the host repeats fill and fold)
    if (c != 0u && (uint64_t)off + c <= (uint64_t)capacity) {
      const uint64_t* e = entries + off;
      int64_t last = -1;
      for (uint32_t j = 0; j < c; ++j) {
        uint64_t best = ~0ull;
        if (c == 1u) {
          best = e[0];
        } else {
          for (uint32_t m = 0; m < c; ++m) {
            const uint64_t v = e[m];
            if ((int64_t)(v >> 32) > last && v < best) best = v;
          }
        }
        if (best == ~0ull) break;
        last = (int64_t)(best >> 32);
        const uint32_t e0 = (uint32_t)best & 255u, e1 = (uint32_t)(best >> 8) & 255u, e2 = (uint32_t)(best >> 16) & 255u;
        if ((uint32_t)best & kOpaque) c0 = e0, c1 = e1, c2 = e2;
        else c0 = (c0 + e0) >> 1, c1 = (c1 + e1) >> 1, c2 = (c2 + e2) >> 1;  // colour * 0.5f + pixel * 0.5f, truncated: exact
      }
    }
    px[k] = c0 | (c1 << 8) | (c2 << 16);
  }
  store_pixels(img, o0, n, px);
}

}  // namespace

int launch_matches_lists(int n, const MatchRecord* records, const MatchBuffers& b, int rows, int cols, hipStream_t s) {
  const long px = (long)rows * cols;
  if (px <= 0) return 0;
  (void)hipMemsetAsync(b.cnt, 0, sizeof(uint32_t) * (size_t)px, s);
  (void)hipMemsetAsync(b.counts, 0, kMatchCounts * sizeof(int), s);
  if (n > 0) hipLaunchKernelGGL(k_match_count, grid1d(n), dim3(256), 0, s, n, records, rows, cols, b.cnt, b.counts);
  hipLaunchKernelGGL(k_draw_offsets, grid1d((px + kOffsetsPerLane - 1) / kOffsetsPerLane), dim3(256), 0, s, px, b.cnt, b.offset,
                     (uint32_t*)&b.counts[kMatchTotal]);
  return (int)hipGetLastError();
}

int launch_matches_paint(int n, const MatchRecord* records, const MatchBuffers& b, const MatchImageArgs& a, uint8_t* img,
                         hipStream_t s) {
  const long px = (long)a.rows * a.cols;
  if (px <= 0) return 0;
  (void)hipMemsetAsync(b.fill, 0, sizeof(uint32_t) * (size_t)px, s);
  if (n > 0)
    hipLaunchKernelGGL(k_match_fill, grid1d(n), dim3(256), 0, s, n, records, a.rows, a.cols, b.offset, b.fill, b.entries, b.capacity);
  hipLaunchKernelGGL(k_match_fold, grid1d((px + kPixelsPerThread - 1) / kPixelsPerThread), dim3(256), 0, s, a, b.cnt, b.offset,
                     b.entries, b.capacity, img);
  return (int)hipGetLastError();
}

}  // namespace flame_hip
