// MapErrorLayout (flame_amd/csrc/side_stage.hpp): where the map-error stage's outputs and its staged inputs lie in its pinned buffer.
// Walks every combination of the want_* flags, copy_out and the two host inputs over sizes that are no multiple of 16 bytes: every
// offset is 16-byte aligned, nothing overlaps, `total` covers everything, the statistics are always there, what is not wanted (or does
// not travel) takes no room -- and a buffer of exactly `total` bytes is written over every span's full extent, under AddressSanitizer
// when built that way.  Also the window rule (map_error_window).
//   map_error_layout_test      exit 0: all held; 1: a violation (printed)
#include <cstdio>
#include <cstring>
#include <vector>

#include "side_stage.hpp"

using flame_hip::host::kMapErrorStatsBytes;
using flame_hip::host::map_error_layout;
using flame_hip::host::map_error_window;
using flame_hip::host::MapErrorLayout;
using flame_hip::host::MapErrorWants;

struct Span {
  const char* name;
  size_t at, bytes;
};

static int check(int rows, int cols, const MapErrorWants& w) {
  const MapErrorLayout m = map_error_layout(rows, cols, w);
  const size_t n = (size_t)rows * (size_t)cols;
  const Span spans[] = {
      {"stats", m.stats, kMapErrorStatsBytes},
      {"error_map", m.error_map, w.copy_out && w.error_map ? sizeof(float) * n : 0},
      {"image", m.image, w.copy_out && w.image ? 3 * n : 0},
      {"truth", m.truth, w.host_truth ? sizeof(float) * n : 0},
      {"gray", m.gray, w.host_gray ? n : 0},
  };
  const size_t count = sizeof(spans) / sizeof(spans[0]);
  int bad = 0;
  size_t used = 0;
  for (size_t i = 0; i < count; ++i) {
    const Span& s = spans[i];
    if (s.at % 16 != 0) std::printf("FAIL: %s at %zu is not 16-byte aligned\n", s.name, s.at), ++bad;
    if (s.at + s.bytes > m.total) std::printf("FAIL: %s ends at %zu, total %zu\n", s.name, s.at + s.bytes, m.total), ++bad;
    for (size_t j = 0; j < i; ++j) {
      const Span& o = spans[j];
      if (s.bytes && o.bytes && s.at < o.at + o.bytes && o.at < s.at + s.bytes) std::printf("FAIL: %s overlaps %s\n", s.name, o.name), ++bad;
    }
    used += (s.bytes + 15) & ~size_t(15);
  }
  if (m.total != used + 16) std::printf("FAIL: total %zu, the spans need %zu\n", m.total, used + 16), ++bad;
  if (bad) return bad;
  std::vector<unsigned char> buf(m.total, 0);
  for (size_t i = 0; i < count; ++i)
    if (spans[i].bytes) std::memset(buf.data() + spans[i].at, (int)(i + 1), spans[i].bytes);
  for (size_t i = 0; i < count; ++i)
    for (size_t b = 0; b < spans[i].bytes; b += spans[i].bytes > 64 ? spans[i].bytes - 1 : 1)
      if (buf[spans[i].at + b] != i + 1) return std::printf("FAIL: %s was overwritten\n", spans[i].name), 1;
  return 0;
}

int main() {
  const int sizes[][2] = {{1, 1}, {7, 69}, {9, 77}, {37, 29}, {480, 640}, {1080, 1920}};
  int bad = 0, walked = 0;
  for (const auto& s : sizes)
    for (int bits = 0; bits < 64; ++bits) {
      MapErrorWants w;
      w.stats = bits & 1, w.error_map = bits & 2, w.image = bits & 4, w.copy_out = bits & 8, w.host_truth = bits & 16, w.host_gray = bits & 32;
      bad += check(s[0], s[1], w);
      ++walked;
    }
  MapErrorWants stats_only{};
  stats_only.stats = true;
  if (map_error_layout(1080, 1920, stats_only).total != 1056 + 16) std::printf("FAIL: the statistics alone take more than their room\n"), ++bad;
  if (kMapErrorStatsBytes != 1048) std::printf("FAIL: the statistics are %zu bytes\n", kMapErrorStatsBytes), ++bad;
  // the window: 0 is the reference's choice by the image's width; odd sizes up to the maximum pass; everything else is refused (0)
  const int win[][4] = {{0, 639, 31, 5}, {0, 640, 31, 11}, {0, 1, 31, 5}, {1, 640, 31, 1}, {3, 640, 31, 3}, {31, 640, 31, 31}, {33, 640, 31, 0},
                        {2, 640, 31, 0}, {10, 100, 31, 0}, {-1, 640, 31, 0}, {-3, 640, 31, 0}};
  for (const auto& c : win)
    if (map_error_window(c[0], c[1], c[2]) != c[3]) std::printf("FAIL: map_error_window(%d, %d, %d) != %d\n", c[0], c[1], c[2], c[3]), ++bad;
  std::printf("%d layouts walked, %d violations\n", walked, bad);
  return bad ? 1 : 0;
}
