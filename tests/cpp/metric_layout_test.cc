// MetricLayout (flame_amd/csrc/side_stage.hpp): where the metric outputs lie in the stage's pinned buffer.  Walks every combination
// of the want_* flags and copy_out over sizes that are no multiple of 16 bytes: every offset is 16-byte aligned, no two outputs
// overlap, `total` covers all of them, an output that is not wanted (or does not travel) takes no room -- and a buffer of exactly
// `total` bytes is written over every output's full extent, under AddressSanitizer when built that way.
//   metric_layout_test      exit 0: all held; 1: a violation (printed)
#include <cstdio>
#include <cstring>
#include <vector>

#include "side_stage.hpp"

using flame_hip::host::metric_layout;
using flame_hip::host::MetricLayout;
using flame_hip::host::MetricWants;

struct Span {
  const char* name;
  size_t at, bytes;
};

static int check(int rows, int cols, int32_t V, int32_t T, const MetricWants& w) {
  const MetricLayout m = metric_layout(rows, cols, V, T, w);
  const size_t n = (size_t)rows * (size_t)cols;
  const bool out = w.copy_out;
  const Span spans[] = {
      {"counts", m.counts, 2 * sizeof(int32_t)},
      {"depth", m.depth, out && w.depth ? sizeof(float) * n : 0},
      {"depth_mm", m.depth_mm, out && w.depth_mm ? sizeof(uint16_t) * n : 0},
      {"organized", m.organized, out && w.organized ? 3 * sizeof(float) * n : 0},
      {"cloud", m.cloud, out && w.cloud ? 3 * sizeof(float) * n : 0},
      {"cloud_pixel", m.cloud_pixel, out && w.cloud ? sizeof(uint32_t) * n : 0},
      {"vertices", m.vertices, out && w.mesh ? 3 * sizeof(float) * (size_t)V : 0},
      {"normals", m.normals, out && w.mesh ? 3 * sizeof(float) * (size_t)V : 0},
      {"triangles", m.triangles, out && w.mesh ? 3 * sizeof(int32_t) * (size_t)T : 0},
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
  // nothing is reserved for what is not wanted: the outputs, rounded up, and one spare 16 bytes
  if (m.total != used + 16) std::printf("FAIL: total %zu, the outputs need %zu\n", m.total, used + 16), ++bad;
  if (bad) return bad;
  // a buffer of exactly `total` bytes takes every output in full, and each keeps its own bytes
  std::vector<unsigned char> buf(m.total, 0);
  for (size_t i = 0; i < count; ++i)
    if (spans[i].bytes) std::memset(buf.data() + spans[i].at, (int)(i + 1), spans[i].bytes);
  for (size_t i = 0; i < count; ++i)
    for (size_t b = 0; b < spans[i].bytes; b += spans[i].bytes > 64 ? spans[i].bytes - 1 : 1)
      if (buf[spans[i].at + b] != i + 1) return std::printf("FAIL: %s was overwritten\n", spans[i].name), 1;
  return 0;
}

int main() {
  const int sizes[][4] = {{1, 1, 1, 0}, {1, 63, 3, 1}, {3, 70, 5, 3}, {37, 29, 131, 237}, {480, 640, 8501, 16890}, {1080, 1920, 8501, 16890}};
  int bad = 0, walked = 0;
  for (const auto& s : sizes)
    for (int bits = 0; bits < 64; ++bits) {
      MetricWants w;
      w.depth = bits & 1, w.depth_mm = bits & 2, w.organized = bits & 4, w.cloud = bits & 8, w.mesh = bits & 16, w.copy_out = bits & 32;
      bad += check(s[0], s[1], s[2], s[3], w);
      ++walked;
    }
  MetricWants none{};
  if (metric_layout(480, 640, 100, 200, none).total != 32) std::printf("FAIL: nothing wanted still takes room\n"), ++bad;
  std::printf("%d layouts walked, %d violations\n", walked, bad);
  return bad ? 1 : 0;
}
