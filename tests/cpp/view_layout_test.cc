// ViewLayout (flame_amd/csrc/side_stage.hpp): where the view renderer's outputs lie in its pinned buffer.  Walks every combination of
// the want_* flags and copy_out over sizes that are no multiple of 16 bytes: every offset is 16-byte aligned, nothing overlaps, `total`
// covers everything, the counters are always there, what is not wanted (or does not travel) takes no room -- and a buffer of exactly
// `total` bytes is written over every span's full extent, under AddressSanitizer when built that way.
//   view_layout_test      exit 0: all held; 1: a violation (printed)
#include <cstdio>
#include <cstring>
#include <vector>

#include "side_stage.hpp"

using flame_hip::host::kViewCountBytes;
using flame_hip::host::view_layout;
using flame_hip::host::ViewLayout;
using flame_hip::host::ViewWants;

struct Span {
  const char* name;
  size_t at, bytes;
};

static int check(int rows, int cols, const ViewWants& w) {
  const ViewLayout v = view_layout(rows, cols, w);
  const size_t n = (size_t)rows * (size_t)cols;
  const Span spans[] = {
      {"counts", v.counts, kViewCountBytes},
      {"map", v.map, w.copy_out && w.map ? sizeof(float) * n : 0},
      {"tri_index", v.tri_index, w.copy_out && w.tri_index ? sizeof(int32_t) * n : 0},
  };
  const size_t count = sizeof(spans) / sizeof(spans[0]);
  int bad = 0;
  size_t used = 0;
  for (size_t i = 0; i < count; ++i) {
    const Span& s = spans[i];
    if (s.at % 16 != 0) std::printf("FAIL: %s at %zu is not 16-byte aligned\n", s.name, s.at), ++bad;
    if (s.at + s.bytes > v.total) std::printf("FAIL: %s ends at %zu, total %zu\n", s.name, s.at + s.bytes, v.total), ++bad;
    for (size_t j = 0; j < i; ++j) {
      const Span& o = spans[j];
      if (s.bytes && o.bytes && s.at < o.at + o.bytes && o.at < s.at + s.bytes) std::printf("FAIL: %s overlaps %s\n", s.name, o.name), ++bad;
    }
    used += (s.bytes + 15) & ~size_t(15);
  }
  if (v.total != used + 16) std::printf("FAIL: total %zu, the spans need %zu\n", v.total, used + 16), ++bad;
  if (bad) return bad;
  std::vector<unsigned char> buf(v.total, 0);
  for (size_t i = 0; i < count; ++i)
    if (spans[i].bytes) std::memset(buf.data() + spans[i].at, (int)(i + 1), spans[i].bytes);
  for (size_t i = 0; i < count; ++i)
    for (size_t b = 0; b < spans[i].bytes; b += spans[i].bytes > 64 ? spans[i].bytes - 1 : 1)
      if (buf[spans[i].at + b] != i + 1) return std::printf("FAIL: %s was overwritten\n", spans[i].name), 1;
  return 0;
}

int main() {
  const int sizes[][2] = {{1, 1}, {3, 5}, {9, 77}, {75, 100}, {480, 640}, {1080, 1920}};
  int bad = 0, walked = 0;
  for (const auto& s : sizes)
    for (int bits = 0; bits < 8; ++bits) {
      ViewWants w;
      w.map = bits & 1, w.tri_index = bits & 2, w.copy_out = bits & 4;
      bad += check(s[0], s[1], w);
      ++walked;
    }
  ViewWants device_only{};
  device_only.map = device_only.tri_index = true;
  if (view_layout(1080, 1920, device_only).total != 16 + 16) std::printf("FAIL: the counters alone take more than their room\n"), ++bad;
  if (kViewCountBytes != 16) std::printf("FAIL: the counters are %zu bytes\n", kViewCountBytes), ++bad;
  std::printf("%d layouts walked, %d violations\n", walked, bad);
  return bad ? 1 : 0;
}
