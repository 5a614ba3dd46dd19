// FuseLayout (flame_amd/csrc/side_stage.hpp): where the fusion stage's outputs lie in its pinned buffer.  Walks every combination of the
// want_* flags and copy_out over sizes that are no multiple of 16 bytes and over 1, 3 and 8 sources: every offset is 16-byte aligned,
// nothing overlaps, `total` covers everything, the counters are always there, what is not wanted (or does not travel) takes no room --
// and a buffer of exactly `total` bytes is written over every span's full extent, under AddressSanitizer when built that way.
//   fuse_layout_test      exit 0: all held; 1: a violation (printed)
#include <cstdio>
#include <cstring>
#include <vector>

#include "side_stage.hpp"

using flame_hip::host::fuse_layout;
using flame_hip::host::FuseLayout;
using flame_hip::host::FuseWants;
using flame_hip::host::kFuseCountBytes;

struct Span {
  const char* name;
  size_t at, bytes;
};

static int check(int rows, int cols, int n_sources, const FuseWants& w) {
  const FuseLayout l = fuse_layout(rows, cols, n_sources, w);
  const size_t n = (size_t)rows * (size_t)cols;
  const bool out = w.copy_out;
  const Span spans[] = {
      {"counts", l.counts, kFuseCountBytes},
      {"fused", l.fused, out && w.fused ? sizeof(float) * n : 0},
      {"present", l.present, out && w.masks ? n : 0},
      {"inlier", l.inlier, out && w.masks ? n : 0},
      {"spread", l.spread, out && w.spread ? sizeof(float) * n : 0},
      {"layers", l.layers, out && w.layers ? sizeof(float) * n * (size_t)n_sources : 0},
  };
  const size_t count = sizeof(spans) / sizeof(spans[0]);
  int bad = 0;
  size_t used = 0;
  for (size_t i = 0; i < count; ++i) {
    const Span& s = spans[i];
    if (s.at % 16 != 0) std::printf("FAIL: %s at %zu is not 16-byte aligned\n", s.name, s.at), ++bad;
    if (s.at + s.bytes > l.total) std::printf("FAIL: %s ends at %zu, total %zu\n", s.name, s.at + s.bytes, l.total), ++bad;
    for (size_t j = 0; j < i; ++j) {
      const Span& o = spans[j];
      if (s.bytes && o.bytes && s.at < o.at + o.bytes && o.at < s.at + s.bytes) std::printf("FAIL: %s overlaps %s\n", s.name, o.name), ++bad;
    }
    used += (s.bytes + 15) & ~size_t(15);
  }
  if (l.total != used + 16) std::printf("FAIL: total %zu, the spans need %zu\n", l.total, used + 16), ++bad;
  if (bad) return bad;
  std::vector<unsigned char> buf(l.total, 0);
  for (size_t i = 0; i < count; ++i)
    if (spans[i].bytes) std::memset(buf.data() + spans[i].at, (int)(i + 1), spans[i].bytes);
  for (size_t i = 0; i < count; ++i)
    for (size_t b = 0; b < spans[i].bytes; b += spans[i].bytes > 64 ? spans[i].bytes - 1 : 1)
      if (buf[spans[i].at + b] != i + 1) return std::printf("FAIL: %s was overwritten\n", spans[i].name), 1;
  return 0;
}

int main() {
  const int sizes[][2] = {{1, 1}, {3, 5}, {9, 77}, {75, 100}, {480, 640}};
  const int sources[] = {1, 3, 8};
  int bad = 0, walked = 0;
  for (const auto& s : sizes)
    for (int n_sources : sources)
      for (int bits = 0; bits < 32; ++bits) {
        FuseWants w;
        w.fused = bits & 1, w.masks = bits & 2, w.spread = bits & 4, w.layers = bits & 8, w.copy_out = bits & 16;
        bad += check(s[0], s[1], n_sources, w);
        ++walked;
      }
  FuseWants device_only{};
  device_only.fused = device_only.masks = device_only.spread = device_only.layers = true;
  if (fuse_layout(1080, 1920, 8, device_only).total != 128 + 16) std::printf("FAIL: the counters alone take more than their room\n"), ++bad;
  if (kFuseCountBytes != 128) std::printf("FAIL: the counters are %zu bytes\n", kFuseCountBytes), ++bad;
  std::printf("%d layouts walked, %d violations\n", walked, bad);
  return bad ? 1 : 0;
}
