// VolumeLayout (flame_amd/csrc/side_stage.hpp): where the outputs of the volume's two stages lie in their pinned buffers, and which
// dimensions a volume may have.  Walks the integration's layout and the raycast's over sizes that are no multiple of 16 bytes, with and
// without copy_out: every offset is 16-byte aligned, nothing overlaps, `total` covers everything, the counters are always there, a map
// that does not travel takes no room -- and a buffer of exactly `total` bytes is written over every span's full extent, under
// AddressSanitizer when built that way.  sum_count_slots: the partial sets of the counters, summed.  volume_voxels: the limits of flame_nltgv2_volume_create, at their edges.
//   volume_layout_test    exit 0: all held; 1: a violation (printed)
#include <cstdio>
#include <cstring>
#include <vector>

#include "side_stage.hpp"

using flame_hip::host::integrate_layout;
using flame_hip::host::kIntegrateCountBytes;
using flame_hip::host::kRaycastCountBytes;
using flame_hip::host::kCountSetsBytes;
using flame_hip::host::kCountSets;
using flame_hip::host::kCountSetWords;
using flame_hip::host::sum_count_slots;
using flame_hip::host::raycast_layout;
using flame_hip::host::volume_voxels;
using flame_hip::host::VolumeLayout;

struct Span {
  const char* name;
  size_t at, bytes;
};

static int check(const VolumeLayout& v, size_t count_bytes, size_t map_bytes) {
  const Span spans[] = {{"counts", v.counts, count_bytes}, {"map", v.map, map_bytes}};
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
  const int sizes[][2] = {{1, 1}, {3, 5}, {5, 7}, {3, 65}, {24, 32}, {480, 640}, {1080, 1920}, {32767, 3}};
  int bad = 0, walked = 0;
  bad += check(integrate_layout(), kCountSetsBytes, 0), ++walked;
  for (const auto& s : sizes)
    for (int copy_out = 0; copy_out < 2; ++copy_out) {
      bad += check(raycast_layout(s[0], s[1], copy_out != 0), kCountSetsBytes, copy_out ? sizeof(float) * (size_t)s[0] * (size_t)s[1] : 0);
      ++walked;
    }
  if (raycast_layout(1080, 1920, false).total != 2048 + 16) std::printf("FAIL: the raycast's counters alone take more than their room\n"), ++bad;
  if (integrate_layout().total != 2048 + 16) std::printf("FAIL: the integration's counters alone take more than their room\n"), ++bad;
  if (kIntegrateCountBytes != 32 || kRaycastCountBytes != 16 || kCountSetsBytes != 2048) std::printf("FAIL: the counters' sizes\n"), ++bad;
  // the partial sets summed: set s holds s + c in word c and rubbish behind the stage's counters
  std::vector<int32_t> slots(kCountSets * kCountSetWords, 1000000);
  for (int s = 0; s < kCountSets; ++s)
    for (int c = 0; c < 8; ++c) slots[s * kCountSetWords + c] = s + c;
  int32_t sums[8];
  sum_count_slots(slots.data(), 8, sums);
  for (int c = 0; c < 8; ++c)
    if (sums[c] != 120 + 16 * c) std::printf("FAIL: sum_count_slots word %d is %d\n", c, sums[c]), ++bad;

  struct Dims {
    int nx, ny, nz;
    unsigned long long want;
  };
  const Dims dims[] = {{1, 1, 1, 1ull},          {5, 3, 7, 105ull},         {1024, 1024, 256, 1ull << 28}, {1024, 1024, 257, 0ull},
                       {1024, 512, 512, 1ull << 28}, {1025, 1, 1, 0ull},     {0, 4, 4, 0ull},               {4, -1, 4, 0ull},
                       {4, 4, 0, 0ull},          {1024, 1024, 1024, 0ull}, {1, 1, 1024, 1024ull},         {1, 1025, 1, 0ull}};
  for (const Dims& d : dims)
    if (volume_voxels(d.nx, d.ny, d.nz) != d.want)
      std::printf("FAIL: volume_voxels(%d, %d, %d) = %llu, expected %llu\n", d.nx, d.ny, d.nz, (unsigned long long)volume_voxels(d.nx, d.ny, d.nz), d.want), ++bad;
  std::printf("%d layouts walked, %zu dimension triples, %d violations\n", walked, sizeof(dims) / sizeof(dims[0]), bad);
  return bad ? 1 : 0;
}
