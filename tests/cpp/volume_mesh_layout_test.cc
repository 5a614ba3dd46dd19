// VolumeMeshLayout and the box check (flame_amd/csrc/side_stage.hpp): where the outputs of the volume's surface extraction lie in its
// pinned buffer, which boxes flame_nltgv2_volume_mesh_begin accepts, and how much room the arrays get.  Walks the layout over rooms that
// are no multiple of 16 bytes, with and without normals and copy_out: every offset is 16-byte aligned, nothing overlaps, `total` covers
// everything, the counters are always there, what does not travel takes no room -- and a buffer of exactly `total` bytes is written over
// every span's full extent, under AddressSanitizer when built that way.
//   volume_mesh_layout_test    exit 0: all held; 1: a violation (printed)
#include <cstdio>
#include <cstring>
#include <vector>

#include "side_stage.hpp"

using namespace flame_hip::host;

struct Span {
  const char* name;
  size_t at, bytes;
};

static int check(const VolumeMeshLayout& m, size_t vb, size_t nb, size_t tb) {
  const Span spans[] = {{"counts", m.counts, kCountSetsBytes}, {"totals", m.totals, kMeshTotalsBytes}, {"vertices", m.vertices, vb},
                        {"normals", m.normals, nb}, {"triangles", m.triangles, tb}};
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
  int bad = 0, walked = 0;
  const long long rooms[][2] = {{0, 0}, {1, 1}, {3, 5}, {950, 1896}, {7, 0}, {0, 12}, {100001, 199999}, {7 * 4096, 12 * 4096}};
  for (const auto& r : rooms)
    for (int normals = 0; normals < 2; ++normals)
      for (int copy_out = 0; copy_out < 2; ++copy_out) {
        const size_t vb = copy_out ? 12 * (size_t)r[0] : 0, tb = copy_out ? 12 * (size_t)r[1] : 0;
        bad += check(volume_mesh_layout(r[0], r[1], normals != 0, copy_out != 0), vb, normals ? vb : 0, tb);
        ++walked;
      }
  if (volume_mesh_layout(1 << 20, 1 << 21, true, false).total != 2048 + 16 + 16) std::printf("FAIL: the counters alone take more than their room\n"), ++bad;
  if (kMeshCountBytes != 32 || kMeshTotalsBytes != 16) std::printf("FAIL: the counters' sizes\n"), ++bad;

  struct Box {
    int32_t dims[3], lo[3], hi[3];
    unsigned long long want;
    int32_t lo_out[3], n_out[3];
  };
  const Box boxes[] = {
      {{4, 5, 6}, {0, 0, 0}, {0, 0, 0}, 120, {0, 0, 0}, {4, 5, 6}},          // all-zero hi: the whole volume
      {{4, 5, 6}, {1, 2, 3}, {4, 5, 6}, 27, {1, 2, 3}, {3, 3, 3}},
      {{4, 5, 6}, {0, 2, 0}, {4, 3, 6}, 24, {0, 2, 0}, {4, 1, 6}},           // one layer
      {{4, 5, 6}, {3, 4, 5}, {4, 5, 6}, 1, {3, 4, 5}, {1, 1, 1}},
      {{4, 5, 6}, {0, 0, 0}, {5, 5, 6}, 0, {0, 0, 0}, {0, 0, 0}},            // hi past the volume
      {{4, 5, 6}, {-1, 0, 0}, {4, 5, 6}, 0, {0, 0, 0}, {0, 0, 0}},
      {{4, 5, 6}, {2, 0, 0}, {2, 5, 6}, 0, {0, 0, 0}, {0, 0, 0}},            // empty
      {{4, 5, 6}, {3, 0, 0}, {2, 5, 6}, 0, {0, 0, 0}, {0, 0, 0}},
      {{4, 5, 6}, {0, 0, 0}, {4, 0, 6}, 0, {0, 0, 0}, {0, 0, 0}},            // one zero in hi is not "the whole volume"
      {{4, 5, 6}, {4, 0, 0}, {0, 0, 0}, 0, {0, 0, 0}, {0, 0, 0}},            // lo past the whole volume
      {{1024, 1024, 256}, {0, 0, 0}, {1024, 1024, 64}, 1ull << 26, {0, 0, 0}, {1024, 1024, 64}},
      {{1024, 1024, 256}, {0, 0, 0}, {1024, 1024, 65}, 0, {0, 0, 0}, {0, 0, 0}},  // over 2^26
      {{1024, 1024, 256}, {0, 0, 0}, {0, 0, 0}, 0, {0, 0, 0}, {0, 0, 0}},         // the whole volume is too
      {{1, 1, 1}, {0, 0, 0}, {0, 0, 0}, 1, {0, 0, 0}, {1, 1, 1}},
  };
  for (const Box& b : boxes) {
    int32_t lo[3] = {0, 0, 0}, n[3] = {0, 0, 0};
    const unsigned long long got = mesh_box_voxels(b.dims, b.lo, b.hi, lo, n);
    bool same = got == b.want;
    if (b.want)
      for (int a = 0; a < 3; ++a) same = same && lo[a] == b.lo_out[a] && n[a] == b.n_out[a];
    if (!same) std::printf("FAIL: box lo (%d, %d, %d) hi (%d, %d, %d) gives %llu voxels, expected %llu\n", b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2], got, b.want), ++bad;
  }
  // the room: the caller's capacity, capped by what the box can give; at 2^26 voxels both caps stay below 2^31
  if (mesh_vertex_room(10, 0) != 0 || mesh_vertex_room(10, 69) != 69 || mesh_vertex_room(10, 70) != 70 || mesh_vertex_room(10, 2147483647) != 70)
    std::printf("FAIL: mesh_vertex_room\n"), ++bad;
  if (mesh_triangle_room(10, 0) != 0 || mesh_triangle_room(10, 119) != 119 || mesh_triangle_room(10, 2147483647) != 120)
    std::printf("FAIL: mesh_triangle_room\n"), ++bad;
  if (mesh_vertex_room(kMeshMaxBoxVoxels, 2147483647) != 7ll << 26 || mesh_triangle_room(kMeshMaxBoxVoxels, 2147483647) != 12ll << 26 ||
      (12ll << 26) >= (1ll << 31))
    std::printf("FAIL: the caps at the largest box\n"), ++bad;
  std::printf("%d layouts walked, %zu boxes, %d violations\n", walked, sizeof(boxes) / sizeof(boxes[0]), bad);
  return bad ? 1 : 0;
}
