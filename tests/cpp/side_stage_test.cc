// tests/cpp/side_stage_test.cc -- host-only check of flame_amd/csrc/side_stage.hpp, built by `make -C flame_amd/csrc sanitize` under
// ASan + UBSan: the record of the resident triangles (ResidentTris), the pinned layouts of the side-stream stages and the triangle
// index check.
// ResidentTris replaced eight loose members of the context that six entry points updated by hand.  `Loose` below restates those
// members and, per entry point and outcome, the statements that entry point held, copied from it; `gates` restates the expressions
// that read them.  The named sequences carry expectations written out by hand from those expressions; the walk then takes every
// entry point from every state the loose members can reach and compares the two records gate by gate.  Neither is derived from the
// code under test.
#include <cstdint>
#include <cstdio>
#include <set>
#include <tuple>
#include <vector>

#include "side_stage.hpp"

using namespace flame_hip::host;

static int fails = 0;
#define EXPECT(cond, ...)                       \
  do {                                          \
    if (!(cond)) {                              \
      std::printf("FAILED %s: ", #cond);        \
      std::printf(__VA_ARGS__);                 \
      std::printf("\n");                        \
      ++fails;                                  \
    }                                           \
  } while (0)

// ---- the record as it was ---------------------------------------------------------------------------------------------------
struct Loose {
  int32_t tris_T = -1;
  uint64_t tris_topo = ~0ull;
  uint64_t tris_gen = 0, keys_gen = 0;
  bool tvalid_have = false;
  uint64_t tvalid_gen = 0, tvalid_topo = 0;
  int32_t tvalid_T = -1;
};

// what the four gates answered: debug_images_begin / debug_wireframe_begin's "resident triangles of this topology", from_keys of
// debug_images_begin (read only behind the first), the validity == 2 test of debug_wireframe_begin (likewise), and
// mesh_outputs_begin(triangles = NULL)'s test
struct Gates {
  bool current, keys, validity, matches;
  bool operator==(const Gates& o) const { return current == o.current && keys == o.keys && validity == o.validity && matches == o.matches; }
};
static Gates gates(const Loose& c, int32_t T, uint64_t topo) {
  Gates g;
  g.current = !(c.tris_T < 0 || c.tris_topo != topo);
  g.keys = g.current && (c.keys_gen != 0 && c.keys_gen == c.tris_gen);
  g.validity = g.current && (c.tvalid_have && c.tvalid_gen == c.tris_gen && c.tvalid_T == c.tris_T && c.tvalid_topo == topo);
  g.matches = !(c.tris_T != T || c.tris_topo != topo);
  return g;
}
static Gates gates(const ResidentTris& r, int32_t T, uint64_t topo) {
  Gates g;
  g.current = r.current(topo);
  g.keys = g.current && r.keys_name_winners();
  g.validity = r.validity_current(topo);
  g.matches = r.matches(T, topo);
  return g;
}

// ---- the entry points, on both records ----------------------------------------------------------------------------------------
enum Kind {
  kBegin,          // interpolate_mesh_begin
  kSync,           // interpolate_mesh, succeeded
  kSyncFailEarly,  // ... failed in its argument checks or its buffers: nothing was uploaded
  kSyncFailLate,   // ... failed behind the upload
  kArrays,         // interpolate_mesh_arrays
  kArraysFailEarly,
  kMeshOwnList,    // mesh_outputs_begin(triangles != NULL)
  kMeshResident,   // mesh_outputs_begin(triangles = NULL); refused (and nothing changes) unless its gate lets it in
  kKinds
};
struct Op {
  Kind kind;
  int32_t T;
  uint64_t topo;  // ctx->topo at the call
  bool masked;
};

// returns false where the call was refused by its gate
static bool apply(Loose& c, const Op& o) {
  switch (o.kind) {
    case kBegin:
      c.tris_gen++, c.keys_gen = o.masked ? 0 : c.tris_gen;
      c.tris_T = o.T, c.tris_topo = o.topo;
      return true;
    case kSync:
    case kSyncFailLate: {
      c.tris_gen++, c.keys_gen = o.masked ? 0 : c.tris_gen;  // (interpolate_common)
      const int rc = o.kind == kSyncFailLate;
      c.tris_T = rc ? -1 : o.T, c.tris_topo = o.topo;
      return true;
    }
    case kSyncFailEarly:
      c.tris_T = -1, c.tris_topo = o.topo;  // (tris_T = rc ? -1 : T)
      return true;
    case kArrays:
      c.tris_T = -1;
      c.tris_gen++, c.keys_gen = o.masked ? 0 : c.tris_gen;  // (interpolate_common)
      return true;
    case kArraysFailEarly:
      c.tris_T = -1;
      return true;
    case kMeshOwnList:
      c.tris_T = o.T, c.tris_topo = o.topo;
      c.tris_gen++;
      c.tvalid_have = true, c.tvalid_gen = c.tris_gen, c.tvalid_T = o.T, c.tvalid_topo = o.topo;
      return true;
    case kMeshResident:
      if (c.tris_T != o.T || c.tris_topo != o.topo) return false;
      c.tvalid_have = true, c.tvalid_gen = c.tris_gen, c.tvalid_T = o.T, c.tvalid_topo = o.topo;
      return true;
    default: return false;
  }
}
static bool apply(ResidentTris& r, const Op& o) {
  switch (o.kind) {
    case kBegin:
    case kSync: r.uploaded(o.T, o.topo, o.masked); return true;
    case kSyncFailLate: r.uploaded(o.T, o.topo, o.masked), r.none_resident(); return true;
    case kSyncFailEarly:
    case kArraysFailEarly: r.none_resident(); return true;
    case kArrays: r.none_resident(), r.uploaded_foreign(o.masked); return true;
    case kMeshOwnList: r.uploaded_unrasterised(o.T, o.topo), r.validity_written(); return true;
    case kMeshResident:
      if (!r.matches(o.T, o.topo)) return false;
      r.validity_written();
      return true;
    default: return false;
  }
}

// ---- the named sequences, expectations by hand --------------------------------------------------------------------------------
struct Step {
  Op op;
  bool allowed;
  Gates want;  // asked with (T, topo) = kAskT, kAskTopo
};
static constexpr int32_t kAskT = 7;
static constexpr uint64_t kAskTopo = 4;

static void run_sequence(const char* what, const std::vector<Step>& steps) {
  Loose c;
  ResidentTris r;
  int i = 0;
  for (const Step& s : steps) {
    const bool ok_c = apply(c, s.op), ok_r = apply(r, s.op);
    EXPECT(ok_c == s.allowed && ok_r == s.allowed, "%s, step %d: allowed %d (as it was) / %d (now), expected %d", what, i, ok_c, ok_r, s.allowed);
    const Gates gc = gates(c, kAskT, kAskTopo), gr = gates(r, kAskT, kAskTopo);
    EXPECT(gc == s.want, "%s, step %d, as it was: current %d keys %d validity %d matches %d", what, i, gc.current, gc.keys, gc.validity, gc.matches);
    EXPECT(gr == s.want, "%s, step %d, now: current %d keys %d validity %d matches %d", what, i, gr.current, gr.keys, gr.validity, gr.matches);
    ++i;
  }
}

static void test_named_sequences() {
  const int32_t T = kAskT;
  const uint64_t A = kAskTopo, B = 5;
  //                                                                  current keys  validity matches
  {
    Loose c;
    ResidentTris r;
    const Gates none{false, false, false, false};
    EXPECT(gates(c, T, A) == none && gates(r, T, A) == none, "a fresh context: nothing is current");
    EXPECT(r.T() == -1, "a fresh context: T %d", r.T());
  }
  run_sequence("unmasked begin: the keys name winners", {{{kBegin, T, A, false}, true, {true, true, false, true}}});
  run_sequence("masked begin: they do not", {{{kBegin, T, A, true}, true, {true, false, false, true}}});
  run_sequence("mesh_outputs_begin with new triangles: triangles and validity current, keys stale",
               {{{kBegin, T, A, false}, true, {true, true, false, true}},
                {{kMeshOwnList, T, A, false}, true, {true, false, true, true}}});
  run_sequence("mesh_outputs_begin(NULL) after a re-upload of the same T: allowed, the validity current again",
               {{{kBegin, T, A, false}, true, {true, true, false, true}},
                {{kMeshResident, T, A, false}, true, {true, true, true, true}},
                {{kSync, T, A, false}, true, {true, true, false, true}},  // the same T, other triangles: the validity speaks of the old ones
                {{kMeshResident, T, A, false}, true, {true, true, true, true}},
                {{kMeshResident, T - 1, A, false}, false, {true, true, true, true}},    // another T: refused, nothing changes
                {{kMeshResident, T, B, false}, false, {true, true, true, true}}});      // another topology: refused
  run_sequence("foreign arrays: nothing current, though the upload count and the key count agree",
               {{{kBegin, T, A, false}, true, {true, true, false, true}},
                {{kMeshResident, T, A, false}, true, {true, true, true, true}},
                {{kArrays, T, A, false}, true, {false, false, false, false}},
                {{kMeshResident, T, A, false}, false, {false, false, false, false}},
                {{kMeshOwnList, T, A, false}, true, {true, false, true, true}}});       // ... and the foreign key image is not taken for the graph's
  run_sequence("foreign arrays that fail in their argument checks: no resident triangles either",
               {{{kSync, T, A, false}, true, {true, true, false, true}}, {{kArraysFailEarly, 0, A, false}, true, {false, false, false, false}}});
  run_sequence("a topology change: nothing current",
               {{{kBegin, T, B, false}, true, {false, false, false, false}},  // (asked for topology A throughout)
                {{kMeshOwnList, T, B, false}, true, {false, false, false, false}},
                {{kBegin, T, A, true}, true, {true, false, false, true}},
                {{kMeshResident, T, A, false}, true, {true, false, true, true}}});
  run_sequence("a failed synchronous interpolate: not current, wherever it failed",
               {{{kBegin, T, A, false}, true, {true, true, false, true}},
                {{kSyncFailEarly, T, A, false}, true, {false, false, false, false}},
                {{kSync, T, A, true}, true, {true, false, false, true}},
                {{kSyncFailLate, T, A, false}, true, {false, false, false, false}},
                {{kMeshResident, T, A, false}, false, {false, false, false, false}}});
  run_sequence("no triangles at all are triangles too", {{{kBegin, 0, A, false}, true, {true, true, false, false}},
                                                          {{kMeshResident, 0, A, false}, true, {true, true, true, false}}});
}

// ---- every entry point from every reachable state -----------------------------------------------------------------------------
// The loose members up to what the gates can tell apart: the counters only ever meet the upload count or have fallen behind it for good.
using Canon = std::tuple<int32_t, uint64_t, int, bool, bool, int32_t, uint64_t>;
static Canon canon(const Loose& c) {
  const int keys = c.keys_gen == 0 ? 0 : c.keys_gen == c.tris_gen ? 1 : 2;
  return Canon{c.tris_T, c.tris_T < 0 ? 0 : c.tris_topo, keys, c.tvalid_have, c.tvalid_have && c.tvalid_gen == c.tris_gen,
               c.tvalid_have ? c.tvalid_T : -1, c.tvalid_have ? c.tvalid_topo : 0};
}

static std::vector<Op> all_ops() {
  std::vector<Op> ops;
  for (int32_t T : {0, 3})
    for (uint64_t topo : {uint64_t(1), uint64_t(2)}) {
      for (bool masked : {false, true})
        for (Kind k : {kBegin, kSync, kSyncFailLate}) ops.push_back(Op{k, T, topo, masked});
      ops.push_back(Op{kMeshOwnList, T, topo, false});
      ops.push_back(Op{kMeshResident, T, topo, false});
    }
  for (uint64_t topo : {uint64_t(1), uint64_t(2)}) ops.push_back(Op{kSyncFailEarly, 3, topo, false});
  for (bool masked : {false, true}) ops.push_back(Op{kArrays, 3, 1, masked});
  ops.push_back(Op{kArraysFailEarly, 3, 1, false});
  return ops;
}

static long walked = 0;
static void walk(const std::vector<Op>& ops, const Loose& c, const ResidentTris& r, int depth, int max_depth, std::vector<std::set<Canon>>* seen) {
  (*seen)[depth].insert(canon(c));
  if (depth == max_depth) return;
  for (const Op& o : ops) {
    Loose c2 = c;
    ResidentTris r2 = r;
    const bool ok_c = apply(c2, o), ok_r = apply(r2, o);
    ++walked;
    bool same = ok_c == ok_r && r2.T() == c2.tris_T;
    for (int32_t T : {0, 3})
      for (uint64_t topo : {uint64_t(1), uint64_t(2)}) same = same && gates(c2, T, topo) == gates(r2, T, topo);
    if (!same) {
      EXPECT(same, "walk: depth %d, entry point %d (T %d, topology %d, masked %d): the two records answer differently", depth, (int)o.kind,
             (int)o.T, (int)o.topo, (int)o.masked);
      return;
    }
    walk(ops, c2, r2, depth + 1, max_depth, seen);
  }
}

static void test_every_transition_from_every_state() {
  const int max_depth = 4;
  std::vector<std::set<Canon>> seen(max_depth + 1);
  walk(all_ops(), Loose{}, ResidentTris{}, 0, max_depth, &seen);
  std::set<Canon> before;
  for (int d = 0; d < max_depth; ++d) before.insert(seen[d].begin(), seen[d].end());
  size_t fresh = 0;
  for (const Canon& s : seen[max_depth]) fresh += before.count(s) == 0;
  // no state first shows up at the last depth: every reachable state was met one level earlier at the latest, and every entry
  // point was taken from it
  EXPECT(fresh == 0, "walk: %zu state(s) first reached at depth %d -- walk deeper", fresh, max_depth);
  EXPECT(before.size() > 20, "walk: only %zu states", before.size());
  std::printf("side stage: %ld transitions from %zu states compared\n", walked, before.size());
}

// ---- layouts --------------------------------------------------------------------------------------------------------------------
struct Region {
  const char* name;
  size_t off, bytes, align;
};
static void check_regions(const char* what, const std::vector<Region>& rs, size_t total) {
  for (size_t i = 0; i < rs.size(); ++i) {
    const Region& a = rs[i];
    EXPECT(a.off % a.align == 0, "%s: %s at %zu is not %zu-byte aligned", what, a.name, a.off, a.align);
    EXPECT(a.off + a.bytes <= total, "%s: %s [%zu, %zu) leaves the buffer of %zu", what, a.name, a.off, a.off + a.bytes, total);
    for (size_t j = i + 1; j < rs.size(); ++j) {
      const Region& b = rs[j];
      const bool apart = a.bytes == 0 || b.bytes == 0 || a.off + a.bytes <= b.off || b.off + b.bytes <= a.off;
      EXPECT(apart, "%s: %s [%zu, %zu) and %s [%zu, %zu) overlap", what, a.name, a.off, a.off + a.bytes, b.name, b.off, b.off + b.bytes);
    }
  }
}

static void test_layouts() {
  const int shapes[3][2] = {{1, 1}, {3, 5}, {50, 70}};
  char what[160];
  for (const auto& sh : shapes) {
    const int rows = sh[0], cols = sh[1];
    const size_t n = (size_t)rows * (size_t)cols;
    for (int32_t V : {0, 1, 5})
      for (int32_t T : {0, 1, 7})
        for (bool want_map : {false, true}) {
          std::snprintf(what, sizeof(what), "mesh_layout(V %d, T %d, %d x %d, map %d)", V, T, rows, cols, (int)want_map);
          const MeshLayout m = mesh_layout(V, T, rows, cols, want_map);
          check_regions(what, {{"normals", m.normals, sizeof(float) * 3 * (size_t)V, 4},
                               {"vtx_idepth", m.idepth, sizeof(float) * (size_t)V, 4},
                               {"n_valid, coverage", m.counts, 2 * sizeof(int32_t), 4},
                               {"filtered map", m.map, want_map ? sizeof(float) * n : 0, 4},
                               {"tri_valid", m.valid, (size_t)T, 1}},
                        m.total);
        }
    for (int flags = 0; flags < 8; ++flags) {
      const bool want_id = flags & 1, want_n = flags & 2, host_gray = flags & 4;
      std::snprintf(what, sizeof(what), "debug_layout(%d x %d, idepth %d, normals %d, host image %d)", rows, cols, (int)want_id, (int)want_n, (int)host_gray);
      const DebugLayout d = debug_layout(rows, cols, want_id, want_n, host_gray);
      check_regions(what, {{"idepth image", d.idimg, want_id ? 3 * n : 0, 16},
                           {"normals image", d.nimg, want_n ? 3 * n : 0, 16},
                           {"w1 map", d.w1, want_n ? sizeof(float) * n : 0, 16},
                           {"w2 map", d.w2, want_n ? sizeof(float) * n : 0, 16},
                           {"grey image", d.gray, host_gray ? n : 0, 16}},
                    d.total);
    }
    for (bool host_gray : {false, true}) {
      std::snprintf(what, sizeof(what), "wire_layout(%d x %d, host image %d)", rows, cols, (int)host_gray);
      const WireLayout w = wire_layout(rows, cols, host_gray);
      check_regions(what, {{"picture", w.img, 3 * n, 16}, {"counters", w.counts, kWireCountBytes, 16}, {"grey image", w.gray, host_gray ? n : 0, 16}},
                    w.total);
    }
  }
  EXPECT(up16(0) == 0 && up16(1) == 16 && up16(16) == 16 && up16(17) == 32, "up16");
}

// ---- triangle indices -------------------------------------------------------------------------------------------------------------
static void test_triangles_in_range() {
  EXPECT(triangles_in_range(nullptr, 0, 5), "no triangles, no list");
  EXPECT(triangles_in_range(nullptr, 0, 0), "no triangles, no vertices");
  const int32_t good[6] = {0, 1, 2, 4, 3, 0};
  EXPECT(triangles_in_range(good, 2, 5), "every index below V");
  EXPECT(!triangles_in_range(good, 2, 4), "an index equal to V");
  EXPECT(triangles_in_range(good, 1, 3), "... in a triangle behind the T the caller gave");
  const int32_t negative[6] = {0, 1, 2, 2, -1, 0};
  EXPECT(!triangles_in_range(negative, 2, 5), "a negative index");
  EXPECT(triangles_in_range(negative, 1, 5), "... behind T");
  EXPECT(!triangles_in_range(good, 1, 0), "triangles of a graph without vertices");
}

int main() {
  test_named_sequences();
  test_every_transition_from_every_state();
  test_layouts();
  test_triangles_in_range();
  std::printf(fails ? "side stage: %d check(s) FAILED\n" : "side stage: all ok\n", fails);
  return fails ? 1 : 0;
}
