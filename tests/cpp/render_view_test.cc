// DeviceGraph::renderViewBegin / End (include/flame_hip/nltgv2_l1_graph_regularizer.hpp) round trip: reads a case the Python test dumped
// (graph, triangles, a validity mask, the camera, and what the Python mirror obtained for them), goes through the facade --
// interpolateMesh, renderViewBegin, renderViewEnd -- and compares byte for byte.
//   render_view_test <case file>      exit 0: all equal; 77: no usable HIP device; 1: a difference or a bad file
#include <cstdio>
#include <cstring>
#include <vector>

#include "flame_hip/nltgv2_l1_graph_regularizer.hpp"

namespace reg = flame::optimizers::nltgv2_l1_graph_regularizer::hip;

template <class T>
static bool take(std::FILE* f, std::vector<T>* v, size_t n) {
  v->resize(n);
  return n == 0 || std::fread(v->data(), sizeof(T), n, f) == n;
}

static bool same(const void* a, const void* b, size_t bytes, const char* what) {
  if (a && (bytes == 0 || std::memcmp(a, b, bytes) == 0)) return true;
  std::printf("FAIL: %s differs\n", what);
  return false;
}

int main(int argc, char** argv) {
  reg::ViewParams defaults;
  if (defaults.Kinv_src[0] != 1.0f || defaults.K_dst[4] != 1.0f || defaults.R[8] != 1.0f || defaults.R[1] != 0.0f || defaults.t[2] != 0.0f ||
      defaults.near_depth != 0.0f || defaults.validity != 0 || defaults.want_map != 1 || defaults.want_tri_index != 1 || defaults.copy_out != 1 ||
      sizeof(reg::ViewParams) != sizeof(flame_nltgv2_view_params)) {
    std::printf("FAIL: defaults\n");
    return 1;
  }
  if (argc < 2) {
    std::printf("usage: render_view_test <case file>\n");
    return 1;
  }
  try {
    reg::DeviceGraph d(0);
    std::FILE* f = std::fopen(argv[1], "rb");
    char magic[4];
    int32_t hdr[7];  // V, E, T, source rows, source cols, target rows, target cols
    bool ok = f && std::fread(magic, 1, 4, f) == 4 && std::memcmp(magic, "RVW1", 4) == 0 && std::fread(hdr, sizeof(int32_t), 7, f) == 7;
    if (!ok) {
      std::printf("FAIL: cannot read %s\n", argv[1]);
      return 1;
    }
    const size_t V = hdr[0], E = hdr[1], T = hdr[2], n = static_cast<size_t>(hdr[5]) * hdr[6];
    const int rows = hdr[5], cols = hdr[6];
    std::vector<float> cam, pos, x, alpha, beta, map_all, map_masked;
    std::vector<int32_t> src, dst, tris, idx_all, idx_masked, counts_all, counts_masked;
    std::vector<uint8_t> mask;
    ok = take(f, &cam, 31) && take(f, &pos, 2 * V) && take(f, &x, V) && take(f, &src, E) && take(f, &dst, E) && take(f, &alpha, E) &&
         take(f, &beta, E) && take(f, &tris, 3 * T) && take(f, &mask, T) && take(f, &map_all, n) && take(f, &idx_all, n) &&
         take(f, &counts_all, 4) && take(f, &map_masked, n) && take(f, &idx_masked, n) && take(f, &counts_masked, 4);
    std::fclose(f);
    if (!ok) {
      std::printf("FAIL: short file\n");
      return 1;
    }
    flame_hip::FlatGraph g;
    g.vertices.resize(V), g.edges.resize(E);
    for (size_t v = 0; v < V; ++v) {
      g.vertices[v].pos_x = pos[2 * v], g.vertices[v].pos_y = pos[2 * v + 1];
      g.vertices[v].x = g.vertices[v].x_bar = g.vertices[v].data_term = x[v];
    }
    for (size_t e = 0; e < E; ++e) g.edges[e].source = src[e], g.edges[e].target = dst[e], g.edges[e].alpha = alpha[e], g.edges[e].beta = beta[e];
    d.upload(g);
    std::vector<float> dense(static_cast<size_t>(hdr[3]) * hdr[4]);
    d.interpolateMesh(tris, hdr[3], hdr[4], 1.0f, dense.data());

    // every triangle valid, everything to the host
    reg::ViewParams p;  // Kinv_src | K_dst | R | t | near_depth
    std::memcpy(p.Kinv_src, cam.data(), sizeof(p.Kinv_src));
    std::memcpy(p.K_dst, cam.data() + 9, sizeof(p.K_dst));
    std::memcpy(p.R, cam.data() + 18, sizeof(p.R));
    std::memcpy(p.t, cam.data() + 27, sizeof(p.t));
    p.near_depth = cam[30];
    reg::RenderedView out = d.renderView(p, nullptr, rows, cols, 1.0f);
    ok = out.rows == rows && out.cols == cols && out.num_triangles == static_cast<int>(T);
    ok = same(out.idepthmap, map_all.data(), sizeof(float) * n, "map") && ok;
    ok = same(out.tri_index, idx_all.data(), sizeof(int32_t) * n, "owner indices") && ok;
    ok = same(&out.counts, counts_all.data(), sizeof(out.counts), "counters") && ok;
    if (!ok) return 1;
    std::printf("all valid: ok\n");

    // a host validity mask, begin and end apart
    p.validity = 1;
    d.renderViewBegin(p, mask.data(), rows, cols, 1.0f);
    out = d.renderViewEnd();
    ok = same(out.idepthmap, map_masked.data(), sizeof(float) * n, "masked map");
    ok = same(out.tri_index, idx_masked.data(), sizeof(int32_t) * n, "masked owner indices") && ok;
    ok = same(&out.counts, counts_masked.data(), sizeof(out.counts), "masked counters") && ok;
    if (!ok) return 1;
    std::printf("masked: ok\n");

    // on the device only: the counters travel, nothing else
    p.copy_out = 0;
    out = d.renderView(p, mask.data(), rows, cols, 1.0f);
    ok = !out.idepthmap && !out.tri_index && out.idepthmap_device && out.tri_index_device &&
         same(&out.counts, counts_masked.data(), sizeof(out.counts), "counters with copy_out = 0");
    if (!ok) {
      std::printf("FAIL: copy_out = 0\n");
      return 1;
    }
    std::printf("device only: ok\n");

    bool threw = false;
    try {
      d.renderViewBegin(p, mask.data(), rows, 40000, 1.0f);
    } catch (const flame_hip::Error& e) {
      threw = e.status == FLAME_NLTGV2_ERR_INVALID_ARG;
    }
    out = d.renderViewEnd();  // (the refused call left the outputs of the one before)
    if (!threw || !same(&out.counts, counts_masked.data(), sizeof(out.counts), "counters after a refused call")) {
      std::printf("FAIL: a target of 40000 columns was accepted\n");
      return 1;
    }
    std::printf("an oversized target refused: ok\n");
    return 0;
  } catch (const flame_hip::Error& e) {
    if (e.status == FLAME_NLTGV2_ERR_NO_DEVICE) {
      std::printf("%s\n", e.what());
      return 77;
    }
    std::printf("FAIL: %s\n", e.what());
    return 1;
  }
}
