// DeviceGraph::keepMesh / dropMesh / fuseViewsBegin / End (include/flame_hip/nltgv2_l1_graph_regularizer.hpp) round trip: reads a case the
// Python test dumped (graph, triangles, three cameras, the vote's parameters, and what the Python mirror obtained for them), goes through
// the facade -- interpolateMesh, keepMesh twice, fuseViewsBegin, fuseViewsEnd -- and compares byte for byte.
//   fuse_views_test <case file>      exit 0: all equal; 77: no usable HIP device; 1: a difference or a bad file
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
  reg::FuseParams defaults;
  if (defaults.n_sources != 1 || defaults.sources[0].slot != -1 || defaults.sources[7].weight != 1.0f || defaults.sources[3].R[4] != 1.0f ||
      defaults.sources[3].R[1] != 0.0f || defaults.sources[5].graph_scale != 1.0f || defaults.K_dst[8] != 1.0f || defaults.near_depth != 0.0f ||
      defaults.rel_tol != 0.05f || defaults.min_support != 1 || defaults.want_fused != 1 || defaults.want_masks != 1 || defaults.want_spread != 1 ||
      defaults.want_layers != 0 || defaults.copy_out != 1 || sizeof(reg::FuseParams) != sizeof(flame_nltgv2_fuse_params)) {
    std::printf("FAIL: defaults\n");
    return 1;
  }
  if (argc < 2) {
    std::printf("usage: fuse_views_test <case file>\n");
    return 1;
  }
  try {
    reg::DeviceGraph d(0);
    std::FILE* f = std::fopen(argv[1], "rb");
    char magic[4];
    int32_t hdr[8];  // V, E, T, source rows, source cols, target rows, target cols, min_support
    bool ok = f && std::fread(magic, 1, 4, f) == 4 && std::memcmp(magic, "FUS1", 4) == 0 && std::fread(hdr, sizeof(int32_t), 8, f) == 8;
    if (!ok) {
      std::printf("FAIL: cannot read %s\n", argv[1]);
      return 1;
    }
    const size_t V = hdr[0], E = hdr[1], T = hdr[2], n = static_cast<size_t>(hdr[5]) * hdr[6];
    const int rows = hdr[5], cols = hdr[6], N = 3;
    // 3 x (Kinv_src 9 | R 9 | t 3 | weight | graph_scale) | K_dst 9 | rel_tol
    std::vector<float> cam, pos, x, alpha, beta, fused, spread, layers;
    std::vector<int32_t> src, dst, tris, counts;
    std::vector<uint8_t> present, inlier;
    ok = take(f, &cam, 3 * 23 + 10) && take(f, &pos, 2 * V) && take(f, &x, V) && take(f, &src, E) && take(f, &dst, E) && take(f, &alpha, E) &&
         take(f, &beta, E) && take(f, &tris, 3 * T) && take(f, &fused, n) && take(f, &present, n) && take(f, &inlier, n) && take(f, &spread, n) &&
         take(f, &layers, N * n) && take(f, &counts, 32);
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

    // two pose-frames keep the mesh (at their own scales); the third source is the live mesh
    reg::FuseParams p;
    p.n_sources = N;
    for (int s = 0; s < N; ++s) {
      const float* c = cam.data() + 23 * s;
      std::memcpy(p.sources[s].Kinv_src, c, sizeof(p.sources[s].Kinv_src));
      std::memcpy(p.sources[s].R, c + 9, sizeof(p.sources[s].R));
      std::memcpy(p.sources[s].t, c + 18, sizeof(p.sources[s].t));
      p.sources[s].weight = c[21];
      if (s < 2) d.keepMesh(s + 4, c[22]), p.sources[s].slot = s + 4;
      else p.sources[s].slot = -1, p.sources[s].graph_scale = c[22];
    }
    std::memcpy(p.K_dst, cam.data() + 69, sizeof(p.K_dst));
    p.rel_tol = cam[78], p.min_support = hdr[7], p.want_layers = 1;
    d.fuseViewsBegin(p, rows, cols);
    reg::FusedView out = d.fuseViewsEnd();
    ok = out.rows == rows && out.cols == cols && out.num_sources == N;
    ok = same(out.idepthmap, fused.data(), sizeof(float) * n, "fused map") && ok;
    ok = same(out.present_mask, present.data(), n, "present mask") && ok;
    ok = same(out.inlier_mask, inlier.data(), n, "inlier mask") && ok;
    ok = same(out.spread, spread.data(), sizeof(float) * n, "spread") && ok;
    ok = same(out.layers, layers.data(), sizeof(float) * n * N, "layers") && ok;
    ok = same(&out.counts, counts.data(), sizeof(out.counts), "counters") && ok;
    if (!ok) return 1;
    std::printf("everything to the host: ok\n");

    // on the device only: the counters travel, nothing else
    p.copy_out = 0;
    d.fuseViewsBegin(p, rows, cols);
    out = d.fuseViewsEnd();
    ok = !out.idepthmap && !out.present_mask && !out.inlier_mask && !out.spread && !out.layers && out.idepthmap_device && out.present_mask_device &&
         out.inlier_mask_device && out.spread_device && out.layers_device &&
         same(&out.counts, counts.data(), sizeof(out.counts), "counters with copy_out = 0");
    if (!ok) {
      std::printf("FAIL: copy_out = 0\n");
      return 1;
    }
    std::printf("device only: ok\n");

    bool threw = false;
    try {
      p.min_support = N + 1;
      d.fuseViewsBegin(p, rows, cols);
    } catch (const flame_hip::Error& e) {
      threw = e.status == FLAME_NLTGV2_ERR_INVALID_ARG;
    }
    out = d.fuseViewsEnd();  // (the refused call left the outputs of the one before)
    if (!threw || !same(&out.counts, counts.data(), sizeof(out.counts), "counters after a refused call")) {
      std::printf("FAIL: min_support beyond the number of sources was accepted\n");
      return 1;
    }
    std::printf("a min_support beyond the sources refused: ok\n");

    threw = false;
    p.min_support = hdr[7];
    d.dropMesh(5);
    try {
      d.fuseViewsBegin(p, rows, cols);
    } catch (const flame_hip::Error& e) {
      threw = e.status == FLAME_NLTGV2_ERR_INVALID_ARG;
    }
    if (!threw) {
      std::printf("FAIL: a dropped slot was accepted\n");
      return 1;
    }
    std::printf("a dropped slot refused: ok\n");
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
