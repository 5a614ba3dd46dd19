// DeviceGraph::meshOutputsBegin / End (include/flame_hip/nltgv2_l1_graph_regularizer.hpp) round trip: reads a case the Python test
// dumped (graph, triangles, Kinv, and the outputs the Python mirror obtained for it), uploads the graph through the facade, asks for
// the mesh outputs -- once with the triangles, once with the ones interpolateMeshBegin left on the device -- and compares bit for bit.
//   mesh_outputs_test <case file>      exit 0: all equal; 77: no usable HIP device; 1: a difference or a bad file
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "flame_hip/nltgv2_l1_graph_regularizer.hpp"

namespace reg = flame::optimizers::nltgv2_l1_graph_regularizer::hip;

template <class T>
static bool take(std::FILE* f, std::vector<T>* v, size_t n) {
  v->resize(n);
  return n == 0 || std::fread(v->data(), sizeof(T), n, f) == n;
}

static bool same(const void* a, const void* b, size_t bytes, const char* what) {
  if (bytes == 0 || std::memcmp(a, b, bytes) == 0) return true;
  std::printf("FAIL: %s differs\n", what);
  return false;
}

int main(int argc, char** argv) {
  reg::MeshFilterParams defaults;
  if (defaults.do_oblique_triangle_filter != 1 || defaults.oblique_normal_thresh != 1.39626f || defaults.edge_length_thresh != 0.333f ||
      defaults.min_triangle_idepth != 0.01f) {
    std::printf("FAIL: defaults\n");
    return 1;
  }
  if (argc < 2) {
    std::printf("usage: mesh_outputs_test <case file>\n");
    return 1;
  }
  try {
    reg::DeviceGraph d(0);
    std::FILE* f = std::fopen(argv[1], "rb");
    char magic[4];
    int32_t hdr[6];  // V, E, T, rows, cols, n_valid
    float scale = 0.0f;
    int32_t coverage = 0;
    std::vector<float> Kinv, pos, x, alpha, beta, idepth, normals, fmap;
    std::vector<int32_t> src, dst, tris;
    std::vector<uint8_t> valid;
    reg::MeshFilterParams filter;
    bool ok = f && std::fread(magic, 1, 4, f) == 4 && std::memcmp(magic, "MSH1", 4) == 0 && std::fread(hdr, sizeof(int32_t), 6, f) == 6 &&
              std::fread(&scale, sizeof(float), 1, f) == 1 && std::fread(&coverage, sizeof(int32_t), 1, f) == 1 &&
              std::fread(&filter, sizeof(filter), 1, f) == 1;
    if (!ok) {
      std::printf("FAIL: cannot read %s\n", argv[1]);
      return 1;
    }
    const size_t V = hdr[0], E = hdr[1], T = hdr[2], n = static_cast<size_t>(hdr[3]) * hdr[4];
    ok = take(f, &Kinv, 9) && take(f, &pos, 2 * V) && take(f, &x, V) && take(f, &src, E) && take(f, &dst, E) && take(f, &alpha, E) &&
         take(f, &beta, E) && take(f, &tris, 3 * T) && take(f, &idepth, V) && take(f, &normals, 3 * V) && take(f, &valid, T) && take(f, &fmap, n);
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
    for (int pass = 0; pass < 2; ++pass) {
      if (pass == 1) d.interpolateMeshBegin(tris, hdr[3], hdr[4], scale);
      d.meshOutputsBegin(pass == 0 ? &tris : nullptr, T, Kinv.data(), filter, hdr[3], hdr[4], scale, true);
      const reg::MeshOutputs m = d.meshOutputsEnd();
      ok = m.num_vertices == V && m.num_triangles == T && m.num_valid_triangles == hdr[5] && m.filtered_coverage == coverage &&
           m.rows == hdr[3] && m.cols == hdr[4];
      if (!ok) std::printf("FAIL: counts (%d valid, coverage %d)\n", m.num_valid_triangles, m.filtered_coverage);
      ok = same(m.vtx_idepths, idepth.data(), sizeof(float) * V, "vtx_idepths") && ok;
      ok = same(m.vtx_normals, normals.data(), sizeof(float) * 3 * V, "vtx_normals") && ok;
      ok = same(m.tri_validity, valid.data(), T, "tri_validity") && ok;
      ok = same(m.filtered_idepthmap, fmap.data(), sizeof(float) * n, "filtered idepthmap") && ok;
      if (pass == 1) {
        const float* dense = nullptr;
        d.interpolateMeshEnd(&dense);
      }
      if (!ok) return 1;
      std::printf("mesh outputs, %s: ok\n", pass == 0 ? "triangles passed" : "resident triangles");
    }
    bool threw = false;
    try {
      d.meshOutputsBegin(nullptr, T + 1, Kinv.data(), filter, hdr[3], hdr[4], scale, false);
    } catch (const flame_hip::Error& e) {
      threw = e.status == FLAME_NLTGV2_ERR_INVALID_ARG;
    }
    if (!threw) {
      std::printf("FAIL: another T than the resident one was accepted\n");
      return 1;
    }
    std::printf("wrong T refused: ok\n");
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
