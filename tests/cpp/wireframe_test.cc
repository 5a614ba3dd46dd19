// DeviceGraph::debugWireframeBegin / End (include/flame_hip/) round trip: reads a case the Python test dumped (graph, triangles, a
// triangle validity, the grey image in a buffer wider than the image, and the pictures the Python mirror obtained for them), goes
// through the facade and compares byte for byte.
//   wireframe_test <case file>      exit 0: all equal; 77: no usable HIP device; 1: a difference or a bad file
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
  reg::WireframeParams defaults;
  if (defaults.scene_color_scale != 1.0f || defaults.debug_flip_images != 0 || defaults.validity != 0) {
    std::printf("FAIL: defaults\n");
    return 1;
  }
  if (argc < 2) {
    std::printf("usage: wireframe_test <case file>\n");
    return 1;
  }
  try {
    reg::DeviceGraph d(0);
    std::FILE* f = std::fopen(argv[1], "rb");
    char magic[4];
    int32_t hdr[9];  // V, E, T, rows, cols, step, flip, lines_drawn (all valid), lines_drawn (masked)
    float sc[2];     // graph_scale, scene_color_scale
    bool ok = f && std::fread(magic, 1, 4, f) == 4 && std::memcmp(magic, "WIR1", 4) == 0 && std::fread(hdr, sizeof(int32_t), 9, f) == 9 &&
              std::fread(sc, sizeof(float), 2, f) == 2;
    if (!ok) {
      std::printf("FAIL: cannot read %s\n", argv[1]);
      return 1;
    }
    const size_t V = hdr[0], E = hdr[1], T = hdr[2], n = static_cast<size_t>(hdr[3]) * hdr[4];
    const int rows = hdr[3], cols = hdr[4], step = hdr[5];
    std::vector<float> pos, x, alpha, beta;
    std::vector<int32_t> src, dst, tris;
    std::vector<uint8_t> gray, tri_valid, img_all, img_masked;
    ok = take(f, &pos, 2 * V) && take(f, &x, V) && take(f, &src, E) && take(f, &dst, E) && take(f, &alpha, E) && take(f, &beta, E) &&
         take(f, &tris, 3 * T) && take(f, &gray, static_cast<size_t>(rows) * step) && take(f, &tri_valid, T) && take(f, &img_all, 3 * n) &&
         take(f, &img_masked, 3 * n);
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
    reg::WireframeParams wp;
    wp.scene_color_scale = sc[1], wp.debug_flip_images = hdr[6];
    const uint8_t* img = gray.data() + 7;  // (the image starts 7 bytes into each row of the buffer)

    // beside the map: interpolateMeshBegin, debugWireframeBegin, the two Ends
    d.interpolateMeshBegin(tris, rows, cols, sc[0]);
    d.debugWireframeBegin(img, nullptr, step, nullptr, wp, rows, cols, sc[0]);
    const float* dense = nullptr;
    d.interpolateMeshEnd(&dense);
    reg::Wireframe out = d.debugWireframeEnd();
    ok = out.rows == rows && out.cols == cols && out.lines_drawn == hdr[7] && out.lines_skipped == 0;
    if (!ok) std::printf("FAIL: size or counters (%d x %d, %d drawn, %d skipped)\n", out.rows, out.cols, out.lines_drawn, out.lines_skipped);
    ok = same(out.debug_img_wireframe, img_all.data(), 3 * n, "debug_img_wireframe") && ok;
    if (!ok) return 1;
    std::printf("wireframe, every triangle valid: ok\n");

    wp.validity = 1;
    d.debugWireframeBegin(img, nullptr, step, tri_valid.data(), wp, rows, cols, sc[0]);
    out = d.debugWireframeEnd();
    ok = out.lines_drawn == hdr[8] && out.lines_skipped == 0;
    if (!ok) std::printf("FAIL: counters (%d drawn, %d skipped)\n", out.lines_drawn, out.lines_skipped);
    ok = same(out.debug_img_wireframe, img_masked.data(), 3 * n, "debug_img_wireframe (tri_validity)") && ok;
    if (!ok) return 1;
    std::printf("wireframe, a triangle validity: ok\n");

    bool threw = false;
    try {
      d.debugWireframeBegin(img, nullptr, step, nullptr, wp, rows, cols, sc[0]);  // validity 1 without an array
    } catch (const flame_hip::Error& e) {
      threw = e.status == FLAME_NLTGV2_ERR_INVALID_ARG;
    }
    if (!threw) {
      std::printf("FAIL: validity 1 without an array was accepted\n");
      return 1;
    }
    std::printf("validity without its array refused: ok\n");
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
