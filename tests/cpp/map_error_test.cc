// DeviceGraph::mapErrorBegin / End (include/flame_hip/nltgv2_l1_graph_regularizer.hpp) round trip: reads a case the Python test dumped
// (graph, triangles, two grey images, KRKinv, Kt, a true map, and what the Python mirror obtained for them from both sources), goes
// through the facade -- interpolateMesh, mapErrorBegin, mapErrorEnd -- and compares byte for byte.
//   map_error_test <case file>      exit 0: all equal; 77: no usable HIP device; 1: a difference or a bad file
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
  reg::MapErrorParams defaults;
  if (defaults.source != FLAME_NLTGV2_MAP_ERROR_PHOTO || defaults.border != 3 || defaults.relative != 1 || defaults.win_size != 0 ||
      defaults.ptile_num != 99 || defaults.ptile_den != 100 || defaults.want_stats != 1 || defaults.want_error_map != 1 ||
      defaults.want_image != 0 || defaults.copy_out != 1 || defaults.map_device || defaults.truth_host || defaults.KRKinv[4] != 1.0f ||
      sizeof(reg::MapErrorParams) != sizeof(flame_nltgv2_map_error_params)) {
    std::printf("FAIL: defaults\n");
    return 1;
  }
  if (argc < 2) {
    std::printf("usage: map_error_test <case file>\n");
    return 1;
  }
  try {
    reg::DeviceGraph d(0);
    std::FILE* f = std::fopen(argv[1], "rb");
    char magic[4];
    int32_t hdr[7];  // V, E, T, rows, cols, border, win_size
    float sc[2];     // max_error of the PHOTO picture, max_error of the TRUTH picture
    bool ok = f && std::fread(magic, 1, 4, f) == 4 && std::memcmp(magic, "MER1", 4) == 0 && std::fread(hdr, sizeof(int32_t), 7, f) == 7 &&
              std::fread(sc, sizeof(float), 2, f) == 2;
    if (!ok) {
      std::printf("FAIL: cannot read %s\n", argv[1]);
      return 1;
    }
    const size_t V = hdr[0], E = hdr[1], T = hdr[2], n = static_cast<size_t>(hdr[3]) * hdr[4];
    const int rows = hdr[3], cols = hdr[4];
    std::vector<float> KRKinv, Kt, pos, x, alpha, beta, truth, photo_err, truth_err;
    std::vector<int32_t> src, dst, tris;
    std::vector<uint8_t> ref, cmp, photo_stats, truth_stats, photo_img, truth_img;
    ok = take(f, &KRKinv, 9) && take(f, &Kt, 3) && take(f, &pos, 2 * V) && take(f, &x, V) && take(f, &src, E) && take(f, &dst, E) &&
         take(f, &alpha, E) && take(f, &beta, E) && take(f, &tris, 3 * T) && take(f, &ref, n) && take(f, &cmp, n) && take(f, &truth, n) &&
         take(f, &photo_err, n) && take(f, &photo_stats, sizeof(flame_nltgv2_map_error_stats)) && take(f, &photo_img, 3 * n) &&
         take(f, &truth_err, n) && take(f, &truth_stats, sizeof(flame_nltgv2_map_error_stats)) && take(f, &truth_img, 3 * n);
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
    std::vector<float> dense(n);
    d.interpolateMesh(tris, rows, cols, 1.0f, dense.data());
    if (flame_nltgv2_photo_set_images(d.handle(), ref.data(), cmp.data(), rows, cols, cols) != FLAME_NLTGV2_OK) {
      std::printf("FAIL: photo_set_images\n");
      return 1;
    }

    // photometric, the resident map, the images of photo_set_images, with the picture
    reg::MapErrorParams pp;
    std::memcpy(pp.KRKinv, KRKinv.data(), sizeof(pp.KRKinv));
    std::memcpy(pp.Kt, Kt.data(), sizeof(pp.Kt));
    pp.border = hdr[5], pp.win_size = hdr[6], pp.want_image = 1, pp.max_error = sc[0];
    d.mapErrorBegin(pp, rows, cols);
    reg::MapError out = d.mapErrorEnd();
    ok = out.rows == rows && out.cols == cols && out.source == FLAME_NLTGV2_MAP_ERROR_PHOTO && out.win_size == hdr[6] && out.hist_scale == 1.0f;
    ok = same(out.error, photo_err.data(), sizeof(float) * n, "photo error map") && ok;
    ok = same(out.stats, photo_stats.data(), photo_stats.size(), "photo statistics") && ok;
    ok = same(out.debug_img_photo_error, photo_img.data(), 3 * n, "photo picture") && ok;
    if (!ok) return 1;
    std::printf("photometric: ok\n");

    // against the true map, relative, a host grey image
    reg::MapErrorParams tp;
    tp.source = FLAME_NLTGV2_MAP_ERROR_TRUTH, tp.truth_host = truth.data(), tp.win_size = hdr[6];
    tp.want_image = 1, tp.max_error = sc[1], tp.gray_host = ref.data(), tp.gray_step_bytes = cols, tp.flip = 1;
    d.mapErrorBegin(tp, rows, cols);
    out = d.mapErrorEnd();
    ok = out.source == FLAME_NLTGV2_MAP_ERROR_TRUTH && out.hist_scale == 1000.0f;
    ok = same(out.error, truth_err.data(), sizeof(float) * n, "truth error map") && ok;
    ok = same(out.stats, truth_stats.data(), truth_stats.size(), "truth statistics") && ok;
    ok = same(out.debug_img_photo_error, truth_img.data(), 3 * n, "truth picture") && ok;
    if (!ok) return 1;
    std::printf("true map: ok\n");

    // on the device only: the statistics travel, nothing else
    tp.copy_out = 0;
    d.mapErrorBegin(tp, rows, cols);
    out = d.mapErrorEnd();
    ok = !out.error && !out.debug_img_photo_error && out.error_device && out.image_device && out.stats_device &&
         same(out.stats, truth_stats.data(), truth_stats.size(), "statistics with copy_out = 0");
    if (!ok) {
      std::printf("FAIL: copy_out = 0\n");
      return 1;
    }
    std::printf("device only: ok\n");

    bool threw = false;
    tp.win_size = 4;
    try {
      d.mapErrorBegin(tp, rows, cols);
    } catch (const flame_hip::Error& e) {
      threw = e.status == FLAME_NLTGV2_ERR_INVALID_ARG;
    }
    out = d.mapErrorEnd();  // (the refused call left the outputs of the one before)
    if (!threw || !same(out.stats, truth_stats.data(), truth_stats.size(), "statistics after a refused call")) {
      std::printf("FAIL: an even window was accepted\n");
      return 1;
    }
    std::printf("an even window refused: ok\n");
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
