// DeviceGraph::metricOutputsBegin / End (include/flame_hip/nltgv2_l1_graph_regularizer.hpp) round trip: reads a case the Python test
// dumped (graph, triangles, Kinv, pose, the depth window, and the outputs the Python mirror obtained for them), goes through the facade
// -- interpolateMeshBegin, meshOutputsBegin, metricOutputsBegin, the three Ends -- and compares byte for byte.
//   metric_outputs_test <case file>      exit 0: all equal; 77: no usable HIP device; 1: a difference or a bad file
#include <cmath>
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
  reg::MetricParams defaults;
  flame_nltgv2_metric_params c_defaults;
  flame_nltgv2_default_metric_params(&c_defaults);
  if (std::memcmp(&defaults, &c_defaults, sizeof(defaults)) != 0 || defaults.min_depth != 0.0f || !std::isinf(defaults.max_depth) ||
      defaults.want_mesh != 0 || defaults.copy_out != 1) {
    std::printf("FAIL: defaults\n");
    return 1;
  }
  if (argc < 2) {
    std::printf("usage: metric_outputs_test <case file>\n");
    return 1;
  }
  try {
    reg::DeviceGraph d(0);
    std::FILE* f = std::fopen(argv[1], "rb");
    char magic[4];
    int32_t hdr[9];  // V, E, T, rows, cols, use_filtered_map, has_pose, n_points, n_valid
    float sc[3];     // graph_scale, min_depth, max_depth
    bool ok = f && std::fread(magic, 1, 4, f) == 4 && std::memcmp(magic, "MET1", 4) == 0 && std::fread(hdr, sizeof(int32_t), 9, f) == 9 &&
              std::fread(sc, sizeof(float), 3, f) == 3;
    if (!ok) {
      std::printf("FAIL: cannot read %s\n", argv[1]);
      return 1;
    }
    const size_t V = hdr[0], E = hdr[1], T = hdr[2], n = static_cast<size_t>(hdr[3]) * hdr[4], NP = hdr[7], NV = hdr[8];
    const int rows = hdr[3], cols = hdr[4];
    std::vector<float> Kinv, pose, pos, x, alpha, beta, depth, organized, cloud, verts, norms;
    std::vector<int32_t> src, dst, tris, mesh_tris;
    std::vector<uint16_t> depth_mm;
    std::vector<uint32_t> pixel;
    ok = take(f, &Kinv, 9) && take(f, &pose, 12) && take(f, &pos, 2 * V) && take(f, &x, V) && take(f, &src, E) && take(f, &dst, E) &&
         take(f, &alpha, E) && take(f, &beta, E) && take(f, &tris, 3 * T) && take(f, &depth, n) && take(f, &depth_mm, n) &&
         take(f, &organized, 3 * n) && take(f, &cloud, 3 * NP) && take(f, &pixel, NP) && take(f, &verts, 3 * V) && take(f, &norms, 3 * V) &&
         take(f, &mesh_tris, 3 * NV);
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

    reg::MetricParams mp;
    mp.min_depth = sc[1], mp.max_depth = sc[2], mp.use_filtered_map = hdr[5], mp.want_mesh = 1;
    const float* T_world_cam = hdr[6] ? pose.data() : nullptr;
    d.interpolateMeshBegin(tris, rows, cols, sc[0]);
    d.meshOutputsBegin(nullptr, T, Kinv.data(), reg::MeshFilterParams(), rows, cols, sc[0], true);
    d.metricOutputsBegin(Kinv.data(), T_world_cam, mp, rows, cols);
    const float* dense = nullptr;
    d.interpolateMeshEnd(&dense);
    const reg::MeshOutputs mo = d.meshOutputsEnd();
    reg::MetricOutputs out = d.metricOutputsEnd();
    ok = out.rows == rows && out.cols == cols && out.num_vertices == V && out.num_triangles == T;
    if (out.num_points != NP || out.num_valid_triangles != NV || static_cast<size_t>(mo.num_valid_triangles) != NV) {
      std::printf("FAIL: counters (%zu points, %zu triangles)\n", out.num_points, out.num_valid_triangles);
      return 1;
    }
    ok = same(out.depth, depth.data(), sizeof(float) * n, "depth") && ok;
    ok = same(out.depth_mm, depth_mm.data(), sizeof(uint16_t) * n, "depth_mm") && ok;
    ok = same(out.organized, organized.data(), sizeof(float) * 3 * n, "organized") && ok;
    ok = same(out.cloud, cloud.data(), sizeof(float) * 3 * NP, "cloud") && ok;
    ok = same(out.cloud_pixel, pixel.data(), sizeof(uint32_t) * NP, "cloud_pixel") && ok;
    if (!ok) return 1;
    std::printf("depth images and clouds: ok\n");
    ok = same(out.mesh_vertices, verts.data(), sizeof(float) * 3 * V, "mesh_vertices");
    ok = same(out.mesh_normals, norms.data(), sizeof(float) * 3 * V, "mesh_normals") && ok;
    ok = same(out.mesh_triangles, mesh_tris.data(), sizeof(int32_t) * 3 * NV, "mesh_triangles") && ok;
    if (!ok) return 1;
    std::printf("mesh: ok\n");

    // on the device only: no host pointers, the same device pointers' kinds, the same counters
    mp.copy_out = 0;
    d.metricOutputsBegin(Kinv.data(), T_world_cam, mp, rows, cols);
    out = d.metricOutputsEnd();
    ok = !out.depth && !out.depth_mm && !out.organized && !out.cloud && !out.cloud_pixel && !out.mesh_vertices && !out.mesh_normals &&
         !out.mesh_triangles && out.depth_device && out.depth_mm_device && out.organized_device && out.cloud_device &&
         out.cloud_pixel_device && out.mesh_vertices_device && out.mesh_normals_device && out.mesh_triangles_device &&
         out.num_points == NP && out.num_valid_triangles == NV;
    if (!ok) {
      std::printf("FAIL: copy_out = 0\n");
      return 1;
    }
    std::printf("device only: ok\n");

    bool threw = false;
    try {
      d.metricOutputsBegin(Kinv.data(), T_world_cam, mp, rows + 1, cols);
    } catch (const flame_hip::Error& e) {
      threw = e.status == FLAME_NLTGV2_ERR_INVALID_ARG;
    }
    if (!threw) {
      std::printf("FAIL: another map size was accepted\n");
      return 1;
    }
    std::printf("another map size refused: ok\n");
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
