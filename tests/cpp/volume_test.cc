// DeviceGraph::volumeCreate / volumeIntegrateBegin / End / volumeRaycastBegin / End / ... (include/flame_hip/nltgv2_l1_graph_regularizer.hpp)
// round trip: reads a case the Python test dumped (graph, triangles, the volume, two cameras, and what the Python mirror obtained for
// them), goes through the facade -- upload, interpolateMesh, volumeCreate, two integrations of the resident map, volumeDownload,
// volumeRaycastBegin / End -- and compares byte for byte.
//   volume_test <case file>      exit 0: all equal; 77: no usable HIP device; 1: a difference or a bad file
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
  reg::VolumeParams vd;
  reg::IntegrateParams id;
  reg::RaycastParams rd;
  if (vd.nx != 64 || vd.ny != 64 || vd.nz != 64 || vd.voxel_size != 0.05f || vd.origin[1] != 0.0f || vd.trunc != 0.15f || vd.max_weight != 64.0f ||
      id.weight != 1.0f || id.near_depth != 0.0f || id.min_depth != 0.0f || !(id.max_depth > 3e38f) || id.use_filtered_map != 0 ||
      id.map_device != nullptr || rd.z_near != 0.1f || rd.dz != 0.05f || rd.n_steps != 64 || rd.copy_out != 1 ||
      sizeof(reg::VolumeParams) != sizeof(flame_nltgv2_volume_params) || sizeof(reg::IntegrateParams) != sizeof(flame_nltgv2_integrate_params) ||
      sizeof(reg::RaycastParams) != sizeof(flame_nltgv2_raycast_params)) {
    std::printf("FAIL: defaults\n");
    return 1;
  }
  if (argc < 2) {
    std::printf("usage: volume_test <case file>\n");
    return 1;
  }
  try {
    reg::DeviceGraph d(0);
    std::FILE* f = std::fopen(argv[1], "rb");
    char magic[4];
    int32_t hdr[11];  // V, E, T, map rows, map cols, nx, ny, nz, target rows, target cols, n_steps
    bool ok = f && std::fread(magic, 1, 4, f) == 4 && std::memcmp(magic, "VOL1", 4) == 0 && std::fread(hdr, sizeof(int32_t), 11, f) == 11;
    if (!ok) {
      std::printf("FAIL: cannot read %s\n", argv[1]);
      return 1;
    }
    const size_t V = hdr[0], E = hdr[1], T = hdr[2], nvox = static_cast<size_t>(hdr[5]) * hdr[6] * hdr[7], n = static_cast<size_t>(hdr[8]) * hdr[9];
    const int rows = hdr[3], cols = hdr[4], trows = hdr[8], tcols = hdr[9];
    // voxel_size | origin 3 | trunc | max_weight | K 9 | Kinv 9 | two T_cam_world 12 + 12 | two weights | T_world_cam 12 | z_near | dz
    std::vector<float> par, pos, x, alpha, beta, tsdf, weight, map;
    std::vector<int32_t> src, dst, tris, icounts, rcounts;
    ok = take(f, &par, 6 + 18 + 24 + 2 + 12 + 2) && take(f, &pos, 2 * V) && take(f, &x, V) && take(f, &src, E) && take(f, &dst, E) && take(f, &alpha, E) &&
         take(f, &beta, E) && take(f, &tris, 3 * T) && take(f, &icounts, 16) && take(f, &tsdf, nvox) && take(f, &weight, nvox) && take(f, &rcounts, 4) &&
         take(f, &map, n);
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

    reg::VolumeParams vp;
    vp.nx = hdr[5], vp.ny = hdr[6], vp.nz = hdr[7];
    vp.voxel_size = par[0], vp.trunc = par[4], vp.max_weight = par[5];
    std::memcpy(vp.origin, par.data() + 1, sizeof(vp.origin));
    d.volumeCreate(vp);  // before any graph: the volume belongs to the context
    d.upload(g);
    std::vector<float> dense(static_cast<size_t>(rows) * cols);
    d.interpolateMesh(tris, rows, cols, 1.0f, dense.data());
    int64_t bytes = 0;
    const reg::VolumeParams got = d.volumeInfo(&bytes);
    if (std::memcmp(&got, &vp, sizeof(flame_nltgv2_volume_params)) != 0 || bytes != static_cast<int64_t>(8 * nvox)) {
      std::printf("FAIL: volumeInfo\n");
      return 1;
    }
    const float* K = par.data() + 6;
    const float* Kinv = par.data() + 15;
    for (int call = 0; call < 2; ++call) {
      reg::IntegrateParams ip;
      ip.weight = par[48 + call];
      d.volumeIntegrateBegin(K, par.data() + 24 + 12 * call, ip, rows, cols);
      const reg::IntegratedMap im = d.volumeIntegrateEnd();
      ok = im.rows == rows && im.cols == cols && same(&im.counts, icounts.data() + 8 * call, sizeof(im.counts), "the integration's counters") && ok;
    }
    std::vector<float> got_tsdf(nvox), got_weight(nvox);
    d.volumeDownload(got_tsdf.data(), got_weight.data());
    ok = same(got_tsdf.data(), tsdf.data(), sizeof(float) * nvox, "tsdf") && ok;
    ok = same(got_weight.data(), weight.data(), sizeof(float) * nvox, "weight") && ok;
    if (!ok) return 1;
    std::printf("two integrations: ok\n");

    reg::RaycastParams rp;
    rp.z_near = par[62], rp.dz = par[63], rp.n_steps = hdr[10];
    d.volumeRaycastBegin(Kinv, par.data() + 50, rp, trows, tcols);
    reg::RaycastView out = d.volumeRaycastEnd();
    ok = out.rows == trows && out.cols == tcols && out.idepthmap_device;
    ok = same(out.idepthmap, map.data(), sizeof(float) * n, "the raycast's map") && ok;
    ok = same(&out.counts, rcounts.data(), sizeof(out.counts), "the raycast's counters") && ok;
    if (!ok) return 1;
    std::printf("raycast to the host: ok\n");

    rp.copy_out = 0;
    d.volumeRaycastBegin(Kinv, par.data() + 50, rp, trows, tcols);
    out = d.volumeRaycastEnd();
    if (out.idepthmap || !out.idepthmap_device || !same(&out.counts, rcounts.data(), sizeof(out.counts), "counters with copy_out = 0")) {
      std::printf("FAIL: copy_out = 0\n");
      return 1;
    }
    std::printf("device only: ok\n");

    bool threw = false;
    try {
      rp.n_steps = 4097;
      d.volumeRaycastBegin(Kinv, par.data() + 50, rp, trows, tcols);
    } catch (const flame_hip::Error& e) {
      threw = e.status == FLAME_NLTGV2_ERR_INVALID_ARG;
    }
    out = d.volumeRaycastEnd();  // (the refused call left the outputs of the one before)
    if (!threw || !same(&out.counts, rcounts.data(), sizeof(out.counts), "counters after a refused call")) {
      std::printf("FAIL: 4097 steps were accepted\n");
      return 1;
    }
    std::printf("4097 steps refused: ok\n");

    // upload what came down, reset, destroy
    d.volumeReset();
    d.volumeDownload(got_tsdf.data(), got_weight.data());
    for (size_t i = 0; i < nvox; ++i) ok = ok && got_tsdf[i] == 1.0f && got_weight[i] == 0.0f;
    d.volumeUpload(tsdf.data(), weight.data());
    d.volumeDownload(got_tsdf.data(), got_weight.data());
    ok = same(got_tsdf.data(), tsdf.data(), sizeof(float) * nvox, "tsdf after upload") && ok;
    d.volumeDestroy();
    threw = false;
    try {
      d.volumeReset();
    } catch (const flame_hip::Error& e) {
      threw = e.status == FLAME_NLTGV2_ERR_INVALID_ARG;
    }
    if (!ok || !threw) {
      std::printf("FAIL: reset, upload or destroy\n");
      return 1;
    }
    std::printf("reset, upload, destroy: ok\n");
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
