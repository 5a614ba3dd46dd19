// DeviceGraph::volumeMeshBegin / volumeMeshEnd (include/flame_hip/nltgv2_l1_graph_regularizer.hpp) round trip: reads a case the Python
// test dumped (a volume's parameters and voxels, a box, and what the Python mirror obtained for them), goes through the facade --
// volumeCreate, volumeUpload, a count query, the call with exactly the counts, the arrays left on the device, a capacity one short, a
// refused box -- and compares byte for byte.
//   volume_mesh_test <case file>      exit 0: all equal; 77: no usable HIP device; 1: a difference or a bad file
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
  reg::VolumeMeshParams md;
  if (md.lo[0] != 0 || md.lo[1] != 0 || md.lo[2] != 0 || md.hi[0] != 0 || md.hi[1] != 0 || md.hi[2] != 0 || md.max_vertices != 0 ||
      md.max_triangles != 0 || md.want_normals != 1 || md.copy_out != 1 || sizeof(reg::VolumeMeshParams) != sizeof(flame_nltgv2_volume_mesh_params) ||
      sizeof(flame_nltgv2_volume_mesh_counts) != 32) {
    std::printf("FAIL: defaults\n");
    return 1;
  }
  if (argc < 2) {
    std::printf("usage: volume_mesh_test <case file>\n");
    return 1;
  }
  try {
    reg::DeviceGraph d(0);
    std::FILE* f = std::fopen(argv[1], "rb");
    char magic[4];
    int32_t hdr[17];  // nx, ny, nz, lo 3, hi 3, the eight counters
    bool ok = f && std::fread(magic, 1, 4, f) == 4 && std::memcmp(magic, "VMS1", 4) == 0 && std::fread(hdr, sizeof(int32_t), 17, f) == 17;
    if (!ok) {
      std::printf("FAIL: cannot read %s\n", argv[1]);
      return 1;
    }
    const size_t nvox = static_cast<size_t>(hdr[0]) * hdr[1] * hdr[2], nv = hdr[9], nt = hdr[10];
    std::vector<float> par, tsdf, weight, vertices, normals;  // par: voxel_size | origin 3 | trunc | max_weight
    std::vector<int32_t> triangles;
    ok = take(f, &par, 6) && take(f, &tsdf, nvox) && take(f, &weight, nvox) && take(f, &vertices, 3 * nv) && take(f, &normals, 3 * nv) &&
         take(f, &triangles, 3 * nt);
    std::fclose(f);
    if (!ok) {
      std::printf("FAIL: short file\n");
      return 1;
    }
    reg::VolumeParams vp;
    vp.nx = hdr[0], vp.ny = hdr[1], vp.nz = hdr[2];
    vp.voxel_size = par[0], vp.trunc = par[4], vp.max_weight = par[5];
    std::memcpy(vp.origin, par.data() + 1, sizeof(vp.origin));
    d.volumeCreate(vp);  // no graph: the volume belongs to the context
    d.volumeUpload(tsdf.data(), weight.data());

    reg::VolumeMeshParams mp;
    std::memcpy(mp.lo, hdr + 3, sizeof(mp.lo));
    std::memcpy(mp.hi, hdr + 6, sizeof(mp.hi));
    d.volumeMeshBegin(mp);  // capacities 0: a count query
    reg::VolumeMesh m = d.volumeMeshEnd();
    int32_t want[8];
    std::memcpy(want, hdr + 9, sizeof(want));
    want[4] = 1;  // overflow
    if (!same(&m.counts, want, sizeof(want), "the count query's counters") || m.vertices || m.normals || m.triangles) {
      std::printf("FAIL: the count query\n");
      return 1;
    }
    std::printf("count query: ok\n");

    mp.max_vertices = m.counts.n_vertices, mp.max_triangles = m.counts.n_triangles;
    d.volumeMeshBegin(mp);
    m = d.volumeMeshEnd();
    ok = same(&m.counts, hdr + 9, sizeof(m.counts), "the counters");
    ok = same(m.vertices, vertices.data(), sizeof(float) * 3 * nv, "the vertices") && ok;
    ok = same(m.normals, normals.data(), sizeof(float) * 3 * nv, "the normals") && ok;
    ok = same(m.triangles, triangles.data(), sizeof(int32_t) * 3 * nt, "the triangles") && ok;
    if (!ok || !m.vertices_device || !m.normals_device || !m.triangles_device) return 1;
    std::printf("exact capacity to the host: ok\n");

    bool threw = false;
    try {
      reg::VolumeMeshParams bad = mp;
      bad.lo[0] = 0, bad.hi[0] = hdr[0] + 1, bad.hi[1] = hdr[1], bad.hi[2] = hdr[2];
      d.volumeMeshBegin(bad);
    } catch (const flame_hip::Error& e) {
      threw = e.status == FLAME_NLTGV2_ERR_INVALID_ARG;
    }
    m = d.volumeMeshEnd();  // (the refused call left the outputs of the one before)
    if (!threw || !same(m.vertices, vertices.data(), sizeof(float) * 3 * nv, "the vertices after a refused call") ||
        !same(m.triangles, triangles.data(), sizeof(int32_t) * 3 * nt, "the triangles after a refused call")) {
      std::printf("FAIL: a box past the volume was accepted\n");
      return 1;
    }
    std::printf("a box past the volume refused: ok\n");

    mp.copy_out = 0, mp.want_normals = 0;
    d.volumeMeshBegin(mp);
    m = d.volumeMeshEnd();
    if (m.vertices || m.normals || m.triangles || !m.vertices_device || m.normals_device || !m.triangles_device ||
        !same(&m.counts, hdr + 9, sizeof(m.counts), "counters with copy_out = 0")) {
      std::printf("FAIL: copy_out = 0\n");
      return 1;
    }
    std::printf("device only: ok\n");

    mp.copy_out = 1, mp.want_normals = 1;
    mp.max_triangles -= 1;
    d.volumeMeshBegin(mp);
    m = d.volumeMeshEnd();
    if (nt > 0 && (!same(&m.counts, want, sizeof(want), "the counters one triangle short") || m.vertices || m.triangles)) {
      std::printf("FAIL: one triangle short\n");
      return 1;
    }
    std::printf("one triangle short: ok\n");
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
