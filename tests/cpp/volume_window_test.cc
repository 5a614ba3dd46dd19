// DeviceGraph::volumeFollow / volumeShiftBegin / End / volumeWindow (include/flame_hip/nltgv2_l1_graph_regularizer.hpp) round trip: reads a
// case the Python test dumped (a volume's contents, a camera, and what the Python mirror obtained: the plan, the shift's counters, the
// shifted volume, a raycast and a mesh at the new base), goes through the facade -- volumeCreate, volumeUpload, volumeFollow,
// volumeShiftBegin / End, volumeWindow, volumeDownload, volumeRaycastBegin / End, volumeMeshBegin / End -- and compares byte for byte.
//   volume_window_test <case file>      exit 0: all equal; 77: no usable HIP device; 1: a difference or a bad file
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
  reg::FollowParams fd;
  if (fd.focus_depth != 0.0f || fd.step != 8 || sizeof(reg::FollowParams) != sizeof(flame_nltgv2_follow_params) ||
      sizeof(reg::FollowPlan) != 32 * sizeof(int32_t) || sizeof(flame_nltgv2_shift_counts) != 8 * sizeof(int32_t)) {
    std::printf("FAIL: defaults\n");
    return 1;
  }
  if (argc < 2) {
    std::printf("usage: volume_window_test <case file>\n");
    return 1;
  }
  try {
    reg::DeviceGraph d(0);
    std::FILE* f = std::fopen(argv[1], "rb");
    char magic[4];
    int32_t hdr[8];  // nx, ny, nz, target rows, target cols, n_steps, n_vertices, n_triangles
    bool ok = f && std::fread(magic, 1, 4, f) == 4 && std::memcmp(magic, "VWN1", 4) == 0 && std::fread(hdr, sizeof(int32_t), 8, f) == 8;
    if (!ok) {
      std::printf("FAIL: cannot read %s\n", argv[1]);
      return 1;
    }
    const size_t nvox = static_cast<size_t>(hdr[0]) * hdr[1] * hdr[2], n = static_cast<size_t>(hdr[3]) * hdr[4];
    const size_t nv = hdr[6], nt = hdr[7];
    const int trows = hdr[3], tcols = hdr[4];
    // voxel_size | origin 3 | trunc | max_weight | Kinv 9 | T_world_cam 12 | z_near | dz | focus_depth
    std::vector<float> par, tsdf0, weight0, tsdf1, weight1, map, vertices;
    // step | the plan 32 | the shift's counters 8 | the base afterwards 3 | record_bytes
    std::vector<int32_t> ints, rcounts, triangles;
    ok = take(f, &par, 30) && take(f, &ints, 45) && take(f, &tsdf0, nvox) && take(f, &weight0, nvox) && take(f, &tsdf1, nvox) &&
         take(f, &weight1, nvox) && take(f, &rcounts, 4) && take(f, &map, n) && take(f, &vertices, 3 * nv) && take(f, &triangles, 3 * nt);
    std::fclose(f);
    if (!ok) {
      std::printf("FAIL: short file\n");
      return 1;
    }
    reg::VolumeParams vp;
    vp.nx = hdr[0], vp.ny = hdr[1], vp.nz = hdr[2];
    vp.voxel_size = par[0], vp.trunc = par[4], vp.max_weight = par[5];
    std::memcpy(vp.origin, par.data() + 1, sizeof(vp.origin));
    d.volumeCreate(vp);
    d.volumeUpload(tsdf0.data(), weight0.data());
    int32_t base[3] = {7, 7, 7};
    int64_t bytes = 0;
    d.volumeWindow(base);
    d.volumeInfo(&bytes);
    if (base[0] != 0 || base[1] != 0 || base[2] != 0 || bytes != static_cast<int64_t>(8 * nvox)) {
      std::printf("FAIL: a fresh window\n");
      return 1;
    }
    const float* Kinv = par.data() + 6;
    const float* T_world_cam = par.data() + 15;
    reg::FollowParams fp;
    fp.focus_depth = par[29], fp.step = ints[0];
    const reg::FollowPlan plan = d.volumeFollow(T_world_cam, fp);
    if (!same(&plan, ints.data() + 1, sizeof(plan), "the plan")) return 1;
    std::printf("follow: ok\n");

    d.volumeShiftBegin(plan.shift);
    const reg::ShiftedWindow w = d.volumeShiftEnd();
    d.volumeWindow(base);
    d.volumeInfo(&bytes);
    ok = same(&w.counts, ints.data() + 33, sizeof(w.counts), "the shift's counters") && same(w.base, ints.data() + 41, sizeof(w.base), "the base") &&
         same(base, ints.data() + 41, sizeof(base), "volumeWindow") && same(w.shift, plan.shift, sizeof(w.shift), "the shift") &&
         w.record_bytes == ints[44] && bytes == static_cast<int64_t>(16 * nvox);
    std::vector<float> got_tsdf(nvox), got_weight(nvox);
    d.volumeDownload(got_tsdf.data(), got_weight.data());
    ok = same(got_tsdf.data(), tsdf1.data(), sizeof(float) * nvox, "tsdf") && ok;
    ok = same(got_weight.data(), weight1.data(), sizeof(float) * nvox, "weight") && ok;
    if (!ok) {
      std::printf("FAIL: the shift\n");
      return 1;
    }
    std::printf("shift: ok\n");

    reg::RaycastParams rp;
    rp.z_near = par[27], rp.dz = par[28], rp.n_steps = hdr[5];
    d.volumeRaycastBegin(Kinv, T_world_cam, rp, trows, tcols);
    const reg::RaycastView out = d.volumeRaycastEnd();
    ok = same(out.idepthmap, map.data(), sizeof(float) * n, "the raycast's map") && same(&out.counts, rcounts.data(), sizeof(out.counts), "the raycast's counters");
    if (!ok) return 1;
    std::printf("raycast at the new base: ok\n");

    reg::VolumeMeshParams mp;
    mp.max_vertices = hdr[6], mp.max_triangles = hdr[7];
    d.volumeMeshBegin(mp);
    const reg::VolumeMesh mesh = d.volumeMeshEnd();
    ok = mesh.counts.n_vertices == hdr[6] && mesh.counts.n_triangles == hdr[7] && mesh.counts.overflow == 0 &&
         same(mesh.vertices, vertices.data(), 3 * sizeof(float) * nv, "the vertices") &&
         same(mesh.triangles, triangles.data(), 3 * sizeof(int32_t) * nt, "the triangles");
    if (!ok) return 1;
    std::printf("mesh at the new base: ok\n");

    bool threw = false;
    try {
      const int32_t far[3] = {0, (1 << 22) + 1 - base[1], 0};
      d.volumeShiftBegin(far);
    } catch (const flame_hip::Error& e) {
      threw = e.status == FLAME_NLTGV2_ERR_INVALID_ARG;
    }
    int32_t after[3];
    d.volumeWindow(after);
    const reg::ShiftedWindow again = d.volumeShiftEnd();  // (the refused call left the outputs of the one before)
    if (!threw || !same(after, base, sizeof(base), "the window after a refused shift") ||
        !same(&again.counts, ints.data() + 33, sizeof(again.counts), "counters after a refused call")) {
      std::printf("FAIL: a base past the limit was accepted\n");
      return 1;
    }
    std::printf("past the limit refused: ok\n");
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
