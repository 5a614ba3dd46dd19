// FeatureTracker::buildPyramid / alignLinearize / alignFrame (include/flame_hip/feature_tracker.hpp), the way Flame::update would use
// them between addFrame and updateFeatureIDepths.  The cases come from a fixture tests/test_gpu_align_cpp.py writes; the program dumps
// what the calls return, as the C structs, for the Python side to compare byte for byte with the ctypes mirror's results.
//   align_test FIXTURE OUT      exit 0: ran; 77: no usable HIP device; 1: an error
// Per case the dump holds, for kind 0, one flame_stereo_align_system; for kind 1, one flame_stereo_align_result, an int32 count and
// that many flame_stereo_align_trace.
#include <cstdio>
#include <cstring>
#include <vector>

#include "flame_hip/feature_tracker.hpp"

struct Mat3 {
  float m[9];
  float operator()(int r, int c) const { return m[3 * r + c]; }
};

template <class T>
static bool read_n(FILE* f, T* out, size_t n) { return std::fread(out, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
  FILE* f = argc > 2 ? std::fopen(argv[1], "rb") : nullptr;
  FILE* out = argc > 2 ? std::fopen(argv[2], "wb") : nullptr;
  int32_t n_cases = 0;
  if (!f || !out || !read_n(f, &n_cases, 1)) {
    std::printf("FAIL: no fixture\n");
    return 1;
  }
  try {
    for (int k = 0; k < n_cases; ++k) {
      int32_t head[6];  // w, h, camera border, kind, n_levels, level
      Mat3 K, Kinv;
      flame_stereo_align_params P;
      double q[4], t[3];
      if (!read_n(f, head, 6) || !read_n(f, K.m, 9) || !read_n(f, Kinv.m, 9) || !read_n(f, &P, 1) || !read_n(f, q, 4) || !read_n(f, t, 3)) {
        std::printf("FAIL: the fixture ends inside case %d\n", k);
        return 1;
      }
      const int w = head[0], h = head[1];
      const size_t px = (size_t)w * (size_t)h;
      std::vector<uint8_t> ref(px), cur(px);
      std::vector<float> map(px);
      if (!read_n(f, ref.data(), px) || !read_n(f, cur.data(), px) || !read_n(f, map.data(), px)) {
        std::printf("FAIL: the fixture ends inside case %d\n", k);
        return 1;
      }
      flame_hip::FeatureTracker tracker(K, Kinv, w, h, head[2]);
      tracker.addFrame(1, ref.data(), w);
      tracker.addFrame(2, cur.data(), w);
      tracker.buildPyramid(1, head[4]);
      tracker.buildPyramid(2, head[4]);
      if (head[3] == 0) {
        const flame_stereo_align_system s = tracker.alignLinearize(P, 1, 2, head[5], map.data(), false, q, t);
        std::fwrite(&s, sizeof s, 1, out);
        std::printf("case %d (linearise %dx%d level %d): %d used\n", k, w, h, head[5], s.n_used);
      } else {
        std::vector<flame_stereo_align_trace> trace;
        const flame_stereo_align_result r = tracker.alignFrame(P, 1, 2, map.data(), false, q, t, &trace, 64);
        const int32_t n = (int32_t)trace.size();
        std::fwrite(&r, sizeof r, 1, out);
        std::fwrite(&n, sizeof n, 1, out);
        if (n > 0) std::fwrite(trace.data(), sizeof trace[0], (size_t)n, out);
        std::printf("case %d (align %dx%d): status %d, %d evaluations\n", k, w, h, r.status, r.n_evals);
      }
      bool threw = false;  // a level that is not built is refused, loudly
      try {
        (void)tracker.alignLinearize(P, 1, 2, head[4], map.data(), false, q, t);
      } catch (const flame_hip::StereoError& e) {
        threw = e.status == FLAME_NLTGV2_ERR_INVALID_ARG;
      }
      if (!threw) {
        std::printf("FAIL: case %d: a level that is not built went through\n", k);
        return 1;
      }
    }
    std::fclose(f);
    std::fclose(out);
    std::printf("align facade: ran\n");
    return 0;
  } catch (const flame_hip::StereoError& e) {
    if (e.status == FLAME_NLTGV2_ERR_NO_DEVICE) {
      std::printf("%s\n", e.what());
      return 77;
    }
    std::printf("FAIL: %s\n", e.what());
    return 1;
  }
}
