// FeatureTracker::setInput / addRawFrame (include/flame_hip/feature_tracker.hpp), the way a front-end that ran cv::cvtColor and
// cv::undistort before Flame::update would use them.  The cases come from a fixture tests/test_gpu_raw_frame_cpp.py writes: per
// case the cameras, the distortion, a raw frame and the three planes the checker (tests/input_ref.py + the frame builder) expects.
// Every case runs from host memory and from device memory (enqueue-only, then with the count); before setInput the call throws.
//   raw_frame_test FIXTURE      exit 0: all equal; 77: no usable HIP device; 1: a difference
#include <cstdio>
#include <cstring>
#include <vector>

#include "flame_hip/feature_tracker.hpp"

extern "C" {  // the three runtime calls a device producer needs here (the program links the HIP runtime)
int hipMalloc(void** p, size_t bytes);
int hipFree(void* p);
int hipMemcpy(void* dst, const void* src, size_t bytes, int kind);
}
static const int kHostToDevice = 1;

struct Mat3 {
  float m[9];
  float operator()(int r, int c) const { return m[3 * r + c]; }
};

struct Case {
  int32_t w, h, border, raw_w, raw_h, format, stride, n_outside;
  Mat3 K, Kinv;
  float K_raw[9], dist[8];
  std::vector<uint8_t> raw, img_pad;
  std::vector<float> gx, gy;
};

template <class T>
static bool read_n(FILE* f, T* out, size_t n) { return std::fread(out, sizeof(T), n, f) == n; }

static bool read_case(FILE* f, Case* c) {
  int32_t head[8];
  if (!read_n(f, head, 8)) return false;
  c->w = head[0], c->h = head[1], c->border = head[2], c->raw_w = head[3], c->raw_h = head[4], c->format = head[5];
  c->stride = head[6], c->n_outside = head[7];
  if (!read_n(f, c->K.m, 9) || !read_n(f, c->Kinv.m, 9) || !read_n(f, c->K_raw, 9) || !read_n(f, c->dist, 8)) return false;
  const size_t px = (size_t)(c->w + 2 * c->border) * (size_t)(c->h + 2 * c->border);
  c->raw.resize((size_t)c->raw_h * c->stride);
  c->img_pad.resize(px), c->gx.resize(px), c->gy.resize(px);
  return read_n(f, c->raw.data(), c->raw.size()) && read_n(f, c->img_pad.data(), px) && read_n(f, c->gx.data(), px) &&
         read_n(f, c->gy.data(), px);
}

static bool frame_equals(flame_hip::FeatureTracker& tracker, uint32_t id, const Case& c, const char* what) {
  const size_t px = c.img_pad.size();
  std::vector<uint8_t> img(px);
  std::vector<float> gx(px), gy(px);
  if (flame_stereo_download_frame(tracker.handle(), id, img.data(), gx.data(), gy.data()) != 0) {
    std::printf("FAIL: %s: download_frame\n", what);
    return false;
  }
  const bool ok = std::memcmp(img.data(), c.img_pad.data(), px) == 0 && std::memcmp(gx.data(), c.gx.data(), px * sizeof(float)) == 0 &&
                  std::memcmp(gy.data(), c.gy.data(), px * sizeof(float)) == 0;
  if (!ok) std::printf("FAIL: %s: the resident frame differs from the checker's\n", what);
  return ok;
}

int main(int argc, char** argv) {
  FILE* f = argc > 1 ? std::fopen(argv[1], "rb") : nullptr;
  int32_t n_cases = 0;
  if (!f || !read_n(f, &n_cases, 1)) {
    std::printf("FAIL: no fixture\n");
    return 1;
  }
  try {
    for (int k = 0; k < n_cases; ++k) {
      Case c;
      if (!read_case(f, &c)) {
        std::printf("FAIL: the fixture ends inside case %d\n", k);
        return 1;
      }
      flame_hip::FeatureTracker tracker(c.K, c.Kinv, c.w, c.h, c.border);
      if (k == 0) {  // before setInput the call throws and adds nothing
        bool threw = false;
        try {
          tracker.addRawFrame(1, c.raw.data(), c.stride);
        } catch (const flame_hip::StereoError& e) {
          threw = e.status == FLAME_NLTGV2_ERR_INVALID_ARG;
        }
        if (!threw || tracker.frameCount() != 0) {
          std::printf("FAIL: addRawFrame without setInput went through\n");
          return 1;
        }
        std::printf("no setInput: ok\n");
      }
      flame_stereo_input_params in;
      flame_stereo_default_input_params(&in);
      in.format = c.format, in.remap = 1, in.raw_width = c.raw_w, in.raw_height = c.raw_h;
      std::memcpy(in.K_raw, c.K_raw, sizeof in.K_raw);
      std::memcpy(in.dist, c.dist, sizeof in.dist);
      tracker.setInput(in);

      flame_stereo_input_stats st;
      st.n_outside = -1;
      tracker.addRawFrame(1, c.raw.data(), c.stride, false, &st);
      if (st.n_outside != c.n_outside || !frame_equals(tracker, 1, c, "host source")) return 1;

      void* dev = nullptr;
      if (hipMalloc(&dev, c.raw.size()) != 0 || hipMemcpy(dev, c.raw.data(), c.raw.size(), kHostToDevice) != 0) {
        std::printf("FAIL: no device buffer\n");
        return 1;
      }
      tracker.addRawFrame(2, dev, c.stride, true);  // enqueue-only; download_frame waits for the stream
      bool ok = frame_equals(tracker, 2, c, "device source");
      st.n_outside = -1;
      tracker.addRawFrame(3, dev, c.stride, true, &st);
      ok = ok && st.n_outside == c.n_outside && frame_equals(tracker, 3, c, "device source with stats") && tracker.frameCount() == 3;
      (void)hipFree(dev);  // (the stream has passed both calls: each download_frame waited)
      if (!ok) return 1;
      std::printf("case %d (%dx%d from %dx%d, format %d, %d outside): ok\n", k, c.w, c.h, c.raw_w, c.raw_h, c.format, c.n_outside);
    }
    std::fclose(f);
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
