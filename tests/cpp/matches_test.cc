// FeatureTracker::recordMatches / getDebugImageMatches (include/flame_hip/feature_tracker.hpp) round trip: reads a case the Python
// test dumped (camera, parameters, frames, pose table, features, and the records, picture and counters the sequential checker
// tests/matches_ref.py obtained for them), goes through the facade and compares byte for byte.
//   matches_test <case file>      exit 0: all equal; 77: no usable HIP device; 1: a difference or a bad file
#include <cstdio>
#include <cstring>
#include <vector>

#include "flame_hip/feature_tracker.hpp"

struct DebugParams {  // the members of flame::Params getDebugImageMatches reads
  bool debug_draw_matches = false;
  bool debug_flip_images = false;
};
struct Mat3 {
  float m[9];
  float operator()(int r, int c) const { return m[3 * r + c]; }
};

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
  if (argc < 2) {
    std::printf("usage: matches_test <case file>\n");
    return 1;
  }
  try {
    const Mat3 eye = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    flame_hip::FeatureTracker probe(eye, eye, 8, 8);  // (throws without a device, before the file is looked at)
    std::FILE* f = std::fopen(argv[1], "rb");
    char magic[4];
    int32_t hdr[9];  // width, height, pad, n_frames, n_poses, n_feats, new_id, curr_pf_id, flip
    Mat3 K, Kinv;
    flame_stereo_params params;
    bool ok = f && std::fread(magic, 1, 4, f) == 4 && std::memcmp(magic, "MAT1", 4) == 0 && std::fread(hdr, sizeof(int32_t), 9, f) == 9 &&
              std::fread(K.m, sizeof(float), 9, f) == 9 && std::fread(Kinv.m, sizeof(float), 9, f) == 9 &&
              std::fread(&params, sizeof params, 1, f) == 1;
    if (!ok) {
      std::printf("FAIL: cannot read %s\n", argv[1]);
      return 1;
    }
    const int width = hdr[0], height = hdr[1];
    const size_t px = static_cast<size_t>(width) * height, NF = hdr[5];
    std::vector<uint32_t> ids;
    std::vector<uint8_t> imgs, want_img;
    std::vector<flame_stereo_pose> poses;
    std::vector<flame_stereo_feature> feats, want_feats;
    std::vector<int32_t> want;  // kind_count[9], lines_drawn, lines_skipped, rings_skipped, entries
    ok = take(f, &ids, hdr[3]) && take(f, &imgs, hdr[3] * px) && take(f, &poses, hdr[4]) && take(f, &feats, NF) &&
         take(f, &want_feats, NF) && take(f, &want_img, 3 * px) && take(f, &want, 13);
    std::fclose(f);
    if (!ok) {
      std::printf("FAIL: short file\n");
      return 1;
    }
    flame_hip::FeatureTracker tracker(K, Kinv, width, height, hdr[2]);
    for (size_t k = 0; k < ids.size(); ++k) tracker.addFrame(ids[k], imgs.data() + k * px, width);
    std::vector<uint8_t> img(3 * px);
    DebugParams dbg;
    dbg.debug_flip_images = hdr[8] != 0;

    // without recording: the update as ever, no picture
    std::vector<flame_stereo_feature> plain(feats);
    flame_stereo_stats st0;
    tracker.updateFeatureIDepths(params, hdr[6], hdr[7], poses, plain.data(), static_cast<int>(NF), &st0);
    bool threw = false;
    try {
      tracker.getDebugImageMatches(img.data(), false);
    } catch (const flame_hip::StereoError& e) {
      threw = e.status == FLAME_NLTGV2_ERR_INVALID_ARG;
    }
    ok = threw && !tracker.getDebugImageMatches(dbg, img.data());
    ok = same(plain.data(), want_feats.data(), NF * sizeof(flame_stereo_feature), "features (not recording)") && ok;
    if (!ok) {
      std::printf("FAIL: a picture without records\n");
      return 1;
    }
    std::printf("not recording: ok\n");

    dbg.debug_draw_matches = true;
    tracker.recordMatches(dbg.debug_draw_matches);
    std::vector<flame_stereo_feature> rec(feats);
    flame_stereo_stats st1;
    tracker.updateFeatureIDepths(params, hdr[6], hdr[7], poses, rec.data(), static_cast<int>(NF), &st1);
    ok = same(rec.data(), want_feats.data(), NF * sizeof(flame_stereo_feature), "features (recording)");
    ok = same(&st1, &st0, sizeof st0, "flame_stereo_stats") && ok;
    flame_hip::MatchesStats ms;
    ok = tracker.getDebugImageMatches(dbg, img.data(), &ms) && ok;
    ok = same(img.data(), want_img.data(), 3 * px, "debug_img_matches") && ok;
    ok = same(ms.kind_count, want.data(), 9 * sizeof(int32_t), "kind_count") && ok;
    if (ms.num_features != static_cast<int>(NF) || ms.lines_drawn != want[9] || ms.lines_skipped != want[10] ||
        ms.rings_skipped != want[11] || ms.entries != want[12] || ms.refilled != 0) {
      std::printf("FAIL: counters (%d features, %d + %d lines, %d rings skipped, %lld entries)\n", ms.num_features, ms.lines_drawn,
                  ms.lines_skipped, ms.rings_skipped, static_cast<long long>(ms.entries));
      ok = false;
    }
    if (!ok) return 1;
    std::printf("matches image: ok\n");

    tracker.recordMatches(false);
    threw = false;
    try {
      tracker.getDebugImageMatches(img.data(), false);
    } catch (const flame_hip::StereoError& e) {
      threw = e.status == FLAME_NLTGV2_ERR_INVALID_ARG;
    }
    if (!threw) {
      std::printf("FAIL: a picture after recordMatches(false)\n");
      return 1;
    }
    std::printf("switched off: ok\n");
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
