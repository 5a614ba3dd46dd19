// The pure host part of the stereo front end (flame_amd/csrc/stereo_host.hpp): the growth counts, the border and the scan
// rectangle, the cell grid and the mask-point check of detectFeatures, the decode of a stage's error words, the sum over counter
// slots and the interior of a padded plane.  Every expected value is worked out by hand from the formula in the comment next to it.
//   stereo_host_test      exit 0: all held; 1: a violation (printed)
#include <climits>
#include <cstdio>
#include <vector>

#include "stereo_host.hpp"

using namespace flame_hip::host;

static int bad = 0;
#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++bad;                                                      \
    }                                                             \
  } while (0)

static bool is(const FirstError& e, ErrorKind kind, int index) { return e.kind == kind && e.index == index; }

int main() {
  // growth: count + count / 2 + 16 on the device, 2 count + 16 pinned
  EXPECT(grown(0) == 16 && grown(1) == 17);  // 1 / 2 = 0
  EXPECT(grown(100) == 166);                 // a first capacity
  EXPECT(grown(165) == 263);                 // just below it: 165 + 82 + 16 (not reached: 165 <= 166 does not grow)
  EXPECT(grown(167) == 266);                 // just above it: 167 + 83 + 16
  EXPECT(grown_pinned(0) == 16 && grown_pinned(1) == 18 && grown_pinned(165) == 346 && grown_pinned(167) == 350);
  for (size_t n : {(size_t)0, (size_t)1, (size_t)165, (size_t)167, (size_t)1 << 20}) {
    EXPECT(grown(n) > n);                  // a grown array holds what it was grown for
    EXPECT(grown_pinned(n) >= grown(n));   // and the pinned one is never the smaller
  }
  // the matches picture's entries: max(2 px, total + total / 4)
  EXPECT(entry_capacity(3072, 0) == 6144);
  EXPECT(entry_capacity(3072, 4915) == 6144);  // 4915 + 1228 = 6143
  EXPECT(entry_capacity(3072, 4916) == 6145);  // 4916 + 1229
  EXPECT(entry_capacity(0, 0) == 0 && entry_capacity(0, 3) == 3);

  // the border: (int)(rescale_factor_max * win_size / 2 + 1), the product in float
  EXPECT(front_border(1.4f, 5) == 4);    // 7 / 2 + 1 = 4.5
  EXPECT(front_border(1.5f, 5) == 4);    // 7.5 / 2 + 1 = 4.75
  EXPECT(front_border(1.0f, 5) == 3);    // a product ending in .5 after the halving: 2.5 + 1 = 3.5
  EXPECT(front_border(0.5f, 5) == 2);    // the product itself ends in .5: 2.5 / 2 + 1 = 2.25
  EXPECT(front_border(0.1f, 5) == 1);    // a product below 1: 0.5 / 2 + 1 = 1.25
  EXPECT(front_border(0.0f, 5) == 1);
  EXPECT(front_border(-0.5f, 5) == 0);   // -1.25 + 1 = -0.25 truncates towards zero
  EXPECT(front_border(-1.0f, 5) == -1);  // -2.5 + 1 = -1.5
  EXPECT(front_border(1.4f, 0) == 1);

  // the scan rectangle: x = border, y = border + off, w = width - 2 border, h = height - 2 border - 2 off, off = height / 3
  {
    const ScanRect r = scan_rect(64, 50, 4, false);  // (50 is not divisible by 3)
    EXPECT(r.c_lo == 4 && r.r_lo == 4 && r.c_hi == 60 && r.r_hi == 46 && r.w() == 56 && r.h() == 42);
    const ScanRect l = scan_rect(64, 50, 4, true);  // off = 16
    EXPECT(l.c_lo == 4 && l.r_lo == 20 && l.c_hi == 60 && l.r_hi == 30 && l.w() == 56 && l.h() == 10);
    const ScanRect z = scan_rect(64, 50, 0, false);
    EXPECT(z.c_lo == 0 && z.r_lo == 0 && z.w() == 64 && z.h() == 50);
    const ScanRect e = scan_rect(7, 50, 4, true);  // wider than the image: an inverted rectangle, not a clamped one
    EXPECT(e.c_lo == 4 && e.c_hi == 3 && e.w() == -1 && e.h() == 10);
    const ScanRect t = scan_rect(64, 5, 1, true);  // off = 1: rows [2, 3)
    EXPECT(t.r_lo == 2 && t.r_hi == 3 && t.h() == 1);
  }

  // the cell grid: fast_ceil((float)size / win)
  EXPECT(ceil_cells(64, 16) == 4 && ceil_cells(65, 16) == 5 && ceil_cells(63, 16) == 4);  // an exact multiple, one above, one below
  EXPECT(ceil_cells(64, 4) == 16 && ceil_cells(48, 4) == 12 && ceil_cells(64, 3) == 22 && ceil_cells(48, 3) == 16);
  EXPECT(ceil_cells(1, 16) == 1 && ceil_cells(5, 1) == 5 && ceil_cells(2, 3) == 1);

  // mask points: inside [0, width) x [0, height) and inside the grid
  {
    const int W = 64, H = 48, win = 16, wc = ceil_cells(W, win), hc = ceil_cells(H, win);
    EXPECT(mask_point_valid(0.0f, 0.0f, W, H, win, wc, hc));
    EXPECT(mask_point_valid(W - 0.5f, 10.0f, W, H, win, wc, hc));   // x = width - 0.5: cell 3 of 4
    EXPECT(!mask_point_valid((float)W, 10.0f, W, H, win, wc, hc));  // x = width
    EXPECT(mask_point_valid(10.0f, H - 0.5f, W, H, win, wc, hc));
    EXPECT(!mask_point_valid(10.0f, (float)H, W, H, win, wc, hc));
    EXPECT(!mask_point_valid(-0.5f, 10.0f, W, H, win, wc, hc) && !mask_point_valid(10.0f, -1.0f, W, H, win, wc, hc));
    const float nan = __builtin_nanf("");
    EXPECT(!mask_point_valid(nan, 10.0f, W, H, win, wc, hc) && !mask_point_valid(10.0f, nan, W, H, win, wc, hc));
    EXPECT(!mask_point_valid(40.0f, 10.0f, W, H, win, 2, hc));  // in the image but past a narrower grid: cell 2 of 2
    EXPECT(!mask_point_valid(10.0f, 40.0f, W, H, win, wc, 2));
  }

  // the decode: which record fails first, by the three rules
  {
    const int none = INT_MAX;
    const ErrorRule B = ErrorRule::kBadFrameFirst, L = ErrorRule::kLowerIndex, A = ErrorRule::kAssertOnly;
    for (ErrorRule r : {B, L, A}) EXPECT(is(first_error(none, none, r), ErrorKind::kNone, -1));         // neither
    for (ErrorRule r : {B, L, A}) EXPECT(is(first_error(5, none, r), ErrorKind::kAssert, 5));           // assert only
    for (ErrorRule r : {B, L}) EXPECT(is(first_error(none, 7, r), ErrorKind::kBadFrame, 7));            // bad-frame only
    EXPECT(is(first_error(none, 7, A), ErrorKind::kNone, -1));
    for (int a : {3, 7, 9}) {                                                                           // both: < / = / >
      EXPECT(is(first_error(a, 7, B), ErrorKind::kBadFrame, 7));
      EXPECT(is(first_error(a, 7, A), ErrorKind::kAssert, a));
    }
    EXPECT(is(first_error(3, 7, L), ErrorKind::kAssert, 3));
    EXPECT(is(first_error(7, 7, L), ErrorKind::kAssert, 7));  // within a record the assert comes first
    EXPECT(is(first_error(9, 7, L), ErrorKind::kBadFrame, 7));
    EXPECT(is(first_error(0, 0, B), ErrorKind::kBadFrame, 0) && is(first_error(0, none, L), ErrorKind::kAssert, 0));
  }

  // the sum over slots: sums[c] = sum over k < slots of words[first + k stride + c]
  {
    const int first = 8, slots = 64, stride = 32, n = 6;
    std::vector<int> w((size_t)first + slots * stride, 0);  // exactly the block: a read past it is the sanitizer's to find
    int sums[6];
    sum_slots(w.data(), first, slots, stride, n, sums);
    for (int c = 0; c < n; ++c) EXPECT(sums[c] == 0);
    w[(size_t)first + (slots - 1) * stride + 5] = 9;  // one counter, set in the last slot alone
    sum_slots(w.data(), first, slots, stride, n, sums);
    for (int c = 0; c < n; ++c) EXPECT(sums[c] == (c == 5 ? 9 : 0));
    for (int k = 0; k < slots; ++k) w[(size_t)first + k * stride + 2] = k + 1;  // every slot: 64 * 65 / 2
    w[0] = w[7] = 1000, w[(size_t)first + 6] = 1000;                            // words before the slots and past the counters: not read
    sum_slots(w.data(), first, slots, stride, n, sums);
    EXPECT(sums[2] == 2080 && sums[5] == 9 && sums[0] == 0);
    std::vector<int> one(63 * 32 + 1, 0);  // a single counter from word 0, as the input stage keeps it
    one[63 * 32] = 4, one[0] = 1;
    int s1 = -1;
    sum_slots(one.data(), 0, 64, 32, 1, &s1);
    EXPECT(s1 == 5);
  }

  // the interior of a padded plane: border rows of `pitch` and border pixels
  EXPECT(interior_offset(0, 64) == 0 && interior_offset(4, 72) == 292 && interior_offset(1, 3) == 4);
  EXPECT(interior_offset(64, 16384 + 128) == (size_t)64 * 16512 + 64);

  if (bad) return 1;
  std::printf("stereo_host_test: ok\n");
  return 0;
}
