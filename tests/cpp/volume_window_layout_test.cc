// side_stage.hpp's pure part of the window that follows the camera (flame_nltgv2_volume_shift_begin, flame_nltgv2_volume_follow), walked
// under the sanitizers on the host: the base limit, the clamped shift, follow's arithmetic, and the plan's boxes against what the Python
// checker (tests/volume_window_ref.py) says for a 16 x 12 x 10 window, read from standard input, one plan per line:
//   shift[3] n_leaving has_kept kept_lo[3] kept_hi[3] then per leaving box lo[3] hi[3]
// Prints "<n> plans, <v> violations"; exit 0 iff v == 0.
#include <cstdio>
#include <cstring>
#include <limits>

#include "side_stage.hpp"

using namespace flame_hip::host;

static int violations = 0;
#define EXPECT(cond)                                             \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("violated at line %d: %s\n", __LINE__, #cond); \
      ++violations;                                              \
    }                                                            \
  } while (0)

int main() {
  const int32_t dims[3] = {16, 12, 10};
  // -- the base limit --------------------------------------------------------------------------------------------------------------------
  {
    const int32_t base[3] = {kVolumeMaxBase - 1, -kVolumeMaxBase, 7};
    int32_t out[3] = {-1, -1, -1};
    const int32_t ok[3] = {1, 0, INT32_MIN / 4096}, over[3] = {2, 0, 0}, under[3] = {0, -1, 0}, wrap[3] = {INT32_MAX, INT32_MAX, INT32_MAX};
    EXPECT(!shifted_base(base, over, out) && out[0] == -1);
    EXPECT(!shifted_base(base, under, out) && out[1] == -1);
    EXPECT(!shifted_base(base, wrap, out));
    EXPECT(shifted_base(base, ok, out) && out[0] == kVolumeMaxBase && out[1] == -kVolumeMaxBase && out[2] == 7 + INT32_MIN / 4096);
  }
  // -- the shift as the kernel takes it --------------------------------------------------------------------------------------------------
  {
    int s[3];
    const int32_t far[3] = {INT32_MIN, 12, -11}, zero[3] = {0, 0, 0};
    EXPECT(clamped_shift(dims, far, s) && s[0] == -16 && s[1] == 12 && s[2] == -10);
    EXPECT(!clamped_shift(dims, zero, s) && s[0] == 0 && s[1] == 0 && s[2] == 0);
  }
  // -- follow ----------------------------------------------------------------------------------------------------------------------------
  {
    const float origin[3] = {-0.8f, -0.6f, 0.5f}, voxel = 0.1f;  // the middle voxel (8, 6, 5) lies at (0, 0, 1)
    const int32_t base[3] = {0, 0, 0};
    float T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1};
    int32_t s[3] = {9, 9, 9};
    T[3] = 0.31f;
    EXPECT(follow_shift(T, 0.0f, 4, origin, voxel, base, dims, s) && s[0] == 0 && s[1] == 0 && s[2] == 0);
    T[3] = 0.41f;
    EXPECT(follow_shift(T, 0.0f, 4, origin, voxel, base, dims, s) && s[0] == 4 && s[1] == 0 && s[2] == 0);
    T[3] = -0.79f;
    EXPECT(follow_shift(T, 0.0f, 4, origin, voxel, base, dims, s) && s[0] == -4);
    T[3] = 0.0f;
    EXPECT(follow_shift(T, 0.85f, 4, origin, voxel, base, dims, s) && s[2] == 8 && s[0] == 0);  // along the third column of R
    s[0] = s[1] = s[2] = 9;
    EXPECT(!follow_shift(T, 0.0f, 0, origin, voxel, base, dims, s) && s[0] == 9);
    EXPECT(!follow_shift(T, std::numeric_limits<float>::infinity(), 4, origin, voxel, base, dims, s));
    T[7] = std::numeric_limits<float>::quiet_NaN();
    EXPECT(!follow_shift(T, 0.0f, 4, origin, voxel, base, dims, s) && s[1] == 9);
    T[7] = 1e6f;  // a quotient past 2^22 with step 1
    EXPECT(!follow_shift(T, 0.0f, 1, origin, voxel, base, dims, s));
    T[7] = 4e5f;  // 4e6 voxels: inside the quotient's limit; times the step it passes int32
    EXPECT(follow_shift(T, 0.0f, 1, origin, voxel, base, dims, s) && s[1] > 3999000 && s[1] < 4001000);
    EXPECT(!follow_shift(T, 0.0f, 1, origin, 1e-4f, base, dims, s));
    T[7] = 3e6f;  // q = 3e6 is inside the quotient's limit, q * step = 3e9 is outside int32
    EXPECT(!follow_shift(T, 0.0f, 1000, origin, 1e-3f, base, dims, s));  }
  // -- the plans -------------------------------------------------------------------------------------------------------------------------
  int n_plans = 0;
  char line[1024];
  while (std::fgets(line, sizeof(line), stdin)) {
    long w[5 + 6 + 18];
    int n = 0, used = 0, at = 0;
    while (n < 29 && std::sscanf(line + at, "%ld%n", &w[n], &used) == 1) at += used, ++n;
    if (n < 11) continue;
    ++n_plans;
    const int32_t shift[3] = {(int32_t)w[0], (int32_t)w[1], (int32_t)w[2]};
    WindowPlan p;
    std::memset(&p, 0x5a, sizeof(p));
    window_plan(dims, shift, &p);
    EXPECT(p.shift[0] == shift[0] && p.shift[1] == shift[1] && p.shift[2] == shift[2]);
    EXPECT(p.n_leaving == w[3] && p.has_kept == w[4] && n == 11 + 6 * p.n_leaving);
    for (int a = 0; a < 3; ++a) EXPECT(p.kept_lo[a] == w[5 + a] && p.kept_hi[a] == w[8 + a] && p.reserved[a] == 0);
    for (int b = 0; b < 3; ++b)
      for (int a = 0; a < 3; ++a) {
        const bool used_box = b < p.n_leaving && n >= 11 + 6 * (b + 1);
        EXPECT(p.leaving_lo[b][a] == (used_box ? w[11 + 6 * b + a] : 0) && p.leaving_hi[b][a] == (used_box ? w[14 + 6 * b + a] : 0));
      }
  }
  std::printf("%d plans, %d violations\n", n_plans, violations);
  return violations == 0 ? 0 : 1;
}
