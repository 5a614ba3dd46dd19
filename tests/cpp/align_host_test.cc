// The host arithmetic of the direct alignment (flame_amd/csrc/align_host.hpp) under AddressSanitizer + UndefinedBehaviorSanitizer
// (`make -C flame_amd/csrc sanitize`): quaternion -> R, the se(3) exponential on both sides of its small-angle threshold, the 6 x 6
// Cholesky solve (a definite system, an indefinite one, NaN), the accept rule at n = 0, and the placement of the pyramid levels.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "align_host.hpp"

using namespace flame_hip::align;

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      ++fails;                                                    \
    }                                                             \
  } while (0)

static void test_index() {
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) CHECK(h_index(i, j) == k++);
  CHECK(k == 21);
}

static void test_rot_and_exp() {
  const double q0[4] = {1.0, 0.0, 0.0, 0.0}, t0[3] = {0.1, -0.2, 0.3};
  double R[9];
  quat_to_rot(q0, R);
  for (int k = 0; k < 9; ++k) CHECK(R[k] == (k % 4 == 0 ? 1.0 : 0.0));
  for (double scale : {0.0, 1e-7, 0.9e-5, 1.1e-5, 1e-3, 0.5, 3.0}) {
    const double d[6] = {0.3 * scale, -0.2 * scale, 0.5 * scale, 0.6 * scale, -0.7 * scale, 0.2 * scale};
    double q1[4], t1[3], qh[4], th[3], q2[4], t2[3], dh[6];
    for (int k = 0; k < 6; ++k) dh[k] = 0.5 * d[k];
    exp_left(d, q0, t0, q1, t1);
    exp_left(dh, q0, t0, qh, th);
    exp_left(dh, qh, th, q2, t2);  // exp(d / 2) exp(d / 2) = exp(d)
    double n = 0.0;
    for (int k = 0; k < 4; ++k) {
      n += q1[k] * q1[k];
      CHECK(std::fabs(q1[k] - q2[k]) < 1e-13);
    }
    for (int k = 0; k < 3; ++k) CHECK(std::fabs(t1[k] - t2[k]) < 1e-13);
    CHECK(std::fabs(n - 1.0) < 1e-15);
    quat_to_rot(q1, R);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double s = 0.0;
        for (int k = 0; k < 3; ++k) s += R[3 * i + k] * R[3 * j + k];
        CHECK(std::fabs(s - (i == j ? 1.0 : 0.0)) < 1e-14);
      }
  }
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const double qbad[4] = {1.0, nan, 0.0, 0.0}, tbad[3] = {0.0, inf, 0.0};
  CHECK(pose_finite(q0, t0) && !pose_finite(qbad, t0) && !pose_finite(q0, tbad));
  float Rf[9], tf[3];
  pose_to_float(q0, t0, Rf, tf);
  CHECK(Rf[0] == 1.0f && tf[2] == (float)0.3);
}

static void test_solve() {
  // H = A^T A + I from a fixed A: definite.  The residual of the solve is at rounding level.
  double A[6][6], H[6][6], H21[21], b[6], x[6];
  unsigned s = 12345u;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      s = s * 1664525u + 1013904223u;
      A[i][j] = (double)(s >> 8) / (double)(1u << 24) - 0.5;
    }
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      H[i][j] = i == j ? 1.0 : 0.0;
      for (int k = 0; k < 6; ++k) H[i][j] += A[k][i] * A[k][j];
    }
  for (int i = 0; i < 6; ++i) {
    b[i] = 0.1 * (i + 1);
    for (int j = i; j < 6; ++j) H21[h_index(i, j)] = H[i][j];
  }
  for (double lambda : {0.0, 0.5}) {
    CHECK(solve(H21, b, lambda, x));
    double hn = 0.0, xn = 0.0, bn = 0.0, rn = 0.0;
    for (int i = 0; i < 6; ++i) {
      double r = b[i], row = 0.0;
      for (int j = 0; j < 6; ++j) {
        const double a = H[i][j] + (i == j ? lambda * H[i][i] : 0.0);
        r += a * x[j], row += std::fabs(a);
      }
      hn = std::fmax(hn, row), xn = std::fmax(xn, std::fabs(x[i])), bn = std::fmax(bn, std::fabs(b[i])), rn = std::fmax(rn, std::fabs(r));
    }
    CHECK(rn <= 1e-13 * (hn * xn + bn));
  }
  double keep[6] = {7, 7, 7, 7, 7, 7};
  double bad[21];
  std::memcpy(bad, H21, sizeof bad);
  bad[h_index(3, 3)] = -1.0;  // indefinite
  CHECK(!solve(bad, b, 0.0, keep) && keep[0] == 7);
  std::memcpy(bad, H21, sizeof bad);
  bad[h_index(0, 4)] = std::numeric_limits<double>::quiet_NaN();
  CHECK(!solve(bad, b, 0.0, keep) && keep[5] == 7);
  double zero[21] = {0};
  CHECK(!solve(zero, b, 0.0, keep));
}

static void test_accept_and_levels() {
  CHECK(accept(9.0, 10, 10.0, 10) && !accept(10.0, 10, 10.0, 10) && !accept(0.0, 0, 10.0, 10) && !accept(5.0, 0, 10.0, 10));
  const double d[6] = {0.0, -3.0, 1.0, 0.0, 2.5, -0.5};
  CHECK(max_abs(d) == 3.0);
  int w, h;
  level_size(33, 17, 2, &w, &h);
  CHECK(w == 9 && h == 5);
  level_size(1920, 1080, 4, &w, &h);
  CHECK(w == 120 && h == 68);
  CHECK(levels_valid(33, 17, 3) && !levels_valid(33, 17, 4) && levels_valid(9, 8, 2) && !levels_valid(9, 8, 3));
  CHECK(!levels_valid(640, 480, 0) && !levels_valid(640, 480, 6) && levels_valid(640, 480, 5));
  // the levels of a block do not overlap and lie inside it; writing every byte of every plane stays inside the allocation
  for (int n = 1; n <= kMaxLevels; ++n) {
    LevelPlace pl[kMaxLevels];
    const size_t bytes = place_levels(67, 45, n, pl);
    std::vector<unsigned char> block(bytes, 0);
    for (int l = 1; l < n; ++l) {
      const size_t px = (size_t)pl[l].w * pl[l].h;
      CHECK(pl[l].gx % 16 == 0 && pl[l].gy % 4 == 0 && pl[l].img + px <= bytes);
      for (size_t k = 0; k < 4 * px; ++k) block[pl[l].gx + k] += 1, block[pl[l].gy + k] += 1;
      for (size_t k = 0; k < px; ++k) block[pl[l].img + k] += 1;
    }
    for (size_t k = 0; k < bytes; ++k) CHECK(block[k] <= 1);
    LevelPlace full[kMaxLevels];
    CHECK(place_levels(67, 45, kMaxLevels, full) >= bytes);
    for (int l = 1; l < n; ++l) CHECK(full[l].img == pl[l].img && full[l].gx == pl[l].gx);  // a level's place does not depend on n
  }
}

int main() {
  test_index();
  test_rot_and_exp();
  test_solve();
  test_accept_and_levels();
  std::printf(fails ? "align host: %d check(s) FAILED\n" : "align host: all ok\n", fails);
  return fails ? 1 : 0;
}
