// align_host.hpp -- the host arithmetic of flame_stereo_align_frame / flame_stereo_align_linearize (include/flame_stereo.h states every
// formula with its association): quaternion -> rotation matrix, the se(3) exponential applied on the left, the 6 x 6 Cholesky solve and
// the accept rule.  All in double, + - * / sqrt sin cos only, no FMA contraction (-ffp-contract=off).  No HIP in here:
// tests/cpp/align_host_test.cc runs it under AddressSanitizer + UndefinedBehaviorSanitizer (make sanitize).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace flame_hip {
namespace align {

constexpr int kSums = 28;       // 21 of H (upper triangle, row-major), 6 of b, the cost
constexpr int kMaxLevels = 5;
constexpr double kSmallAngle2 = 1e-10;  // theta^2 below which exp() takes the series (flame_stereo.h)

// Index of H_ij (i <= j) among the 21: row-major over the upper triangle.
inline int h_index(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

// q = (w, x, y, z) -> R row-major; the association of load_geometry (stereo_kernels.h), in double.
inline void quat_to_rot(const double q[4], double R[9]) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
  R[3] = txy + twz, R[4] = 1.0 - (txx + tzz), R[5] = tyz - twx;
  R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1.0 - (txx + tyy);
}

inline bool pose_finite(const double q[4], const double t[3]) {
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(q[k])) return false;
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(t[k])) return false;
  return true;
}

// The 12 floats the kernel sees: R and t rounded to float32.
inline void pose_to_float(const double q[4], const double t[3], float Rf[9], float tf[3]) {
  double R[9];
  quat_to_rot(q, R);
  for (int k = 0; k < 9; ++k) Rf[k] = (float)R[k];
  for (int k = 0; k < 3; ++k) tf[k] = (float)t[k];
}

inline void cross(const double a[3], const double b[3], double c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// T' = exp(delta) * T, delta = (v, omega); q renormalised.  flame_stereo.h writes the formula out.
inline void exp_left(const double delta[6], const double q[4], const double t[3], double q_out[4], double t_out[3]) {
  const double* v = delta;
  const double* o = delta + 3;
  const double th2 = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2];
  double A, B, Cc, Hs, Hc;  // sin(th)/th, (1 - cos th)/th^2, (th - sin th)/th^3, sin(th/2)/th, cos(th/2)
  if (th2 < kSmallAngle2) {
    A = 1.0 - th2 / 6.0;
    B = 0.5 - th2 / 24.0;
    Cc = 1.0 / 6.0 - th2 / 120.0;
    Hs = 0.5 - th2 / 48.0;
    Hc = 1.0 - th2 / 8.0;
  } else {
    const double th = std::sqrt(th2);
    const double s = std::sin(th), c = std::cos(th);
    A = s / th;
    B = (1.0 - c) / th2;
    Cc = (th - s) / (th2 * th);
    Hs = std::sin(0.5 * th) / th;
    Hc = std::cos(0.5 * th);
  }
  // translation: (t + A (o x t) + B (o x (o x t))) + (v + B (o x v) + Cc (o x (o x v)))
  double ot[3], oot[3], ov[3], oov[3];
  cross(o, t, ot);
  cross(o, ot, oot);
  cross(o, v, ov);
  cross(o, ov, oov);
  for (int k = 0; k < 3; ++k) t_out[k] = ((t[k] + A * ot[k]) + B * oot[k]) + ((v[k] + B * ov[k]) + Cc * oov[k]);
  // rotation: dq = (Hc, Hs o), q' = dq (x) q (Hamilton), then / |q'|
  const double a = Hc, b = Hs * o[0], c = Hs * o[1], d = Hs * o[2];
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  double r[4];
  r[0] = ((a * w - b * x) - c * y) - d * z;
  r[1] = ((a * x + b * w) + c * z) - d * y;
  r[2] = ((a * y - b * z) + c * w) + d * x;
  r[3] = ((a * z + b * y) - c * x) + d * w;
  const double n = std::sqrt(((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]);
  for (int k = 0; k < 4; ++k) q_out[k] = r[k] / n;
}

// Solves (H + lambda diag H) delta = -b by Cholesky (H: the 21 upper-triangle sums).  false: not positive definite (a pivot that is not
// > 0, NaN included); delta is then untouched.
inline bool solve(const double H21[21], const double b[6], double lambda, double delta[6]) {
  double L[6][6];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) L[i][j] = 0.0;
  for (int j = 0; j < 6; ++j) {
    const double hjj = H21[h_index(j, j)];
    double d = hjj + lambda * hjj;
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    const double ljj = std::sqrt(d);
    L[j][j] = ljj;
    for (int i = j + 1; i < 6; ++i) {
      double s = H21[h_index(j, i)];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / ljj;
    }
  }
  double y[6];
  for (int i = 0; i < 6; ++i) {
    double s = -b[i];
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
  double x[6];
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
    for (int k = i + 1; k < 6; ++k) s -= L[k][i] * x[k];
    x[i] = s / L[i][i];
  }
  for (int i = 0; i < 6; ++i)
    if (!std::isfinite(x[i])) return false;
  for (int i = 0; i < 6; ++i) delta[i] = x[i];
  return true;
}

// Accept iff cost' / n' < cost / n, compared in double (n' == 0: NaN or inf, not accepted).
inline bool accept(double cost_new, int32_t n_new, double cost_old, int32_t n_old) {
  return cost_new / (double)n_new < cost_old / (double)n_old;
}

inline double max_abs(const double d[6]) {
  double m = 0.0;
  for (int k = 0; k < 6; ++k) {
    const double a = std::fabs(d[k]);
    if (a > m) m = a;
  }
  return m;
}

// Size of level l of a w x h frame: ((w + 1) / 2, (h + 1) / 2) per level.
inline void level_size(int w, int h, int level, int* wl, int* hl) {
  for (int l = 0; l < level; ++l) w = (w + 1) / 2, h = (h + 1) / 2;
  *wl = w, *hl = h;
}

// 1 <= n_levels <= 5 and every level keeps w_l, h_l >= 4.
inline bool levels_valid(int w, int h, int n_levels) {
  if (n_levels < 1 || n_levels > kMaxLevels) return false;
  int wl, hl;
  level_size(w, h, n_levels - 1, &wl, &hl);
  return wl >= 4 && hl >= 4;
}

// Byte offsets of level l >= 1 inside a frame's pyramid block: gradx, grady (float planes), then the image; every level starts on a
// multiple of 16 bytes.  Returns the block's size for `n_levels` levels.
struct LevelPlace {
  size_t gx, gy, img;
  int w, h;
};
inline size_t place_levels(int w, int h, int n_levels, LevelPlace place[kMaxLevels]) {
  size_t off = 0;
  for (int l = 1; l < n_levels; ++l) {
    int wl, hl;
    level_size(w, h, l, &wl, &hl);
    const size_t px = (size_t)wl * (size_t)hl;
    place[l].w = wl, place[l].h = hl;
    place[l].gx = off;
    place[l].gy = off + 4 * px;
    place[l].img = off + 8 * px;
    off += 9 * px;
    off = (off + 15) / 16 * 16;
  }
  return off;
}

}  // namespace align
}  // namespace flame_hip
