// Wind at one grid point: speed and direction from the components, the components from speed and direction, the Coriolis
// parameter, and the bin search of the wind rose.  One statement of the arithmetic for the gfx950 kernels (wind.hip) and
// the host test twin (host_twin.cpp).
// Reference: wind/array/wind.py:15-189 (speed, direction, xy_to_polar, polar_to_xy), :225-251 (coriolis), :254-328 (windrose).
//
// Float64 (and mixed or integer) input is computed in double, float32 fields in float.  The inverse tangent and the
// hypotenuse are written here, for host and device alike, from fma, compares, ONE division (atan2) and ONE square
// root (hypot): both are IEEE operations that the compiler expands in line and rounds correctly on either side, so the
// host twin and the kernel agree bit for bit.  No call into a math library, no table, no private array.
//
// atan2(y, x).  With n = min(|x|, |y|), d = max(|x|, |y|) the ratio r = n / d is in [0, 1] and is never formed: the
// interval is cut at 7/16 and 11/16 by comparing n with d, and
//   atan(r) = atan(k) + atan(t),  t = (n - k d) / (d + k n),  k = 0, 1/2 or 1,
// where n - k d is exact (k = 0 trivially; otherwise n and k d are within a factor of two of each other) and d + k n is
// rounded once, so t carries the division's rounding plus one more: |t| <= 7/16, 0.14 and 0.19.  atan(t) is the odd
// minimax polynomial of degree 23 in the classic even/odd split (error below 1 ulp for |t| <= 7/16), atan(k) a
// high / low pair.  The octant is undone with pi/2 and pi as high / low pairs in forms that give the correctly rounded
// -pi/2, pi, ... when atan(r) = 0, which is what puts the axes on the right side of the branch point of the
// meteorological direction.  Error: within 3 ulp of the result (2 ulp measured against libm on 4 M points).
#pragma once

#include <cmath>
#include <cstdint>

#include "solar_point.hpp"  // sol_sincos_deg, sol_fma
#include "thermo_math.hpp"

namespace ekm {

enum { WIND_METEO = 0, WIND_POLAR_POSITIVE = 1, WIND_POLAR_SIGNED = 2 };  // direction conventions (polar_to_xy: 0 or 1)
enum { WIND_KIND_POLAR = 0, WIND_KIND_XY = 1, WIND_KIND_CORIOLIS = 2 };
enum { WIND_SPEED = 1, WIND_DIRECTION = 2 };                              // outputs of the polar kind, as bits

constexpr double kWindDegree = 0x1.ca5dc1a63c1f8p+5;     // 180 / pi, the reference's constants.degree
constexpr double kWindMinusPi2 = -0x1.921fb54442d18p+0;  // -pi / 2
constexpr double kWindPi15 = 0x1.2d97c7f3321d2p+2;       // 1.5 * pi
// 2 * constants.omega, omega = 2 pi / sideral_day, sideral_day = solar_day / (1 + solar_day / sideral_year) with
// (constants/constants.py:62-72): omega = 7.292115083046062e-05 1/s
constexpr double kWindTwoOmega = 0x1.31da7d4fedf5fp-13;

// sqrt(x^2 + y^2) without overflow or underflow of the intermediate; +inf if either is infinite (even beside a NaN).
EKM_HD double wind_hypot(double x, double y) {
  const double ax = __builtin_fabs(x), ay = __builtin_fabs(y);
  double d = ax < ay ? ay : ax, n = ax < ay ? ax : ay;
  if (ax != ax || ay != ay) d = n = ax + ay;  // NaN
  if (ax == __builtin_inf() || ay == __builtin_inf()) return __builtin_inf();
  // powers of two, exact: above 2^500 down by 2^-600, below 2^-500 up by 2^600; the result goes back in one rounding
  const double up = d > 0x1p+500 ? 0x1p-600 : d < 0x1p-500 ? 0x1p+600 : 1.0;
  const double back = d > 0x1p+500 ? 0x1p+600 : d < 0x1p-500 ? 0x1p-600 : 1.0;
  d *= up;
  n *= up;
  return __builtin_sqrt(sol_fma(d, d, n * n)) * back;
}

// atan(n / d) for 0 <= n <= d, d > 0 and finite
EKM_HD double wind_atan_ratio(double n, double d) {
  constexpr double kHi0 = 4.63647609000806093515e-01, kLo0 = 2.26987774529616870924e-17;  // atan(1/2)
  constexpr double kHi1 = 7.85398163397448278999e-01, kLo1 = 3.06161699786838301793e-17;  // atan(1)
  const bool low = n < 0.4375 * d, mid = n < 0.6875 * d;
  const double num = low ? n : mid ? sol_fma(2.0, n, -d) : n - d;
  const double den = low ? d : mid ? sol_fma(2.0, d, n) : d + n;
  const double t = num / den;
  const double z = t * t, w = z * z;
  constexpr double A0 = 3.33333333333329318027e-01, A1 = -1.99999999998764832476e-01, A2 = 1.42857142725034663711e-01,
                   A3 = -1.11111104054623557880e-01, A4 = 9.09088713343650656196e-02, A5 = -7.69187620504482999495e-02,
                   A6 = 6.66107313738753120669e-02, A7 = -5.83357013379057348645e-02, A8 = 4.97687799461593236017e-02,
                   A9 = -3.65315727442169155270e-02, A10 = 1.62858201153657823623e-02;
  const double s1 = z * sol_fma(w, sol_fma(w, sol_fma(w, sol_fma(w, sol_fma(w, A10, A8), A6), A4), A2), A0);
  const double s2 = w * sol_fma(w, sol_fma(w, sol_fma(w, sol_fma(w, A9, A7), A5), A3), A1);
  const double corr = t * (s1 + s2);
  const double hi = mid ? kHi0 : kHi1, lo = mid ? kLo0 : kLo1;
  return low ? t - corr : hi - ((corr - lo) - t);
}

// atan2(y, x) with the IEEE values for +-0 and +-inf in every combination; NaN if either is NaN.
EKM_HD double wind_atan2(double y, double x) {
  constexpr double kPi2Hi = 1.57079632679489655800e+00, kPi2Lo = 6.12323399573676603587e-17;
  constexpr double kPiHi = 3.14159265358979311600e+00, kPiLo = 1.22464679914735317723e-16;
  const double ax = __builtin_fabs(x), ay = __builtin_fabs(y);
  const bool swap = ay > ax;
  double d = swap ? ay : ax, n = swap ? ax : ay;
  if (d == __builtin_inf()) {  // inf / inf = 1, finite / inf = 0
    n = n == __builtin_inf() ? 1.0 : 0.0;
    d = 1.0;
  }
  if (d == 0.0) d = 1.0;       // 0 / 0 = 0: the sign bits alone decide
  if (d > 0x1p+1021) {         // d + n and 2 d + n stay finite
    n *= 0.25;
    d *= 0.25;
  }
  if (d < 0x1p-1000) {         // 7/16 d and 11/16 d stay exact among the denormals
    n *= 0x1p+64;
    d *= 0x1p+64;
  }
  const double a = wind_atan_ratio(n, d);
  const bool west = __builtin_signbit(x);
  double r;
  if (swap)
    r = west ? kPi2Hi + (a + kPi2Lo) : kPi2Hi - (a - kPi2Lo);
  else
    r = west ? kPiHi - (a - kPiLo) : a;
  r = __builtin_signbit(y) ? -r : r;
  return (x != x || y != y) ? x + y : r;
}

// The reference's direction from d = atan2(v, u), in its own operations (wind.py:37-61).
EKM_HD double wind_direction_of(double d, double u, double v, int mode) {
  (void)u;
  (void)v;
  if (mode == WIND_METEO) return d <= kWindMinusPi2 ? (kWindMinusPi2 - d) * kWindDegree : (kWindPi15 - d) * kWindDegree;
  const double deg = d * kWindDegree;
  return (mode == WIND_POLAR_POSITIVE && deg < 0.0) ? 360.0 + deg : deg;
}

// ---- float32: the same algorithms in float arithmetic, for float32 fields ----
// (The double routines on the upcast input ran at half the memory roof for float32 fields: profiles/HISTORY.md.)
// hypot: scaled by 2^-+90 outside 2^+-40, so the squares stay normal; error 1 eps32 relative (square eps/2 and fma eps/2
// on the sum, halved by the root, plus the root's eps/2).
EKM_HD float wind_hypot(float x, float y) {
  const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
  float d = ax < ay ? ay : ax, n = ax < ay ? ax : ay;
  if (ax != ax || ay != ay) d = n = ax + ay;  // NaN
  if (ax == __builtin_inff() || ay == __builtin_inff()) return __builtin_inff();
  const float up = d > 0x1p+40f ? 0x1p-90f : d < 0x1p-40f ? 0x1p+90f : 1.0f;
  const float back = d > 0x1p+40f ? 0x1p+90f : d < 0x1p-40f ? 0x1p-90f : 1.0f;
  d *= up;
  n *= up;
  return __builtin_sqrtf(__builtin_fmaf(d, d, n * n)) * back;
}

// atan(n / d) for 0 <= n <= d: the same cuts at 7/16 and 11/16, an odd polynomial of degree 11 on |t| <= 7/16
EKM_HD float wind_atan_ratio(float n, float d) {
  constexpr float kHi0 = 4.6364760399e-01f, kLo0 = 5.0121582440e-09f;  // atan(1/2)
  constexpr float kHi1 = 7.8539812565e-01f, kLo1 = 3.7748947079e-08f;  // atan(1)
  const bool low = n < 0.4375f * d, mid = n < 0.6875f * d;
  const float num = low ? n : mid ? __builtin_fmaf(2.0f, n, -d) : n - d;
  const float den = low ? d : mid ? __builtin_fmaf(2.0f, d, n) : d + n;
  const float t = num / den;
  const float z = t * t, w = z * z;
  constexpr float A0 = 3.3333328366e-01f, A1 = -1.9999158382e-01f, A2 = 1.4253635705e-01f, A3 = -1.0648017377e-01f,
                  A4 = 6.1687607318e-02f;
  const float s1 = z * __builtin_fmaf(w, __builtin_fmaf(w, A4, A2), A0);
  const float s2 = w * __builtin_fmaf(w, A3, A1);
  const float corr = t * (s1 + s2);
  const float hi = mid ? kHi0 : kHi1, lo = mid ? kLo0 : kLo1;
  return low ? t - corr : hi - ((corr - lo) - t);
}

EKM_HD float wind_atan2(float y, float x) {
  constexpr float kPi2Hi = 1.5707963705e+00f, kPi2Lo = -4.3711388287e-08f;
  constexpr float kPiHi = 3.1415927410e+00f, kPiLo = -8.7422776573e-08f;
  const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
  const bool swap = ay > ax;
  float d = swap ? ay : ax, n = swap ? ax : ay;
  if (d == __builtin_inff()) {
    n = n == __builtin_inff() ? 1.0f : 0.0f;
    d = 1.0f;
  }
  if (d == 0.0f) d = 1.0f;
  if (d > 0x1p+125f) {
    n *= 0.25f;
    d *= 0.25f;
  }
  if (d < 0x1p-100f) {
    n *= 0x1p+30f;
    d *= 0x1p+30f;
  }
  const float a = wind_atan_ratio(n, d);
  const bool west = __builtin_signbit(x);
  float r;
  if (swap)
    r = west ? kPi2Hi + (a + kPi2Lo) : kPi2Hi - (a - kPi2Lo);
  else
    r = west ? kPiHi - (a - kPiLo) : a;
  r = __builtin_signbit(y) ? -r : r;
  return (x != x || y != y) ? x + y : r;
}

// The direction in float, with the constants rounded to float as the reference's float32 run rounds them.  Where
// n / d underflows, d is -0 for a v < 0: the polar convention then still adds 360, as the true angle is negative (beside
// an infinite u it is exactly -0, and stays).
EKM_HD float wind_direction_of(float d, float u, float v, int mode) {
  constexpr float kMinusPi2 = (float)kWindMinusPi2, kPi15 = (float)kWindPi15, kDegree = (float)kWindDegree;
  if (mode == WIND_METEO) return d <= kMinusPi2 ? (kMinusPi2 - d) * kDegree : (kPi15 - d) * kDegree;
  const float deg = d * kDegree;
  return (mode == WIND_POLAR_POSITIVE && (deg < 0.0f || (v < 0.0f && __builtin_fabsf(u) < __builtin_inff()))) ? 360.0f + deg : deg;
}

EKM_HD void wind_sincos_deg(double x, double& s, double& c) { sol_sincos_deg(x, s, c); }

// sin and cos of x DEGREES in float.  |x| < 2^22: the reduction x - 360 rint(x / 360), t = r - 90 k is exact in float
// (each one fma), t * pi/180 is a float-float product, and the kernels on [-pi/4, pi/4] are polynomials of degree 9 and
// 10 (truncation below 0.03 ulp) with the low word as a correction: within 1.5 ulp.  Anything else -- larger angles,
// NaN, infinities -- takes the double routine and is rounded.
EKM_HD void wind_sincos_deg(float x, float& s, float& c) {
  if (!(__builtin_fabsf(x) < 4194304.0f)) {
    double sd, cd;
    sol_sincos_deg((double)x, sd, cd);
    s = (float)sd;
    c = (float)cd;
    return;
  }
  const float turns = __builtin_rintf(x * (1.0f / 360.0f));
  const float r = __builtin_fmaf(-turns, 360.0f, x);
  const float k = __builtin_rintf(r * (1.0f / 90.0f));
  const float t = __builtin_fmaf(-k, 90.0f, r);
  constexpr float kRadHi = 0x1.1df46ap-6f, kRadLo = 0x1.294e9cp-33f;  // pi / 180 = hi + lo
  const float y = t * kRadHi;
  const float yl = __builtin_fmaf(t, kRadLo, __builtin_fmaf(t, kRadHi, -y));
  const float z = y * y;
  constexpr float S1 = -1.6666667163e-01f, S2 = 8.3333337680e-03f, S3 = -1.9841270114e-04f, S4 = 2.7557314297e-06f;
  const float ps = __builtin_fmaf(z, __builtin_fmaf(z, __builtin_fmaf(z, S4, S3), S2), S1);
  const float sn = __builtin_fmaf(y * z, ps, yl) + y;
  constexpr float C1 = 4.1666667908e-02f, C2 = -1.3888889225e-03f, C3 = 2.4801587642e-05f, C4 = -2.7557314297e-07f;
  const float pc = z * __builtin_fmaf(z, __builtin_fmaf(z, __builtin_fmaf(z, C4, C3), C2), C1);
  const float hz = 0.5f * z;
  const float wc = 1.0f - hz;
  const float cs = wc + (((1.0f - wc) - hz) + __builtin_fmaf(z, pc, -(y * yl)));
  const int quad = (int)k & 3;
  const float s0 = (quad & 1) ? cs : sn;
  const float c0 = (quad & 1) ? sn : cs;
  s = (quad & 2) ? -s0 : s0;
  c = ((quad + 1) & 2) ? -c0 : c0;
}

// One point of one kind in the arithmetic W (float for float32 fields, else double): inputs a, b (coriolis: a alone),
// outputs o0, o1 (the polar kind: those of WHICH; coriolis: o0).
template <class W, int KIND, int MODE, int WHICH>
EKM_HD void wind_point(W a, W b, W& o0, W& o1) {
  o0 = o1 = W(0);
  if constexpr (KIND == WIND_KIND_POLAR) {
    if constexpr ((WHICH & WIND_SPEED) != 0) o0 = wind_hypot(a, b);
    if constexpr ((WHICH & WIND_DIRECTION) != 0) o1 = wind_direction_of(wind_atan2(b, a), a, b, MODE);
  } else if constexpr (KIND == WIND_KIND_XY) {
    W s, c;
    wind_sincos_deg(MODE == WIND_METEO ? W(270) - b : b, s, c);
    o0 = a * c;
    o1 = a * s;
  } else {
    W s, c;
    wind_sincos_deg(a, s, c);
    o0 = (W)kWindTwoOmega * s;
  }
}

// ---- wind rose ----
// Number of edges e[0..m) (non-decreasing) that are <= x, as np.searchsorted(e, x, side="right"): `guess` is corrected
// against its neighbours until e[k-1] <= x < e[k] holds, so any guess gives the same answer.  x is not NaN.
template <class Edges>
EKM_HD unsigned wind_count_le(Edges e, unsigned m, double x, unsigned guess) {
  unsigned k = guess > m ? m : guess;
  while (k < m && e(k) <= x) ++k;
  while (k > 0 && e(k - 1) > x) --k;
  return k;
}
template <class Edges>
EKM_HD unsigned wind_search_le(Edges e, unsigned m, double x) {  // the same count by bisection
  unsigned lo = 0, hi = m;
  while (lo < hi) {
    const unsigned mid = (lo + hi) >> 1;
    if (e(mid) <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Cell of one sample in the [ns - 1][nd - 1] table of np.histogram2d, or -1 if it is dropped: bin k holds
// e[k] <= x < e[k + 1], the last bin also x == e[last]; NaN and anything outside either axis drop the whole sample.
// `inv_step` = (nd - 1) / (de[nd - 1] - de[0]) (or 0): the sector's first guess is one multiply.
template <class SE, class DE>
EKM_HD int wind_cell(double speed, double dir, SE se, unsigned ns, DE de, unsigned nd, double inv_step) {
  if (speed != speed || dir != dir) return -1;
  unsigned ks = wind_search_le(se, ns, speed);
  if (speed == se(ns - 1)) ks = ns - 1;
  if (ks < 1 || ks > ns - 1) return -1;
  const double g = (dir - de(0)) * inv_step;
  const unsigned guess = g >= 0.0 && g < (double)nd ? (unsigned)g + 1u : 0u;
  unsigned kd = wind_count_le(de, nd, dir, guess);
  if (dir == de(nd - 1)) kd = nd - 1;
  if (kd < 1 || kd > nd - 1) return -1;
  return (int)((ks - 1) * (nd - 1) + (kd - 1));
}

// The finished table: the last direction column is added to the first and dropped, counts become doubles, and with
// `percent` each is count * 100 / total (both operations correctly rounded; 0 * 100 / 0 = NaN when nothing was counted).
EKM_HD double wind_rose_value(unsigned long long count, unsigned long long total, int percent) {
  const double c = (double)count;
  return percent ? c * 100.0 / (double)total : c;
}

}  // namespace ekm
