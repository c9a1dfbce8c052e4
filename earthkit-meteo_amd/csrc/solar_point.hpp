// Cosine of the solar zenith angle at one grid point, summed over time nodes: the instantaneous value, its time average
// and the top-of-atmosphere incident radiation.  One statement of the arithmetic for the gfx950 kernel (solar.hip) and
// the host test twin (host_twin.cpp).
// Reference: solar/array/solar.py:51-96 (cos_solar_zenith_angle), :99-179 (_integrate), :232-254 (toa).
//
// Every function of the reference is the same sum over time nodes n,
//   acc += w[n] * (isr[n] * clip0(sd[n] * sin(lat) + cd[n] * cos(lat) * cos(rad(h15[n] + lon + tc[n])))),
// with sd / cd the sine / cosine of the node's declination, h15 its integer-hour angle and tc its time correction: all
// of them host-made (ekm_hip/solar.py builds them operation for operation as the reference does).  The node angle
// a[n] = h15[n] + tc[n] is applied by angle addition,
//   cos(rad(lon + a)) = cos(rad lon) cos(rad a) - sin(rad lon) sin(rad a),
// so the point pays ONE sine/cosine pair of lon and one of lat, and every node two fma, a product, a compare-select and
// the accumulate.  The node record is five doubles: p = sd, q = cd * cos(rad a), r = -cd * sin(rad a), w, isr.
//
// The sine and cosine are written here, for host and device alike: the arguments are DEGREES, so the reduction is exact
// (x - 360 * rint(x / 360) and t = x - 90 * k are representable and each is one fma), pi/180 is applied to |t| <= 45 as
// a double-double product, and the kernels on [-pi/4, pi/4] are the classic minimax polynomials with the low word of the
// argument carried as a correction (error below 1 ulp).  No call into a math library, no table, no private array.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "thermo_math.hpp"

namespace ekm {

constexpr int kSolarRecord = 5;  // doubles per time node: p, q, r, w, isr

EKM_HD double sol_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// x modulo 360 for |x| >= 2^52 (every such double is a whole number m * 2^e, e >= 0), exactly, in whole-number arithmetic:
// no longitude is that large, but a finite input must give a finite cosine as it does in the reference.
EKM_HD double sol_mod360_huge(double x) {
  uint64_t bits;
#if defined(__HIP_DEVICE_COMPILE__)
  bits = (uint64_t)__double_as_longlong(x);
#else
  std::memcpy(&bits, &x, sizeof bits);
#endif
  const uint64_t m = (bits & 0x000fffffffffffffull) | 0x0010000000000000ull;
  const int e = (int)((bits >> 52) & 0x7ff) - 1075;  // x = +-m * 2^e
  uint64_t r = m % 360u;
  for (int i = 0; i < e; ++i) {
    r <<= 1;  // < 720
    if (r >= 360u) r -= 360u;
  }
  const double v = (double)r;
  return (bits >> 63) ? -v : v;
}

// sin and cos of x DEGREES.  NaN for NaN and for +-inf.
EKM_HD void sol_sincos_deg(double x, double& s, double& c) {
  if (__builtin_fabs(x) >= 4503599627370496.0 && __builtin_fabs(x) < __builtin_inf()) x = sol_mod360_huge(x);
  const double turns = __builtin_rint(x * (1.0 / 360.0));
  const double r = sol_fma(-turns, 360.0, x);           // exact; |r| <= 180 (+ one ulp of the quotient's rounding)
  const double k = __builtin_rint(r * (1.0 / 90.0));    // -2 .. 2
  const double t = sol_fma(-k, 90.0, r);                // exact; |t| <= 45
  // y + yl = t * pi/180 to about 2^-106 relative
  constexpr double kRadHi = 0x1.1df46a2529d39p-6, kRadLo = 0x1.5c1d8becdd291p-62;
  const double y = t * kRadHi;
  const double yl = sol_fma(t, kRadLo, sol_fma(t, kRadHi, -y));
  const double z = y * y;
  // sin(y + yl), |y| <= pi/4
  constexpr double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                   S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  const double v = z * y;
  const double ps = sol_fma(z, sol_fma(z, sol_fma(z, sol_fma(z, S6, S5), S4), S3), S2);
  const double sn = y - (sol_fma(z, sol_fma(0.5, yl, -(v * ps)), -yl) - v * S1);
  // cos(y + yl)
  constexpr double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                   C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  const double pc = z * sol_fma(z, sol_fma(z, sol_fma(z, sol_fma(z, sol_fma(z, C6, C5), C4), C3), C2), C1);
  const double hz = 0.5 * z;
  const double wc = 1.0 - hz;
  const double cs = wc + (((1.0 - wc) - hz) + sol_fma(z, pc, -(y * yl)));
  // quadrant: (k mod 4) quarter turns
  const int quad = k == k ? ((int)k & 3) : 0;  // (x NaN or infinite: sn and cs are NaN already)
  const double s0 = (quad & 1) ? cs : sn;
  const double c0 = (quad & 1) ? sn : cs;
  s = (quad & 2) ? -s0 : s0;
  c = ((quad + 1) & 2) ? -c0 : c0;
}

// What the node loop needs of one point: a = sin(lat), b = cos(lat) cos(lon), c = cos(lat) sin(lon).
struct SolarPoint {
  double a, b, c;
};

EKM_HD SolarPoint solar_prepare(double lat, double lon) {
  double slat, clat, slon, clon;
  sol_sincos_deg(lat, slat, clat);
  sol_sincos_deg(lon, slon, clon);
  SolarPoint pt;
  pt.a = slat;
  pt.b = clat * clon;
  pt.c = clat * slon;
  return pt;
}

// clip(z, 0, None) of the reference: a NaN stays a NaN
EKM_HD double sol_clip0(double z) { return z < 0.0 ? 0.0 : z; }

// One node: w * (isr * clip0(p * a + q * b + r * c)) added to acc.
EKM_HD double solar_node(const SolarPoint& pt, double acc, double p, double q, double r, double w, double isr) {
  const double z = sol_fma(p, pt.a, sol_fma(q, pt.b, r * pt.c));
  return sol_fma(w, isr * sol_clip0(z), acc);
}

// All nodes of one point; `rec(n, j)` reads value j of node n.  Out is rounded once, here.
template <class Out, class Rec>
EKM_HD Out solar_point(double lat, double lon, unsigned nnodes, Rec rec) {
  const SolarPoint pt = solar_prepare(lat, lon);
  double acc = 0.0;
  for (unsigned n = 0; n < nnodes; ++n) acc = solar_node(pt, acc, rec(n, 0), rec(n, 1), rec(n, 2), rec(n, 3), rec(n, 4));
  return (Out)acc;
}

}  // namespace ekm
