// Vertical interpolation of one column to one target: bracket -> weight -> blend, and the pressure of a hybrid full
// level formed from A, B, sp.  One statement of the arithmetic for the gfx950 kernels (interp.hip) and the host test
// twin (host_twin.cpp).  Reference: vertical/array/monotonic.py (MonotonicInterpolator), vertical/array/vertical.py:663, 708.
//
// The bracket decision and the NaN pattern are discontinuous in the coordinate, so every operation here is rounded
// once, in the reference's order: no a*b+c is contracted into an fma (device code contracts by default; the host twin
// is built with -ffp-contract=off), divisions are IEEE divisions.
//
// Levels are addressed in the reference's DESCENDING VIEW: view level 0 holds the largest coordinate.  The reference
// flips data and coord in memory when coord[0] < coord[-1] in the first column (monotonic.py:82-91); here the caller
// passes that decision as `descending` and view level v is memory level v (descending) or nlev-1-v (ascending).
#pragma once

#include <cmath>

#include "thermo_math.hpp"

namespace ekm {

enum InterpMode { INTERP_LINEAR = 0, INTERP_LOG = 1, INTERP_NEAREST = 2 };

template <class T>
EKM_HD T ip_add(T a, T b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a + b;
}
template <class T>
EKM_HD T ip_sub(T a, T b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a - b;
}
template <class T>
EKM_HD T ip_mul(T a, T b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a * b;
}

// p_full[k] = p_half[k] + 0.5*(p_half[k+1] - p_half[k]),  p_half[h] = A[h] + B[h]*sp   (vertical.py:663, 708)
template <class T>
EKM_HD T hybrid_p_full(T a0, T b0, T a1, T b1, T sp) {
  const T ph0 = ip_add(a0, ip_mul(b0, sp));
  const T ph1 = ip_add(a1, ip_mul(b1, sp));
  return ip_add(ph0, ip_mul(T(0.5), ip_sub(ph1, ph0)));
}

// Height from geopotential as interpolate_pressure_to_height_levels forms it (vertical.py:1593-1601, 344, 500-501):
// mode 2 geometric above sea, 3 geopotential height above sea, 4 geometric above ground, 5 geopotential above ground
template <class T>
EKM_HD T height_from_geopotential(T z, T zs, int mode) {
  const T g = T(k::g), re = T(6371229.0);  // constants/constants.py:53, 57
  if (mode == 3) return z / g;
  if (mode == 5) return ip_sub(z, zs) / g;
  const T zz = z / g;
  const T h = ip_mul(re, zz) / ip_sub(re, zz);
  if (mode == 2) return h;
  const T zzs = zs / g;
  return ip_sub(h, ip_mul(re, zzs) / ip_sub(re, zzs));
}

// numpy.isclose(x, y) with its default rtol = 1e-5, atol = 1e-8, in the arithmetic dtype:
// |x - y| <= atol + rtol*|y| and y finite, or x == y
template <class T>
EKM_HD bool ip_isclose(T x, T y) {
  const T lim = ip_add(T(1e-8), ip_mul(T(1e-5), std::fabs(y)));
  const bool y_finite = ip_sub(y, y) == T(0);
  return (std::fabs(ip_sub(x, y)) <= lim && y_finite) || x == y;
}

// monotonic.py:360-370
template <class T>
EKM_HD T interp_factor(T c_top, T c_bottom, T tc, int mode) {
  if (mode == INTERP_LINEAR) return ip_sub(tc, c_bottom) / ip_sub(c_top, c_bottom);
  if (mode == INTERP_LOG) {
    const T lb = std::log(c_bottom);
    return ip_sub(std::log(tc), lb) / ip_sub(std::log(c_top), lb);
  }
  return std::fabs(ip_sub(c_top, tc)) < std::fabs(ip_sub(c_bottom, tc)) ? T(1) : T(0);
}

// (1.0 - factor) * d_bottom + factor * d_top   (monotonic.py:247, 275, 295): `nearest` takes the same blend, so a
// non-finite value at the unused end of the bracket propagates as it does in the reference
template <class T>
EKM_HD T interp_blend(T f, T d_bottom, T d_top) {
  return ip_add(ip_mul(ip_sub(T(1), f), d_bottom), ip_mul(f, d_top));
}

// idx = count(coord > tc) of a column that descends in the view (monotonic.py:192), by bisection: at most
// ceil(log2(nlev + 1)) probes, every probe inside [0, nlev), whatever the column holds.  A NaN coordinate or target
// compares false everywhere: idx = 0.  `coord(m)` is the coordinate at MEMORY level m.
template <class T, class Coord>
EKM_HD unsigned interp_bracket(unsigned nlev, int descending, T tc, Coord coord) {
  unsigned lo = 0, hi = nlev;
  while (lo < hi) {
    const unsigned mid = (lo + hi) >> 1;
    const T c = coord(descending ? mid : nlev - 1 - mid);
    if (c > tc)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// An aux layer beyond one end of the column (monotonic.py:15-46): active when `on`
template <class T>
struct InterpAux {
  bool on;
  T coord, data;
};

// The value at the target given its bracket index (monotonic.py:179-295).  `bottom` is the aux layer beyond view level
// 0 (the reference's aux_max_level_*), `top` the one beyond view level nlev-1 (aux_min_level_*).
template <class T, class Coord, class Data>
EKM_HD T interp_value(unsigned idx, unsigned nlev, int descending, int mode, T tc, Coord coord, Data data,
                      InterpAux<T> bottom, InterpAux<T> top) {
  if (idx == 0 || idx >= nlev) {  // outside the column
    const bool below = idx == 0;
    const unsigned m = (below == (descending != 0)) ? 0u : nlev - 1;  // memory level of the end level
    const InterpAux<T> aux = below ? bottom : top;
    const T d_end = data(m);
    if (!aux.on) {
      if (mode == INTERP_NEAREST) return d_end;
      return ip_isclose(coord(m), tc) ? d_end : nan_v<T>();  // monotonic.py:229-233, 254-258
    }
    const T c_end = coord(m);
    if (below) {
      // AuxBottomLayer: the aux level where it lies strictly beyond the end level, else the end level itself;
      // used when it is strictly beyond and reaches the target (monotonic.py:27-29, 236)
      if (!(aux.coord > c_end && aux.coord >= tc)) return nan_v<T>();
      return interp_blend(interp_factor(c_end, aux.coord, tc, mode), aux.data, d_end);
    }
    if (!(aux.coord < c_end && aux.coord <= tc)) return nan_v<T>();  // monotonic.py:44-46, 263
    return interp_blend(interp_factor(aux.coord, c_end, tc, mode), d_end, aux.data);
  }
  const unsigned mt = descending ? idx : nlev - 1 - idx;
  const unsigned mb = descending ? idx - 1 : nlev - idx;
  return interp_blend(interp_factor(coord(mt), coord(mb), tc, mode), data(mb), data(mt));
}

}  // namespace ekm
