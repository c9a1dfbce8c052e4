// Reductions over the member axis of one grid point: Extreme Forecast Index, Shift of Tails and CRPS of an ensemble
// against a model climate or an analysis, per-point quantiles, and the Gumbel fit with its cdf and ppf.  One statement
// of the arithmetic for the gfx950 kernels (ensemble.hip) and the host test twin (host_twin.cpp).
// Reference: extreme/array/efi.py:34-89, extreme/array/sot.py:13-103, extreme/array/cpf.py:13-155,
// score/array/ensemble.py:34-82, stats/array/quantiles.py:18-84, stats/array/extreme_values.py:24-155.
//
// All of them work on the point's ensemble SORTED ascending; `s(j)` below reads sorted member j.  The results are held to
// the reference bit for bit, so every operation is rounded once in the reference's order: nothing is contracted into
// an fma (en_* below; the host twin is built with -ffp-contract=off), divisions are IEEE divisions, and the f64 sums
// run sequentially in the reference's loop order.
#pragma once

#include <cmath>

#include "thermo_math.hpp"

namespace ekm {

template <class T>
EKM_HD T en_add(T a, T b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a + b;
}
template <class T>
EKM_HD T en_sub(T a, T b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a - b;
}
template <class T>
EKM_HD T en_mul(T a, T b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a * b;
}

// numpy.maximum / numpy.minimum: a NaN in either operand comes back
EKM_HD double en_max(double a, double b) { return (a >= b || a != a) ? a : b; }
EKM_HD double en_min(double a, double b) { return (a <= b || a != a) ? a : b; }

// Member v goes into the sorted run s[0..k) (insertion from the top).  A NaN stays where it lands: every caller flags
// a column that holds one and gives it the reference's NaN, so its order is never read.
template <class T, class Get, class Set>
EKM_HD void ens_insert(unsigned k, T v, Get get, Set set) {
  unsigned j = k;
  while (j > 0) {
    const T u = get(j - 1);
    if (!(u > v)) break;
    set(j, u);
    --j;
  }
  set(j, v);
}

// Member v goes into the sorted run s[0..k) as numpy.sort orders it: a NaN above every number (cpf.py:140-143 sorts and
// then compares as usual, so the place of a NaN is read).
template <class T, class Get, class Set>
EKM_HD void ens_insert_nan_last(unsigned k, T v, Get get, Set set) {
  const bool v_nan = v != v;
  unsigned j = k;
  while (j > 0) {
    const T u = get(j - 1);
    if (!(u > v || (u != u && !v_nan))) break;
    set(j, u);
    --j;
  }
  set(j, v);
}

// A point's column of rows, row j at ptr[j * STRIDE]: the lane's LDS column in the kernels (STRIDE 64, lane-minor), a
// plain array in the host twin (STRIDE 1).  Reads as the `s(j)` of the routines below.
template <class T, unsigned STRIDE>
struct Column {
  T* ptr;
  EKM_HD T operator()(unsigned j) const { return ptr[j * STRIDE]; }
  EKM_HD void set(unsigned j, T v) const { ptr[j * STRIDE] = v; }
};

// Streams the `rows` values of one point (row j at base[j * stride]) into its column, kStageBatch loads in flight.
//  * Ascending: ens_insert; returns "a value is NaN".  zero_below: sot.py:88 (values below teps become 0 first).
//  * NanLast: as numpy.sort orders them (ens_insert_nan_last).  AsGiven: copied.
enum class ColumnOrder { Ascending, NanLast, AsGiven };
constexpr int kStageBatch = 8;

template <class T, ColumnOrder ORDER, class Col>
EKM_HD bool stage_column(const T* __restrict__ base, unsigned long long stride, unsigned rows, Col col,
                         bool zero_below = false, T teps = T(0)) {
  auto get = [&](unsigned j) -> T { return col(j); };
  auto set = [&](unsigned j, T v) { col.set(j, v); };
  bool has_nan = false;
  for (unsigned m0 = 0; m0 < rows; m0 += kStageBatch) {
    T v[kStageBatch];
#pragma unroll
    for (int b = 0; b < kStageBatch; ++b)
      if (m0 + b < rows) v[b] = base[(unsigned long long)(m0 + b) * stride];
#pragma unroll
    for (int b = 0; b < kStageBatch; ++b)
      if (m0 + b < rows) {
        if constexpr (ORDER == ColumnOrder::Ascending) {
          T x = v[b];
          if (zero_below && x < teps) x = T(0);
          has_nan = has_nan || x != x;
          ens_insert<T>(m0 + b, x, get, set);
        } else if constexpr (ORDER == ColumnOrder::NanLast) {
          ens_insert_nan_last<T>(m0 + b, v[b], get, set);
        } else {
          set(m0 + b, v[b]);
        }
      }
  }
  return has_nan;
}

// efi.py:40-89.  clim(i) is row i of the point's climate, read ONCE each, in order; it need not be sorted: the count
// of members <= clim(i) (efi.py:49) is the upper-bound rank in the sorted ensemble, found by a cursor that walks either
// way from the previous row's rank.  frac and dFdp are formed in T (zeros_like(clim), efi.py:46, 51, 55), the terms and
// the sum in double (the coefficient tables are float64, efi.py:57-60).  acosdiff, proddiff, acoef: nclim-1 values each.
template <class T, class Clim, class Sorted>
EKM_HD double efi_point(unsigned nclim, unsigned nens, bool ens_nan, Clim clim, Sorted s, const double* acosdiff,
                        const double* proddiff, const double* acoef, double eps) {
  const T tn = T(nens), scale = T(nclim - 1), teps = T(eps);
  const bool masked = eps > 0.0;
  unsigned cur = 0;
  auto rank = [&](T c) -> unsigned {
    while (cur > 0 && s(cur - 1) > c) --cur;
    while (cur < nens && s(cur) <= c) ++cur;
    return cur;
  };
  const T c0 = clim(0);
  bool missing = ens_nan || c0 != c0;
  T f0 = T(rank(c0)) / tn;
  double efi = 0.0, efimax = 0.0;
  for (unsigned icl = 0; icl + 1 < nclim; ++icl) {
    const T c1 = clim(icl + 1);
    missing = missing || c1 != c1;
    const T f1 = T(rank(c1)) / tn;
    const T dfdp = en_mul(en_sub(f1, f0), scale);
    const double a = (double)en_sub(en_mul(T(2), f0), T(1));
    const double d = en_sub(en_add(en_mul(a, acosdiff[icl]), en_mul(acoef[icl], (double)dfdp)), proddiff[icl]);
    if (masked) {
      const bool m = c1 > teps;  // efi.py:68
      efi = en_add(efi, m ? d : 0.0);
      efimax = en_add(efimax, m ? en_sub(-acosdiff[icl], proddiff[icl]) : 0.0);
    } else {
      efi = en_add(efi, d);
    }
    f0 = f1;
  }
  if (masked)
    efi = efi / en_max(efimax, eps);
  else
    efi = en_mul(efi, 2.0 / 3.14159265358979323846);
  return missing ? nan_v<double>() : efi;
}

// numpy.percentile(ens, q=perc, axis=0) with a Python int perc (method "linear"), as sot.py:91 calls it: the quantile
// is perc / T(100), the virtual index (n - 1) * quantile, gamma its fractional part -- all in T, the dtype of ens.
template <class T>
struct Percentile {
  unsigned lo, hi;
  T gamma;
};

template <class T>
inline Percentile<T> percentile_position(unsigned nens, int perc) {
  Percentile<T> p;
  const T q = T(perc) / T(100);
  const T vi = en_mul(T(nens - 1), q);
  if (vi >= T(nens - 1)) {  // numpy clips both neighbours to the last member and leaves -1 as "previous index"
    p.lo = p.hi = nens - 1;
    p.gamma = en_sub(vi, T(-1));
  } else {
    const T fl = std::floor(vi);
    p.lo = (unsigned)fl;
    p.hi = p.lo + 1;
    p.gamma = en_sub(vi, fl);
  }
  return p;
}

// numpy's _lerp(a, b, t)
template <class T>
EKM_HD T en_lerp(T a, T b, T t) {
  const T diff = en_sub(b, a);
  if (t >= T(0.5)) return en_sub(b, en_mul(diff, en_sub(T(1), t)));
  return en_add(a, en_mul(diff, t));
}

// sot.py:42-48
template <class T>
EKM_HD T sot_func_point(T qc_tail, T qc, T qf, T min_den, T lower, T upper) {
  const T den = en_sub(qc_tail, qc);
  T r = std::fabs(den) > min_den ? en_sub(qf, qc_tail) / den : nan_v<T>();
  if (r < lower) r = lower;
  if (r > upper) r = upper;
  return r;
}

// sot.py:85-103 for one point whose members were zeroed below eps (when eps > 0) BEFORE they were sorted (sot.py:88)
template <class T, class Sorted>
EKM_HD T sot_point(T qc, T qc_tail, bool ens_nan, Sorted s, Percentile<T> pos, double eps) {
  if (eps > 0.0 && qc < T(eps)) qc = T(0);  // sot.py:89
  const T qf = ens_nan ? nan_v<T>() : en_lerp(s(pos.lo), s(pos.hi), pos.gamma);
  return sot_func_point<T>(qc_tail, qc, qf, T(eps > 0.0 ? eps : 0.0), T(-10), T(10));
}

// cpf.py:13-91 for one point: the Crossing Point Forecast of the column ens(0..nens) against the climate column
// clim(0..nclim), both used as given (the caller sorts them or not, cpf.py:140-143).  The state of the reference's scan
// is three scalars per point: the value so far (float32, cpf.py:22), `done` (its `mask`) and `primed` (its `prim`).
// Climate row icl has level icl / (nclim-1), member iq level (iq+1) / (nens+1), both Python floats (float64) in the
// reference.  Two quotients of whole numbers below 2^32 that differ as fractions differ by far more than an ulp and
// equal fractions round alike, so "member level < row level" is decided exactly by cross-multiplying whole numbers; the
// first member at or above a row's level (`cross`) never moves down from one row to the next, so it is a cursor.
//  * members iq0 .. cross-1 prime the point where member >= row and nothing is written yet (cpf.py:41-43);
//  * member `cross` does the three writes in the reference's order (cpf.py:45-81), then the row is finished (cpf.py:84):
//    the lower-tail interpolation (only iq < 2; does not test `done`, sets it), the plain crossing (writes the member
//    level, sets `done`), the upper-tail interpolation against the top row (only the last member; does not set `done`,
//    so a later row may overwrite it).
// The interpolation runs in T: with f32 fields the Python-float levels act as f32 scalars (NumPy 2), with f64 fields
// everything is f64 and the store rounds to float32.  Once `done` is set and cross >= 2 no later row can change
// anything (priming, the plain crossing and the upper tail all need !done), so the scan stops there.
template <class T>
EKM_HD T cpf_intersection(T tau_c, T tau_c2, T qc, T qc2, T qf) {
  return en_add(en_mul(tau_c, en_sub(qc2, qf)), en_mul(tau_c2, en_sub(qf, qc))) / en_sub(qc2, qc);
}

template <class T, class Clim, class Ens>
EKM_HD float cpf_point(unsigned nclim, unsigned nens, bool from_zero, Clim clim, Ens ens) {
  float value = 0.0f;
  bool done = false, primed = false;
  if (nclim < 3 || nens < 1) return value;
  const unsigned iq0 = from_zero ? 0u : nens / 2;
  const unsigned long long dc = nclim - 1, df = (unsigned long long)nens + 1;
  const T top = clim(nclim - 1);
  unsigned cross = iq0;
  for (unsigned icl = 1; icl + 1 < nclim; ++icl) {
    while (cross < nens && (cross + 1ull) * dc < icl * df) ++cross;
    if (done && cross >= 2) break;
    const T qc = clim(icl);
    for (unsigned iq = iq0; iq < cross; ++iq)
      if (ens(iq) >= qc && !done) primed = true;
    if (cross >= nens) continue;  // no member reaches this row's level
    const T qf = ens(cross);
    if (cross < 2) {  // cpf.py:47-62
      const T qc2 = clim(icl - 1);
      if (qf < qc && qc2 < qc && primed) {
        const T tau_c = T((double)icl / ((double)nclim - 1.0)), tau_c2 = T((double)(icl - 1) / (double)(nclim - 1));
        // numpy.maximum(x, 0) as recorded: the 0 comes back unless x is above it (so -0.0 gives +0.0), a NaN stays
        const double x = (double)cpf_intersection<T>(tau_c, tau_c2, qc, qc2, qf);
        value = (float)((x > 0.0 || x != x) ? x : 0.0);
        done = true;
      }
    }
    if (qf < qc && !done && primed) {  // cpf.py:65-67
      value = (float)(((double)cross + 1.0) / ((double)nens + 1.0));
      done = true;
    }
    if (cross == nens - 1 && qf > qc && top > qc && !done && primed) {  // cpf.py:70-81
      const T tau_c = T((double)icl / ((double)nclim - 1.0));
      value = (float)en_min((double)cpf_intersection<T>(tau_c, T(1), qc, top, qf), 1.0);
    }
  }
  return value;
}

// cpf.py:145-155 and 86-89: `epsilon` zeroes the points whose last member is below it, compared in T, and is ignored
// when `symmetric`; `symmetric` replaces a direct value below 0.5 by 1 - (the value of the negated, row-reversed
// columns), formed in float32.  The reversed run does not depend on the direct one, so it runs only where it is read.
template <class T, class Clim, class Ens>
EKM_HD float cpf_value(unsigned nclim, unsigned nens, bool from_zero, bool symmetric, bool use_epsilon, T epsilon,
                       Clim clim, Ens ens) {
  float value = cpf_point<T>(nclim, nens, from_zero, clim, ens);
  if (symmetric) {
    if (value < 0.5f)
      value = en_sub(1.0f, cpf_point<T>(
                               nclim, nens, from_zero, [&](unsigned i) -> T { return -clim(nclim - 1 - i); },
                               [&](unsigned j) -> T { return -ens(nens - 1 - j); }));
  } else if (use_epsilon && ens(nens - 1) < epsilon) {
    value = 0.0f;
  }
  return value;
}

// cpf_point in O(nclim + nens) for the long member axes (long_cpf_tiles of long_ensemble.hip): the same arguments,
// accessors, cursor, three writes and early exit; only the priming step differs.  cpf_point asks, at every row, whether
// any member iq in [iq0, cross) has ens(iq) >= qc.  Here the members the cursor has passed are folded, once each, into
// the maximum of the non-NaN ones among them (`top_seen`, valid where `seen`), and the row asks top_seen >= qc.  The two
// are the same truth value for every qc:
//  * a NaN member compares false with every qc and is left out of the maximum; if qc is a NaN both sides are false;
//  * over the non-NaN members, max >= qc holds exactly where some member >= qc holds (the maximum is one of them, and
//    >= is transitive); -0.0 == +0.0, so which of the two zeros the maximum keeps decides nothing.
// Nothing in this assumes an order of the members, so it holds for sorted and as-given columns alike, and for the
// negated, reversed accessors of `symmetric` (they are just another pair of columns).  `primed` never goes back to
// false and `done` is read as cpf_point reads it, so every write happens at the same (row, member) with the same
// operands: the result is cpf_point's, bit for bit (tests/test_zz_long_cpf_cpu.py holds the two against each other).
template <class T, class Clim, class Ens>
EKM_HD float cpf_point_running(unsigned nclim, unsigned nens, bool from_zero, Clim clim, Ens ens) {
  float value = 0.0f;
  bool done = false, primed = false;
  if (nclim < 3 || nens < 1) return value;
  const unsigned iq0 = from_zero ? 0u : nens / 2;
  const unsigned long long dc = nclim - 1, df = (unsigned long long)nens + 1;
  const T top = clim(nclim - 1);
  unsigned cross = iq0;
  T top_seen = T(0);  // the largest non-NaN member of [iq0, cross)
  bool seen = false;  // there is one
  for (unsigned icl = 1; icl + 1 < nclim; ++icl) {
    while (cross < nens && (cross + 1ull) * dc < icl * df) {
      const T v = ens(cross);
      if (v == v && (!seen || v > top_seen)) {
        top_seen = v;
        seen = true;
      }
      ++cross;
    }
    if (done && cross >= 2) break;
    const T qc = clim(icl);
    if (seen && !done && top_seen >= qc) primed = true;
    if (cross >= nens) continue;  // no member reaches this row's level
    const T qf = ens(cross);
    if (cross < 2) {  // cpf.py:47-62
      const T qc2 = clim(icl - 1);
      if (qf < qc && qc2 < qc && primed) {
        const T tau_c = T((double)icl / ((double)nclim - 1.0)), tau_c2 = T((double)(icl - 1) / (double)(nclim - 1));
        const double x = (double)cpf_intersection<T>(tau_c, tau_c2, qc, qc2, qf);
        value = (float)((x > 0.0 || x != x) ? x : 0.0);
        done = true;
      }
    }
    if (qf < qc && !done && primed) {  // cpf.py:65-67
      value = (float)(((double)cross + 1.0) / ((double)nens + 1.0));
      done = true;
    }
    if (cross == nens - 1 && qf > qc && top > qc && !done && primed) {  // cpf.py:70-81
      const T tau_c = T((double)icl / ((double)nclim - 1.0));
      value = (float)en_min((double)cpf_intersection<T>(tau_c, T(1), qc, top, qf), 1.0);
    }
  }
  return value;
}

// cpf_value over cpf_point_running
template <class T, class Clim, class Ens>
EKM_HD float cpf_value_running(unsigned nclim, unsigned nens, bool from_zero, bool symmetric, bool use_epsilon, T epsilon,
                               Clim clim, Ens ens) {
  float value = cpf_point_running<T>(nclim, nens, from_zero, clim, ens);
  if (symmetric) {
    if (value < 0.5f)
      value = en_sub(1.0f, cpf_point_running<T>(
                               nclim, nens, from_zero, [&](unsigned i) -> T { return -clim(nclim - 1 - i); },
                               [&](unsigned j) -> T { return -ens(nens - 1 - j); }));
  } else if (use_epsilon && ens(nens - 1) < epsilon) {
    value = 0.0f;
  }
  return value;
}

// quantiles.py:60-84: one quantile level of one point.  The position record (lo, hi, w) of the level is computed by the
// host exactly as the reference (method "sort") or numpy.quantile (methods "numpy_bulk", "numpy") computes it; nothing is
// floored here.  `mode` is EKM_QUANTILE_SORT / EKM_QUANTILE_LERP of include/ekm_thermo.h:
constexpr int kQuantileSort = 0, kQuantileLerp = 1;
//  * EKM_QUANTILE_SORT (quantiles.py:76-83): s(lo) * (1 - w) + s(hi) * w with both products and the sum rounded once in
//    float64 (a NumPy float64 scalar promotes an f32 array).  No shortcut for w == 0: an infinite s(hi) gives NaN there,
//    as in the reference.
//  * EKM_QUANTILE_LERP (numpy's _lerp as numpy.quantile calls it): the difference s(hi) - s(lo) is formed in T, the
//    dtype of the data, then it and both members are promoted to Out, the dtype of gamma (float64 for "numpy_bulk", T for
//    "numpy"); for T == Out this is en_lerp.
template <class T, class Out, class Sorted>
EKM_HD Out quantile_point(bool col_nan, Sorted s, unsigned lo, unsigned hi, double w, int mode) {
  if (col_nan) return nan_v<Out>();
  const T a = s(lo), b = s(hi);
  if (mode == kQuantileSort)
    return Out(en_add(en_mul((double)a, en_sub(1.0, w)), en_mul((double)b, w)));
  const Out t = Out(w), diff = Out(en_sub(b, a));
  if (t >= Out(0.5)) return en_sub(Out(b), en_mul(diff, en_sub(Out(1), t)));
  return en_add(Out(a), en_mul(diff, t));
}

// The long-axis quantiles (long_quantiles.hip) sort whole-number keys, not floats: the order-preserving image of the
// float's bits (negative values: every bit flipped; the others: the sign bit set).  The order of the keys is total, so
// the sorted column is unique whatever network or library sorts it: -0.0 comes before +0.0 (NumPy leaves their order
// open).  A NaN takes the largest key, which is also what fills the padding slots; no number maps to it (+inf is
// 0xff80...).  A column with a NaN is flagged and never read, so that its NaNs lose their payload does not matter.
template <class T>
struct SortKey;
template <>
struct SortKey<float> {
  using type = unsigned;
  static constexpr type kMax = 0xffffffffu;
  static EKM_HD type of(float x) {
    type u;
    __builtin_memcpy(&u, &x, sizeof u);
    return x != x ? kMax : (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  static EKM_HD float value(type k) {
    const type u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float x;
    __builtin_memcpy(&x, &u, sizeof x);
    return x;
  }
};
template <>
struct SortKey<double> {
  using type = unsigned long long;
  static constexpr type kMax = 0xffffffffffffffffull;
  static EKM_HD type of(double x) {
    type u;
    __builtin_memcpy(&u, &x, sizeof u);
    return x != x ? kMax : (u >> 63) ? ~u : (u | 0x8000000000000000ull);
  }
  static EKM_HD double value(type k) {
    const type u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double x;
    __builtin_memcpy(&x, &u, sizeof x);
    return x;
  }
};

// ensemble.py:52-77 (Hersbach 2000).  The differences are formed in T, alpha and beta are float64 (xp.zeros), the sum
// over i = 0..nens runs in order, starting from the i = 0 term.  p2[i] = (i/n)^2, q2[i] = (1 - i/n)^2: nens+1 values.
template <class T, class Sorted>
EKM_HD double crps_point(unsigned n, T y, Sorted s, const double* p2, const double* q2) {
  double sum = 0.0;
  T xm = s(0);
  for (unsigned i = 0; i <= n; ++i) {
    double alpha, beta;
    if (i == 0) {
      alpha = 0.0;
      beta = en_max((double)en_sub(xm, y), 0.0);
    } else if (i == n) {
      alpha = en_max(-(double)en_sub(xm, y), 0.0);
      beta = 0.0;
    } else {
      const T xi = s(i);
      const double dxx = (double)en_sub(xi, xm);
      alpha = en_min(dxx, en_max(-(double)en_sub(xm, y), 0.0));
      beta = en_min(dxx, en_max((double)en_sub(xi, y), 0.0));
      xm = xi;
    }
    const double term = en_add(en_mul(alpha, p2[i]), en_mul(beta, q2[i]));
    sum = i == 0 ? term : en_add(sum, term);
  }
  return sum;
}

// extreme_values.py:44-64 (GumbelDistribution.fit) for one point: the first two sample L-moments of the column sorted
// ascending, formed as the reference's own lmoment (_polyfill.py:30-65) forms them, then sigma = l2 / log(2) and
// mu = l1 - sigma * 0.5772.  Everything is float64 whatever T is (an f32 sample is widened on read); every operation is
// rounded once, in the polyfill's order.  The polyfill's third sum is never read by `fit` and is not formed.  Infinities
// go through the arithmetic as written: a leading -inf gives -inf * 0 = NaN in s1.
template <class T, class Sorted>
EKM_HD void gumbel_fit_point(unsigned n, bool col_nan, Sorted s, double& mu, double& sigma) {
  double s0 = 0.0, s1 = 0.0;
  for (unsigned i = 0; i < n; ++i) {
    const double x = (double)s(i);
    s0 = en_add(s0, x);
    s1 = en_add(s1, en_mul(x, (double)i));
  }
  const double b0 = s0 / (double)n;
  const double b1 = s1 / en_mul((double)n, (double)(n - 1));
  const double l2 = en_add(en_mul(-1.0, b0), en_mul(2.0, b1));
  const double sg = l2 / 0.6931471805599453;  // numpy.log(2)
  const double m = en_sub(b0, en_mul(sg, 0.5772));
  mu = col_nan ? nan_v<double>() : m;
  sigma = col_nan ? nan_v<double>() : sg;
}

// extreme_values.py:76-92 (cdf) and :113-133 (value_to_return_period) for one point and one level.  `mode` is
// EKM_GUMBEL_CDF / EKM_GUMBEL_RETURN_PERIOD of include/ekm_thermo.h: the cdf, or freq / cdf by IEEE division, so the
// return period is freq / cdf formed from the same cdf bit for bit.
// The exponentials are the platform libm's `exp` (the device library's on gfx950), NOT the project's m_exp: m_exp is
// built to 4e-11 relative, which is right for the thermo bar, but the subtraction from 1 turns that into 4e-11 ABSOLUTE
// on the cdf -- a cdf can be 1e-12, and its reciprocal, the return period, is the product the user wants.
constexpr int kGumbelCdf = 0, kGumbelReturnPeriod = 1;
EKM_HD double gumbel_cdf_point(double mu, double sigma, double x, double freq, int mode) {
  const double z = en_sub(mu, x) / sigma;
  const double c = en_sub(1.0, ::exp(-::exp(z)));
  return mode == kGumbelReturnPeriod ? freq / c : c;
}

// extreme_values.py:94-110 (ppf) and :136-155 (return_period_to_value): mu - sigma * t, the product and then the
// difference, no fma.  t = log(-log(1 - p)) is computed by the host with NumPy exactly as the reference computes it (as
// for the quantile positions above); no logarithm is evaluated here, so the result is the reference's bit for bit.
EKM_HD double gumbel_ppf_point(double mu, double sigma, double t) { return en_sub(mu, en_mul(sigma, t)); }

// ---- one point p of a sorted-column kernel of ensemble.hip; the host twin loops over the same.  Fields: [rows, npts] ----

template <class T, class Col>
EKM_HD void efi_body(const T* clim, const T* ens, unsigned nclim, unsigned nens,
                     unsigned long long npts, unsigned long long p, double eps, const double* acosdiff,
                     const double* proddiff, const double* acoef, Col col,
                     double* out) {
  const bool has_nan = stage_column<T, ColumnOrder::Ascending>(ens + p, npts, nens, col);
  out[p] = efi_point<T>(
      nclim, nens, has_nan, [&](unsigned i) -> T { return clim[(unsigned long long)i * npts + p]; }, col, acosdiff,
      proddiff, acoef, eps);
}

template <class T, class Col>
EKM_HD void sot_body(const T* qc, const T* qc_tail, const T* ens, unsigned nens,
                     unsigned long long npts, unsigned long long p, Percentile<T> pos, double eps, Col col,
                     T* out) {
  const bool has_nan = stage_column<T, ColumnOrder::Ascending>(ens + p, npts, nens, col, eps > 0.0, T(eps));
  out[p] = sot_point<T>(qc[p], qc_tail[p], has_nan, col, pos, eps);
}

// missing: one flag byte per point, or null
template <class T, class Col>
EKM_HD void crps_body(const T* x, const T* y, unsigned nens, unsigned long long npts,
                      unsigned long long p, const double* p2, const double* q2, Col col,
                      double* out, unsigned char* missing) {
  const bool has_nan = stage_column<T, ColumnOrder::Ascending>(x + p, npts, nens, col);
  const T yp = y[p];
  const bool miss = has_nan || yp != yp;  // ensemble.py:44
  const double r = crps_point<T>(nens, yp, col, p2, q2);
  out[p] = miss ? nan_v<double>() : r;
  if (missing) missing[p] = miss ? 1 : 0;
}

// arr: [outer, m, inner]; the column of point p = o * inner + i starts here and has stride `inner`
template <class T>
EKM_HD const T* sample_column(const T* arr, unsigned m, unsigned long long inner, unsigned long long p) {
  const unsigned long long o = p / inner, i = p - o * inner;
  return arr + o * m * inner + i;
}

// extreme_values.py:44-64.  mu, sigma: float64 [npts].
template <class T, class Col>
EKM_HD void gumbel_fit_body(const T* sample, unsigned m, unsigned long long inner, unsigned long long p,
                            Col col, double* mu, double* sigma) {
  const bool has_nan = stage_column<T, ColumnOrder::Ascending>(sample_column<T>(sample, m, inner, p), inner, m, col);
  double mu_p, sigma_p;
  gumbel_fit_point<T>(m, has_nan, col, mu_p, sigma_p);
  mu[p] = mu_p;
  sigma[p] = sigma_p;
}

// cpf.py:13-155: what cpf_points of ensemble.hip reads in its `flags`
constexpr unsigned kCpfSortClim = 1, kCpfSortEns = 2, kCpfFromZero = 4, kCpfSymmetric = 8, kCpfEpsilon = 16;

inline unsigned cpf_flags(int sort_clim, int sort_ens, int from_zero, int symmetric, int use_epsilon) {
  return (sort_clim ? kCpfSortClim : 0) | (sort_ens ? kCpfSortEns : 0) | (from_zero ? kCpfFromZero : 0) |
         (symmetric ? kCpfSymmetric : 0) | (use_epsilon && !symmetric ? kCpfEpsilon : 0);
}

}  // namespace ekm
