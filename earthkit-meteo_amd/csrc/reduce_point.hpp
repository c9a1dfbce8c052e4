// Reductions along a long axis: the projection of fields onto weather-regime patterns, the standardisation of the
// projections into a regime index, the Pearson correlation of two arrays along one axis, and the NaN-skipping weighted
// mean along one axis.  One statement of the arithmetic for the gfx950 kernels (reduce.hip) and the host test twin
// (host_twin.cpp).
// Reference: regimes/array/index.py:10-76, score/array/deterministic.py:13-37, stats/array/numpy_extended.py:13-61.
//
// Where lanes share a sum, the ORDER is part of the statement: a lane forms its partial sum over the elements it owns in
// increasing index, the 64 partial sums of a wave are added by the butterfly wave_tree (lane i adds the value of lane
// i ^ 32, then i ^ 16, ... i ^ 1: every lane ends with the same bits, because a + b == b + a), and the sums of the waves
// of a workgroup are added in wave order.  The kernels do this with __shfl_xor and LDS, the twin with host_wave_tree
// over an array of 64 "lanes", so both give the same bits and neither depends on timing.  Nothing is contracted into an
// fma except where fma is written (en_* of ensemble_point.hpp; the twin is built with -ffp-contract=off).
#pragma once

#include <cmath>
#include <cstddef>

#include "ensemble_point.hpp"

namespace ekm {

constexpr int kWaveLanes = 64;
constexpr int kProjThreads = 256;  // project_fields: lanes of the workgroup that owns one field (four waves)
constexpr int kProjGroup = 8;      // patterns accumulated per pass over the field
constexpr int kProjVecBytes = 16;  // a lane reads the field and the coefficients in chunks of 16 bytes

EKM_HD float red_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
EKM_HD double red_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// V elements from an address that is aligned to its element only (a row of K elements starts anywhere when K is odd)
template <class T, int V>
EKM_HD void red_load(const T* src, T (&dst)[V]) {
  __builtin_memcpy(dst, src, sizeof(T) * V);
}

// index.py:52-56 for lane t of kProjThreads, one field row f[0..K) and NP coefficient rows c[p * K + k] (pattern times
// normalised weight, formed by the caller): acc[p] += f[k] * c[p][k] by one fma each, over the chunks t, t + 256, ... of
// 16 bytes, elements in increasing k.  Which lane owns an element depends on k alone, never on the row's address, so a
// field gives the same bits wherever it lies.  The accumulators are T: an f32 call accumulates in f32.
template <class T, int NP>
EKM_HD void project_partial(const T* f, const T* c, size_t K, unsigned t, T (&acc)[NP]) {
  constexpr int V = kProjVecBytes / (int)sizeof(T);
#pragma unroll
  for (int p = 0; p < NP; ++p) acc[p] = T(0);
  for (size_t k0 = (size_t)t * V; k0 < K; k0 += (size_t)kProjThreads * V) {
    if (k0 + V <= K) {
      T fv[V];
      red_load<T, V>(f + k0, fv);
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        T cv[V];
        red_load<T, V>(c + (size_t)p * K + k0, cv);
#pragma unroll
        for (int j = 0; j < V; ++j) acc[p] = red_fma(fv[j], cv[j], acc[p]);
      }
    } else {  // the ragged tail of the row: at most V - 1 elements, one lane
      for (size_t k = k0; k < K; ++k) {
        const T fk = f[k];
#pragma unroll
        for (int p = 0; p < NP; ++p) acc[p] = red_fma(fk, c[(size_t)p * K + k], acc[p]);
      }
    }
  }
}

// the sums of the waves of a workgroup, in wave order; then the modulator of the field (ModulatedPatterns), if any
template <class T>
EKM_HD T project_finish(const T* wave_sums, int nwaves, bool scaled, T scale) {
  T s = wave_sums[0];
  for (int w = 1; w < nwaves; ++w) s = en_add(s, wave_sums[w]);
  return scaled ? en_mul(scale, s) : s;
}

// index.py:76: (projection - mean) / std, the difference and then an IEEE division
template <class T>
EKM_HD T standardise_point(T proj, T mean, T std) {
  return en_sub(proj, mean) / std;
}

// deterministic.py:32-37 for one point whose m samples are read in order by x(i) and y(i): what NumPy computes when the
// sample axis is not the contiguous one (every reduction adds the rows one after the other, starting from the first):
// mean = (x0 + x1 + ...) / m; centre; norm = sqrt(xc0^2 + xc1^2 + ...); (xc / norm) * (yc / norm) summed in order.
// Three passes over the samples; every operation rounded once in T.  m == 1 and a constant column give 0 / 0 = NaN.
template <class T, class GetX, class GetY>
EKM_HD T pearson_point(size_t m, GetX x, GetY y) {
  T sx = x(0), sy = y(0);
  for (size_t i = 1; i < m; ++i) {
    sx = en_add(sx, x(i));
    sy = en_add(sy, y(i));
  }
  const T mx = sx / T(m), my = sy / T(m);
  T qx, qy;
  {
    const T dx = en_sub(x(0), mx), dy = en_sub(y(0), my);
    qx = en_mul(dx, dx);
    qy = en_mul(dy, dy);
  }
  for (size_t i = 1; i < m; ++i) {
    const T dx = en_sub(x(i), mx), dy = en_sub(y(i), my);
    qx = en_add(qx, en_mul(dx, dx));
    qy = en_add(qy, en_mul(dy, dy));
  }
  const T nx = std::sqrt(qx), ny = std::sqrt(qy);
  T r = en_mul(en_sub(x(0), mx) / nx, en_sub(y(0), my) / ny);
  for (size_t i = 1; i < m; ++i) r = en_add(r, en_mul(en_sub(x(i), mx) / nx, en_sub(y(i), my) / ny));
  return r;
}

// The same three passes when the sample axis IS the contiguous one: a wave owns the row, lane l the samples l, l + 64,
// ...; each pass ends in a wave_tree.  These are the lane's partial sums of the three passes.
template <class T>
EKM_HD T rows_partial_sum(const T* x, size_t m, unsigned lane) {
  T s = T(0);
  for (size_t i = lane; i < m; i += kWaveLanes) s = en_add(s, x[i]);
  return s;
}
template <class T>
EKM_HD T rows_partial_squares(const T* x, size_t m, unsigned lane, T mean) {
  T s = T(0);
  for (size_t i = lane; i < m; i += kWaveLanes) {
    const T d = en_sub(x[i], mean);
    s = en_add(s, en_mul(d, d));
  }
  return s;
}
template <class T>
EKM_HD T rows_partial_products(const T* x, const T* y, size_t m, unsigned lane, T mx, T my, T nx, T ny) {
  T s = T(0);
  for (size_t i = lane; i < m; i += kWaveLanes) s = en_add(s, en_mul(en_sub(x[i], mx) / nx, en_sub(y[i], my) / ny));
  return s;
}

// ---- nanaverage: the NaN-skipping (weighted) mean along one axis, reference stats/array/numpy_extended.py:13-61 ----
// Three layouts of [outer, m, inner] (m the averaged axis):
//   points (inner > 1)  one lane per output point walks its m samples in increasing index: NumPy's order along a
//                       non-contiguous axis, so the result is the reference's bit for bit (nanavg_point*);
//   rows   (inner == 1) one wave per row; lane l owns the 16-byte chunks l, l + 64, ... of the row (which lane owns an
//                       element depends on its index alone, never on the row's address), then the butterfly;
//   split  (inner == 1, few long rows) a row is cut into chunks of kNanSplitChunk elements, one workgroup of
//                       kNanSplitThreads lanes per (row, chunk): lanes own 16-byte chunks as above, butterfly per wave,
//                       the waves in wave order, one partial pair per chunk; a second kernel adds the pairs of a row in
//                       chunk order, starting from +0.  The number of chunks depends on m alone.
// Unweighted: sum of `isnan(d) ? +0 : d` from an accumulator that starts at +0, and the count of the others; the sum is
// divided by the count in double and rounded once to T (numpy.nanmean).
// Weighted, points: the reference's formula in its order, two passes: den = sum of w where neither d nor w is NaN (NaN
// terms enter as +0), then the sum of d * (w / den), a NaN product entering as +0; every quotient and product rounded once.
// Weighted, rows and split: ONE pass.  sum d * w (a NaN product enters as +0) and sum w (where neither is NaN) are formed
// together and divided once at the end; 0 / 0 (no valid sample, or weights that are all zero) gives +0 as the reference
// does.  This is not the reference's order of roundings (it normalises every weight by den first, which would cost a
// second pass over the row): the results are judged against the exact value within a rounding bound, tests/_nanaverage_numpy.py.
constexpr int kNanBatch = 8;                // samples a lane of nanavg_points has in flight before it adds them, in order
constexpr int kNanRowWaves = 4;             // nanavg_rows: rows (waves) per workgroup
constexpr int kNanSplitThreads = 256;       // nanavg_split: lanes of the workgroup that owns one chunk
constexpr size_t kNanSplitChunk = 32768;    // elements per chunk: a multiple of kNanSplitThreads * 16 B / sizeof(T)
constexpr size_t kNanSplitMinLen = 2 * kNanSplitChunk;  // path 0 takes split for rows at least this long ...
constexpr size_t kNanSplitMaxRows = 2048;   // ... when there are fewer rows than this (one wave per row would leave CUs idle)
constexpr int kNanAuto = 0, kNanPoints = 1, kNanRows = 2, kNanSplit = 3;

// the path of `path == 0`: a function of the shape alone
EKM_HD int nanavg_path(size_t nrows, size_t m, size_t inner) {
  if (inner != 1) return kNanPoints;
  return m >= kNanSplitMinLen && nrows < kNanSplitMaxRows ? kNanSplit : kNanRows;
}
EKM_HD size_t nanavg_chunks(size_t m) { return m == 0 ? 1 : (m + kNanSplitChunk - 1) / kNanSplitChunk; }

// the second accumulator: the sum of the weights (weighted), the count of valid samples (unweighted)
template <class T, bool W>
struct NanSecond {
  using type = T;
};
template <class T>
struct NanSecond<T, false> {
  using type = unsigned long long;
};
template <class T, bool W>
using nan_q_t = typename NanSecond<T, W>::type;

template <class T>
EKM_HD T nanavg_mean(T sum, unsigned long long count) {
  return (T)((double)sum / (double)count);  // 0 / 0 = NaN: an all-NaN or empty slice
}

template <class T, class Get>
EKM_HD T nanavg_point(size_t m, Get d) {
  T acc = T(0);
  unsigned long long cnt = 0;
  size_t i = 0;
  for (; i + kNanBatch <= m; i += kNanBatch) {
    T v[kNanBatch];
#pragma unroll
    for (int j = 0; j < kNanBatch; ++j) v[j] = d(i + j);
#pragma unroll
    for (int j = 0; j < kNanBatch; ++j) {
      acc = en_add(acc, v[j] != v[j] ? T(0) : v[j]);
      cnt += v[j] == v[j];
    }
  }
  for (; i < m; ++i) {
    const T v = d(i);
    acc = en_add(acc, v != v ? T(0) : v);
    cnt += v == v;
  }
  return nanavg_mean<T>(acc, cnt);
}

template <class T, class GetD, class GetW>
EKM_HD T nanavg_point_weighted(size_t m, GetD d, GetW w) {
  T den = T(0);
  size_t i = 0;
  for (; i + kNanBatch <= m; i += kNanBatch) {
    T dv[kNanBatch], wv[kNanBatch];
#pragma unroll
    for (int j = 0; j < kNanBatch; ++j) dv[j] = d(i + j), wv[j] = w(i + j);
#pragma unroll
    for (int j = 0; j < kNanBatch; ++j) den = en_add(den, (dv[j] != dv[j] || wv[j] != wv[j]) ? T(0) : wv[j]);
  }
  for (; i < m; ++i) {
    const T dv = d(i), wv = w(i);
    den = en_add(den, (dv != dv || wv != wv) ? T(0) : wv);
  }
  T acc = T(0);
  for (i = 0; i + kNanBatch <= m; i += kNanBatch) {
    T dv[kNanBatch], wv[kNanBatch];
#pragma unroll
    for (int j = 0; j < kNanBatch; ++j) dv[j] = d(i + j), wv[j] = w(i + j);
#pragma unroll
    for (int j = 0; j < kNanBatch; ++j) {
      const T p = en_mul(dv[j], wv[j] / den);
      acc = en_add(acc, p != p ? T(0) : p);
    }
  }
  for (; i < m; ++i) {
    const T p = en_mul(d(i), w(i) / den);
    acc = en_add(acc, p != p ? T(0) : p);
  }
  return acc;
}

// one sample of the contiguous paths
template <class T, bool W>
EKM_HD void nanavg_term(T d, T w, T& s, nan_q_t<T, W>& q) {
  if constexpr (W) {
    q = en_add(q, (d != d || w != w) ? T(0) : w);
    const T p = en_mul(d, w);
    s = en_add(s, p != p ? T(0) : p);
  } else {
    s = en_add(s, d != d ? T(0) : d);
    q += d == d;
  }
}
// two partial pairs
template <class T, bool W>
EKM_HD void nanavg_add(T& s, nan_q_t<T, W>& q, T ps, nan_q_t<T, W> pq) {
  s = en_add(s, ps);
  if constexpr (W)
    q = en_add(q, pq);
  else
    q += pq;
}

// Lane t of nthreads over the elements [begin, end) of a row d (weights w[k * ws], ws 1 or any other stride, 0 = one
// weight for the row): the 16-byte chunks t, t + nthreads, ... counted from `begin`, elements in increasing k.  `begin`
// is a multiple of nthreads * V, so the owner of an element depends on k alone.
template <class T, bool W>
EKM_HD void nanavg_partial(const T* d, const T* w, size_t ws, size_t begin, size_t end, unsigned t, unsigned nthreads, T& s,
                           nan_q_t<T, W>& q) {
  constexpr int V = kProjVecBytes / (int)sizeof(T);
  s = T(0);
  q = 0;
  size_t k0 = begin + (size_t)t * V;
#pragma unroll 4
  for (; k0 + V <= end; k0 += (size_t)nthreads * V) {
    T dv[V], wv[V];
    red_load<T, V>(d + k0, dv);
    if constexpr (W) {
      if (ws == 1) {
        red_load<T, V>(w + k0, wv);
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) wv[j] = w[(k0 + j) * ws];
      }
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) wv[j] = T(0);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) nanavg_term<T, W>(dv[j], wv[j], s, q);
  }
  for (size_t k = k0; k < end; ++k) {  // the ragged tail of the row: at most V - 1 elements, one lane
    T wk = T(0);
    if constexpr (W) wk = w[k * ws];
    nanavg_term<T, W>(d[k], wk, s, q);
  }
}

template <class T, bool W>
EKM_HD T nanavg_finish(T s, nan_q_t<T, W> q) {
  if constexpr (W)
    return (q == T(0) && s == T(0)) ? T(0) : s / q;
  else
    return nanavg_mean<T>(s, q);
}

// A chunk's pair as the split path stores it: two T.  A chunk holds at most kNanSplitChunk samples, so its count is
// exact in f32.  The pairs of a row are added in chunk order from (+0, 0).
template <class T, bool W>
EKM_HD T nanavg_split_total(const T* pairs, size_t nchunks) {
  T s = T(0);
  nan_q_t<T, W> q = 0;
  for (size_t c = 0; c < nchunks; ++c) nanavg_add<T, W>(s, q, pairs[2 * c], (nan_q_t<T, W>)pairs[2 * c + 1]);
  return nanavg_finish<T, W>(s, q);
}

// The butterfly over 64 values on the host: after it every entry holds the sum the kernels' lanes hold.
template <class T>
inline T host_wave_tree(T (&v)[kWaveLanes]) {
  for (int off = kWaveLanes / 2; off >= 1; off >>= 1) {
    T next[kWaveLanes];
    for (int i = 0; i < kWaveLanes; ++i) next[i] = en_add(v[i], v[i ^ off]);
    for (int i = 0; i < kWaveLanes; ++i) v[i] = next[i];
  }
  return v[0];
}

}  // namespace ekm
