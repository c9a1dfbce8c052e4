// Reductions along a long axis: the projection of fields onto weather-regime patterns, the standardisation of the
// projections into a regime index, and the Pearson correlation of two arrays along one axis.  One statement of the
// arithmetic for the gfx950 kernels (reduce.hip) and the host test twin (host_twin.cpp).
// Reference: regimes/array/index.py:10-76, score/array/deterministic.py:13-37.
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
