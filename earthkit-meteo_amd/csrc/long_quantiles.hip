// Quantiles of a LONG sample axis on gfx950: stats.long_quantiles / ekm_long_quantiles_* (reference
// stats/array/quantiles.py:18-84).  quantile_points of ensemble.hip insertion-sorts one column per lane, O(m^2), and holds
// 64 columns in 64 KiB of LDS: 256 samples in f32, 128 in f64.  Here ONE WORKGROUP sorts a tile of whole columns together
// with a bitonic network over whole-number keys (SortKey, ensemble_point.hpp), O(m log^2 m), and then reads every level
// off the sorted columns with quantile_point, the arithmetic the short kernel and the host twin use.
//
// Tile: E = 256 * R keys (256 threads, R keys per thread in registers).  A column is padded to n = 2^k >= max(m, 32)
// slots with the largest key, so a tile holds C = E / n columns, each n-aligned: the network runs over the tile's index
// e with the direction taken from e's bits below n, which sorts every column at once.  The last tile has fewer than C
// live columns; its dead columns are all padding and go through the network like the others: NO THREAD RETURNS OR
// BRANCHES ROUND A BARRIER, every loop bound and branch that encloses one depends on kernel arguments only.
//   full tile   f32 R = 64 (16384 keys), f64 R = 32 (8192 keys): 64 KiB of keys, the cap of the sample axis;
//   small tile  f32 R = 16, f64 R = 8: 16 KiB of keys, taken when the padded column fits (more workgroups per CU).
// Thread t holds elements e = r * 256 + t (r < R).  A stage with partner distance j is then
//   j >= 256     in the thread's own registers (partner r ^ (j / 256)): no traffic at all;
//   64 <= j < 256 through LDS: every thread stores its keys at e and reads e ^ j -- the lanes of a wave touch consecutive
//                words in both, so no access has a bank conflict;
//   j < 64       a cross-lane move inside the wave (__shfl_xor).
// LDS layout: element e lives at e + e / n (one spare slot per column), E + E/32 slots declared.  Consecutive e of one
// column stay consecutive (the network stages and the tile load), and the same slot of consecutive columns, which is what
// the lanes of the read-out and of the strided load touch, is n + 1 apart: odd, so those are conflict-free too.
//
// Traffic: every sample is read once, nothing is written but out[k * npts + p].  With the sample axis last (inner == 1)
// a tile is ONE contiguous run of live * m elements: read 16 B per lane from the first 16-B boundary on, the ragged head
// and tail one element per lane, and scattered to (column, slot) with a multiply-high in place of the division by m.
// With inner > 1 a tile is m runs of `live` elements at stride `inner`: the lanes run along the columns, so a wave reads
// min(C, 64) consecutive elements per sample -- short runs when the columns are long.
#include <hip/hip_runtime.h>

#include "../../include/ekm_thermo.h"
#include "ensemble_point.hpp"
#include "launch_checks.hpp"
#include "map_kernel.hpp"

namespace ekm {

constexpr unsigned kLongThreads = 256;
constexpr unsigned kLongMinColumn = 32;            // the shortest padded column: at most E / 32 columns per tile
constexpr size_t kLongKeyBytes = 64 * 1024;        // the keys of a full tile: the cap of the sample axis
constexpr size_t kLongSmallKeyBytes = 16 * 1024;   // the keys of a small tile

// A thread's R keys: a vector value, so that they stay in registers whatever the optimiser makes of the loops round them
template <class K, int R>
using LongKeys = K __attribute__((ext_vector_type(R)));

template <class K>
__device__ __forceinline__ K long_pick(K a, K b, bool keep_min) {
  const K mn = a < b ? a : b, mx = a < b ? b : a;
  return keep_min ? mn : mx;
}

// Partner distance j = JR * 256: both keys are the thread's own.  kr: the stage's direction bit over 256.
template <class K, int R, int JR>
__device__ __forceinline__ void long_register_stage(LongKeys<K, R>& key, unsigned kr) {
#pragma unroll
  for (int r = 0; r < R; ++r)
    if ((r & JR) == 0) {
      const bool up = ((unsigned)r & kr) == 0;
      const K a = key[r], b = key[r | JR];
      key[r] = long_pick(a, b, up);
      key[r | JR] = long_pick(a, b, !up);
    }
}

template <class K, int R, int JR>
__device__ __forceinline__ void long_register_stages(LongKeys<K, R>& key, unsigned jr, unsigned kr) {
  if constexpr (JR < R) {
    if (jr == JR)
      long_register_stage<K, R, JR>(key, kr);
    else
      long_register_stages<K, R, JR * 2>(key, jr, kr);
  }
}

template <class T, class Out, int R>
__global__ __launch_bounds__(kLongThreads) void long_quantile_tiles(const T* __restrict__ arr, unsigned m, unsigned log2n,
                                                                    unsigned magic, unsigned long long inner,
                                                                    unsigned long long npts, const double* __restrict__ lo,
                                                                    const double* __restrict__ hi, const double* __restrict__ w,
                                                                    unsigned nq, int mode, Out* __restrict__ out) {
  using Key = SortKey<T>;
  using K = typename Key::type;
  constexpr unsigned E = R * kLongThreads;
  constexpr unsigned V = 16 / sizeof(T);
  struct alignas(16) Vec {
    T v[V];
  };
  __shared__ K lds[E + E / kLongMinColumn];
  __shared__ unsigned col_nan[E / kLongMinColumn];

  const unsigned t = threadIdx.x;
  const unsigned n = 1u << log2n, columns = E >> log2n;
  const unsigned long long p0 = (unsigned long long)blockIdx.x * columns;
  const unsigned live = npts - p0 < columns ? (unsigned)(npts - p0) : columns;  // >= 1: the grid is ceil(npts / columns)
  auto slot = [&](unsigned e) -> unsigned { return e + (e >> log2n); };

  // ---- the tile into LDS as keys: padding first (slots past m, dead columns), then the samples ----
  for (unsigned c = t; c < columns; c += kLongThreads) col_nan[c] = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const unsigned e = (unsigned)r * kLongThreads + t;
    if ((e & (n - 1)) >= m || (e >> log2n) >= live) lds[slot(e)] = Key::kMax;
  }
  __syncthreads();  // the flags are zero before any is raised
  if (inner == 1) {
    const T* run = arr + p0 * m;
    const unsigned len = live * m;
    unsigned head = (unsigned)((16 - reinterpret_cast<uintptr_t>(run) % 16) % 16 / sizeof(T));
    if (head > len) head = len;
    const unsigned nvec = (len - head) / V, tail = head + nvec * V;
    auto place = [&](unsigned q, T x) {
      const unsigned c = m == 1 ? q : __umulhi(q, magic);  // q / m: exact for q * m < 2^32 (launch_long_quantiles)
      if (x != x) col_nan[c] = 1;
      lds[slot((c << log2n) + (q - c * m))] = Key::of(x);
    };
    for (unsigned v = t; v < nvec; v += kLongThreads) {
      const Vec x = *reinterpret_cast<const Vec*>(run + head + v * V);
#pragma unroll
      for (unsigned u = 0; u < V; ++u) place(head + v * V + u, x.v[u]);
    }
    if (t < head) place(t, run[t]);
    if (t < len - tail) place(tail + t, run[tail + t]);
  } else {
    const unsigned log2c = 31 - __builtin_clz(columns);
    const unsigned log2w = log2c < 8 ? log2c : 8;  // lanes along the columns, the rest of the workgroup along the samples
    const unsigned width = 1u << log2w, rows = kLongThreads >> log2w;
    for (unsigned c = t & (width - 1); c < live; c += width) {
      const T* col = sample_column<T>(arr, m, inner, p0 + c);
#pragma unroll 4
      for (unsigned i = t >> log2w; i < m; i += rows) {
        const T x = col[(unsigned long long)i * inner];
        if (x != x) col_nan[c] = 1;
        lds[slot((c << log2n) + i)] = Key::of(x);
      }
    }
  }
  __syncthreads();
  LongKeys<K, R> key;
#pragma unroll
  for (int r = 0; r < R; ++r) key[r] = lds[slot((unsigned)r * kLongThreads + t)];

  // ---- the bitonic network: merges of k = 2, 4, .. n, each in stages of partner distance j = k/2 .. 1 ----
  for (unsigned k = 2; k <= n; k <<= 1) {
    const unsigned dir = k & (n - 1);  // the index bit that turns a run downwards; none in the last merge
    for (unsigned j = k >> 1; j > 0; j >>= 1) {
      if (j >= kLongThreads) {
        long_register_stages<K, R, 1>(key, j / kLongThreads, dir / kLongThreads);
      } else if (j >= 64) {
        __syncthreads();  // every read of the stage (or of the load) before is done
#pragma unroll
        for (int r = 0; r < R; ++r) lds[slot((unsigned)r * kLongThreads + t)] = key[r];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const unsigned e = (unsigned)r * kLongThreads + t;
          key[r] = long_pick(key[r], lds[slot(e ^ j)], ((e & j) == 0) == ((e & dir) == 0));
        }
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const unsigned e = (unsigned)r * kLongThreads + t;
          key[r] = long_pick(key[r], (K)__shfl_xor(key[r], (int)j), ((e & j) == 0) == ((e & dir) == 0));
        }
      }
    }
  }

  // ---- the sorted columns back to LDS, every level read off them: lanes along the columns, out[k * npts + p] ----
  __syncthreads();
#pragma unroll
  for (int r = 0; r < R; ++r) lds[slot((unsigned)r * kLongThreads + t)] = key[r];
  __syncthreads();
  const unsigned long long items = (unsigned long long)nq * columns;
  for (unsigned long long idx = t; idx < items; idx += kLongThreads) {
    const unsigned c = (unsigned)idx & (columns - 1), k = (unsigned)(idx >> (31 - __builtin_clz(columns)));
    if (c >= live) continue;
    auto s = [&](unsigned i) -> T { return Key::value(lds[slot((c << log2n) + i)]); };
    out[(unsigned long long)k * npts + p0 + c] =
        quantile_point<T, Out>(col_nan[c] != 0, s, (unsigned)lo[k], (unsigned)hi[k], w[k], mode);
  }
}

template <class T, class Out, int R>
static void launch_long_tiles(unsigned grid, void* stream, const T* arr, uint32_t m, unsigned log2n, size_t inner,
                              size_t npts, const double* lo, const double* hi, const double* w, uint32_t nq, int mode,
                              Out* out) {
  const unsigned magic = m > 1 ? (unsigned)((1ull << 32) / m + 1) : 0;
  hipLaunchKernelGGL((long_quantile_tiles<T, Out, R>), dim3(grid), dim3(kLongThreads), 0, static_cast<hipStream_t>(stream), arr,
                     m, log2n, magic, (unsigned long long)inner, (unsigned long long)npts, lo, hi, w, nq, mode, out);
}

template <class T, class Out>
static int launch_long_quantiles(int dev, void* stream, const T* arr, size_t outer, uint32_t m, size_t inner,
                                 const double* lo, const double* hi, const double* w, uint32_t nq, int mode, Out* out) {
  constexpr unsigned kCap = kLongKeyBytes / sizeof(T), kSmall = kLongSmallKeyBytes / sizeof(T);
  // (a tile's run of at most kCap elements and a sample count of at most kCap: q * m < 2^32 in the kernel's q / m)
  static_assert((unsigned long long)kCap * kCap < (1ull << 32), "the multiply-high division of the tile load");
  if (outer == 0 || inner == 0 || nq == 0) return EKM_OK;
  if (mode != EKM_QUANTILE_SORT && mode != EKM_QUANTILE_LERP)
    return set_error(EKM_ERR_ENUM, "long_quantiles: mode=%d is not EKM_QUANTILE_SORT or EKM_QUANTILE_LERP", mode);
  if (mode == EKM_QUANTILE_SORT && sizeof(Out) != sizeof(double))
    return set_error(EKM_ERR_ARG,
                     "long_quantiles: EKM_QUANTILE_SORT gives float64 (use ekm_long_quantiles_f32_f64 for float input)");
  if (inner > ~(size_t)0 / outer) return set_error(EKM_ERR_ARG, "long_quantiles: too many points");
  const size_t npts = outer * inner;
  if (!lo || !hi || !w) return set_error(EKM_ERR_ARG, "long_quantiles: null position table");
  int rc = check_pointers("long_quantiles", sizeof(Out), {out});
  if (rc != EKM_OK) return rc;
  if (m < 1) return set_error(EKM_ERR_ARG, "long_quantiles: at least one sample is required");
  if (m > kCap)
    return set_error(EKM_ERR_ARG, "long_quantiles: %u samples are past the cap of %u (one column, padded to a power of two, in "
                     "%zu KiB of LDS)", m, kCap, kLongKeyBytes / 1024);
  if ((rc = check_pointers("long_quantiles", sizeof(T), {arr})) != EKM_OK) return rc;
  unsigned log2n = 5;  // kLongMinColumn
  while ((1u << log2n) < m) ++log2n;
  const bool small = (1u << log2n) <= kSmall;
  unsigned grid;
  if ((rc = launch_grid("long_quantiles", npts, (small ? kSmall : kCap) >> log2n, &grid)) != EKM_OK) return rc;
  if ((rc = use_device(dev)) != EKM_OK) return rc;
  if (small)
    launch_long_tiles<T, Out, kSmall / kLongThreads>(grid, stream, arr, m, log2n, inner, npts, lo, hi, w, nq, mode, out);
  else
    launch_long_tiles<T, Out, kCap / kLongThreads>(grid, stream, arr, m, log2n, inner, npts, lo, hi, w, nq, mode, out);
  return launched("long_quantiles");
}

}  // namespace ekm

extern "C" {

int ekm_long_quantiles_f32(int dev, void* stream, const float* arr, size_t outer, uint32_t m, size_t inner, const double* lo,
                           const double* hi, const double* w, uint32_t nq, int mode, float* out) {
  return ekm::launch_long_quantiles<float, float>(dev, stream, arr, outer, m, inner, lo, hi, w, nq, mode, out);
}
int ekm_long_quantiles_f64(int dev, void* stream, const double* arr, size_t outer, uint32_t m, size_t inner, const double* lo,
                           const double* hi, const double* w, uint32_t nq, int mode, double* out) {
  return ekm::launch_long_quantiles<double, double>(dev, stream, arr, outer, m, inner, lo, hi, w, nq, mode, out);
}
int ekm_long_quantiles_f32_f64(int dev, void* stream, const float* arr, size_t outer, uint32_t m, size_t inner,
                               const double* lo, const double* hi, const double* w, uint32_t nq, int mode, double* out) {
  return ekm::launch_long_quantiles<float, double>(dev, stream, arr, outer, m, inner, lo, hi, w, nq, mode, out);
}

}  // extern "C"
