// The tile sort of the long-axis kernels on gfx950 (long_ensemble.hip; long_quantiles.hip states the same phases in its
// own kernel body): ONE WORKGROUP sorts a tile of whole columns together with a bitonic network over whole-number keys
// (SortKey, ensemble_point.hpp), O(m log^2 m).  The phases, each a __forceinline__ device function of the 256 threads:
//   long_tile_pad      the flags to zero, the padding slots (past m, dead columns) to the largest key;
//   long_tile_load_run / long_tile_load_strided
//                      the samples to keys in LDS with the per-column NaN flag, a per-element transform applied first;
//   long_tile_sort     the keys to registers, the network, the sorted keys back to LDS.
// long_tile_columns runs them in order for a kernel whose array is [outer, m, inner]; long_tile_columns_as_given pads
// and loads without the network (a column used in the order the array has it: cpf with a sort flag off).
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
// the lanes of a read-out and of the strided load touch, is n + 1 apart: odd, so those are conflict-free too.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ensemble_point.hpp"

namespace ekm {

constexpr unsigned kLongThreads = 256;
constexpr unsigned kLongMinColumn = 32;            // the shortest padded column: at most E / 32 columns per tile
constexpr size_t kLongKeyBytes = 64 * 1024;        // the keys of a full tile: the cap of the sample axis
constexpr size_t kLongSmallKeyBytes = 16 * 1024;   // the keys of a small tile

// A thread's R keys: a vector value, so that they stay in registers whatever the optimiser makes of the loops round them
template <class K, int R>
using LongKeys = K __attribute__((ext_vector_type(R)));

// What a kernel declares in LDS for a tile of R keys per thread: K lds[kSlots]; unsigned col_nan[kFlags]
template <int R>
struct LongTile {
  static constexpr unsigned kKeys = R * kLongThreads;
  static constexpr unsigned kSlots = kKeys + kKeys / kLongMinColumn;
  static constexpr unsigned kFlags = kKeys / kLongMinColumn;
};

__device__ __forceinline__ unsigned long_slot(unsigned e, unsigned log2n) { return e + (e >> log2n); }

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

// The flags to zero and the padding (slots past m, dead columns) to the largest key; ends with a barrier: the flags are
// zero before any is raised
template <class T, int R>
__device__ __forceinline__ void long_tile_pad(typename SortKey<T>::type* lds, unsigned* col_nan, unsigned t, unsigned m,
                                              unsigned log2n, unsigned live) {
  const unsigned n = 1u << log2n, columns = LongTile<R>::kKeys >> log2n;
  for (unsigned c = t; c < columns; c += kLongThreads) col_nan[c] = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const unsigned e = (unsigned)r * kLongThreads + t;
    if ((e & (n - 1)) >= m || (e >> log2n) >= live) lds[long_slot(e, log2n)] = SortKey<T>::kMax;
  }
  __syncthreads();
}

// The sample axis last (inner == 1): the tile is ONE contiguous run of len = live * m elements.  Read 16 B per lane from
// the first 16-B boundary on, the ragged head and tail one element per lane, and scattered to (column, slot) with a
// multiply-high in place of the division by m (magic = 2^32 / m + 1: exact for q * m < 2^32).  f: the transform of an
// element before it is keyed.
template <class T, class F>
__device__ __forceinline__ void long_tile_load_run(const T* __restrict__ run, unsigned len, unsigned m, unsigned log2n,
                                                   unsigned magic, typename SortKey<T>::type* lds, unsigned* col_nan,
                                                   unsigned t, F f) {
  using Key = SortKey<T>;
  constexpr unsigned V = 16 / sizeof(T);
  struct alignas(16) Vec {
    T v[V];
  };
  unsigned head = (unsigned)((16 - reinterpret_cast<uintptr_t>(run) % 16) % 16 / sizeof(T));
  if (head > len) head = len;
  const unsigned nvec = (len - head) / V, tail = head + nvec * V;
  auto place = [&](unsigned q, T x) {
    const unsigned c = m == 1 ? q : __umulhi(q, magic);
    x = f(x);
    if (x != x) col_nan[c] = 1;
    lds[long_slot((c << log2n) + (q - c * m), log2n)] = Key::of(x);
  };
  for (unsigned v = t; v < nvec; v += kLongThreads) {
    const Vec x = *reinterpret_cast<const Vec*>(run + head + v * V);
#pragma unroll
    for (unsigned u = 0; u < V; ++u) place(head + v * V + u, x.v[u]);
  }
  if (t < head) place(t, run[t]);
  if (t < len - tail) place(tail + t, run[tail + t]);
}

// inner > 1: the tile is m runs of `live` elements at stride `inner`.  The lanes run along the columns (a wave reads
// min(C, 64) consecutive elements per sample), the rest of the workgroup along the samples.
template <class T, int R, class F>
__device__ __forceinline__ void long_tile_load_strided(const T* __restrict__ arr, unsigned m, unsigned long long inner,
                                                       unsigned long long p0, unsigned live, unsigned log2n,
                                                       typename SortKey<T>::type* lds, unsigned* col_nan, unsigned t,
                                                       F f) {
  using Key = SortKey<T>;
  const unsigned columns = LongTile<R>::kKeys >> log2n;
  const unsigned log2c = 31 - __builtin_clz(columns);
  const unsigned log2w = log2c < 8 ? log2c : 8;
  const unsigned width = 1u << log2w, rows = kLongThreads >> log2w;
  for (unsigned c = t & (width - 1); c < live; c += width) {
    const T* col = sample_column<T>(arr, m, inner, p0 + c);
#pragma unroll 4
    for (unsigned i = t >> log2w; i < m; i += rows) {
      const T x = f(col[(unsigned long long)i * inner]);
      if (x != x) col_nan[c] = 1;
      lds[long_slot((c << log2n) + i, log2n)] = Key::of(x);
    }
  }
}

// The bitonic network over the tile in LDS: merges of k = 2, 4, .. n, each in stages of partner distance j = k/2 .. 1.
// Begins with a barrier (the load is done) and ends with one (the sorted columns are in LDS for every thread to read).
template <class K, int R>
__device__ __forceinline__ void long_tile_sort(K* lds, unsigned t, unsigned log2n) {
  const unsigned n = 1u << log2n;
  __syncthreads();
  LongKeys<K, R> key;
#pragma unroll
  for (int r = 0; r < R; ++r) key[r] = lds[long_slot((unsigned)r * kLongThreads + t, log2n)];
  for (unsigned k = 2; k <= n; k <<= 1) {
    const unsigned dir = k & (n - 1);  // the index bit that turns a run downwards; none in the last merge
    for (unsigned j = k >> 1; j > 0; j >>= 1) {
      if (j >= kLongThreads) {
        long_register_stages<K, R, 1>(key, j / kLongThreads, dir / kLongThreads);
      } else if (j >= 64) {
        __syncthreads();  // every read of the stage (or of the load) before is done
#pragma unroll
        for (int r = 0; r < R; ++r) lds[long_slot((unsigned)r * kLongThreads + t, log2n)] = key[r];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const unsigned e = (unsigned)r * kLongThreads + t;
          key[r] = long_pick(key[r], lds[long_slot(e ^ j, log2n)], ((e & j) == 0) == ((e & dir) == 0));
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
  __syncthreads();
#pragma unroll
  for (int r = 0; r < R; ++r) lds[long_slot((unsigned)r * kLongThreads + t, log2n)] = key[r];
  __syncthreads();
}

// All phases for the tile that starts at point p0 of arr [outer, m, inner]: afterwards column c < live of the tile is
// sorted ascending at lds[long_slot((c << log2n) + i)], i < m, and col_nan[c] says whether it holds a NaN.
template <class T, int R, class F>
__device__ __forceinline__ void long_tile_columns(const T* __restrict__ arr, unsigned m, unsigned log2n, unsigned magic,
                                                  unsigned long long inner, unsigned long long p0, unsigned live,
                                                  typename SortKey<T>::type* lds, unsigned* col_nan, F f) {
  const unsigned t = threadIdx.x;
  long_tile_pad<T, R>(lds, col_nan, t, m, log2n, live);
  if (inner == 1)
    long_tile_load_run<T>(arr + p0 * m, live * m, m, log2n, magic, lds, col_nan, t, f);
  else
    long_tile_load_strided<T, R>(arr, m, inner, p0, live, log2n, lds, col_nan, t, f);
  long_tile_sort<typename SortKey<T>::type, R>(lds, t, log2n);
}

// The same tile WITHOUT the network: afterwards column c < live holds its m values in the order the array has them (a
// key reads back every non-NaN value bit for bit and a NaN as a NaN), and col_nan[c] is set as above.  Ends with a
// barrier, as long_tile_sort does.
template <class T, int R, class F>
__device__ __forceinline__ void long_tile_columns_as_given(const T* __restrict__ arr, unsigned m, unsigned log2n,
                                                           unsigned magic, unsigned long long inner,
                                                           unsigned long long p0, unsigned live,
                                                           typename SortKey<T>::type* lds, unsigned* col_nan, F f) {
  const unsigned t = threadIdx.x;
  long_tile_pad<T, R>(lds, col_nan, t, m, log2n, live);
  if (inner == 1)
    long_tile_load_run<T>(arr + p0 * m, live * m, m, log2n, magic, lds, col_nan, t, f);
  else
    long_tile_load_strided<T, R>(arr, m, inner, p0, live, log2n, lds, col_nan, t, f);
  __syncthreads();
}

}  // namespace ekm
