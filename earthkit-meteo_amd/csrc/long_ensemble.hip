// The sorted-column reductions for a LONG member or sample axis on gfx950: extreme.long_efi, extreme.long_sot,
// score.long_crps_from_ensemble, stats.GumbelDistribution.long_fit / ekm_long_efi_*, ekm_long_sot_*,
// ekm_long_crps_from_ensemble_*, ekm_long_gumbel_fit_* (reference extreme/array/efi.py:34-89, extreme/array/sot.py:51-103,
// score/array/ensemble.py:34-82, stats/array/extreme_values.py:44-64).  The short kernels of ensemble.hip insertion-sort
// one column per lane, O(m^2), and hold 64 columns in 64 KiB of LDS: 256 members in f32, 128 in f64.  Here one workgroup
// sorts a tile of whole columns with the bitonic network of long_sort.hpp (the tile, its two sizes, its LDS layout and
// the barrier rule are stated there), up to 16384 members in f32 and 8192 in f64, and then lane c of the workgroup
// takes column c of the tile and calls the per-point function of ensemble_point.hpp the short kernel and the host twin
// call, with s(i) read from the sorted keys in LDS and the column's NaN flag.
//
// The member-major fields of efi / sot / crps, [nens, npts], are the strided case of the tile load (outer = 1, m = nens,
// inner = npts); the Gumbel sample is [outer, m, inner] as for long_quantiles.  Traffic: every member is read once; efi
// streams its climate rows from global memory, once each, never staged; 8 B (efi, crps; + 1 B missing), sizeof(T) (sot)
// or 16 B (fit) written per point.
//
// The read-out is SERIAL per column: the sums of gumbel_fit_point and crps_point and the cursor of efi_point run in the
// reference's order, which is what makes them the reference's bits, so a tile of C columns keeps C of the 256 lanes busy
// (8 at 1980 members in f32).  DESIGN.md section 4 has the measured cost.
//
// extreme.long_cpf / ekm_long_cpf_* (reference extreme/array/cpf.py:13-155) is here too: long_cpf_tiles holds TWO tiles,
// the ensemble's and the climate's, and its read-out is cpf_value_running of ensemble_point.hpp (stated at the kernel).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/ekm_thermo.h"
#include "ensemble_point.hpp"
#include "launch_checks.hpp"
#include "long_sort.hpp"
#include "map_kernel.hpp"

namespace ekm {

// What every kernel below begins with: the tile's LDS, its first point p0, its live columns (>= 1: the grid is
// ceil(npts / columns)) and the reader s(c, i) of sorted member i of column c
#define EKM_LONG_TILE(T, R)                                                                                     \
  using Key = SortKey<T>;                                                                                       \
  using K = typename Key::type;                                                                                 \
  __shared__ K lds[LongTile<R>::kSlots];                                                                        \
  __shared__ unsigned col_nan[LongTile<R>::kFlags];                                                             \
  const unsigned t = threadIdx.x, columns = LongTile<R>::kKeys >> log2n;                                        \
  const unsigned long long p0 = (unsigned long long)blockIdx.x * columns;                                       \
  const unsigned live = npts - p0 < columns ? (unsigned)(npts - p0) : columns;                                  \
  auto sorted = [&](unsigned c, unsigned i) -> T { return Key::value(lds[long_slot((c << log2n) + i, log2n)]); }

template <class T, int R>
__global__ __launch_bounds__(kLongThreads) void long_efi_tiles(const T* __restrict__ clim, const T* __restrict__ ens,
                                                               unsigned nclim, unsigned nens, unsigned log2n,
                                                               unsigned magic, unsigned long long npts, double eps,
                                                               const double* __restrict__ acosdiff,
                                                               const double* __restrict__ proddiff,
                                                               const double* __restrict__ acoef,
                                                               double* __restrict__ out) {
  EKM_LONG_TILE(T, R);
  long_tile_columns<T, R>(ens, nens, log2n, magic, npts, p0, live, lds, col_nan, [](T x) -> T { return x; });
  for (unsigned c = t; c < columns; c += kLongThreads) {
    if (c >= live) continue;
    const unsigned long long p = p0 + c;
    out[p] = efi_point<T>(
        nclim, nens, col_nan[c] != 0, [&](unsigned i) -> T { return clim[(unsigned long long)i * npts + p]; },
        [&](unsigned i) -> T { return sorted(c, i); }, acosdiff, proddiff, acoef, eps);
  }
}

template <class T, int R>
__global__ __launch_bounds__(kLongThreads) void long_sot_tiles(const T* __restrict__ qc, const T* __restrict__ qc_tail,
                                                               const T* __restrict__ ens, unsigned nens, unsigned log2n,
                                                               unsigned magic, unsigned long long npts,
                                                               Percentile<T> pos, double eps, T* __restrict__ out) {
  EKM_LONG_TILE(T, R);
  const bool zero_below = eps > 0.0;  // sot.py:88: members below eps become 0 before they are sorted
  const T teps = T(eps);
  long_tile_columns<T, R>(ens, nens, log2n, magic, npts, p0, live, lds, col_nan,
                          [&](T x) -> T { return zero_below && x < teps ? T(0) : x; });
  for (unsigned c = t; c < columns; c += kLongThreads) {
    if (c >= live) continue;
    const unsigned long long p = p0 + c;
    out[p] = sot_point<T>(qc[p], qc_tail[p], col_nan[c] != 0, [&](unsigned i) -> T { return sorted(c, i); }, pos, eps);
  }
}

// missing: one flag byte per point, or null (crps_body of ensemble_point.hpp)
template <class T, int R>
__global__ __launch_bounds__(kLongThreads) void long_crps_tiles(const T* __restrict__ x, const T* __restrict__ y,
                                                                unsigned nens, unsigned log2n, unsigned magic,
                                                                unsigned long long npts, const double* __restrict__ p2,
                                                                const double* __restrict__ q2, double* __restrict__ out,
                                                                unsigned char* __restrict__ missing) {
  EKM_LONG_TILE(T, R);
  long_tile_columns<T, R>(x, nens, log2n, magic, npts, p0, live, lds, col_nan, [](T v) -> T { return v; });
  for (unsigned c = t; c < columns; c += kLongThreads) {
    if (c >= live) continue;
    const unsigned long long p = p0 + c;
    const T yp = y[p];
    const bool miss = col_nan[c] != 0 || yp != yp;  // ensemble.py:44
    const double r = crps_point<T>(nens, yp, [&](unsigned i) -> T { return sorted(c, i); }, p2, q2);
    out[p] = miss ? nan_v<double>() : r;
    if (missing) missing[p] = miss ? 1 : 0;
  }
}

// sample: [outer, m, inner]; mu, sigma: float64 [npts]
template <class T, int R>
__global__ __launch_bounds__(kLongThreads) void long_gumbel_fit_tiles(const T* __restrict__ sample, unsigned m,
                                                                      unsigned log2n, unsigned magic,
                                                                      unsigned long long inner, unsigned long long npts,
                                                                      double* __restrict__ mu,
                                                                      double* __restrict__ sigma) {
  EKM_LONG_TILE(T, R);
  long_tile_columns<T, R>(sample, m, log2n, magic, inner, p0, live, lds, col_nan, [](T x) -> T { return x; });
  for (unsigned c = t; c < columns; c += kLongThreads) {
    if (c >= live) continue;
    double mu_p, sigma_p;
    gumbel_fit_point<T>(m, col_nan[c] != 0, [&](unsigned i) -> T { return sorted(c, i); }, mu_p, sigma_p);
    mu[p0 + c] = mu_p;
    sigma[p0 + c] = sigma_p;
  }
}

#undef EKM_LONG_TILE

// cpf.py:13-155 for long columns: TWO tiles, the ensemble's (RE keys per thread, columns of 2^log2e slots) and the
// climate's (RC, 2^log2c), each the small or the full tile of T.  The workgroup takes `columns` = min(columns of the two
// tiles) whole points; the tile that could hold more treats the rest as dead columns.  A column is sorted where its flag
// asks for it (SortKey puts every NaN last, as numpy.sort does, and reads it back as a NaN; the scan only compares NaNs)
// and loaded as given otherwise; both flags are kernel arguments, so every branch round a barrier is uniform.  The scan
// never reads the NaN flags of the tiles: a column with a NaN does not give NaN in cpf.  Then lane c runs
// cpf_value_running, O(nclim + nens), over the two columns of point p0 + c.  flags: kCpf* of ensemble_point.hpp.
// LDS, static: full + full 2 * (64 KiB + 2 KiB of spare slots + 2 KiB of flags) = 136 KiB, full + small 85 KiB,
// small + small 34 KiB.
template <class T, int RE, int RC>
__global__ __launch_bounds__(kLongThreads) void long_cpf_tiles(const T* __restrict__ clim, const T* __restrict__ ens,
                                                               unsigned nclim, unsigned nens, unsigned log2c,
                                                               unsigned log2e, unsigned magic_c, unsigned magic_e,
                                                               unsigned columns, unsigned long long npts, unsigned flags,
                                                               T epsilon, float* __restrict__ out) {
  using Key = SortKey<T>;
  using K = typename Key::type;
  __shared__ K lds_e[LongTile<RE>::kSlots];
  __shared__ K lds_c[LongTile<RC>::kSlots];
  __shared__ unsigned nan_e[LongTile<RE>::kFlags];
  __shared__ unsigned nan_c[LongTile<RC>::kFlags];
  const unsigned t = threadIdx.x;
  const unsigned long long p0 = (unsigned long long)blockIdx.x * columns;
  const unsigned live = npts - p0 < columns ? (unsigned)(npts - p0) : columns;
  auto same = [](T x) -> T { return x; };
  if (flags & kCpfSortEns)
    long_tile_columns<T, RE>(ens, nens, log2e, magic_e, npts, p0, live, lds_e, nan_e, same);
  else
    long_tile_columns_as_given<T, RE>(ens, nens, log2e, magic_e, npts, p0, live, lds_e, nan_e, same);
  if (flags & kCpfSortClim)
    long_tile_columns<T, RC>(clim, nclim, log2c, magic_c, npts, p0, live, lds_c, nan_c, same);
  else
    long_tile_columns_as_given<T, RC>(clim, nclim, log2c, magic_c, npts, p0, live, lds_c, nan_c, same);
  if (t < live)  // (columns <= 128: a small tile holds at most 4096 / 32 of them)
    out[p0 + t] = cpf_value_running<T>(
        nclim, nens, (flags & kCpfFromZero) != 0, (flags & kCpfSymmetric) != 0, (flags & kCpfEpsilon) != 0, epsilon,
        [&](unsigned i) -> T { return Key::value(lds_c[long_slot((t << log2c) + i, log2c)]); },
        [&](unsigned i) -> T { return Key::value(lds_e[long_slot((t << log2e) + i, log2e)]); });
}

// The tile of a launch: the padded column, which of the two tile sizes holds it, the grid, the divisor of the tile load
struct LongShape {
  unsigned log2n, magic, grid;
  bool small;
};

// What the launchers share: the axis length against the cap, the T pointers, the tile, the grid, the device.
// noun: what the axis holds ("members", "samples").
template <class T>
static int long_prepare(int dev, const char* what, const char* noun, size_t npts, uint32_t m, uint32_t least,
                        std::initializer_list<const void*> ptrs, LongShape* shape) {
  constexpr unsigned kCap = kLongKeyBytes / sizeof(T), kSmall = kLongSmallKeyBytes / sizeof(T);
  // (a tile's run of at most kCap elements and an axis of at most kCap: q * m < 2^32 in the tile load's q / m)
  static_assert((unsigned long long)kCap * kCap < (1ull << 32), "the multiply-high division of the tile load");
  if (m < least) return set_error(EKM_ERR_ARG, "%s: at least %u %s are required, got %u", what, least, noun, m);
  if (m > kCap)
    return set_error(EKM_ERR_ARG, "%s: %u %s are past the cap of %u (one column, padded to a power of two, in %zu KiB of LDS)",
                     what, m, noun, kCap, kLongKeyBytes / 1024);
  int rc = check_pointers(what, sizeof(T), ptrs);
  if (rc != EKM_OK) return rc;
  shape->log2n = 5;  // kLongMinColumn
  while ((1u << shape->log2n) < m) ++shape->log2n;
  shape->small = (1u << shape->log2n) <= kSmall;
  shape->magic = m > 1 ? (unsigned)((1ull << 32) / m + 1) : 0;
  if ((rc = launch_grid(what, npts, (shape->small ? kSmall : kCap) >> shape->log2n, &shape->grid)) != EKM_OK) return rc;
  return use_device(dev);
}

// launch(R): the kernel instantiated for the small or the full tile of T
template <class T, class Launch>
static void long_dispatch(bool small, Launch launch) {
  if (small)
    launch(std::integral_constant<int, (int)(kLongSmallKeyBytes / sizeof(T) / kLongThreads)>{});
  else
    launch(std::integral_constant<int, (int)(kLongKeyBytes / sizeof(T) / kLongThreads)>{});
}

template <class T>
static int launch_long_efi(int dev, void* stream, const T* clim, const T* ens, uint32_t nclim, uint32_t nens, size_t npts,
                           double eps, const double* acosdiff, const double* proddiff, const double* acoef, double* out) {
  if (npts == 0) return EKM_OK;
  if (nclim < 1) return set_error(EKM_ERR_ARG, "long_efi: at least one climate row is required");
  if (nclim > 1 && (!acosdiff || !proddiff || !acoef)) return set_error(EKM_ERR_ARG, "long_efi: null coefficient table");
  int rc = check_pointers("long_efi", sizeof(double), {out});
  if (rc != EKM_OK) return rc;
  LongShape sh;
  if ((rc = long_prepare<T>(dev, "long_efi", "members", npts, nens, 1, {clim, ens}, &sh)) != EKM_OK) return rc;
  long_dispatch<T>(sh.small, [&](auto r) {
    hipLaunchKernelGGL((long_efi_tiles<T, decltype(r)::value>), dim3(sh.grid), dim3(kLongThreads), 0,
                       static_cast<hipStream_t>(stream), clim, ens, nclim, nens, sh.log2n, sh.magic,
                       (unsigned long long)npts, eps, acosdiff, proddiff, acoef, out);
  });
  return launched("long_efi");
}

template <class T>
static int launch_long_sot(int dev, void* stream, const T* qc, const T* qc_tail, const T* ens, uint32_t nens, size_t npts,
                           int perc, double eps, T* out) {
  if (npts == 0) return EKM_OK;
  if (perc < 2 || perc > 98 || perc == 50)
    return set_error(EKM_ERR_ARG, "long_sot: perc=%d must be in [2, 98] and not 50", perc);
  LongShape sh;
  int rc = long_prepare<T>(dev, "long_sot", "members", npts, nens, 1, {qc, qc_tail, ens, out}, &sh);
  if (rc != EKM_OK) return rc;
  const Percentile<T> pos = percentile_position<T>(nens, perc);
  long_dispatch<T>(sh.small, [&](auto r) {
    hipLaunchKernelGGL((long_sot_tiles<T, decltype(r)::value>), dim3(sh.grid), dim3(kLongThreads), 0,
                       static_cast<hipStream_t>(stream), qc, qc_tail, ens, nens, sh.log2n, sh.magic,
                       (unsigned long long)npts, pos, eps, out);
  });
  return launched("long_sot");
}

template <class T>
static int launch_long_crps(int dev, void* stream, const T* x, const T* y, uint32_t nens, size_t npts, const double* p2,
                            const double* q2, double* out, uint8_t* missing) {
  if (npts == 0) return EKM_OK;
  if (!p2 || !q2) return set_error(EKM_ERR_ARG, "long_crps_from_ensemble: null weight table");
  int rc = check_pointers("long_crps_from_ensemble", sizeof(double), {out});
  if (rc != EKM_OK) return rc;
  LongShape sh;
  if ((rc = long_prepare<T>(dev, "long_crps_from_ensemble", "members", npts, nens, 1, {x, y}, &sh)) != EKM_OK) return rc;
  long_dispatch<T>(sh.small, [&](auto r) {
    hipLaunchKernelGGL((long_crps_tiles<T, decltype(r)::value>), dim3(sh.grid), dim3(kLongThreads), 0,
                       static_cast<hipStream_t>(stream), x, y, nens, sh.log2n, sh.magic, (unsigned long long)npts, p2,
                       q2, out, missing);
  });
  return launched("long_crps_from_ensemble");
}

template <class T>
static int launch_long_gumbel_fit(int dev, void* stream, const T* sample, size_t outer, uint32_t m, size_t inner,
                                  double* mu, double* sigma) {
  if (outer == 0 || inner == 0) return EKM_OK;
  if (inner > ~(size_t)0 / outer) return set_error(EKM_ERR_ARG, "long_gumbel_fit: too many points");
  const size_t npts = outer * inner;
  int rc = check_pointers("long_gumbel_fit", sizeof(double), {mu, sigma});
  if (rc != EKM_OK) return rc;
  LongShape sh;
  if ((rc = long_prepare<T>(dev, "long_gumbel_fit", "samples", npts, m, 2, {sample}, &sh)) != EKM_OK) return rc;
  long_dispatch<T>(sh.small, [&](auto r) {
    hipLaunchKernelGGL((long_gumbel_fit_tiles<T, decltype(r)::value>), dim3(sh.grid), dim3(kLongThreads), 0,
                       static_cast<hipStream_t>(stream), sample, m, sh.log2n, sh.magic, (unsigned long long)inner,
                       (unsigned long long)npts, mu, sigma);
  });
  return launched("long_gumbel_fit");
}

// The two axes are held to the cap separately; the workgroup takes as many points as the tile with fewer columns holds
template <class T>
static int launch_long_cpf(int dev, void* stream, const T* clim, const T* ens, uint32_t nclim, uint32_t nens, size_t npts,
                           int sort_clim, int sort_ens, int from_zero, int symmetric, int use_epsilon, double epsilon,
                           float* out) {
  if (npts == 0) return EKM_OK;
  int rc = check_pointers("long_cpf", sizeof(float), {out});
  if (rc != EKM_OK) return rc;
  LongShape se, sc;
  if ((rc = long_prepare<T>(dev, "long_cpf", "members", npts, nens, 1, {ens}, &se)) != EKM_OK) return rc;
  if ((rc = long_prepare<T>(dev, "long_cpf", "climate rows", npts, nclim, 1, {clim}, &sc)) != EKM_OK) return rc;
  constexpr unsigned kCap = kLongKeyBytes / sizeof(T), kSmall = kLongSmallKeyBytes / sizeof(T);
  const unsigned cols_e = (se.small ? kSmall : kCap) >> se.log2n, cols_c = (sc.small ? kSmall : kCap) >> sc.log2n;
  const unsigned columns = cols_e < cols_c ? cols_e : cols_c;
  unsigned grid;
  if ((rc = launch_grid("long_cpf", npts, columns, &grid)) != EKM_OK) return rc;
  const unsigned flags = cpf_flags(sort_clim, sort_ens, from_zero, symmetric, use_epsilon);
  long_dispatch<T>(se.small, [&](auto re) {
    long_dispatch<T>(sc.small, [&](auto rcl) {
      hipLaunchKernelGGL((long_cpf_tiles<T, decltype(re)::value, decltype(rcl)::value>), dim3(grid), dim3(kLongThreads), 0,
                         static_cast<hipStream_t>(stream), clim, ens, nclim, nens, sc.log2n, se.log2n, sc.magic, se.magic,
                         columns, (unsigned long long)npts, flags, T(epsilon), out);
    });
  });
  return launched("long_cpf");
}

}  // namespace ekm

extern "C" {

int ekm_long_efi_f32(int dev, void* stream, const float* clim, const float* ens, uint32_t nclim, uint32_t nens,
                     size_t npts, double eps, const double* acosdiff, const double* proddiff, const double* acoef,
                     double* out) {
  return ekm::launch_long_efi<float>(dev, stream, clim, ens, nclim, nens, npts, eps, acosdiff, proddiff, acoef, out);
}
int ekm_long_efi_f64(int dev, void* stream, const double* clim, const double* ens, uint32_t nclim, uint32_t nens,
                     size_t npts, double eps, const double* acosdiff, const double* proddiff, const double* acoef,
                     double* out) {
  return ekm::launch_long_efi<double>(dev, stream, clim, ens, nclim, nens, npts, eps, acosdiff, proddiff, acoef, out);
}

int ekm_long_sot_f32(int dev, void* stream, const float* qc, const float* qc_tail, const float* ens, uint32_t nens,
                     size_t npts, int perc, double eps, float* out) {
  return ekm::launch_long_sot<float>(dev, stream, qc, qc_tail, ens, nens, npts, perc, eps, out);
}
int ekm_long_sot_f64(int dev, void* stream, const double* qc, const double* qc_tail, const double* ens, uint32_t nens,
                     size_t npts, int perc, double eps, double* out) {
  return ekm::launch_long_sot<double>(dev, stream, qc, qc_tail, ens, nens, npts, perc, eps, out);
}

int ekm_long_crps_from_ensemble_f32(int dev, void* stream, const float* x, const float* y, uint32_t nens, size_t npts,
                                    const double* p2, const double* q2, double* out, uint8_t* missing) {
  return ekm::launch_long_crps<float>(dev, stream, x, y, nens, npts, p2, q2, out, missing);
}
int ekm_long_crps_from_ensemble_f64(int dev, void* stream, const double* x, const double* y, uint32_t nens, size_t npts,
                                    const double* p2, const double* q2, double* out, uint8_t* missing) {
  return ekm::launch_long_crps<double>(dev, stream, x, y, nens, npts, p2, q2, out, missing);
}

int ekm_long_gumbel_fit_f32(int dev, void* stream, const float* sample, size_t outer, uint32_t m, size_t inner,
                            double* mu, double* sigma) {
  return ekm::launch_long_gumbel_fit<float>(dev, stream, sample, outer, m, inner, mu, sigma);
}
int ekm_long_gumbel_fit_f64(int dev, void* stream, const double* sample, size_t outer, uint32_t m, size_t inner,
                            double* mu, double* sigma) {
  return ekm::launch_long_gumbel_fit<double>(dev, stream, sample, outer, m, inner, mu, sigma);
}

int ekm_long_cpf_f32(int dev, void* stream, const float* clim, const float* ens, uint32_t nclim, uint32_t nens,
                     size_t npts, int sort_clim, int sort_ens, int from_zero, int symmetric, int use_epsilon,
                     double epsilon, float* out) {
  return ekm::launch_long_cpf<float>(dev, stream, clim, ens, nclim, nens, npts, sort_clim, sort_ens, from_zero, symmetric,
                                     use_epsilon, epsilon, out);
}
int ekm_long_cpf_f64(int dev, void* stream, const double* clim, const double* ens, uint32_t nclim, uint32_t nens,
                     size_t npts, int sort_clim, int sort_ens, int from_zero, int symmetric, int use_epsilon,
                     double epsilon, float* out) {
  return ekm::launch_long_cpf<double>(dev, stream, clim, ens, nclim, nens, npts, sort_clim, sort_ens, from_zero, symmetric,
                                      use_epsilon, epsilon, out);
}

}  // extern "C"
