// Ensemble reductions on gfx950: Extreme Forecast Index, Shift of Tails, Crossing Point Forecast, CRPS, per-point
// quantiles and the Gumbel extreme-value fit with its cdf and ppf.
// Reference: extreme/array/efi.py:34-89, extreme/array/sot.py:13-103, extreme/array/cpf.py:13-155,
// score/array/ensemble.py:34-82, stats/array/quantiles.py:18-84, stats/array/extreme_values.py:24-155.
//
// One kernel family: one lane per grid point, one wave (64 lanes) per workgroup.  The fields are member-major,
// ens [nens, npts] and clim [nclim, npts], so a wave reads a member row as one coalesced run.  The lane's ensemble is
// insertion-sorted as it streams in and kept in LDS as [nens][64], lane-minor: the 64 lanes of a step touch 64
// consecutive words (two per lane in fp64), which is free of bank conflicts whatever slot each lane is at.
//  * efi:  the climate rows are streamed once, never staged; each row's rank in the sorted ensemble comes from a
//          cursor that moves on from the previous row's rank (either way, so an unsorted climate is counted right).
//          Traffic: (nclim + nens) elements read, 8 B written per point.
//  * sot:  the percentile of the sorted ensemble (numpy's lerp) against two climate rows.
//  * crps: Hersbach's alpha/beta walk over the sorted ensemble; optional 1-B "missing" flag per point.
//  * quantiles: nq levels of the sorted column from host-computed position records, written level-major
//          (out[k * npts + p]: one coalesced run per level and wave).  The sample axis need not lead: the array is
//          [outer, m, inner] and point p = o * inner + i reads sample j at (o * m + j) * inner + i.  With the sample axis
//          last (inner == 1) every lane reads its own contiguous column; staging the wave's run through LDS first was
//          measured slower and is not kept (profiles/HISTORY.md).
//  * gumbel_fit: the first two L-moments of the sorted column, summed in float64 in the reference polyfill's order, then
//          mu and sigma (extreme_values.py:44-64); [outer, m, inner] addressing as for quantiles.  Traffic: m elements
//          read, 16 B written per point.  gumbel_cdf / gumbel_ppf are plain outer products of nx levels and npts points
//          (256 lanes per workgroup, no LDS): 16 B read and 8 nx B written per point.
//  * cpf:  the crossing-point scan of the sorted ensemble against the interior climate rows, `symmetric` included, in one
//          launch.  The ensemble column always goes to LDS (sorted NaN-last, or copied as given): the scan re-reads
//          members for every row.  The climate goes to LDS only when it has to be sorted; as given it streams from
//          global memory (rows icl, icl-1 and the top row are all that is read).  The LDS is a static array in one of
//          four sizes (20 / 40 / 80 / 160 KiB: 8 / 4 / 2 / 1 workgroups per CU), chosen by the rows the call needs, so
//          101 x 51 with both sorts runs in f32 (38 KiB) and in f64 (76 KiB); beyond 160 KiB: EKM_ERR_ARG.
// LDS (all but cpf): nens * 64 * sizeof(T) <= 64 KiB per workgroup: nens <= 256 (fp32) / 128 (fp64); beyond that the entry points
// return EKM_ERR_ARG.  The per-point arithmetic is ensemble_point.hpp, shared with the host twin.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/ekm_thermo.h"
#include "ensemble_point.hpp"
#include "launch_checks.hpp"
#include "map_kernel.hpp"

namespace ekm {

constexpr int kEnsLanes = 64;                   // one wave per workgroup
constexpr size_t kEnsLdsBytes = 64 * 1024;      // the sorted ensembles of a workgroup

template <class T>
using LaneColumn = Column<T, kEnsLanes>;  // the lane's column of the workgroup's LDS

// quantile_points and cpf_points keep their earlier bodies and stagers: with the shared ones their instruction streams
// changed and the timing did not hold (profiles/refactor_launch_ab.json).
constexpr int kEnsBatch = 8;                    // member rows in flight per lane while sorting
template <class T>
__device__ __forceinline__ bool sort_members(const T* __restrict__ base, unsigned long long stride, unsigned nens, T* col,
                                             bool zero_below, T teps) {
  auto get = [&](unsigned j) -> T { return col[j * kEnsLanes]; };
  auto set = [&](unsigned j, T v) { col[j * kEnsLanes] = v; };
  bool has_nan = false;
  for (unsigned m0 = 0; m0 < nens; m0 += kEnsBatch) {
    T v[kEnsBatch];
#pragma unroll
    for (int b = 0; b < kEnsBatch; ++b)
      if (m0 + b < nens) v[b] = base[(unsigned long long)(m0 + b) * stride];
#pragma unroll
    for (int b = 0; b < kEnsBatch; ++b)
      if (m0 + b < nens) {
        T x = v[b];
        if (zero_below && x < teps) x = T(0);
        has_nan = has_nan || x != x;
        ens_insert<T>(m0 + b, x, get, set);
      }
  }
  return has_nan;
}

// (cpf) sorted as numpy.sort orders them (NaN last), or as given
template <class T>
__device__ __forceinline__ void cpf_stage_column(const T* __restrict__ base, unsigned long long stride, unsigned rows, T* col,
                                                 bool sort) {
  auto get = [&](unsigned j) -> T { return col[j * kEnsLanes]; };
  auto set = [&](unsigned j, T v) { col[j * kEnsLanes] = v; };
  for (unsigned m0 = 0; m0 < rows; m0 += kEnsBatch) {
    T v[kEnsBatch];
#pragma unroll
    for (int b = 0; b < kEnsBatch; ++b)
      if (m0 + b < rows) v[b] = base[(unsigned long long)(m0 + b) * stride];
#pragma unroll
    for (int b = 0; b < kEnsBatch; ++b)
      if (m0 + b < rows) {
        if (sort)
          ens_insert_nan_last<T>(m0 + b, v[b], get, set);
        else
          set(m0 + b, v[b]);
      }
  }
}

template <class T>
__global__ __launch_bounds__(kEnsLanes) void efi_points(const T* __restrict__ clim, const T* __restrict__ ens,
                                                        unsigned nclim, unsigned nens, unsigned long long npts,
                                                        double eps, const double* __restrict__ acosdiff,
                                                        const double* __restrict__ proddiff,
                                                        const double* __restrict__ acoef, double* __restrict__ out) {
  const unsigned long long p = (unsigned long long)blockIdx.x * kEnsLanes + threadIdx.x;
  if (p >= npts) return;
  const LaneColumn<T> col{reinterpret_cast<T*>(ekm_lds_raw) + threadIdx.x};
  efi_body<T>(clim, ens, nclim, nens, npts, p, eps, acosdiff, proddiff, acoef, col, out);
}

template <class T>
__global__ __launch_bounds__(kEnsLanes) void sot_points(const T* __restrict__ qc, const T* __restrict__ qc_tail,
                                                        const T* __restrict__ ens, unsigned nens,
                                                        unsigned long long npts, Percentile<T> pos, double eps,
                                                        T* __restrict__ out) {
  const unsigned long long p = (unsigned long long)blockIdx.x * kEnsLanes + threadIdx.x;
  if (p >= npts) return;
  const LaneColumn<T> col{reinterpret_cast<T*>(ekm_lds_raw) + threadIdx.x};
  sot_body<T>(qc, qc_tail, ens, nens, npts, p, pos, eps, col, out);
}

template <class T>
__global__ __launch_bounds__(kEnsLanes) void crps_points(const T* __restrict__ x, const T* __restrict__ y, unsigned nens,
                                                         unsigned long long npts, const double* __restrict__ p2,
                                                         const double* __restrict__ q2, double* __restrict__ out,
                                                         unsigned char* __restrict__ missing) {
  const unsigned long long p = (unsigned long long)blockIdx.x * kEnsLanes + threadIdx.x;
  if (p >= npts) return;
  const LaneColumn<T> col{reinterpret_cast<T*>(ekm_lds_raw) + threadIdx.x};
  crps_body<T>(x, y, nens, npts, p, p2, q2, col, out, missing);
}

// quantiles.py:60-84.  arr: [outer, m, inner]; lo, hi, w: the nq position records; out: [nq, npts] in Out.
static_assert(kQuantileSort == EKM_QUANTILE_SORT && kQuantileLerp == EKM_QUANTILE_LERP, "ensemble_point.hpp and the header disagree");

template <class T, class Out>
__global__ __launch_bounds__(kEnsLanes) void quantile_points(const T* __restrict__ arr, unsigned m,
                                                             unsigned long long inner, unsigned long long npts,
                                                             const double* __restrict__ lo, const double* __restrict__ hi,
                                                             const double* __restrict__ w, unsigned nq, int mode,
                                                             Out* __restrict__ out) {
  const unsigned long long p = (unsigned long long)blockIdx.x * kEnsLanes + threadIdx.x;
  if (p >= npts) return;
  T* col = reinterpret_cast<T*>(ekm_lds_raw) + threadIdx.x;
  const unsigned long long o = p / inner, i = p - o * inner;
  const bool has_nan = sort_members<T>(arr + o * m * inner + i, inner, m, col, false, T(0));
  auto s = [&](unsigned k) -> T { return col[k * kEnsLanes]; };
  for (unsigned k = 0; k < nq; ++k)
    out[(unsigned long long)k * npts + p] = quantile_point<T, Out>(has_nan, s, (unsigned)lo[k], (unsigned)hi[k], w[k], mode);
}

// extreme_values.py:44-64.  sample: [outer, m, inner] as for quantile_points; mu, sigma: float64 [npts].
static_assert(kGumbelCdf == EKM_GUMBEL_CDF && kGumbelReturnPeriod == EKM_GUMBEL_RETURN_PERIOD, "ensemble_point.hpp and the header disagree");

template <class T>
__global__ __launch_bounds__(kEnsLanes) void gumbel_fit_points(const T* __restrict__ sample, unsigned m,
                                                               unsigned long long inner, unsigned long long npts,
                                                               double* __restrict__ mu, double* __restrict__ sigma) {
  const unsigned long long p = (unsigned long long)blockIdx.x * kEnsLanes + threadIdx.x;
  if (p >= npts) return;
  const LaneColumn<T> col{reinterpret_cast<T*>(ekm_lds_raw) + threadIdx.x};
  gumbel_fit_body<T>(sample, m, inner, p, col, mu, sigma);
}

// extreme_values.py:76-110: the outer product of nx levels and npts points, out[k * npts + p].  One lane per point keeps
// mu and sigma in registers across the levels; the level table is the same address for every lane of a wave.
constexpr int kGumbelLanes = 256;

__global__ __launch_bounds__(kGumbelLanes) void gumbel_cdf_points(const double* __restrict__ mu,
                                                                  const double* __restrict__ sigma,
                                                                  unsigned long long npts, const double* __restrict__ x,
                                                                  unsigned nx, double freq, int mode,
                                                                  double* __restrict__ out) {
  const unsigned long long p = (unsigned long long)blockIdx.x * kGumbelLanes + threadIdx.x;
  if (p >= npts) return;
  const double m = mu[p], s = sigma[p];
  for (unsigned k = 0; k < nx; ++k) out[(unsigned long long)k * npts + p] = gumbel_cdf_point(m, s, x[k], freq, mode);
}

__global__ __launch_bounds__(kGumbelLanes) void gumbel_ppf_points(const double* __restrict__ mu,
                                                                  const double* __restrict__ sigma,
                                                                  unsigned long long npts, const double* __restrict__ t,
                                                                  unsigned nt, double* __restrict__ out) {
  const unsigned long long p = (unsigned long long)blockIdx.x * kGumbelLanes + threadIdx.x;
  if (p >= npts) return;
  const double m = mu[p], s = sigma[p];
  for (unsigned k = 0; k < nt; ++k) out[(unsigned long long)k * npts + p] = gumbel_ppf_point(m, s, t[k]);
}

// cpf.py:13-155.  KIB: the static LDS of the workgroup; rows [0, nens) hold the ensemble column, rows [nens, nens+nclim)
// the sorted climate column when sort_clim.
constexpr size_t kCpfLdsMaxBytes = 160 * 1024;  // the LDS of a gfx950 workgroup

template <class T, int KIB>
__global__ __launch_bounds__(kEnsLanes) void cpf_points(const T* __restrict__ clim, const T* __restrict__ ens,
                                                        unsigned nclim, unsigned nens, unsigned long long npts,
                                                        unsigned flags, T epsilon, float* __restrict__ out) {
  __shared__ T lds[(size_t)KIB * 1024 / sizeof(T)];
  const unsigned long long p = (unsigned long long)blockIdx.x * kEnsLanes + threadIdx.x;
  if (p >= npts) return;
  T* ecol = lds + threadIdx.x;
  T* ccol = ecol + (size_t)nens * kEnsLanes;
  cpf_stage_column<T>(ens + p, npts, nens, ecol, (flags & kCpfSortEns) != 0);
  auto member = [&](unsigned j) -> T { return ecol[j * kEnsLanes]; };
  const bool from_zero = (flags & kCpfFromZero) != 0, symmetric = (flags & kCpfSymmetric) != 0,
             use_eps = (flags & kCpfEpsilon) != 0;
  if (flags & kCpfSortClim) {
    cpf_stage_column<T>(clim + p, npts, nclim, ccol, true);
    out[p] = cpf_value<T>(nclim, nens, from_zero, symmetric, use_eps, epsilon,
                          [&](unsigned i) -> T { return ccol[i * kEnsLanes]; }, member);
  } else {
    out[p] = cpf_value<T>(nclim, nens, from_zero, symmetric, use_eps, epsilon,
                          [&](unsigned i) -> T { return clim[(unsigned long long)i * npts + p]; }, member);
  }
}

template <class T>
__global__ __launch_bounds__(256) void sot_func_points(const T* __restrict__ qc_tail, const T* __restrict__ qc,
                                                       const T* __restrict__ qf, unsigned long long n, T min_den, T lower,
                                                       T upper, T* __restrict__ out) {
  const unsigned long long p = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  out[p] = sot_func_point<T>(qc_tail[p], qc[p], qf[p], min_den, lower, upper);
}

// What the sorted-column launchers share: the member count against the LDS, the T pointers, the grid, the device
template <class T>
static int ens_prepare(int dev, const char* what, size_t npts, uint32_t nens, std::initializer_list<const void*> ptrs,
                       unsigned* grid, size_t* lds) {
  if (nens < 1) return set_error(EKM_ERR_ARG, "%s: at least one member is required", what);
  *lds = (size_t)nens * kEnsLanes * sizeof(T);
  if (*lds > kEnsLdsBytes)
    return set_error(EKM_ERR_ARG, "%s: %u members need %zu B of LDS per workgroup (max %zu: %zu members)", what, nens, *lds,
                     kEnsLdsBytes, kEnsLdsBytes / (kEnsLanes * sizeof(T)));
  int rc = check_pointers(what, sizeof(T), ptrs);
  if (rc == EKM_OK) rc = launch_grid(what, npts, kEnsLanes, grid);
  return rc == EKM_OK ? use_device(dev) : rc;
}

template <class T>
static int launch_efi(int dev, void* stream, const T* clim, const T* ens, uint32_t nclim, uint32_t nens, size_t npts,
                      double eps, const double* acosdiff, const double* proddiff, const double* acoef, double* out) {
  if (npts == 0) return EKM_OK;
  if (nclim < 1) return set_error(EKM_ERR_ARG, "efi: at least one climate row is required");
  if (nclim > 1 && (!acosdiff || !proddiff || !acoef)) return set_error(EKM_ERR_ARG, "efi: null coefficient table");
  int rc = check_pointers("efi", sizeof(double), {out});
  if (rc != EKM_OK) return rc;
  unsigned grid;
  size_t lds;
  if ((rc = ens_prepare<T>(dev, "efi", npts, nens, {clim, ens}, &grid, &lds)) != EKM_OK) return rc;
  hipLaunchKernelGGL((efi_points<T>), dim3(grid), dim3(kEnsLanes), lds, static_cast<hipStream_t>(stream), clim, ens, nclim,
                     nens, (unsigned long long)npts, eps, acosdiff, proddiff, acoef, out);
  return launched("efi");
}

template <class T>
static int launch_sot(int dev, void* stream, const T* qc, const T* qc_tail, const T* ens, uint32_t nens, size_t npts,
                      int perc, double eps, T* out) {
  if (npts == 0) return EKM_OK;
  if (perc < 2 || perc > 98 || perc == 50) return set_error(EKM_ERR_ARG, "sot: perc=%d must be in [2, 98] and not 50", perc);
  unsigned grid;
  size_t lds;
  int rc = ens_prepare<T>(dev, "sot", npts, nens, {qc, qc_tail, ens, out}, &grid, &lds);
  if (rc != EKM_OK) return rc;
  hipLaunchKernelGGL((sot_points<T>), dim3(grid), dim3(kEnsLanes), lds, static_cast<hipStream_t>(stream), qc, qc_tail, ens,
                     nens, (unsigned long long)npts, percentile_position<T>(nens, perc), eps, out);
  return launched("sot");
}

template <class T>
static int launch_sot_func(int dev, void* stream, const T* qc_tail, const T* qc, const T* qf, size_t n, double eps,
                           double lower, double upper, T* out) {
  if (n == 0) return EKM_OK;
  int rc = check_pointers("sot_func", sizeof(T), {qc_tail, qc, qf, out});
  unsigned grid;
  if (rc == EKM_OK) rc = launch_grid("sot_func", n, 256, &grid);
  if (rc == EKM_OK) rc = use_device(dev);
  if (rc != EKM_OK) return rc;
  hipLaunchKernelGGL((sot_func_points<T>), dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), qc_tail, qc, qf,
                     (unsigned long long)n, T(eps > 0.0 ? eps : 0.0), T(lower), T(upper), out);
  return launched("sot_func");
}

template <class T, int KIB>
static void launch_cpf_bucket(unsigned grid, void* stream, const T* clim, const T* ens, uint32_t nclim, uint32_t nens,
                              size_t npts, unsigned flags, double epsilon, float* out) {
  hipLaunchKernelGGL((cpf_points<T, KIB>), dim3(grid), dim3(kEnsLanes), 0, static_cast<hipStream_t>(stream), clim, ens, nclim,
                     nens, (unsigned long long)npts, flags, T(epsilon), out);
}

template <class T>
static int launch_cpf(int dev, void* stream, const T* clim, const T* ens, uint32_t nclim, uint32_t nens, size_t npts,
                      int sort_clim, int sort_ens, int from_zero, int symmetric, int use_epsilon, double epsilon,
                      float* out) {
  if (npts == 0) return EKM_OK;
  if (nclim < 1 || nens < 1) return set_error(EKM_ERR_ARG, "cpf: at least one climate row and one member are required");
  const size_t rows = (size_t)nens + (sort_clim ? (size_t)nclim : 0);
  const size_t lds = rows * kEnsLanes * sizeof(T);
  if (lds > kCpfLdsMaxBytes)
    return set_error(EKM_ERR_ARG, "cpf: %u members%s need %zu B of LDS per workgroup (max %zu: %zu rows)", nens,
                     sort_clim ? " and the climate rows to sort" : "", lds, kCpfLdsMaxBytes,
                     kCpfLdsMaxBytes / (kEnsLanes * sizeof(T)));
  int rc = check_pointers("cpf", sizeof(T), {clim, ens});
  if (rc == EKM_OK) rc = check_pointers("cpf", sizeof(float), {out});
  unsigned g;
  if (rc == EKM_OK) rc = launch_grid("cpf", npts, kEnsLanes, &g);
  if (rc == EKM_OK) rc = use_device(dev);
  if (rc != EKM_OK) return rc;
  const unsigned flags = cpf_flags(sort_clim, sort_ens, from_zero, symmetric, use_epsilon);
  if (lds <= 20 * 1024)
    launch_cpf_bucket<T, 20>(g, stream, clim, ens, nclim, nens, npts, flags, epsilon, out);
  else if (lds <= 40 * 1024)
    launch_cpf_bucket<T, 40>(g, stream, clim, ens, nclim, nens, npts, flags, epsilon, out);
  else if (lds <= 80 * 1024)
    launch_cpf_bucket<T, 80>(g, stream, clim, ens, nclim, nens, npts, flags, epsilon, out);
  else
    launch_cpf_bucket<T, 160>(g, stream, clim, ens, nclim, nens, npts, flags, epsilon, out);
  return launched("cpf");
}

template <class T>
static int launch_crps(int dev, void* stream, const T* x, const T* y, uint32_t nens, size_t npts, const double* p2,
                       const double* q2, double* out, uint8_t* missing) {
  if (npts == 0) return EKM_OK;
  if (!p2 || !q2) return set_error(EKM_ERR_ARG, "crps_from_ensemble: null weight table");
  int rc = check_pointers("crps_from_ensemble", sizeof(double), {out});
  if (rc != EKM_OK) return rc;
  unsigned grid;
  size_t lds;
  if ((rc = ens_prepare<T>(dev, "crps_from_ensemble", npts, nens, {x, y}, &grid, &lds)) != EKM_OK) return rc;
  hipLaunchKernelGGL((crps_points<T>), dim3(grid), dim3(kEnsLanes), lds, static_cast<hipStream_t>(stream), x, y, nens,
                     (unsigned long long)npts, p2, q2, out, missing);
  return launched("crps_from_ensemble");
}

template <class T, class Out>
static int launch_quantiles(int dev, void* stream, const T* arr, size_t outer, uint32_t m, size_t inner, const double* lo,
                            const double* hi, const double* w, uint32_t nq, int mode, Out* out) {
  if (outer == 0 || inner == 0 || nq == 0) return EKM_OK;
  if (mode != EKM_QUANTILE_SORT && mode != EKM_QUANTILE_LERP)
    return set_error(EKM_ERR_ENUM, "quantiles: mode=%d is not EKM_QUANTILE_SORT or EKM_QUANTILE_LERP", mode);
  if (mode == EKM_QUANTILE_SORT && sizeof(Out) != sizeof(double))
    return set_error(EKM_ERR_ARG, "quantiles: EKM_QUANTILE_SORT gives float64 (use ekm_quantiles_f32_f64 for float input)");
  if (inner > ~(size_t)0 / outer) return set_error(EKM_ERR_ARG, "quantiles: too many points");
  const size_t npts = outer * inner;
  if (!lo || !hi || !w) return set_error(EKM_ERR_ARG, "quantiles: null position table");
  int rc = check_pointers("quantiles", sizeof(Out), {out});
  if (rc != EKM_OK) return rc;
  unsigned grid;
  size_t lds;
  if ((rc = ens_prepare<T>(dev, "quantiles", npts, m, {arr}, &grid, &lds)) != EKM_OK) return rc;
  hipLaunchKernelGGL((quantile_points<T, Out>), dim3(grid), dim3(kEnsLanes), lds, static_cast<hipStream_t>(stream), arr, m,
                     (unsigned long long)inner, (unsigned long long)npts, lo, hi, w, nq, mode, out);
  return launched("quantiles");
}

template <class T>
static int launch_gumbel_fit(int dev, void* stream, const T* sample, size_t outer, uint32_t m, size_t inner, double* mu,
                             double* sigma) {
  if (outer == 0 || inner == 0) return EKM_OK;
  if (m < 2) return set_error(EKM_ERR_ARG, "gumbel_fit: at least two samples are required, got %u", m);
  if (inner > ~(size_t)0 / outer) return set_error(EKM_ERR_ARG, "gumbel_fit: too many points");
  const size_t npts = outer * inner;
  int rc = check_pointers("gumbel_fit", sizeof(double), {mu, sigma});
  if (rc != EKM_OK) return rc;
  unsigned grid;
  size_t lds;
  if ((rc = ens_prepare<T>(dev, "gumbel_fit", npts, m, {sample}, &grid, &lds)) != EKM_OK) return rc;
  hipLaunchKernelGGL((gumbel_fit_points<T>), dim3(grid), dim3(kEnsLanes), lds, static_cast<hipStream_t>(stream), sample, m,
                     (unsigned long long)inner, (unsigned long long)npts, mu, sigma);
  return launched("gumbel_fit");
}

// The argument checks the two outer-product entry points share; returns the grid size in *grid
static int gumbel_prepare(int dev, const char* what, size_t npts, uint32_t nlev, std::initializer_list<const void*> ptrs,
                          unsigned* grid) {
  int rc = check_pointers(what, sizeof(double), ptrs);
  if (rc != EKM_OK) return rc;
  if (npts > ~(size_t)0 / sizeof(double) / nlev) return set_error(EKM_ERR_ARG, "%s: too many points", what);
  if ((rc = launch_grid(what, npts, kGumbelLanes, grid)) != EKM_OK) return rc;
  return use_device(dev);
}

static int launch_gumbel_cdf(int dev, void* stream, const double* mu, const double* sigma, size_t npts, const double* x,
                             uint32_t nx, double freq, int mode, double* out) {
  if (npts == 0 || nx == 0) return EKM_OK;
  if (mode != EKM_GUMBEL_CDF && mode != EKM_GUMBEL_RETURN_PERIOD)
    return set_error(EKM_ERR_ENUM, "gumbel_cdf: mode=%d is not EKM_GUMBEL_CDF or EKM_GUMBEL_RETURN_PERIOD", mode);
  unsigned grid;
  int rc = gumbel_prepare(dev, "gumbel_cdf", npts, nx, {mu, sigma, x, out}, &grid);
  if (rc != EKM_OK) return rc;
  hipLaunchKernelGGL(gumbel_cdf_points, dim3(grid), dim3(kGumbelLanes), 0, static_cast<hipStream_t>(stream), mu, sigma,
                     (unsigned long long)npts, x, nx, freq, mode, out);
  return launched("gumbel_cdf");
}

static int launch_gumbel_ppf(int dev, void* stream, const double* mu, const double* sigma, size_t npts, const double* t,
                             uint32_t nt, double* out) {
  if (npts == 0 || nt == 0) return EKM_OK;
  unsigned grid;
  int rc = gumbel_prepare(dev, "gumbel_ppf", npts, nt, {mu, sigma, t, out}, &grid);
  if (rc != EKM_OK) return rc;
  hipLaunchKernelGGL(gumbel_ppf_points, dim3(grid), dim3(kGumbelLanes), 0, static_cast<hipStream_t>(stream), mu, sigma,
                     (unsigned long long)npts, t, nt, out);
  return launched("gumbel_ppf");
}

}  // namespace ekm

extern "C" {

int ekm_gumbel_fit_f32(int dev, void* stream, const float* sample, size_t outer, uint32_t m, size_t inner, double* mu,
                       double* sigma) {
  return ekm::launch_gumbel_fit<float>(dev, stream, sample, outer, m, inner, mu, sigma);
}
int ekm_gumbel_fit_f64(int dev, void* stream, const double* sample, size_t outer, uint32_t m, size_t inner, double* mu,
                       double* sigma) {
  return ekm::launch_gumbel_fit<double>(dev, stream, sample, outer, m, inner, mu, sigma);
}
int ekm_gumbel_cdf_f64(int dev, void* stream, const double* mu, const double* sigma, size_t npts, const double* x,
                       uint32_t nx, double freq, int mode, double* out) {
  return ekm::launch_gumbel_cdf(dev, stream, mu, sigma, npts, x, nx, freq, mode, out);
}
int ekm_gumbel_ppf_f64(int dev, void* stream, const double* mu, const double* sigma, size_t npts, const double* t,
                       uint32_t nt, double* out) {
  return ekm::launch_gumbel_ppf(dev, stream, mu, sigma, npts, t, nt, out);
}

int ekm_quantiles_f32(int dev, void* stream, const float* arr, size_t outer, uint32_t m, size_t inner, const double* lo,
                      const double* hi, const double* w, uint32_t nq, int mode, float* out) {
  return ekm::launch_quantiles<float, float>(dev, stream, arr, outer, m, inner, lo, hi, w, nq, mode, out);
}
int ekm_quantiles_f64(int dev, void* stream, const double* arr, size_t outer, uint32_t m, size_t inner, const double* lo,
                      const double* hi, const double* w, uint32_t nq, int mode, double* out) {
  return ekm::launch_quantiles<double, double>(dev, stream, arr, outer, m, inner, lo, hi, w, nq, mode, out);
}
int ekm_quantiles_f32_f64(int dev, void* stream, const float* arr, size_t outer, uint32_t m, size_t inner, const double* lo,
                          const double* hi, const double* w, uint32_t nq, int mode, double* out) {
  return ekm::launch_quantiles<float, double>(dev, stream, arr, outer, m, inner, lo, hi, w, nq, mode, out);
}

int ekm_efi_f32(int dev, void* stream, const float* clim, const float* ens, uint32_t nclim, uint32_t nens, size_t npts,
                double eps, const double* acosdiff, const double* proddiff, const double* acoef, double* out) {
  return ekm::launch_efi<float>(dev, stream, clim, ens, nclim, nens, npts, eps, acosdiff, proddiff, acoef, out);
}
int ekm_efi_f64(int dev, void* stream, const double* clim, const double* ens, uint32_t nclim, uint32_t nens, size_t npts,
                double eps, const double* acosdiff, const double* proddiff, const double* acoef, double* out) {
  return ekm::launch_efi<double>(dev, stream, clim, ens, nclim, nens, npts, eps, acosdiff, proddiff, acoef, out);
}

int ekm_sot_f32(int dev, void* stream, const float* qc, const float* qc_tail, const float* ens, uint32_t nens, size_t npts,
                int perc, double eps, float* out) {
  return ekm::launch_sot<float>(dev, stream, qc, qc_tail, ens, nens, npts, perc, eps, out);
}
int ekm_sot_f64(int dev, void* stream, const double* qc, const double* qc_tail, const double* ens, uint32_t nens,
                size_t npts, int perc, double eps, double* out) {
  return ekm::launch_sot<double>(dev, stream, qc, qc_tail, ens, nens, npts, perc, eps, out);
}

int ekm_sot_func_f32(int dev, void* stream, const float* qc_tail, const float* qc, const float* qf, size_t n, double eps,
                     double lower_bound, double upper_bound, float* out) {
  return ekm::launch_sot_func<float>(dev, stream, qc_tail, qc, qf, n, eps, lower_bound, upper_bound, out);
}
int ekm_sot_func_f64(int dev, void* stream, const double* qc_tail, const double* qc, const double* qf, size_t n, double eps,
                     double lower_bound, double upper_bound, double* out) {
  return ekm::launch_sot_func<double>(dev, stream, qc_tail, qc, qf, n, eps, lower_bound, upper_bound, out);
}

int ekm_cpf_f32(int dev, void* stream, const float* clim, const float* ens, uint32_t nclim, uint32_t nens, size_t npts,
                int sort_clim, int sort_ens, int from_zero, int symmetric, int use_epsilon, double epsilon, float* out) {
  return ekm::launch_cpf<float>(dev, stream, clim, ens, nclim, nens, npts, sort_clim, sort_ens, from_zero, symmetric,
                                use_epsilon, epsilon, out);
}
int ekm_cpf_f64(int dev, void* stream, const double* clim, const double* ens, uint32_t nclim, uint32_t nens, size_t npts,
                int sort_clim, int sort_ens, int from_zero, int symmetric, int use_epsilon, double epsilon, float* out) {
  return ekm::launch_cpf<double>(dev, stream, clim, ens, nclim, nens, npts, sort_clim, sort_ens, from_zero, symmetric,
                                 use_epsilon, epsilon, out);
}

int ekm_crps_from_ensemble_f32(int dev, void* stream, const float* x, const float* y, uint32_t nens, size_t npts,
                               const double* p2, const double* q2, double* out, uint8_t* missing) {
  return ekm::launch_crps<float>(dev, stream, x, y, nens, npts, p2, q2, out, missing);
}
int ekm_crps_from_ensemble_f64(int dev, void* stream, const double* x, const double* y, uint32_t nens, size_t npts,
                               const double* p2, const double* q2, double* out, uint8_t* missing) {
  return ekm::launch_crps<double>(dev, stream, x, y, nens, npts, p2, q2, out, missing);
}

}  // extern "C"
