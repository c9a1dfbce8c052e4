// The reduce family: sums along a LONG axis, streamed from memory and added across lanes in a fixed order.
//  * project_fields: out[p, n] = scale[n] * sum_k f[n, k] * c[p, k] (reference regimes/array/index.py:10-56).  One
//          workgroup of 256 lanes per field; a lane reads the field row in 16-byte chunks and keeps up to 8 pattern
//          sums in registers, so the row is read once per group of 8 patterns; the coefficient rows (P * K values) are
//          read by every workgroup and stay in L2.  Wave butterfly, then the four wave sums through LDS in wave order.
//  * standardise: (proj - mean) / std, elementwise (index.py:59-76).
//  * pearson_points: sample axis not contiguous (inner > 1): one lane per point walks its m samples three times
//          (mean; norms; products), rows coalesced along `inner`.  2 * 3 * m * sizeof(T) bytes read per point.
//  * pearson_rows: sample axis contiguous (inner == 1): one wave per row, lanes stride the row, three passes each
//          ended by the wave butterfly; passes two and three re-read the row from cache.
// No floating-point atomics: every sum has one order, stated in reduce_point.hpp and shared with the host twin.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/ekm_thermo.h"
#include "launch_checks.hpp"
#include "map_kernel.hpp"
#include "reduce_point.hpp"

namespace ekm {

constexpr int kProjWaves = kProjThreads / kWaveLanes;
constexpr int kPointLanes = 256;  // standardise, pearson_points: one lane per point
constexpr int kRowWaves = 4;      // pearson_rows: rows (waves) per workgroup

template <class T>
__device__ __forceinline__ T wave_tree(T v) {
#pragma unroll
  for (int off = kWaveLanes / 2; off >= 1; off >>= 1) v = en_add(v, __shfl_xor(v, off, kWaveLanes));
  return v;
}

// field: [nfields, K]; coef: row p of field n at coef[n * cstride + p * K] (cstride 0: shared by all fields);
// scale: [nfields] or null; out: [NP, nfields] with row stride nfields.
template <class T, int NP>
__global__ __launch_bounds__(kProjThreads) void project_fields(const T* __restrict__ field, const T* __restrict__ coef,
                                                              unsigned long long K, unsigned long long cstride,
                                                              const T* __restrict__ scale, unsigned long long nfields,
                                                              T* __restrict__ out) {
  __shared__ T part[NP][kProjWaves];
  const unsigned long long n = blockIdx.x;
  const unsigned t = threadIdx.x, wave = t / kWaveLanes;
  T acc[NP];
  project_partial<T, NP>(field + n * K, coef + n * cstride, (size_t)K, t, acc);
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const T s = wave_tree(acc[p]);
    if (t % kWaveLanes == 0) part[p][wave] = s;
  }
  __syncthreads();
  if (t < NP) out[(unsigned long long)t * nfields + n] = project_finish<T>(part[t], kProjWaves, scale != nullptr, scale ? scale[n] : T(0));
}

template <class T>
__global__ __launch_bounds__(kPointLanes) void standardise(const T* __restrict__ proj, const T* __restrict__ mean, T mean_value,
                                                           const T* __restrict__ std, T std_value, unsigned long long n,
                                                           T* __restrict__ out) {
  const unsigned long long i = (unsigned long long)blockIdx.x * kPointLanes + threadIdx.x;
  if (i >= n) return;
  out[i] = standardise_point<T>(proj[i], mean ? mean[i] : mean_value, std ? std[i] : std_value);
}

// x, y: [outer, m, inner]; out: [outer * inner]
template <class T>
__global__ __launch_bounds__(kPointLanes) void pearson_points(const T* __restrict__ x, const T* __restrict__ y,
                                                              unsigned long long m, unsigned long long inner,
                                                              unsigned long long npts, T* __restrict__ out) {
  const unsigned long long p = (unsigned long long)blockIdx.x * kPointLanes + threadIdx.x;
  if (p >= npts) return;
  const unsigned long long o = p / inner, base = o * m * inner + (p - o * inner);
  out[p] = pearson_point<T>(
      (size_t)m, [&](size_t i) -> T { return x[base + i * inner]; }, [&](size_t i) -> T { return y[base + i * inner]; });
}

// x, y: [nrows, m]; out: [nrows].  The whole wave leaves together: there is no barrier in this kernel.
template <class T>
__global__ __launch_bounds__(kRowWaves* kWaveLanes) void pearson_rows(const T* __restrict__ x, const T* __restrict__ y,
                                                                      unsigned long long m, unsigned long long nrows,
                                                                      T* __restrict__ out) {
  const unsigned lane = threadIdx.x % kWaveLanes;
  const unsigned long long row = (unsigned long long)blockIdx.x * kRowWaves + threadIdx.x / kWaveLanes;
  if (row >= nrows) return;
  const T* xr = x + row * m;
  const T* yr = y + row * m;
  const T mx = wave_tree(rows_partial_sum<T>(xr, (size_t)m, lane)) / T(m);
  const T my = wave_tree(rows_partial_sum<T>(yr, (size_t)m, lane)) / T(m);
  const T nx = std::sqrt(wave_tree(rows_partial_squares<T>(xr, (size_t)m, lane, mx)));
  const T ny = std::sqrt(wave_tree(rows_partial_squares<T>(yr, (size_t)m, lane, my)));
  const T r = wave_tree(rows_partial_products<T>(xr, yr, (size_t)m, lane, mx, my, nx, ny));
  if (lane == 0) out[row] = r;
}

template <class T, int NP>
static void project_group(hipStream_t s, unsigned grid, const T* field, const T* coef, size_t k, size_t cstride, const T* scale,
                          size_t nfields, T* out) {
  hipLaunchKernelGGL((project_fields<T, NP>), dim3(grid), dim3(kProjThreads), 0, s, field, coef, (unsigned long long)k,
                     (unsigned long long)cstride, scale, (unsigned long long)nfields, out);
}

template <class T>
static int launch_project(int dev, void* stream, const T* field, size_t nfields, size_t k, const T* coef, uint32_t npat,
                          size_t cstride, const T* scale, T* out) {
  if (nfields == 0 || npat == 0) return EKM_OK;
  if (k < 1) return set_error(EKM_ERR_ARG, "regimes_project: a pattern needs at least one grid point");
  if (k > ~(size_t)0 / sizeof(T) / nfields) return set_error(EKM_ERR_ARG, "regimes_project: too many points");
  if (cstride != 0 && cstride < (size_t)npat * k)
    return set_error(EKM_ERR_ARG, "regimes_project: coef_stride=%zu is neither 0 nor at least npat * k = %zu", cstride, (size_t)npat * k);
  int rc = check_pointers("regimes_project", sizeof(T), {field, coef, out});
  if (rc != EKM_OK) return rc;
  if ((rc = check_aligned_if_given("regimes_project", sizeof(T), {scale})) != EKM_OK) return rc;
  unsigned grid;
  if ((rc = launch_grid("regimes_project", nfields, 1, &grid)) != EKM_OK) return rc;
  if ((rc = use_device(dev)) != EKM_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  for (uint32_t p0 = 0; p0 < npat; p0 += kProjGroup) {
    const T* c = coef + (size_t)p0 * k;
    T* o = out + (size_t)p0 * nfields;
    switch (npat - p0 < (uint32_t)kProjGroup ? npat - p0 : (uint32_t)kProjGroup) {
      case 1: project_group<T, 1>(s, grid, field, c, k, cstride, scale, nfields, o); break;
      case 2: project_group<T, 2>(s, grid, field, c, k, cstride, scale, nfields, o); break;
      case 3: project_group<T, 3>(s, grid, field, c, k, cstride, scale, nfields, o); break;
      case 4: project_group<T, 4>(s, grid, field, c, k, cstride, scale, nfields, o); break;
      case 5: project_group<T, 5>(s, grid, field, c, k, cstride, scale, nfields, o); break;
      case 6: project_group<T, 6>(s, grid, field, c, k, cstride, scale, nfields, o); break;
      case 7: project_group<T, 7>(s, grid, field, c, k, cstride, scale, nfields, o); break;
      default: project_group<T, 8>(s, grid, field, c, k, cstride, scale, nfields, o); break;
    }
    if ((rc = launched("regimes_project")) != EKM_OK) return rc;
  }
  return EKM_OK;
}

template <class T>
static int launch_index(int dev, void* stream, const T* proj, const T* mean, T mean_value, const T* std, T std_value, T* out,
                        size_t n) {
  if (n == 0) return EKM_OK;
  int rc = check_pointers("regimes_index", sizeof(T), {proj, out});
  if (rc != EKM_OK) return rc;
  if ((rc = check_aligned_if_given("regimes_index", sizeof(T), {mean, std})) != EKM_OK) return rc;
  unsigned grid;
  if ((rc = launch_grid("regimes_index", n, kPointLanes, &grid)) != EKM_OK) return rc;
  if ((rc = use_device(dev)) != EKM_OK) return rc;
  hipLaunchKernelGGL((standardise<T>), dim3(grid), dim3(kPointLanes), 0, static_cast<hipStream_t>(stream), proj, mean, mean_value,
                     std, std_value, (unsigned long long)n, out);
  return launched("regimes_index");
}

template <class T>
static int launch_pearson(int dev, void* stream, const T* x, const T* y, size_t outer, size_t m, size_t inner, T* out) {
  if (outer == 0 || inner == 0) return EKM_OK;
  if (m < 1) return set_error(EKM_ERR_ARG, "pearson: the sample axis is empty");
  if (inner > ~(size_t)0 / outer || m > ~(size_t)0 / sizeof(T) / (outer * inner)) return set_error(EKM_ERR_ARG, "pearson: too many points");
  int rc = check_pointers("pearson", sizeof(T), {x, y, out});
  if (rc != EKM_OK) return rc;
  const unsigned long long npts = (unsigned long long)outer * inner;
  unsigned grid;
  const int per_block = inner == 1 ? kRowWaves : kPointLanes;
  if ((rc = launch_grid("pearson", npts, per_block, &grid)) != EKM_OK) return rc;
  if ((rc = use_device(dev)) != EKM_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (inner == 1)
    hipLaunchKernelGGL((pearson_rows<T>), dim3(grid), dim3(kRowWaves * kWaveLanes), 0, s, x, y, (unsigned long long)m, npts, out);
  else
    hipLaunchKernelGGL((pearson_points<T>), dim3(grid), dim3(kPointLanes), 0, s, x, y, (unsigned long long)m,
                       (unsigned long long)inner, npts, out);
  return launched("pearson");
}

}  // namespace ekm

extern "C" {

int ekm_regimes_project_f32(int dev, void* stream, const float* field, size_t nfields, size_t k, const float* coef, uint32_t npat,
                            size_t coef_stride, const float* scale, float* out) {
  return ekm::launch_project<float>(dev, stream, field, nfields, k, coef, npat, coef_stride, scale, out);
}
int ekm_regimes_project_f64(int dev, void* stream, const double* field, size_t nfields, size_t k, const double* coef,
                            uint32_t npat, size_t coef_stride, const double* scale, double* out) {
  return ekm::launch_project<double>(dev, stream, field, nfields, k, coef, npat, coef_stride, scale, out);
}
int ekm_regimes_index_f32(int dev, void* stream, const float* proj, const float* mean, float mean_value, const float* std,
                          float std_value, float* out, size_t n) {
  return ekm::launch_index<float>(dev, stream, proj, mean, mean_value, std, std_value, out, n);
}
int ekm_regimes_index_f64(int dev, void* stream, const double* proj, const double* mean, double mean_value, const double* std,
                          double std_value, double* out, size_t n) {
  return ekm::launch_index<double>(dev, stream, proj, mean, mean_value, std, std_value, out, n);
}
int ekm_pearson_f32(int dev, void* stream, const float* x, const float* y, size_t outer, size_t m, size_t inner, float* out) {
  return ekm::launch_pearson<float>(dev, stream, x, y, outer, m, inner, out);
}
int ekm_pearson_f64(int dev, void* stream, const double* x, const double* y, size_t outer, size_t m, size_t inner, double* out) {
  return ekm::launch_pearson<double>(dev, stream, x, y, outer, m, inner, out);
}

}  // extern "C"
