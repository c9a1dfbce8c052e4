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
//  * nanavg_points / nanavg_rows / nanavg_split (+ nanavg_split_finish): the NaN-skipping (weighted) mean of one axis
//          (reference stats/array/numpy_extended.py:13-61).  Lane per point when the axis is not contiguous (NumPy's
//          order: bit for bit), wave per row when it is, and for few long rows one workgroup per chunk of 32768 elements
//          with the chunks' pairs added in chunk order by a second kernel.  The data is read once (twice by the weighted
//          lane-per-point kernel, which follows the reference's two passes).
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

// ---- nanaverage (reduce_point.hpp states the three layouts and their orders) ----
inline __device__ unsigned long long wave_tree(unsigned long long v) {
#pragma unroll
  for (int off = kWaveLanes / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWaveLanes);
  return v;
}

// The weights of a weighted kernel: element w[o * so + i * sm + j * si] belongs to data[o, i, j]; a stride of 0
// broadcasts.  The unweighted kernels carry none.
template <class T, bool W>
struct NanWeights {
  const T* w;
  unsigned long long so, sm, si;
};
template <class T>
struct NanWeights<T, false> {};

// data: [outer, m, inner]; out: [outer * inner]
template <class T, bool W>
__global__ __launch_bounds__(kPointLanes) void nanavg_points(const T* __restrict__ data, NanWeights<T, W> wt, unsigned long long m,
                                                             unsigned long long inner, unsigned long long npts, T* __restrict__ out) {
  const unsigned long long p = (unsigned long long)blockIdx.x * kPointLanes + threadIdx.x;
  if (p >= npts) return;
  const unsigned long long o = p / inner, j = p - o * inner, base = o * m * inner + j;
  auto d = [&](size_t i) -> T { return data[base + i * inner]; };
  if constexpr (W) {
    const T* w = wt.w + o * wt.so + j * wt.si;
    const unsigned long long sm = wt.sm;
    out[p] = nanavg_point_weighted<T>((size_t)m, d, [&](size_t i) -> T { return w[i * sm]; });
  } else {
    out[p] = nanavg_point<T>((size_t)m, d);
  }
}

// data: [nrows, m]; out: [nrows].  The whole wave leaves together: there is no barrier in this kernel.
template <class T, bool W>
__global__ __launch_bounds__(kNanRowWaves* kWaveLanes) void nanavg_rows(const T* __restrict__ data, NanWeights<T, W> wt,
                                                                        unsigned long long m, unsigned long long nrows,
                                                                        T* __restrict__ out) {
  const unsigned lane = threadIdx.x % kWaveLanes;
  const unsigned long long row = (unsigned long long)blockIdx.x * kNanRowWaves + threadIdx.x / kWaveLanes;
  if (row >= nrows) return;
  const T* w = nullptr;
  size_t ws = 0;
  if constexpr (W) w = wt.w + row * wt.so, ws = (size_t)wt.sm;
  T s;
  nan_q_t<T, W> q;
  nanavg_partial<T, W>(data + row * m, w, ws, 0, (size_t)m, lane, kWaveLanes, s, q);
  s = wave_tree(s);
  q = wave_tree(q);
  if (lane == 0) out[row] = nanavg_finish<T, W>(s, q);
}

// One workgroup per (row, chunk): work[2 * (row * nchunks + chunk)] = the chunk's sum, [.. + 1] = its weight sum or count.
template <class T, bool W>
__global__ __launch_bounds__(kNanSplitThreads) void nanavg_split(const T* __restrict__ data, NanWeights<T, W> wt,
                                                                 unsigned long long m, unsigned long long nchunks,
                                                                 T* __restrict__ work) {
  constexpr int kWaves = kNanSplitThreads / kWaveLanes;
  __shared__ T part_s[kWaves];
  __shared__ nan_q_t<T, W> part_q[kWaves];
  const unsigned long long row = blockIdx.x / nchunks, chunk = blockIdx.x - row * nchunks;
  const unsigned t = threadIdx.x, wave = t / kWaveLanes;
  const size_t begin = (size_t)chunk * kNanSplitChunk;
  const size_t end = begin + kNanSplitChunk < (size_t)m ? begin + kNanSplitChunk : (size_t)m;
  const T* w = nullptr;
  size_t ws = 0;
  if constexpr (W) w = wt.w + row * wt.so, ws = (size_t)wt.sm;
  T s;
  nan_q_t<T, W> q;
  nanavg_partial<T, W>(data + row * m, w, ws, begin, end, t, kNanSplitThreads, s, q);
  s = wave_tree(s);
  q = wave_tree(q);
  if (t % kWaveLanes == 0) part_s[wave] = s, part_q[wave] = q;
  __syncthreads();
  if (t == 0) {
    s = part_s[0], q = part_q[0];
    for (int v = 1; v < kWaves; ++v) nanavg_add<T, W>(s, q, part_s[v], part_q[v]);
    work[2ull * blockIdx.x] = s;
    work[2ull * blockIdx.x + 1] = (T)q;
  }
}

// One wave per row adds the row's pairs in chunk order: 64 pairs are read at a time, then taken lane by lane.
template <class T, bool W>
__global__ __launch_bounds__(kWaveLanes) void nanavg_split_finish(const T* __restrict__ work, unsigned long long nchunks,
                                                                  T* __restrict__ out) {
  const unsigned lane = threadIdx.x;
  const T* pairs = work + 2 * (unsigned long long)blockIdx.x * nchunks;
  T s = T(0);
  nan_q_t<T, W> q = 0;
  for (unsigned long long c0 = 0; c0 < nchunks; c0 += kWaveLanes) {
    const unsigned long long c = c0 + lane;
    const T ps = c < nchunks ? pairs[2 * c] : T(0), pq = c < nchunks ? pairs[2 * c + 1] : T(0);
    const int n = nchunks - c0 < (unsigned long long)kWaveLanes ? (int)(nchunks - c0) : kWaveLanes;
    for (int j = 0; j < n; ++j) nanavg_add<T, W>(s, q, __shfl(ps, j, kWaveLanes), (nan_q_t<T, W>)__shfl(pq, j, kWaveLanes));
  }
  if (lane == 0) out[blockIdx.x] = nanavg_finish<T, W>(s, q);
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

// bytes of `work` the call needs: the pairs of the split path, nothing on the other paths; 0 for arguments that are refused
static size_t nanaverage_work_bytes(size_t elem, size_t outer, size_t m, size_t inner, int path) {
  if (path < kNanAuto || path > kNanSplit || outer == 0 || inner == 0) return 0;
  if ((path == kNanAuto ? nanavg_path(outer, m, inner) : path) != kNanSplit || inner != 1) return 0;
  const size_t nchunks = nanavg_chunks(m);
  if (nchunks > ~(size_t)0 / (2 * elem) / outer) return 0;
  return outer * nchunks * 2 * elem;
}

template <class T, bool W>
static int launch_nanaverage_as(hipStream_t s, int path, const T* data, size_t outer, size_t m, size_t inner, NanWeights<T, W> wt,
                                T* work, T* out) {
  const unsigned long long npts = (unsigned long long)outer * inner;
  unsigned grid;
  int rc;
  if (path == kNanPoints) {
    if ((rc = launch_grid("nanaverage", npts, kPointLanes, &grid)) != EKM_OK) return rc;
    hipLaunchKernelGGL((nanavg_points<T, W>), dim3(grid), dim3(kPointLanes), 0, s, data, wt, (unsigned long long)m,
                       (unsigned long long)inner, npts, out);
  } else if (path == kNanRows) {
    if ((rc = launch_grid("nanaverage", npts, kNanRowWaves, &grid)) != EKM_OK) return rc;
    hipLaunchKernelGGL((nanavg_rows<T, W>), dim3(grid), dim3(kNanRowWaves * kWaveLanes), 0, s, data, wt, (unsigned long long)m, npts,
                       out);
  } else {
    const unsigned long long nchunks = nanavg_chunks(m);
    unsigned rows;
    if ((rc = launch_grid("nanaverage", npts * nchunks, 1, &grid)) != EKM_OK) return rc;
    if ((rc = launch_grid("nanaverage", npts, 1, &rows)) != EKM_OK) return rc;
    hipLaunchKernelGGL((nanavg_split<T, W>), dim3(grid), dim3(kNanSplitThreads), 0, s, data, wt, (unsigned long long)m, nchunks, work);
    if ((rc = launched("nanaverage")) != EKM_OK) return rc;
    hipLaunchKernelGGL((nanavg_split_finish<T, W>), dim3(rows), dim3(kWaveLanes), 0, s, work, nchunks, out);
  }
  return launched("nanaverage");
}

template <class T>
static int launch_nanaverage(int dev, void* stream, const T* data, size_t outer, size_t m, size_t inner, const T* weights,
                             size_t wso, size_t wsm, size_t wsi, int path, void* work, size_t work_bytes, T* out) {
  if (path < kNanAuto || path > kNanSplit)
    return set_error(EKM_ERR_ENUM, "nanaverage: path=%d is not 0 (by shape), 1 (points), 2 (rows) or 3 (split)", path);
  if (outer == 0 || inner == 0) return EKM_OK;
  if (path >= kNanRows && inner != 1)
    return set_error(EKM_ERR_ARG, "nanaverage: path=%d needs a contiguous averaged axis (inner == 1), got inner=%zu", path, inner);
  if (inner > ~(size_t)0 / outer || (m != 0 && m > ~(size_t)0 / sizeof(T) / (outer * inner)))
    return set_error(EKM_ERR_ARG, "nanaverage: too many points");
  int rc = check_pointers("nanaverage", sizeof(T), {data, out});
  if (rc != EKM_OK) return rc;
  if ((rc = check_aligned_if_given("nanaverage", sizeof(T), {weights})) != EKM_OK) return rc;
  if (path == kNanAuto) path = nanavg_path(outer, m, inner);
  if (path == kNanSplit) {
    const size_t need = nanaverage_work_bytes(sizeof(T), outer, m, inner, path);
    if (need == 0) return set_error(EKM_ERR_ARG, "nanaverage: too many points");
    if (!work || work_bytes < need)
      return set_error(EKM_ERR_ARG, "nanaverage: the split path needs %zu bytes of work (ekm_nanaverage_work_bytes), got %zu%s", need,
                       work ? work_bytes : (size_t)0, work ? "" : " (null)");
    if ((rc = check_aligned_if_given("nanaverage", sizeof(T), {work})) != EKM_OK) return rc;
  }
  if ((rc = use_device(dev)) != EKM_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (weights) {
    NanWeights<T, true> wt{weights, (unsigned long long)wso, (unsigned long long)wsm, (unsigned long long)wsi};
    return launch_nanaverage_as<T, true>(s, path, data, outer, m, inner, wt, static_cast<T*>(work), out);
  }
  return launch_nanaverage_as<T, false>(s, path, data, outer, m, inner, NanWeights<T, false>{}, static_cast<T*>(work), out);
}

}  // namespace ekm

extern "C" {

int ekm_nanaverage_f32(int dev, void* stream, const float* data, size_t outer, size_t m, size_t inner, const float* weights,
                       size_t wstride_outer, size_t wstride_m, size_t wstride_inner, int path, void* work, size_t work_bytes,
                       float* out) {
  return ekm::launch_nanaverage<float>(dev, stream, data, outer, m, inner, weights, wstride_outer, wstride_m, wstride_inner, path, work,
                                       work_bytes, out);
}
int ekm_nanaverage_f64(int dev, void* stream, const double* data, size_t outer, size_t m, size_t inner, const double* weights,
                       size_t wstride_outer, size_t wstride_m, size_t wstride_inner, int path, void* work, size_t work_bytes,
                       double* out) {
  return ekm::launch_nanaverage<double>(dev, stream, data, outer, m, inner, weights, wstride_outer, wstride_m, wstride_inner, path, work,
                                        work_bytes, out);
}
size_t ekm_nanaverage_work_bytes(size_t elem_size, size_t outer, size_t m, size_t inner, int weighted, int path) {
  (void)weighted;  // the pairs have the same size with and without weights
  if (elem_size != 4 && elem_size != 8) return 0;
  return ekm::nanaverage_work_bytes(elem_size, outer, m, inner, path);
}

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
