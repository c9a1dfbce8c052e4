// Wind on gfx950: speed and direction from the components, the components from speed and direction, the Coriolis
// parameter, and the wind rose (a two-dimensional histogram of speed and direction).
// Reference: wind/array/wind.py:15-189, :225-328.
//
// Kernel 1, the elementwise family (wind_fields / wind_bcast over wind_point of wind_point.hpp).  Two inputs (coriolis:
// one), one or two outputs, every field read once and written once: xy_to_polar is one launch, 2 reads + 2 writes per
// point.  When every operand is a full field the kernel streams as the map kernels do -- 16 B per lane and access,
// coalesced, non-temporal, one 256-lane tile per workgroup, the n % V ragged tail done element by element by the first
// lanes of workgroup 0.  When an operand is a scalar or a vector along one axis (solar's operand modes) the kernel is
// one lane per point and indexes it.  No LDS, no scratch.  The arithmetic is float for float32 fields, double for float64.
//
// Kernel 2, the wind rose (windrose_count + windrose_finish).  One lane per sample: the speed bin by bisection and the
// sector by one multiply plus a correction against the neighbouring edges, both edge arrays (doubles, made by the host
// with the reference's own expressions) staged in LDS; counts go into a per-workgroup LDS table of 32-bit counters that
// is flushed with one 64-bit global vector atomic per non-zero cell.  Aggregating equal cells within
// the wave before the LDS atomic (readfirstlane + ballot) measured 2-5 % slower on a constant, a smooth and a random
// field alike and is not built (profiles/HISTORY.md).  Tables above kRoseLdsCells go straight to the global table (same kernel, template flag).
// windrose_finish (one workgroup) adds the last direction column to the first, converts to double and applies
// `percent`.  Integer atomics commute, so the counts -- and with them every byte of the result -- are reproducible.
#include <hip/hip_runtime.h>

#include <cmath>

// a * b + c is fused only where the source says fma, as in the host twin (built with -ffp-contract=off): kernel and twin
// then agree bit for bit, which tests/test_gpu_wind.py holds them to
#pragma clang fp contract(off)

#include "../../include/ekm_thermo.h"
#include "launch_checks.hpp"
#include "map_kernel.hpp"
#include "wind_point.hpp"

namespace ekm {

constexpr int kWindThreads = 256;

template <int KIND, int WHICH>
struct WindShape {
  static constexpr int NIN = KIND == WIND_KIND_CORIOLIS ? 1 : 2;
  static constexpr bool kOut0 = KIND != WIND_KIND_POLAR || (WHICH & WIND_SPEED) != 0;
  static constexpr bool kOut1 = KIND == WIND_KIND_XY || (KIND == WIND_KIND_POLAR && (WHICH & WIND_DIRECTION) != 0);
};

// ---- every operand a full field ----
template <class T, int KIND, int MODE, int WHICH>
__global__ __launch_bounds__(kWindThreads) void wind_fields(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out0,
                                                            T* __restrict__ out1, unsigned long long n) {
  typedef WindShape<KIND, WHICH> S;
  typedef typename VecOf<T>::type Vec;
  constexpr int V = VecOf<T>::N;
  const unsigned long long nvec = n / V;
  const unsigned long long v = (unsigned long long)blockIdx.x * kWindThreads + threadIdx.x;
  if (v < nvec) {
    const Vec va = ld_stream<T>(a + v * V);
    Vec vb = va;
    if constexpr (S::NIN == 2) vb = ld_stream<T>(b + v * V);
    Vec y0, y1;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      T o0, o1;
      wind_point<T, KIND, MODE, WHICH>(va[j], vb[j], o0, o1);
      y0[j] = o0;
      y1[j] = o1;
    }
    if constexpr (S::kOut0) st_stream<T>(out0 + v * V, y0);
    if constexpr (S::kOut1) st_stream<T>(out1 + v * V, y1);
  }
  // ragged tail: n % V single elements, done by the first lanes of workgroup 0
  const unsigned long long e = nvec * V + v;
  if (e < n) {
    T o0, o1;
    wind_point<T, KIND, MODE, WHICH>(a[e], S::NIN == 2 ? b[e] : T(0), o0, o1);
    if constexpr (S::kOut0) out0[e] = o0;
    if constexpr (S::kOut1) out1[e] = o1;
  }
}

// ---- some operand a scalar or a vector along one axis ----
template <class T, int KIND, int MODE, int WHICH>
__global__ __launch_bounds__(kWindThreads) void wind_bcast(const PointOperand<T> a, const PointOperand<T> b, T* __restrict__ out0,
                                                           T* __restrict__ out1, unsigned long long n, int small) {
  typedef WindShape<KIND, WHICH> S;
  const unsigned long long p = (unsigned long long)blockIdx.x * kWindThreads + threadIdx.x;
  if (p >= n) return;
  const T x = (T)point_fetch<T>(a, p, small != 0);  // (point_fetch hands the element back as a double: exact both ways)
  const T y = S::NIN == 2 ? (T)point_fetch<T>(b, p, small != 0) : T(0);
  T o0, o1;
  wind_point<T, KIND, MODE, WHICH>(x, y, o0, o1);
  if constexpr (S::kOut0) out0[p] = o0;
  if constexpr (S::kOut1) out1[p] = o1;
}

template <class T, int KIND, int MODE, int WHICH>
static int launch_wind_as(int dev, hipStream_t s, const PointOperand<T>& a, const PointOperand<T>& b, bool fields, bool small, T* out0,
                          T* out1, size_t n) {
  constexpr int V = VecOf<T>::N;
  const unsigned long long items = fields ? ((unsigned long long)n / V > 0 ? (unsigned long long)n / V : 1ull) : (unsigned long long)n;
  unsigned g;
  int rc = launch_grid("wind", items, kWindThreads, &g);
  if (rc == EKM_OK) rc = use_device(dev);
  if (rc != EKM_OK) return rc;
  if (fields)
    hipLaunchKernelGGL((wind_fields<T, KIND, MODE, WHICH>), dim3(g), dim3(kWindThreads), 0, s, a.data, b.data, out0, out1,
                       (unsigned long long)n);
  else
    hipLaunchKernelGGL((wind_bcast<T, KIND, MODE, WHICH>), dim3(g), dim3(kWindThreads), 0, s, a, b, out0, out1,
                       (unsigned long long)n, small ? 1 : 0);
  return launched("wind");
}

template <class T, int KIND>
static int launch_wind(const char* what, int dev, void* stream, const ekm_operand* a, const ekm_operand* b, int mode, T* out0, T* out1,
                       size_t n) {
  if (n == 0) return EKM_OK;
  const int nmodes = KIND == WIND_KIND_POLAR ? 3 : KIND == WIND_KIND_XY ? 2 : 1;
  if (mode < 0 || mode >= nmodes) return set_error(EKM_ERR_ENUM, "%s: convention %d out of range", what, mode);
  if (KIND == WIND_KIND_POLAR ? (!out0 && !out1) : (!out0 || (KIND == WIND_KIND_XY && !out1)))
    return set_error(EKM_ERR_ARG, "%s: an output is null", what);
  int rc = check_aligned_if_given(what, sizeof(T), {out0, out1});
  if (rc != EKM_OK) return rc;
  bool small = (unsigned long long)n <= 0x100000000ull, fields = true;
  PointOperand<T> oa, ob;
  if ((rc = check_point_operand<T>(what, "the first operand", a, n, &oa, &small, &fields)) != EKM_OK) return rc;
  ob = oa;
  if (KIND != WIND_KIND_CORIOLIS && (rc = check_point_operand<T>(what, "the second operand", b, n, &ob, &small, &fields)) != EKM_OK)
    return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
#define EKM_WIND_GO(MODE_, WHICH_) return launch_wind_as<T, KIND, MODE_, WHICH_>(dev, s, oa, ob, fields, small, out0, out1, n)
  if constexpr (KIND == WIND_KIND_POLAR) {
    if (!out1) EKM_WIND_GO(WIND_METEO, WIND_SPEED);  // the speed does not depend on the convention
    if (!out0) {
      if (mode == WIND_METEO) EKM_WIND_GO(WIND_METEO, WIND_DIRECTION);
      if (mode == WIND_POLAR_POSITIVE) EKM_WIND_GO(WIND_POLAR_POSITIVE, WIND_DIRECTION);
      EKM_WIND_GO(WIND_POLAR_SIGNED, WIND_DIRECTION);
    }
    if (mode == WIND_METEO) EKM_WIND_GO(WIND_METEO, WIND_SPEED | WIND_DIRECTION);
    if (mode == WIND_POLAR_POSITIVE) EKM_WIND_GO(WIND_POLAR_POSITIVE, WIND_SPEED | WIND_DIRECTION);
    EKM_WIND_GO(WIND_POLAR_SIGNED, WIND_SPEED | WIND_DIRECTION);
  } else if constexpr (KIND == WIND_KIND_XY) {
    if (mode == WIND_METEO) EKM_WIND_GO(WIND_METEO, 3);
    EKM_WIND_GO(WIND_POLAR_POSITIVE, 3);
  } else {
    EKM_WIND_GO(WIND_METEO, 1);
  }
#undef EKM_WIND_GO
}

// ---- wind rose ----
constexpr unsigned kRoseLdsCells = 8192;   // largest table kept in LDS (32 KiB of 32-bit counters)
constexpr unsigned kRoseMaxEdges = 2048;   // speed + direction edges staged in LDS (16 KiB of doubles)
constexpr unsigned kRoseMaxGrid = 2048;    // workgroups; each walks its samples with a grid stride

extern __shared__ __align__(16) unsigned char rose_lds_raw[];

template <class T, bool LDS_TABLE>
__global__ __launch_bounds__(kWindThreads) void windrose_count(const T* __restrict__ speed, const T* __restrict__ dir,
                                                              unsigned long long n, const double* __restrict__ edges, unsigned ns,
                                                              unsigned nd, double inv_step, unsigned cells,
                                                              unsigned long long* __restrict__ table) {
  double* e_lds = reinterpret_cast<double*>(rose_lds_raw);
  unsigned* t_lds = reinterpret_cast<unsigned*>(rose_lds_raw + (size_t)(ns + nd) * sizeof(double));
  for (unsigned i = threadIdx.x; i < ns + nd; i += kWindThreads) e_lds[i] = edges[i];
  if constexpr (LDS_TABLE)
    for (unsigned i = threadIdx.x; i < cells; i += kWindThreads) t_lds[i] = 0u;
  __syncthreads();
  const double* se = e_lds;
  const double* de = e_lds + ns;
  const unsigned long long stride = (unsigned long long)gridDim.x * kWindThreads;
  const unsigned long long first = (unsigned long long)blockIdx.x * kWindThreads;
  for (unsigned long long base = first; base < n; base += stride) {
    const unsigned long long p = base + threadIdx.x;
    int cell = -1;
    if (p < n)
      cell = wind_cell((double)speed[p], (double)dir[p], [&](unsigned k) { return se[k]; }, ns, [&](unsigned k) { return de[k]; }, nd,
                       inv_step);
    if (cell >= 0) {
      if constexpr (LDS_TABLE)
        atomicAdd(&t_lds[cell], 1u);
      else
        atomicAdd(&table[cell], 1ull);
    }
  }
  if constexpr (LDS_TABLE) {
    __syncthreads();
    for (unsigned i = threadIdx.x; i < cells; i += kWindThreads) {
      const unsigned c = t_lds[i];
      if (c != 0u) atomicAdd(&table[i], (unsigned long long)c);
    }
  }
}

// table[rows][cols] of counts -> out[rows][cols - 1]: column cols - 1 joins column 0; one workgroup.
__global__ __launch_bounds__(kWindThreads) void windrose_finish(const unsigned long long* __restrict__ table, unsigned rows, unsigned cols,
                                                               int percent, double* __restrict__ out) {
  __shared__ unsigned long long part[kWindThreads];
  const unsigned cells = rows * cols;
  unsigned long long mine = 0;
  for (unsigned i = threadIdx.x; i < cells; i += kWindThreads) mine += table[i];
  part[threadIdx.x] = mine;
  __syncthreads();
  for (unsigned w = kWindThreads / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  const unsigned long long total = part[0];
  const unsigned oc = cols - 1;
  for (unsigned i = threadIdx.x; i < rows * oc; i += kWindThreads) {
    const unsigned r = i / oc, c = i % oc;
    unsigned long long v = table[r * cols + c];
    if (c == 0) v += table[r * cols + cols - 1];
    out[i] = wind_rose_value(v, total, percent);
  }
}

template <class T>
static int launch_windrose(int dev, void* stream, const T* speed, const T* dir, size_t n, const double* edges, uint32_t ns, uint32_t nd,
                           double inv_step, int percent, unsigned long long* table, double* out) {
  if (ns < 2 || nd < 3) return set_error(EKM_ERR_ARG, "windrose: needs at least 2 speed edges and 3 direction edges (got %u, %u)", ns, nd);
  if ((unsigned long long)ns + nd > kRoseMaxEdges)
    return set_error(EKM_ERR_ARG, "windrose: %u + %u edges, at most %u together", ns, nd, kRoseMaxEdges);
  int rc = n > 0 ? check_pointers("windrose", sizeof(T), {speed, dir}) : EKM_OK;
  if (rc == EKM_OK) rc = check_pointers("windrose", 8, {edges, table, out});
  if (rc != EKM_OK) return rc;
  if (!(inv_step == inv_step)) return set_error(EKM_ERR_ARG, "windrose: inv_step is NaN");
  const unsigned cells = (ns - 1) * (nd - 1);
  if ((rc = use_device(dev)) != EKM_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(table, 0, (size_t)cells * sizeof(unsigned long long), s);
  if (e != hipSuccess) return set_error(EKM_ERR_HIP, "windrose memset: %s", hipGetErrorString(e));
  if (n > 0) {
    unsigned long long g = ((unsigned long long)n + kWindThreads - 1) / kWindThreads;
    if (g > kRoseMaxGrid) g = kRoseMaxGrid;
    if ((unsigned long long)n / g >= 0xffffffffull) return set_error(EKM_ERR_ARG, "windrose: too many samples for the 32-bit counters");
    const bool lds = cells <= kRoseLdsCells;
    const size_t bytes = (size_t)(ns + nd) * sizeof(double) + (lds ? (size_t)cells * sizeof(unsigned) : 0);
    if (lds)
      hipLaunchKernelGGL((windrose_count<T, true>), dim3((unsigned)g), dim3(kWindThreads), bytes, s, speed, dir, (unsigned long long)n, edges,
                         ns, nd, inv_step, cells, table);
    else
      hipLaunchKernelGGL((windrose_count<T, false>), dim3((unsigned)g), dim3(kWindThreads), bytes, s, speed, dir, (unsigned long long)n, edges,
                         ns, nd, inv_step, cells, table);
    if ((rc = launched("windrose")) != EKM_OK) return rc;
  }
  hipLaunchKernelGGL(windrose_finish, dim3(1), dim3(kWindThreads), 0, s, table, ns - 1, nd - 1, percent, out);
  return launched("windrose finish");
}

}  // namespace ekm

extern "C" {

#define EKM_WIND_ENTRIES(tag, T)                                                                                                   \
  int ekm_wind_polar_##tag(int dev, void* stream, const ekm_operand* u, const ekm_operand* v, int mode, T* speed, T* direction,    \
                           size_t n) {                                                                                             \
    return ekm::launch_wind<T, ekm::WIND_KIND_POLAR>("wind_polar", dev, stream, u, v, mode, speed, direction, n);                  \
  }                                                                                                                                \
  int ekm_wind_xy_##tag(int dev, void* stream, const ekm_operand* magnitude, const ekm_operand* direction, int mode, T* x, T* y,   \
                        size_t n) {                                                                                                \
    return ekm::launch_wind<T, ekm::WIND_KIND_XY>("wind_xy", dev, stream, magnitude, direction, mode, x, y, n);                    \
  }                                                                                                                                \
  int ekm_wind_coriolis_##tag(int dev, void* stream, const ekm_operand* lat, T* out, size_t n) {                                   \
    return ekm::launch_wind<T, ekm::WIND_KIND_CORIOLIS>("wind_coriolis", dev, stream, lat, nullptr, 0, out, nullptr, n);           \
  }                                                                                                                                \
  int ekm_windrose_##tag(int dev, void* stream, const T* speed, const T* direction, size_t n, const double* edges, uint32_t ns,    \
                         uint32_t nd, double inv_step, int percent, unsigned long long* table, double* out) {                      \
    return ekm::launch_windrose<T>(dev, stream, speed, direction, n, edges, ns, nd, inv_step, percent, table, out);                \
  }
EKM_WIND_ENTRIES(f32, float)
EKM_WIND_ENTRIES(f64, double)
#undef EKM_WIND_ENTRIES

}  // extern "C"
