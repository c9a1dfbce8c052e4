// Vertical interpolation from model levels to pressure / height levels on gfx950.
// Reference: vertical/array/monotonic.py and vertical/array/vertical.py:1206-1719 (interpolate_monotonic,
// interpolate_hybrid_to_pressure_levels; the two ->height functions feed the generic kernel a height field).
//
// Output-driven: one workgroup per (column tile, target).  A lane owns 4 (fp32) / 2 (fp64) consecutive columns of a
// level-major [level, npts] field, finds the bracket of its target in each by bisection over the levels (at most 8
// probes for 137 levels), gathers the two bracketing data rows and writes one 16-B non-temporal store.  Neighbouring
// columns bracket at the same or adjacent levels, so the gathers stay mostly coalesced; a lane whose columns all
// bracket at the same interior level takes the two rows as 16-B loads.
//  * FUSED (hybrid -> pressure): the coordinate is p_full formed from sp and the A/B half-level tables in LDS
//    (interp_point.hpp::hybrid_p_full); the pressure field is never read from or written to HBM.  The grid runs bands
//    of surface pressure, all targets of a band before the next band (as hybrid_rows does with its levels), so sp is
//    re-read from L2.  Algorithmic traffic: 2 data elements read + 1 written per output point, + sp once.
//  * generic: the coordinate is a field streamed like the data (probed by the same bisection: ~log2(nlev) + 2 gathers
//    per point) or a level vector (stride 0).
// The per-point arithmetic is interp_point.hpp, shared with the host twin.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/ekm_thermo.h"
#include "interp_point.hpp"
#include "launch_checks.hpp"
#include "map_kernel.hpp"

namespace ekm {

template <class T>
struct InterpArgs {
  const T* data;    // [nlev, npts]
  const T* coord;   // generic: [nlev, npts] (coord_stride = npts) or [nlev] (coord_stride = 0); FUSED: unused
  const T* A;       // FUSED: nlev + 1 half-level coefficients
  const T* B;
  const T* sp;      // FUSED: [npts]
  const T* target;  // [ntarget] or [ntarget, npts]
  const T* aux[4];  // min_data, min_coord, max_data, max_coord: NULL, one value, or [npts] (aux_field bit i)
  T* out;           // [ntarget, npts]
  unsigned long long npts, coord_stride;
  unsigned nlev;
  int target_is_field, aux_field, descending, mode, vec_ok;
};

template <class T, bool FUSED>
__global__ __launch_bounds__(kThreads) void interp_columns(const InterpArgs<T> a) {
  constexpr int V = VecOf<T>::N;
  typedef typename VecOf<T>::type Vec;
  T* tab = reinterpret_cast<T*>(ekm_lds_raw);  // FUSED: A[0..nlev], B[0..nlev]
  if (FUSED) {
    for (unsigned s = threadIdx.x; s <= a.nlev; s += kThreads) {
      tab[s] = a.A[s];
      tab[a.nlev + 1 + s] = a.B[s];
    }
    __syncthreads();
  }
  const unsigned t = blockIdx.y;  // target, wave-uniform
  const unsigned long long tile = (unsigned long long)blockIdx.z * gridDim.x + blockIdx.x;
  const unsigned long long i0 = (tile * kThreads + threadIdx.x) * V;
  if (i0 >= a.npts) return;
  const bool whole = a.vec_ok && (i0 + V <= a.npts);
  const unsigned nlev = a.nlev;
  const unsigned long long npts = a.npts;

  Vec s, tcv;
#pragma unroll
  for (int j = 0; j < V; ++j) s[j] = tcv[j] = T(1);
  if (FUSED) {
    if (whole) {
      s = ld_cached<T>(a.sp + i0);  // cached: the other targets of the band re-read it
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (i0 + j < npts) s[j] = a.sp[i0 + j];
    }
  }
  if (a.target_is_field) {
    const T* src = a.target + (unsigned long long)t * npts + i0;
    if (whole) {
      tcv = ld_stream<T>(src);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j)
        if (i0 + j < npts) tcv[j] = src[j];
    }
  } else {
    const T tc = a.target[t];
#pragma unroll
    for (int j = 0; j < V; ++j) tcv[j] = tc;
  }

  auto coord_of = [&](int j, unsigned m) -> T {
    if (FUSED) return hybrid_p_full(tab[m], tab[nlev + 1 + m], tab[m + 1], tab[nlev + 2 + m], s[j]);
    return a.coord[a.coord_stride ? (unsigned long long)m * a.coord_stride + i0 + j : (unsigned long long)m];
  };

  unsigned idx[V];
  bool same = whole;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    idx[j] = 0;
    if (i0 + j < npts) idx[j] = interp_bracket<T>(nlev, a.descending, tcv[j], [&](unsigned m) { return coord_of(j, m); });
    same = same && idx[j] == idx[0];
  }
  same = same && idx[0] > 0 && idx[0] < nlev;
  Vec db, dt;
  unsigned mb = 0;
  if (same) {  // one interior bracket for the lane's V columns: the two data rows as 16-B loads
    mb = a.descending ? idx[0] - 1 : nlev - idx[0];
    const unsigned mt = a.descending ? idx[0] : nlev - 1 - idx[0];
    db = ld_stream<T>(a.data + (unsigned long long)mb * npts + i0);
    dt = ld_stream<T>(a.data + (unsigned long long)mt * npts + i0);
  }

  Vec o;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    o[j] = T(0);
    if (i0 + j < npts) {
      InterpAux<T> lay[2];  // [0]: beyond the smallest coordinate (aux_min_level_*), [1]: beyond the largest
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const T* ad = a.aux[2 * e];
        const T* ac = a.aux[2 * e + 1];
        lay[e].on = ad && ac;
        lay[e].data = lay[e].coord = T(0);
        if (lay[e].on) {
          lay[e].data = ad[(a.aux_field >> (2 * e)) & 1 ? i0 + j : 0ull];
          lay[e].coord = ac[(a.aux_field >> (2 * e + 1)) & 1 ? i0 + j : 0ull];
        }
      }
      auto data_of = [&](unsigned m) -> T {
        if (same) return m == mb ? db[j] : dt[j];
        return a.data[(unsigned long long)m * npts + i0 + j];
      };
      o[j] = interp_value<T>(idx[j], nlev, a.descending, a.mode, tcv[j], [&](unsigned m) { return coord_of(j, m); },
                             data_of, lay[1], lay[0]);
    }
  }
  T* dst = a.out + (unsigned long long)t * npts + i0;
  if (whole) {
    st_stream<T>(dst, o);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (i0 + j < npts) dst[j] = o[j];
  }
}

template <class T, bool FUSED>
static int launch_interp(int dev, void* stream, InterpArgs<T> a, uint32_t ntarget, const char* what) {
  if (a.npts == 0 || ntarget == 0) return EKM_OK;
  if (!a.data || !a.target || !a.out) return set_error(EKM_ERR_ARG, "%s: null data/target/out", what);
  if (FUSED ? (!a.A || !a.B || !a.sp) : !a.coord) return set_error(EKM_ERR_ARG, "%s: null coordinate", what);
  if (a.nlev < 2) return set_error(EKM_ERR_ARG, "%s: at least two levels are required (got %u)", what, a.nlev);
  if (a.mode < 0 || a.mode > 2) return set_error(EKM_ERR_ENUM, "%s: interpolation=%d", what, a.mode);
  if (ntarget > 65535u) return set_error(EKM_ERR_ARG, "%s: at most 65535 targets per call (got %u)", what, ntarget);
  const size_t lds = FUSED ? 2 * (size_t)(a.nlev + 1) * sizeof(T) : 0;
  if (lds > kMaxLdsBytes) return set_error(EKM_ERR_ARG, "%s: %u levels need %zu B of LDS (max %zu)", what, a.nlev, lds, (size_t)kMaxLdsBytes);
  int rc = use_device(dev);
  if (rc != EKM_OK) return rc;
  constexpr int V = VecOf<T>::N;
  a.vec_ok = (a.npts % V == 0);  // rows of data / target / out start at multiples of npts elements
  rc = check_aligned_if_given(what, sizeof(T), {a.data, a.coord, a.sp, a.target, a.out, a.aux[0], a.aux[1], a.aux[2], a.aux[3]});
  unsigned grid;  // workgroups of kThreads lanes, V columns per lane
  if (rc == EKM_OK) rc = launch_grid(what, a.npts, kThreads * V, &grid);
  if (rc != EKM_OK) return rc;
  // bands of surface pressure / columns, every target of a band before the next band (hybrid_rows does the same)
  unsigned long long band = (unsigned long long)tuning_hybrid_band_bytes() / ((unsigned long long)kThreads * V * sizeof(T));
  if (band < 8) band = 8;
  if (band > grid) band = grid;
  while ((grid + band - 1) / band > 65535ull) band *= 2;
  hipLaunchKernelGGL((interp_columns<T, FUSED>), dim3((unsigned)band, ntarget, (unsigned)((grid + band - 1) / band)),
                     dim3(kThreads), lds, static_cast<hipStream_t>(stream), a);
  return launched(what);
}

// Height of pressure-level fields from their geopotential (vertical.py:330-345, 472-501, 1593-1601), the coordinate of
// interpolate_pressure_to_height_levels: one workgroup per (tile, level), z [nlev, npts] streamed once, zs [npts]
// re-read from L2.  mode as in the geopotential chain: 2 geometric above sea, 3 geopotential height above sea,
// 4 geometric above ground, 5 geopotential height above ground.
template <class T>
__global__ __launch_bounds__(kThreads) void height_rows(const T* __restrict__ z, const T* __restrict__ zs,
                                                       unsigned long long npts, int mode, T* __restrict__ out, int vec_ok) {
  constexpr int V = VecOf<T>::N;
  typedef typename VecOf<T>::type Vec;
  const unsigned long long tile = (unsigned long long)blockIdx.z * gridDim.x + blockIdx.x;
  const unsigned long long i0 = (tile * kThreads + threadIdx.x) * V;
  if (i0 >= npts) return;
  const bool whole = vec_ok && (i0 + V <= npts);
  const bool ground = mode == 4 || mode == 5;
  const unsigned long long row = (unsigned long long)blockIdx.y * npts + i0;
  Vec zv, sv, o;
#pragma unroll
  for (int j = 0; j < V; ++j) zv[j] = sv[j] = o[j] = T(0);
  if (whole) {
    zv = ld_stream<T>(z + row);
    if (ground) sv = ld_cached<T>(zs + i0);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (i0 + j < npts) {
        zv[j] = z[row + j];
        if (ground) sv[j] = zs[i0 + j];
      }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) o[j] = height_from_geopotential(zv[j], sv[j], mode);
  if (whole) {
    st_stream<T>(out + row, o);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j)
      if (i0 + j < npts) out[row + j] = o[j];
  }
}

template <class T>
static int launch_height(int dev, void* stream, const T* z, const T* zs, size_t npts, uint32_t nlev, int mode, T* out) {
  if (npts == 0 || nlev == 0) return EKM_OK;
  if (mode < 2 || mode > 5) return set_error(EKM_ERR_ENUM, "height_from_geopotential: mode=%d", mode);
  if (!z || !out || ((mode == 4 || mode == 5) && !zs)) return set_error(EKM_ERR_ARG, "height_from_geopotential: null pointer");
  if (nlev > 65535u) return set_error(EKM_ERR_ARG, "height_from_geopotential: at most 65535 levels (got %u)", nlev);
  int rc = check_aligned_if_given("height_from_geopotential", sizeof(T), {z, zs, out});
  if (rc == EKM_OK) rc = use_device(dev);
  constexpr int V = VecOf<T>::N;
  unsigned grid;
  if (rc == EKM_OK) rc = launch_grid("height_from_geopotential", npts, kThreads * V, &grid);
  if (rc != EKM_OK) return rc;
  unsigned long long band = (unsigned long long)tuning_hybrid_band_bytes() / ((unsigned long long)kThreads * V * sizeof(T));
  if (band < 8) band = 8;
  if (band > grid) band = grid;
  while ((grid + band - 1) / band > 65535ull) band *= 2;
  hipLaunchKernelGGL((height_rows<T>), dim3((unsigned)band, nlev, (unsigned)((grid + band - 1) / band)), dim3(kThreads), 0,
                     static_cast<hipStream_t>(stream), z, zs, (unsigned long long)npts, mode, out, (int)(npts % V == 0));
  return launched("height_from_geopotential");
}

template <class T>
static int interp_generic(int dev, void* stream, const T* data, const T* coord, int coord_is_field, const T* target,
                          int target_is_field, uint32_t ntarget, size_t npts, uint32_t nlev, int descending, int mode,
                          const T* aux_min_data, const T* aux_min_coord, const T* aux_max_data, const T* aux_max_coord,
                          uint32_t aux_field_mask, T* out) {
  InterpArgs<T> a = {};
  a.data = data;
  a.coord = coord;
  a.target = target;
  a.aux[0] = aux_min_data, a.aux[1] = aux_min_coord, a.aux[2] = aux_max_data, a.aux[3] = aux_max_coord;
  a.out = out;
  a.npts = npts;
  a.coord_stride = coord_is_field ? npts : 0;
  a.nlev = nlev;
  a.target_is_field = target_is_field != 0;
  a.aux_field = (int)(aux_field_mask & 15u);
  a.descending = descending != 0;
  a.mode = mode;
  return launch_interp<T, false>(dev, stream, a, ntarget, "interpolate_monotonic");
}

template <class T>
static int interp_hybrid(int dev, void* stream, const T* data, const T* A, const T* B, const T* sp, const T* target,
                         int target_is_field, uint32_t ntarget, size_t npts, uint32_t nfull, int descending, int mode,
                         const T* aux_min_data, const T* aux_min_coord, const T* aux_max_data, const T* aux_max_coord,
                         uint32_t aux_field_mask, T* out) {
  InterpArgs<T> a = {};
  a.data = data;
  a.A = A, a.B = B, a.sp = sp;
  a.target = target;
  a.aux[0] = aux_min_data, a.aux[1] = aux_min_coord, a.aux[2] = aux_max_data, a.aux[3] = aux_max_coord;
  a.out = out;
  a.npts = npts;
  a.nlev = nfull;
  a.target_is_field = target_is_field != 0;
  a.aux_field = (int)(aux_field_mask & 15u);
  a.descending = descending != 0;
  a.mode = mode;
  return launch_interp<T, true>(dev, stream, a, ntarget, "interpolate_hybrid_to_pressure_levels");
}

}  // namespace ekm

extern "C" {

int ekm_interpolate_monotonic_f32(int dev, void* stream, const float* data, const float* coord, int coord_is_field,
                                  const float* target, int target_is_field, uint32_t ntarget, size_t npts,
                                  uint32_t nlev, int descending, int mode, const float* aux_min_data,
                                  const float* aux_min_coord, const float* aux_max_data, const float* aux_max_coord,
                                  uint32_t aux_field_mask, float* out) {
  return ekm::interp_generic<float>(dev, stream, data, coord, coord_is_field, target, target_is_field, ntarget, npts,
                                    nlev, descending, mode, aux_min_data, aux_min_coord, aux_max_data, aux_max_coord,
                                    aux_field_mask, out);
}

int ekm_interpolate_monotonic_f64(int dev, void* stream, const double* data, const double* coord, int coord_is_field,
                                  const double* target, int target_is_field, uint32_t ntarget, size_t npts,
                                  uint32_t nlev, int descending, int mode, const double* aux_min_data,
                                  const double* aux_min_coord, const double* aux_max_data, const double* aux_max_coord,
                                  uint32_t aux_field_mask, double* out) {
  return ekm::interp_generic<double>(dev, stream, data, coord, coord_is_field, target, target_is_field, ntarget, npts,
                                     nlev, descending, mode, aux_min_data, aux_min_coord, aux_max_data, aux_max_coord,
                                     aux_field_mask, out);
}

int ekm_interpolate_hybrid_to_pressure_f32(int dev, void* stream, const float* data, const float* A, const float* B,
                                           const float* sp, const float* target, int target_is_field,
                                           uint32_t ntarget, size_t npts, uint32_t nfull, int descending, int mode,
                                           const float* aux_min_data, const float* aux_min_coord,
                                           const float* aux_max_data, const float* aux_max_coord,
                                           uint32_t aux_field_mask, float* out) {
  return ekm::interp_hybrid<float>(dev, stream, data, A, B, sp, target, target_is_field, ntarget, npts, nfull,
                                   descending, mode, aux_min_data, aux_min_coord, aux_max_data, aux_max_coord,
                                   aux_field_mask, out);
}

int ekm_interpolate_hybrid_to_pressure_f64(int dev, void* stream, const double* data, const double* A, const double* B,
                                           const double* sp, const double* target, int target_is_field,
                                           uint32_t ntarget, size_t npts, uint32_t nfull, int descending, int mode,
                                           const double* aux_min_data, const double* aux_min_coord,
                                           const double* aux_max_data, const double* aux_max_coord,
                                           uint32_t aux_field_mask, double* out) {
  return ekm::interp_hybrid<double>(dev, stream, data, A, B, sp, target, target_is_field, ntarget, npts, nfull,
                                    descending, mode, aux_min_data, aux_min_coord, aux_max_data, aux_max_coord,
                                    aux_field_mask, out);
}

int ekm_height_from_geopotential_f32(int dev, void* stream, const float* z, const float* zs, size_t npts, uint32_t nlev,
                                     int mode, float* out) {
  return ekm::launch_height<float>(dev, stream, z, zs, npts, nlev, mode, out);
}

int ekm_height_from_geopotential_f64(int dev, void* stream, const double* z, const double* zs, size_t npts, uint32_t nlev,
                                     int mode, double* out) {
  return ekm::launch_height<double>(dev, stream, z, zs, npts, nlev, mode, out);
}

}  // extern "C"
