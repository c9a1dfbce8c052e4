// Host twin of the kernels' per-point math -- TEST INFRASTRUCTURE ONLY.
//
// Compiles ops.hpp / thermo_math.hpp with g++ so the exact formulas the gfx950
// kernels run can be checked against the golden vectors in a container without
// a GPU.  The product (ekm_hip) never loads this library and has no CPU path.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ensemble_point.hpp"
#include "interp_point.hpp"
#include "ops.hpp"
#include "point_operand.hpp"
#include "reduce_point.hpp"
#include "solar_point.hpp"
#include "wind_point.hpp"

// Ops that keep a per-workgroup LDS table on the device (ops.hpp::OpTable, the bisection lattice) take the SAME path
// here -- table filled once, OpTable<Op>::apply per point -- so the table arithmetic the kernels run is what the golden
// vectors check.  EKM_TWIN_TABLE_FREE=1 selects Op::apply, the table-free statement of the same search;
// EKM_TWIN_BISECT_EXACT=1 makes every step of the tree walk take the reference's own residual (the kernels' tuning
// parameter bisect_exact), against which tests/test_hosttwin_fuzz.py compares the default walk bit for bit.
template <class Op, class T>
static int host_map(const T* const* ins, T* const* outs, size_t n, double rp) {
  std::vector<T> tab;
  bool all_exact = false;
  if constexpr (ekm::OpTable<Op>::elems > 0) {
    const char* ex = std::getenv("EKM_TWIN_BISECT_EXACT");
    all_exact = ex && ex[0] == '1';
    const char* env = std::getenv("EKM_TWIN_TABLE_FREE");
    if (!(env && env[0] == '1')) {
      tab.resize(ekm::OpTable<Op>::template count<T>());
      ekm::OpTable<Op>::template fill<T>(tab.data(), 0, 1);
    }
  }
  // fp64: the kernels' two passes (map_kernel.hpp::apply_points) -- fdouble first, whose primitives poison to NaN where
  // the plain ones apply an IEEE special-operand fix-up, then plain double for a point with a non-finite output.
  // EKM_TWIN_PLAIN_F64=1 skips the first pass.
  const char* plain = std::getenv("EKM_TWIN_PLAIN_F64");  // read per call: tests compare the two in one process
  const bool two_pass = !(plain && plain[0] == '1');
  (void)all_exact;
  for (size_t i = 0; i < n; ++i) {
    T x[Op::NIN], y[Op::NOUT];
    for (int k = 0; k < Op::NIN; ++k) x[k] = ins[k][i];
    if constexpr (sizeof(T) == 8) {
      if (two_pass) {
        ekm::fdouble xf[Op::NIN], yf[Op::NOUT];
        for (int k = 0; k < Op::NIN; ++k) xf[k] = ekm::fdouble(x[k]);
        if constexpr (ekm::OpTable<Op>::elems > 0) {
          if (!tab.empty())
            ekm::OpTable<Op>::template apply<ekm::fdouble>(xf, yf, ekm::fdouble(rp), reinterpret_cast<const ekm::fdouble*>(tab.data()), all_exact);
          else
            Op::template apply<ekm::fdouble>(xf, yf, ekm::fdouble(rp));
        } else {
          Op::template apply<ekm::fdouble>(xf, yf, ekm::fdouble(rp));
        }
        double yv[Op::NOUT];
        for (int k = 0; k < Op::NOUT; ++k) yv[k] = yf[k].v;
        if (!ekm::two_pass_redo_needed<Op>(x, yv)) {  // every output finite, or non-finite because an input it depends on is NaN
          for (int k = 0; k < Op::NOUT; ++k) outs[k][i] = yf[k].v;
          continue;
        }
      }
    }
    if constexpr (ekm::OpTable<Op>::elems > 0) {
      if (!tab.empty())
        ekm::OpTable<Op>::template apply<T>(x, y, T(rp), tab.data(), all_exact);
      else
        Op::template apply<T>(x, y, T(rp));
    } else {
      Op::template apply<T>(x, y, T(rp));
    }
    for (int k = 0; k < Op::NOUT; ++k) outs[k][i] = y[k];
  }
  return 0;
}

static int host_bad_enum(const char*, ...) { return -3; }

#include "gen/host_entries.inc"

// ---- vertical interpolation: the column routine of interp.hip (interp_point.hpp) on the CPU, same arguments as the
// ekm_interpolate_* entry points of include/ekm_thermo.h without dev / stream ----
template <class T, bool FUSED>
static int host_interp(const T* data, const T* coord, int coord_is_field, const T* A, const T* B, const T* sp,
                       const T* target, int target_is_field, unsigned ntarget, size_t npts, unsigned nlev, int descending,
                       int mode, const T* const (&aux)[4], unsigned aux_field_mask, T* out) {
  if (nlev < 2 || mode < 0 || mode > 2) return -2;
  for (unsigned t = 0; t < ntarget; ++t) {
    for (size_t i = 0; i < npts; ++i) {
      const T tc = target_is_field ? target[(size_t)t * npts + i] : target[t];
      auto coord_of = [&](unsigned m) -> T {
        if (FUSED) return ekm::hybrid_p_full(A[m], B[m], A[m + 1], B[m + 1], sp[i]);
        return coord_is_field ? coord[(size_t)m * npts + i] : coord[m];
      };
      auto data_of = [&](unsigned m) -> T { return data[(size_t)m * npts + i]; };
      ekm::InterpAux<T> lay[2];
      for (int e = 0; e < 2; ++e) {
        lay[e].on = aux[2 * e] && aux[2 * e + 1];
        lay[e].data = lay[e].coord = T(0);
        if (lay[e].on) {
          lay[e].data = aux[2 * e][(aux_field_mask >> (2 * e)) & 1 ? i : 0];
          lay[e].coord = aux[2 * e + 1][(aux_field_mask >> (2 * e + 1)) & 1 ? i : 0];
        }
      }
      const unsigned idx = ekm::interp_bracket<T>(nlev, descending, tc, coord_of);
      out[(size_t)t * npts + i] = ekm::interp_value<T>(idx, nlev, descending, mode, tc, coord_of, data_of, lay[1], lay[0]);
    }
  }
  return 0;
}

#define EKM_HOST_INTERP(tag, T)                                                                                      \
  extern "C" int ekm_host_interpolate_monotonic_##tag(                                                               \
      const T* data, const T* coord, int coord_is_field, const T* target, int target_is_field, unsigned ntarget,     \
      size_t npts, unsigned nlev, int descending, int mode, const T* aux_min_data, const T* aux_min_coord,           \
      const T* aux_max_data, const T* aux_max_coord, unsigned aux_field_mask, T* out) {                              \
    const T* const aux[4] = {aux_min_data, aux_min_coord, aux_max_data, aux_max_coord};                              \
    return host_interp<T, false>(data, coord, coord_is_field, nullptr, nullptr, nullptr, target, target_is_field,    \
                                 ntarget, npts, nlev, descending, mode, aux, aux_field_mask, out);                   \
  }                                                                                                                  \
  extern "C" int ekm_host_interpolate_hybrid_to_pressure_##tag(                                                      \
      const T* data, const T* A, const T* B, const T* sp, const T* target, int target_is_field, unsigned ntarget,    \
      size_t npts, unsigned nfull, int descending, int mode, const T* aux_min_data, const T* aux_min_coord,          \
      const T* aux_max_data, const T* aux_max_coord, unsigned aux_field_mask, T* out) {                              \
    const T* const aux[4] = {aux_min_data, aux_min_coord, aux_max_data, aux_max_coord};                              \
    return host_interp<T, true>(data, nullptr, 0, A, B, sp, target, target_is_field, ntarget, npts, nfull,           \
                                descending, mode, aux, aux_field_mask, out);                                         \
  }
#define EKM_HOST_HEIGHT(tag, T)                                                                                      \
  extern "C" int ekm_host_height_from_geopotential_##tag(const T* z, const T* zs, size_t npts, unsigned nlev, int mode, \
                                                         T* out) {                                                   \
    if (mode < 2 || mode > 5) return -3;                                                                             \
    for (unsigned k = 0; k < nlev; ++k)                                                                              \
      for (size_t i = 0; i < npts; ++i)                                                                              \
        out[k * npts + i] = ekm::height_from_geopotential<T>(z[k * npts + i], mode >= 4 ? zs[i] : T(0), mode);       \
    return 0;                                                                                                        \
  }
EKM_HOST_HEIGHT(f32, float)
EKM_HOST_HEIGHT(f64, double)
#undef EKM_HOST_HEIGHT
EKM_HOST_INTERP(f32, float)
EKM_HOST_INTERP(f64, double)
#undef EKM_HOST_INTERP

// ---- ensemble reductions: the per-point routines of ensemble.hip (ensemble_point.hpp) on the CPU, same arguments as
// the ekm_efi_* / ekm_sot_* / ekm_sot_func_* / ekm_crps_from_ensemble_* entry points without dev / stream ----
// A point's column on the host: a plain array
template <class T>
using HostColumn = ekm::Column<T, 1>;

#define EKM_HOST_ENSEMBLE(tag, T)                                                                                    \
  extern "C" int ekm_host_efi_##tag(const T* clim, const T* ens, unsigned nclim, unsigned nens, size_t npts,         \
                                    double eps, const double* acosdiff, const double* proddiff, const double* acoef, \
                                    double* out) {                                                                   \
    if (nclim < 1 || nens < 1) return -2;                                                                            \
    std::vector<T> col(nens);                                                                                        \
    for (size_t p = 0; p < npts; ++p)                                                                                \
      ekm::efi_body<T>(clim, ens, nclim, nens, npts, p, eps, acosdiff, proddiff, acoef, HostColumn<T>{col.data()}, out); \
    return 0;                                                                                                        \
  }                                                                                                                  \
  extern "C" int ekm_host_sot_##tag(const T* qc, const T* qc_tail, const T* ens, unsigned nens, size_t npts,         \
                                    int perc, double eps, T* out) {                                                  \
    if (nens < 1 || perc < 2 || perc > 98 || perc == 50) return -2;                                                  \
    std::vector<T> col(nens);                                                                                        \
    const ekm::Percentile<T> pos = ekm::percentile_position<T>(nens, perc);                                          \
    for (size_t p = 0; p < npts; ++p)                                                                                \
      ekm::sot_body<T>(qc, qc_tail, ens, nens, npts, p, pos, eps, HostColumn<T>{col.data()}, out);                   \
    return 0;                                                                                                        \
  }                                                                                                                  \
  extern "C" int ekm_host_sot_func_##tag(const T* qc_tail, const T* qc, const T* qf, size_t n, double eps,           \
                                         double lower_bound, double upper_bound, T* out) {                           \
    for (size_t p = 0; p < n; ++p)                                                                                   \
      out[p] = ekm::sot_func_point<T>(qc_tail[p], qc[p], qf[p], T(eps > 0.0 ? eps : 0.0), T(lower_bound),            \
                                      T(upper_bound));                                                               \
    return 0;                                                                                                        \
  }                                                                                                                  \
  extern "C" int ekm_host_crps_from_ensemble_##tag(const T* x, const T* y, unsigned nens, size_t npts,               \
                                                   const double* p2, const double* q2, double* out,                  \
                                                   unsigned char* missing) {                                         \
    if (nens < 1) return -2;                                                                                         \
    std::vector<T> col(nens);                                                                                        \
    for (size_t p = 0; p < npts; ++p)                                                                                \
      ekm::crps_body<T>(x, y, nens, npts, p, p2, q2, HostColumn<T>{col.data()}, out, missing);                       \
    return 0;                                                                                                        \
  }
EKM_HOST_ENSEMBLE(f32, float)
EKM_HOST_ENSEMBLE(f64, double)
#undef EKM_HOST_ENSEMBLE

// ---- cpf: cpf_value of ensemble_point.hpp on the CPU, same arguments as ekm_cpf_* without dev / stream ----
template <class T>
static int host_cpf(const T* clim, const T* ens, unsigned nclim, unsigned nens, size_t npts, int sort_clim, int sort_ens,
                    int from_zero, int symmetric, int use_epsilon, double epsilon, float* out) {
  if (nclim < 1 || nens < 1) return -2;
  std::vector<T> ccol(nclim), ecol(nens);
  const HostColumn<T> cc{ccol.data()}, ec{ecol.data()};
  for (size_t p = 0; p < npts; ++p) {  // (cpf_points keeps a body of its own: this is its restatement)
    if (sort_clim) ekm::stage_column<T, ekm::ColumnOrder::NanLast>(clim + p, npts, nclim, cc);
    else ekm::stage_column<T, ekm::ColumnOrder::AsGiven>(clim + p, npts, nclim, cc);
    if (sort_ens) ekm::stage_column<T, ekm::ColumnOrder::NanLast>(ens + p, npts, nens, ec);
    else ekm::stage_column<T, ekm::ColumnOrder::AsGiven>(ens + p, npts, nens, ec);
    out[p] = ekm::cpf_value<T>(nclim, nens, from_zero != 0, symmetric != 0, use_epsilon != 0, T(epsilon), cc, ec);
  }
  return 0;
}
#define EKM_HOST_CPF(tag, T)                                                                                         \
  extern "C" int ekm_host_cpf_##tag(const T* clim, const T* ens, unsigned nclim, unsigned nens, size_t npts,         \
                                    int sort_clim, int sort_ens, int from_zero, int symmetric, int use_epsilon,      \
                                    double epsilon, float* out) {                                                    \
    return host_cpf<T>(clim, ens, nclim, nens, npts, sort_clim, sort_ens, from_zero, symmetric, use_epsilon, epsilon, \
                       out);                                                                                         \
  }
EKM_HOST_CPF(f32, float)
EKM_HOST_CPF(f64, double)
#undef EKM_HOST_CPF

// ---- solar: solar_point of solar_point.hpp on the CPU, the operands described as for ekm_solar_* (mode, len, inner) ----
template <class T, class Out>
static int host_solar(const T* lat, int lat_mode, unsigned long long lat_len, unsigned long long lat_inner, const T* lon,
                      int lon_mode, unsigned long long lon_len, unsigned long long lon_inner, const double* nodes,
                      unsigned nnodes, Out* out, size_t n) {
  const ekm::PointOperand<T> la{lat, lat_mode, lat_len ? lat_len : 1, lat_inner ? lat_inner : 1};
  const ekm::PointOperand<T> lo{lon, lon_mode, lon_len ? lon_len : 1, lon_inner ? lon_inner : 1};
  for (size_t p = 0; p < n; ++p)
    out[p] = ekm::solar_point<Out>(ekm::point_fetch<T>(la, p, false), ekm::point_fetch<T>(lo, p, false), nnodes,
                                   [&](unsigned k, int j) { return nodes[(size_t)k * ekm::kSolarRecord + j]; });
  return 0;
}
#define EKM_HOST_SOLAR(tag, T, Out)                                                                                      \
  extern "C" int ekm_host_solar_##tag(const T* lat, int lat_mode, unsigned long long lat_len, unsigned long long lat_inner, \
                                      const T* lon, int lon_mode, unsigned long long lon_len, unsigned long long lon_inner, \
                                      const double* nodes, unsigned nnodes, Out* out, size_t n) {                        \
    return host_solar<T, Out>(lat, lat_mode, lat_len, lat_inner, lon, lon_mode, lon_len, lon_inner, nodes, nnodes, out, n); \
  }
EKM_HOST_SOLAR(f32, float, float)
EKM_HOST_SOLAR(f64, double, double)
EKM_HOST_SOLAR(f32_f64, float, double)
#undef EKM_HOST_SOLAR
// (for the tests of the sine / cosine themselves)
extern "C" void ekm_host_sincos_deg(const double* x, double* s, double* c, size_t n) {
  for (size_t i = 0; i < n; ++i) ekm::sol_sincos_deg(x[i], s[i], c[i]);
}

// ---- quantiles: quantile_point of ensemble_point.hpp on the CPU, same arguments as ekm_quantiles_* without dev / stream ----
template <class T, class Out>
static int host_quantiles(const T* arr, size_t outer, unsigned m, size_t inner, const double* lo, const double* hi,
                          const double* w, unsigned nq, int mode, Out* out) {
  if (outer == 0 || inner == 0 || nq == 0) return 0;
  if (mode != ekm::kQuantileSort && mode != ekm::kQuantileLerp) return -3;
  if (m < 1 || (mode == ekm::kQuantileSort && sizeof(Out) != sizeof(double))) return -2;
  const size_t npts = outer * inner;
  std::vector<T> col(m);
  const HostColumn<T> c{col.data()};
  for (size_t p = 0; p < npts; ++p) {  // (quantile_points keeps a body of its own: this is its restatement)
    const bool has_nan = ekm::stage_column<T, ekm::ColumnOrder::Ascending>(ekm::sample_column<T>(arr, m, inner, p), inner, m, c);
    for (unsigned k = 0; k < nq; ++k)
      out[(size_t)k * npts + p] = ekm::quantile_point<T, Out>(has_nan, c, (unsigned)lo[k], (unsigned)hi[k], w[k], mode);
  }
  return 0;
}
#define EKM_HOST_QUANTILES(tag, T, Out)                                                                              \
  extern "C" int ekm_host_quantiles_##tag(const T* arr, size_t outer, unsigned m, size_t inner, const double* lo,    \
                                          const double* hi, const double* w, unsigned nq, int mode, Out* out) {      \
    return host_quantiles<T, Out>(arr, outer, m, inner, lo, hi, w, nq, mode, out);                                   \
  }
EKM_HOST_QUANTILES(f32, float, float)
EKM_HOST_QUANTILES(f64, double, double)
EKM_HOST_QUANTILES(f32_f64, float, double)
#undef EKM_HOST_QUANTILES

// ---- long-axis quantiles: std::sort on the keys long_quantile_tiles sorts (SortKey), then quantile_point; same arguments
// as ekm_long_quantiles_* without dev / stream.  The keys order -0.0 before +0.0, so the sorted column is the kernel's ----
template <class T, class Out>
static int host_long_quantiles(const T* arr, size_t outer, unsigned m, size_t inner, const double* lo, const double* hi,
                               const double* w, unsigned nq, int mode, Out* out) {
  using Key = ekm::SortKey<T>;
  if (outer == 0 || inner == 0 || nq == 0) return 0;
  if (mode != ekm::kQuantileSort && mode != ekm::kQuantileLerp) return -3;
  if (m < 1 || m > 65536 / sizeof(T) || (mode == ekm::kQuantileSort && sizeof(Out) != sizeof(double))) return -2;
  const size_t npts = outer * inner;
  std::vector<typename Key::type> keys(m);
  for (size_t p = 0; p < npts; ++p) {
    const T* col = ekm::sample_column<T>(arr, m, inner, p);
    bool has_nan = false;
    for (unsigned j = 0; j < m; ++j) {
      const T x = col[(size_t)j * inner];
      has_nan = has_nan || x != x;
      keys[j] = Key::of(x);
    }
    std::sort(keys.begin(), keys.end());
    auto s = [&](unsigned j) -> T { return Key::value(keys[j]); };
    for (unsigned k = 0; k < nq; ++k)
      out[(size_t)k * npts + p] = ekm::quantile_point<T, Out>(has_nan, s, (unsigned)lo[k], (unsigned)hi[k], w[k], mode);
  }
  return 0;
}
#define EKM_HOST_LONG_QUANTILES(tag, T, Out)                                                                            \
  extern "C" int ekm_host_long_quantiles_##tag(const T* arr, size_t outer, unsigned m, size_t inner, const double* lo,  \
                                               const double* hi, const double* w, unsigned nq, int mode, Out* out) {    \
    return host_long_quantiles<T, Out>(arr, outer, m, inner, lo, hi, w, nq, mode, out);                                 \
  }
EKM_HOST_LONG_QUANTILES(f32, float, float)
EKM_HOST_LONG_QUANTILES(f64, double, double)
EKM_HOST_LONG_QUANTILES(f32_f64, float, double)
#undef EKM_HOST_LONG_QUANTILES
// (for the tests of the keys themselves: the sorted column as values)
extern "C" void ekm_host_sort_by_key_f32(float* x, size_t n) {
  std::sort(x, x + n, [](float a, float b) { return ekm::SortKey<float>::of(a) < ekm::SortKey<float>::of(b); });
}
extern "C" void ekm_host_sort_by_key_f64(double* x, size_t n) {
  std::sort(x, x + n, [](double a, double b) { return ekm::SortKey<double>::of(a) < ekm::SortKey<double>::of(b); });
}

// ---- long-axis reductions: std::sort on the keys the tiles of long_ensemble.hip sort, then the *_point call of the kernel's
// read-out; same arguments as ekm_long_efi_* / ekm_long_sot_* / ekm_long_crps_from_ensemble_* / ekm_long_gumbel_fit_* without
// dev / stream.  base: the column's first value, `stride` apart; f: the transform of a value before it is keyed ----
template <class T, class F>
static bool host_sorted_keys(const T* base, size_t stride, unsigned m, std::vector<typename ekm::SortKey<T>::type>& keys, F f) {
  bool has_nan = false;
  for (unsigned j = 0; j < m; ++j) {
    const T x = f(base[(size_t)j * stride]);
    has_nan = has_nan || x != x;
    keys[j] = ekm::SortKey<T>::of(x);
  }
  std::sort(keys.begin(), keys.end());
  return has_nan;
}
template <class T>
static bool host_long_axis_ok(unsigned m, unsigned least) { return m >= least && m <= 65536 / sizeof(T); }

#define EKM_HOST_LONG_ENSEMBLE(tag, T)                                                                                  \
  extern "C" int ekm_host_long_efi_##tag(const T* clim, const T* ens, unsigned nclim, unsigned nens, size_t npts,       \
                                         double eps, const double* acosdiff, const double* proddiff,                    \
                                         const double* acoef, double* out) {                                            \
    using Key = ekm::SortKey<T>;                                                                                        \
    if (nclim < 1 || !host_long_axis_ok<T>(nens, 1)) return -2;                                                         \
    std::vector<Key::type> keys(nens);                                                                                  \
    for (size_t p = 0; p < npts; ++p) {                                                                                 \
      const bool has_nan = host_sorted_keys<T>(ens + p, npts, nens, keys, [](T x) -> T { return x; });                  \
      out[p] = ekm::efi_point<T>(                                                                                       \
          nclim, nens, has_nan, [&](unsigned i) -> T { return clim[(size_t)i * npts + p]; },                            \
          [&](unsigned j) -> T { return Key::value(keys[j]); }, acosdiff, proddiff, acoef, eps);                        \
    }                                                                                                                   \
    return 0;                                                                                                           \
  }                                                                                                                     \
  extern "C" int ekm_host_long_sot_##tag(const T* qc, const T* qc_tail, const T* ens, unsigned nens, size_t npts,       \
                                         int perc, double eps, T* out) {                                                \
    using Key = ekm::SortKey<T>;                                                                                        \
    if (!host_long_axis_ok<T>(nens, 1) || perc < 2 || perc > 98 || perc == 50) return -2;                               \
    std::vector<Key::type> keys(nens);                                                                                  \
    const ekm::Percentile<T> pos = ekm::percentile_position<T>(nens, perc);                                             \
    const bool zero_below = eps > 0.0;                                                                                  \
    const T teps = T(eps);                                                                                              \
    for (size_t p = 0; p < npts; ++p) {                                                                                 \
      const bool has_nan =                                                                                              \
          host_sorted_keys<T>(ens + p, npts, nens, keys, [&](T x) -> T { return zero_below && x < teps ? T(0) : x; });  \
      out[p] = ekm::sot_point<T>(qc[p], qc_tail[p], has_nan, [&](unsigned j) -> T { return Key::value(keys[j]); }, pos, \
                                 eps);                                                                                  \
    }                                                                                                                   \
    return 0;                                                                                                           \
  }                                                                                                                     \
  extern "C" int ekm_host_long_crps_from_ensemble_##tag(const T* x, const T* y, unsigned nens, size_t npts,             \
                                                        const double* p2, const double* q2, double* out,                \
                                                        unsigned char* missing) {                                       \
    using Key = ekm::SortKey<T>;                                                                                        \
    if (!host_long_axis_ok<T>(nens, 1)) return -2;                                                                      \
    std::vector<Key::type> keys(nens);                                                                                  \
    for (size_t p = 0; p < npts; ++p) {                                                                                 \
      const bool has_nan = host_sorted_keys<T>(x + p, npts, nens, keys, [](T v) -> T { return v; });                    \
      const T yp = y[p];                                                                                                \
      const bool miss = has_nan || yp != yp;                                                                            \
      const double r = ekm::crps_point<T>(nens, yp, [&](unsigned j) -> T { return Key::value(keys[j]); }, p2, q2);      \
      out[p] = miss ? ekm::nan_v<double>() : r;                                                                         \
      if (missing) missing[p] = miss ? 1 : 0;                                                                           \
    }                                                                                                                   \
    return 0;                                                                                                           \
  }                                                                                                                     \
  extern "C" int ekm_host_long_gumbel_fit_##tag(const T* sample, size_t outer, unsigned m, size_t inner, double* mu,    \
                                                double* sigma) {                                                        \
    using Key = ekm::SortKey<T>;                                                                                        \
    if (outer == 0 || inner == 0) return 0;                                                                             \
    if (!host_long_axis_ok<T>(m, 2)) return -2;                                                                         \
    std::vector<Key::type> keys(m);                                                                                     \
    for (size_t p = 0; p < outer * inner; ++p) {                                                                        \
      const bool has_nan =                                                                                              \
          host_sorted_keys<T>(ekm::sample_column<T>(sample, m, inner, p), inner, m, keys, [](T x) -> T { return x; });  \
      ekm::gumbel_fit_point<T>(m, has_nan, [&](unsigned j) -> T { return Key::value(keys[j]); }, mu[p], sigma[p]);      \
    }                                                                                                                   \
    return 0;                                                                                                           \
  }
EKM_HOST_LONG_ENSEMBLE(f32, float)
EKM_HOST_LONG_ENSEMBLE(f64, double)
#undef EKM_HOST_LONG_ENSEMBLE

// ---- long cpf: the two columns as the keys long_cpf_tiles holds (std::sort where the flag asks for it, the given order
// otherwise), then cpf_value_running; same arguments as ekm_long_cpf_* without dev / stream ----
template <class T>
static int host_long_cpf(const T* clim, const T* ens, unsigned nclim, unsigned nens, size_t npts, int sort_clim,
                         int sort_ens, int from_zero, int symmetric, int use_epsilon, double epsilon, float* out) {
  using Key = ekm::SortKey<T>;
  if (!host_long_axis_ok<T>(nclim, 1) || !host_long_axis_ok<T>(nens, 1)) return -2;
  std::vector<typename Key::type> ckeys(nclim), ekeys(nens);
  auto keys_of = [&](const T* base, unsigned m, std::vector<typename Key::type>& keys, int sorted) {
    for (unsigned j = 0; j < m; ++j) keys[j] = Key::of(base[(size_t)j * npts]);
    if (sorted) std::sort(keys.begin(), keys.end());
  };
  for (size_t p = 0; p < npts; ++p) {
    keys_of(clim + p, nclim, ckeys, sort_clim);
    keys_of(ens + p, nens, ekeys, sort_ens);
    out[p] = ekm::cpf_value_running<T>(
        nclim, nens, from_zero != 0, symmetric != 0, use_epsilon != 0, T(epsilon),
        [&](unsigned i) -> T { return Key::value(ckeys[i]); }, [&](unsigned j) -> T { return Key::value(ekeys[j]); });
  }
  return 0;
}
#define EKM_HOST_LONG_CPF(tag, T)                                                                                         \
  extern "C" int ekm_host_long_cpf_##tag(const T* clim, const T* ens, unsigned nclim, unsigned nens, size_t npts,         \
                                         int sort_clim, int sort_ens, int from_zero, int symmetric, int use_epsilon,      \
                                         double epsilon, float* out) {                                                    \
    return host_long_cpf<T>(clim, ens, nclim, nens, npts, sort_clim, sort_ens, from_zero, symmetric, use_epsilon, epsilon, \
                            out);                                                                                         \
  }
EKM_HOST_LONG_CPF(f32, float)
EKM_HOST_LONG_CPF(f64, double)
#undef EKM_HOST_LONG_CPF

// ---- Gumbel fit, cdf and ppf: gumbel_*_point of ensemble_point.hpp on the CPU, same arguments as ekm_gumbel_* without
// dev / stream (the exponentials are this host's libm, the device library's on the GPU) ----
template <class T>
static int host_gumbel_fit(const T* sample, size_t outer, unsigned m, size_t inner, double* mu, double* sigma) {
  if (outer == 0 || inner == 0) return 0;
  if (m < 2) return -2;
  std::vector<T> col(m);
  for (size_t p = 0; p < outer * inner; ++p)
    ekm::gumbel_fit_body<T>(sample, m, inner, p, HostColumn<T>{col.data()}, mu, sigma);
  return 0;
}
extern "C" int ekm_host_gumbel_fit_f32(const float* sample, size_t outer, unsigned m, size_t inner, double* mu, double* sigma) {
  return host_gumbel_fit<float>(sample, outer, m, inner, mu, sigma);
}
extern "C" int ekm_host_gumbel_fit_f64(const double* sample, size_t outer, unsigned m, size_t inner, double* mu, double* sigma) {
  return host_gumbel_fit<double>(sample, outer, m, inner, mu, sigma);
}
extern "C" int ekm_host_gumbel_cdf_f64(const double* mu, const double* sigma, size_t npts, const double* x, unsigned nx,
                                       double freq, int mode, double* out) {
  if (mode != ekm::kGumbelCdf && mode != ekm::kGumbelReturnPeriod) return -3;
  for (unsigned k = 0; k < nx; ++k)
    for (size_t p = 0; p < npts; ++p) out[(size_t)k * npts + p] = ekm::gumbel_cdf_point(mu[p], sigma[p], x[k], freq, mode);
  return 0;
}
extern "C" int ekm_host_gumbel_ppf_f64(const double* mu, const double* sigma, size_t npts, const double* t, unsigned nt,
                                       double* out) {
  for (unsigned k = 0; k < nt; ++k)
    for (size_t p = 0; p < npts; ++p) out[(size_t)k * npts + p] = ekm::gumbel_ppf_point(mu[p], sigma[p], t[k]);
  return 0;
}

// ---- wind: wind_point of wind_point.hpp on the CPU, the operands described as for ekm_wind_* (mode, len, inner); a null
// output is not written ----
template <class T, int KIND, int MODE, int WHICH>
static void host_wind_as(const ekm::PointOperand<T>& a, const ekm::PointOperand<T>& b, T* out0, T* out1, size_t n) {
  for (size_t p = 0; p < n; ++p) {
    T o0, o1;
    ekm::wind_point<T, KIND, MODE, WHICH>((T)ekm::point_fetch<T>(a, p, false),
                                          KIND == ekm::WIND_KIND_CORIOLIS ? T(0) : (T)ekm::point_fetch<T>(b, p, false), o0, o1);
    if (out0) out0[p] = (T)o0;
    if (out1) out1[p] = (T)o1;
  }
}
template <class T>
static int host_wind(int kind, const T* a, int a_mode, unsigned long long a_len, unsigned long long a_inner, const T* b, int b_mode,
                     unsigned long long b_len, unsigned long long b_inner, int mode, T* out0, T* out1, size_t n) {
  const ekm::PointOperand<T> oa{a, a_mode, a_len ? a_len : 1, a_inner ? a_inner : 1};
  const ekm::PointOperand<T> ob{b ? b : a, b ? b_mode : a_mode, b_len ? b_len : 1, b_inner ? b_inner : 1};
  using namespace ekm;
  if (kind == WIND_KIND_POLAR && mode == WIND_METEO) host_wind_as<T, WIND_KIND_POLAR, WIND_METEO, 3>(oa, ob, out0, out1, n);
  else if (kind == WIND_KIND_POLAR && mode == WIND_POLAR_POSITIVE) host_wind_as<T, WIND_KIND_POLAR, WIND_POLAR_POSITIVE, 3>(oa, ob, out0, out1, n);
  else if (kind == WIND_KIND_POLAR && mode == WIND_POLAR_SIGNED) host_wind_as<T, WIND_KIND_POLAR, WIND_POLAR_SIGNED, 3>(oa, ob, out0, out1, n);
  else if (kind == WIND_KIND_XY && mode == WIND_METEO) host_wind_as<T, WIND_KIND_XY, WIND_METEO, 3>(oa, ob, out0, out1, n);
  else if (kind == WIND_KIND_XY && mode == WIND_POLAR_POSITIVE) host_wind_as<T, WIND_KIND_XY, WIND_POLAR_POSITIVE, 3>(oa, ob, out0, out1, n);
  else if (kind == WIND_KIND_CORIOLIS) host_wind_as<T, WIND_KIND_CORIOLIS, WIND_METEO, 1>(oa, ob, out0, out1, n);
  else return -1;
  return 0;
}
// the wind rose: the count and the finish of wind.hip, one sample after the other
template <class T>
static int host_windrose(const T* speed, const T* dir, size_t n, const double* edges, unsigned ns, unsigned nd, double inv_step,
                         int percent, double* out) {
  if (ns < 2 || nd < 3) return -1;
  const unsigned rows = ns - 1, cols = nd - 1;
  std::vector<unsigned long long> table((size_t)rows * cols, 0ull);
  const double* se = edges;
  const double* de = edges + ns;
  unsigned long long total = 0;
  for (size_t p = 0; p < n; ++p) {
    const int cell = ekm::wind_cell((double)speed[p], (double)dir[p], [&](unsigned k) { return se[k]; }, ns,
                                    [&](unsigned k) { return de[k]; }, nd, inv_step);
    if (cell >= 0) {
      table[(size_t)cell] += 1;
      total += 1;
    }
  }
  for (unsigned r = 0; r < rows; ++r)
    for (unsigned c = 0; c + 1 < cols; ++c)
      out[(size_t)r * (cols - 1) + c] =
          ekm::wind_rose_value(table[(size_t)r * cols + c] + (c == 0 ? table[(size_t)r * cols + cols - 1] : 0ull), total, percent);
  return 0;
}
#define EKM_HOST_WIND(tag, T)                                                                                                      \
  extern "C" int ekm_host_wind_##tag(int kind, const T* a, int a_mode, unsigned long long a_len, unsigned long long a_inner,       \
                                     const T* b, int b_mode, unsigned long long b_len, unsigned long long b_inner, int mode,       \
                                     T* out0, T* out1, size_t n) {                                                                 \
    return host_wind<T>(kind, a, a_mode, a_len, a_inner, b, b_mode, b_len, b_inner, mode, out0, out1, n);                          \
  }                                                                                                                                \
  extern "C" int ekm_host_windrose_##tag(const T* speed, const T* dir, size_t n, const double* edges, unsigned ns, unsigned nd,    \
                                         double inv_step, int percent, double* out) {                                              \
    return host_windrose<T>(speed, dir, n, edges, ns, nd, inv_step, percent, out);                                                 \
  }
EKM_HOST_WIND(f32, float)
EKM_HOST_WIND(f64, double)
#undef EKM_HOST_WIND
// (for the tests of the primitives themselves)
extern "C" void ekm_host_wind_primitives_f32(const float* y, const float* x, float* at, float* hy, float* sn, float* cs, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    at[i] = ekm::wind_atan2(y[i], x[i]);
    hy[i] = ekm::wind_hypot(x[i], y[i]);
    ekm::wind_sincos_deg(x[i], sn[i], cs[i]);
  }
}
extern "C" void ekm_host_atan2_hypot(const double* y, const double* x, double* at, double* hy, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    at[i] = ekm::wind_atan2(y[i], x[i]);
    hy[i] = ekm::wind_hypot(x[i], y[i]);
  }
}

// ---- the reduce family: project_partial / pearson_point / rows_partial_* of reduce_point.hpp on the CPU, same arguments
// as ekm_regimes_project_*, ekm_regimes_index_* and ekm_pearson_* without dev / stream.  The workgroup is a loop over
// its 256 lanes, a wave's butterfly is host_wave_tree over 64 of them: the order of every sum is the kernels' ----
template <class T, int NP>
static void host_project_group(const T* field, const T* coef, size_t k, size_t cstride, const T* scale, size_t nfields, T* out) {
  constexpr int kWaves = ekm::kProjThreads / ekm::kWaveLanes;
  for (size_t n = 0; n < nfields; ++n) {
    T lanes[NP][kWaves][ekm::kWaveLanes];
    for (unsigned t = 0; t < (unsigned)ekm::kProjThreads; ++t) {
      T acc[NP];
      ekm::project_partial<T, NP>(field + n * k, coef + n * cstride, k, t, acc);
      for (int p = 0; p < NP; ++p) lanes[p][t / ekm::kWaveLanes][t % ekm::kWaveLanes] = acc[p];
    }
    for (int p = 0; p < NP; ++p) {
      T part[kWaves];
      for (int w = 0; w < kWaves; ++w) part[w] = ekm::host_wave_tree<T>(lanes[p][w]);
      out[(size_t)p * nfields + n] = ekm::project_finish<T>(part, kWaves, scale != nullptr, scale ? scale[n] : T(0));
    }
  }
}
template <class T>
static int host_project(const T* field, size_t nfields, size_t k, const T* coef, unsigned npat, size_t cstride, const T* scale, T* out) {
  if (nfields == 0 || npat == 0) return 0;
  if (k < 1 || (cstride != 0 && cstride < (size_t)npat * k)) return -2;
  for (unsigned p0 = 0; p0 < npat; p0 += ekm::kProjGroup) {
    const T* c = coef + (size_t)p0 * k;
    T* o = out + (size_t)p0 * nfields;
    switch (npat - p0 < (unsigned)ekm::kProjGroup ? npat - p0 : (unsigned)ekm::kProjGroup) {
      case 1: host_project_group<T, 1>(field, c, k, cstride, scale, nfields, o); break;
      case 2: host_project_group<T, 2>(field, c, k, cstride, scale, nfields, o); break;
      case 3: host_project_group<T, 3>(field, c, k, cstride, scale, nfields, o); break;
      case 4: host_project_group<T, 4>(field, c, k, cstride, scale, nfields, o); break;
      case 5: host_project_group<T, 5>(field, c, k, cstride, scale, nfields, o); break;
      case 6: host_project_group<T, 6>(field, c, k, cstride, scale, nfields, o); break;
      case 7: host_project_group<T, 7>(field, c, k, cstride, scale, nfields, o); break;
      default: host_project_group<T, 8>(field, c, k, cstride, scale, nfields, o); break;
    }
  }
  return 0;
}
template <class T>
static int host_pearson(const T* x, const T* y, size_t outer, size_t m, size_t inner, T* out) {
  if (outer == 0 || inner == 0) return 0;
  if (m < 1) return -2;
  for (size_t p = 0; p < outer * inner; ++p) {
    if (inner != 1) {
      const size_t o = p / inner, base = o * m * inner + (p - o * inner);
      out[p] = ekm::pearson_point<T>(
          m, [&](size_t i) { return x[base + i * inner]; }, [&](size_t i) { return y[base + i * inner]; });
      continue;
    }
    const T *xr = x + p * m, *yr = y + p * m;
    T a[ekm::kWaveLanes], b[ekm::kWaveLanes];
    for (unsigned l = 0; l < (unsigned)ekm::kWaveLanes; ++l) a[l] = ekm::rows_partial_sum<T>(xr, m, l), b[l] = ekm::rows_partial_sum<T>(yr, m, l);
    const T mx = ekm::host_wave_tree<T>(a) / T(m), my = ekm::host_wave_tree<T>(b) / T(m);
    for (unsigned l = 0; l < (unsigned)ekm::kWaveLanes; ++l)
      a[l] = ekm::rows_partial_squares<T>(xr, m, l, mx), b[l] = ekm::rows_partial_squares<T>(yr, m, l, my);
    const T nx = std::sqrt(ekm::host_wave_tree<T>(a)), ny = std::sqrt(ekm::host_wave_tree<T>(b));
    for (unsigned l = 0; l < (unsigned)ekm::kWaveLanes; ++l) a[l] = ekm::rows_partial_products<T>(xr, yr, m, l, mx, my, nx, ny);
    out[p] = ekm::host_wave_tree<T>(a);
  }
  return 0;
}
// nanaverage: same arguments as ekm_nanaverage_* without dev / stream / work; `path` as there
template <class T, bool W>
static void host_nanavg_waves(const T* d, const T* w, size_t ws, size_t begin, size_t end, unsigned nthreads, T& s, ekm::nan_q_t<T, W>& q) {
  // the lanes' partial pairs, a butterfly per wave, the waves in wave order
  const unsigned nwaves = nthreads / ekm::kWaveLanes;
  for (unsigned v = 0; v < nwaves; ++v) {
    T ls[ekm::kWaveLanes];
    ekm::nan_q_t<T, W> lq[ekm::kWaveLanes], wq;
    for (unsigned l = 0; l < (unsigned)ekm::kWaveLanes; ++l)
      ekm::nanavg_partial<T, W>(d, w, ws, begin, end, v * ekm::kWaveLanes + l, nthreads, ls[l], lq[l]);
    const T wsum = ekm::host_wave_tree<T>(ls);
    if constexpr (W) {
      wq = ekm::host_wave_tree<T>(lq);
    } else {
      wq = 0;
      for (unsigned l = 0; l < (unsigned)ekm::kWaveLanes; ++l) wq += lq[l];
    }
    if (v == 0)
      s = wsum, q = wq;
    else
      ekm::nanavg_add<T, W>(s, q, wsum, wq);
  }
}
template <class T, bool W>
static int host_nanaverage_as(const T* data, size_t outer, size_t m, size_t inner, const T* w, size_t so, size_t sm, size_t si, int path,
                              T* out) {
  for (size_t p = 0; p < outer * inner; ++p) {
    const size_t o = p / inner, j = p - o * inner;
    if (path == ekm::kNanPoints) {
      const size_t base = o * m * inner + j;
      auto d = [&](size_t i) { return data[base + i * inner]; };
      if constexpr (W) {
        const T* wp = w + o * so + j * si;
        out[p] = ekm::nanavg_point_weighted<T>(m, d, [&](size_t i) { return wp[i * sm]; });
      } else {
        out[p] = ekm::nanavg_point<T>(m, d);
      }
      continue;
    }
    const T* row = data + p * m;
    const T* wrow = W ? w + p * so : nullptr;
    T s;
    ekm::nan_q_t<T, W> q;
    if (path == ekm::kNanRows) {
      host_nanavg_waves<T, W>(row, wrow, sm, 0, m, ekm::kWaveLanes, s, q);
      out[p] = ekm::nanavg_finish<T, W>(s, q);
      continue;
    }
    const size_t nchunks = ekm::nanavg_chunks(m);
    T* pairs = new T[2 * nchunks];
    for (size_t c = 0; c < nchunks; ++c) {
      const size_t begin = c * ekm::kNanSplitChunk, end = begin + ekm::kNanSplitChunk < m ? begin + ekm::kNanSplitChunk : m;
      host_nanavg_waves<T, W>(row, wrow, sm, begin, end, ekm::kNanSplitThreads, s, q);
      pairs[2 * c] = s, pairs[2 * c + 1] = (T)q;
    }
    out[p] = ekm::nanavg_split_total<T, W>(pairs, nchunks);
    delete[] pairs;
  }
  return 0;
}
template <class T>
static int host_nanaverage(const T* data, size_t outer, size_t m, size_t inner, const T* w, size_t so, size_t sm, size_t si, int path,
                           T* out) {
  if (path < ekm::kNanAuto || path > ekm::kNanSplit) return -3;
  if (outer == 0 || inner == 0) return 0;
  if (path >= ekm::kNanRows && inner != 1) return -2;
  if (path == ekm::kNanAuto) path = ekm::nanavg_path(outer, m, inner);
  return w ? host_nanaverage_as<T, true>(data, outer, m, inner, w, so, sm, si, path, out)
           : host_nanaverage_as<T, false>(data, outer, m, inner, nullptr, 0, 0, 0, path, out);
}
#define EKM_HOST_REDUCE(tag, T)                                                                                           \
  extern "C" int ekm_host_regimes_project_##tag(const T* field, size_t nfields, size_t k, const T* coef, unsigned npat,      \
                                                size_t coef_stride, const T* scale, T* out) {                                \
    return host_project<T>(field, nfields, k, coef, npat, coef_stride, scale, out);                                          \
  }                                                                                                                          \
  extern "C" int ekm_host_regimes_index_##tag(const T* proj, const T* mean, T mean_value, const T* sd, T sd_value, T* out,   \
                                                size_t n) {                                                                  \
    for (size_t i = 0; i < n; ++i) out[i] = ekm::standardise_point<T>(proj[i], mean ? mean[i] : mean_value, sd ? sd[i] : sd_value); \
    return 0;                                                                                                                \
  }                                                                                                                          \
  extern "C" int ekm_host_pearson_##tag(const T* x, const T* y, size_t outer, size_t m, size_t inner, T* out) {              \
    return host_pearson<T>(x, y, outer, m, inner, out);                                                                      \
  }                                                                                                                          \
  extern "C" int ekm_host_nanaverage_##tag(const T* data, size_t outer, size_t m, size_t inner, const T* weights,            \
                                           size_t wstride_outer, size_t wstride_m, size_t wstride_inner, int path, T* out) { \
    return host_nanaverage<T>(data, outer, m, inner, weights, wstride_outer, wstride_m, wstride_inner, path, out);           \
  }
EKM_HOST_REDUCE(f32, float)
EKM_HOST_REDUCE(f64, double)
#undef EKM_HOST_REDUCE
