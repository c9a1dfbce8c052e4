#!/usr/bin/env python3
"""Single source of truth for the C ABI of libekm_thermo.so.

Emits (all committed):
  include/ekm_thermo.h                          the public header
  earthkit-meteo_amd/csrc/gen/entries_<g>_<dtype>.hip   extern "C" definitions, one file per group and dtype
  earthkit-meteo_amd/csrc/gen/host_entries.inc  the host-twin definitions (test infrastructure)
  earthkit-meteo_amd/ekm_hip/_optable.py        the ctypes signature table

Run `python tools/gen_abi.py` after editing OPS.
"""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PHASE = ("phase", "EKM_PHASE_*", 3)
EPT = ("ept_method", "EKM_EPT_*", 3)
LCL = ("method", "EKM_LCL_*", 2)
EPTM = ("method", "EKM_EPT_*", 3)
TM2 = ("t_method", "EKM_T_BISECT | EKM_T_NEWTON", 2)
TM3 = ("t_method", "EKM_T_BISECT | EKM_T_NEWTON | EKM_T_DIRECT", 3)

# name, functor, inputs, outputs, int params, has eps, reference lines (thermo.py unless noted), group
OPS = [
    ("celsius_to_kelvin", "OpCelsiusToKelvin", ["t"], ["out"], [], False, "21-35", "basic"),
    ("kelvin_to_celsius", "OpKelvinToCelsius", ["t"], ["out"], [], False, "38-52", "basic"),
    ("specific_humidity_from_mixing_ratio", "OpQFromW", ["w"], ["out"], [], False, "55-77", "basic"),
    ("mixing_ratio_from_specific_humidity", "OpWFromQ", ["q"], ["out"], [], False, "80-102", "basic"),
    ("vapour_pressure_from_specific_humidity", "OpEFromQ", ["q", "p"], ["out"], [], False, "105-131", "basic"),
    ("vapour_pressure_from_mixing_ratio", "OpEFromW", ["w", "p"], ["out"], [], False, "134-159", "basic"),
    ("specific_humidity_from_vapour_pressure", "OpQFromE", ["e", "p"], ["out"], [], True, "162-196", "basic"),
    ("mixing_ratio_from_vapour_pressure", "OpWFromE", ["e", "p"], ["out"], [], True, "199-232", "basic"),
    ("saturation_vapour_pressure", "OpSvp", ["t"], ["out"], [PHASE], False, "235-279; es_comp.py:31-79,133-166", "svp"),
    ("saturation_mixing_ratio", "OpSatW", ["t", "p"], ["out"], [PHASE], False, "282-310", "svp"),
    ("saturation_specific_humidity", "OpSatQ", ["t", "p"], ["out"], [PHASE], False, "313-341", "svp"),
    ("saturation_vapour_pressure_slope", "OpSvpSlope", ["t"], ["out"], [PHASE], False, "344-364; es_comp.py:82-106,169-200", "svp"),
    ("saturation_mixing_ratio_slope", "OpSatWSlope", ["t", "p"], ["out"], [PHASE], True, "367-415", "svp"),
    ("saturation_specific_humidity_slope", "OpSatQSlope", ["t", "p"], ["out"], [PHASE], True, "418-467", "svp"),
    ("saturation_mixing_ratio_slope_from_es", "OpSatWSlopeFromEs", ["p", "es", "es_slope"], ["out"], [], True,
     "407-415 (caller-supplied es, es_slope)", "svp"),
    ("saturation_specific_humidity_slope_from_es", "OpSatQSlopeFromEs", ["p", "es", "es_slope"], ["out"], [], True,
     "459-467 (caller-supplied es, es_slope)", "svp"),
    ("temperature_from_saturation_vapour_pressure", "OpTFromEs", ["es"], ["out"], [], False, "470-491; es_comp.py:109-130", "basic"),
    ("relative_humidity_from_dewpoint", "OpRhFromTd", ["t", "td"], ["out"], [], False, "494-521", "basic"),
    ("relative_humidity_from_specific_humidity", "OpRhFromQ", ["t", "q", "p"], ["out"], [], False, "524-556", "basic"),
    ("specific_humidity_from_dewpoint", "OpQFromTd", ["td", "p"], ["out"], [], False, "559-591", "basic"),
    ("mixing_ratio_from_dewpoint", "OpWFromTd", ["td", "p"], ["out"], [], False, "594-626", "basic"),
    ("specific_humidity_from_relative_humidity", "OpQFromRh", ["t", "r", "p"], ["out"], [], False, "629-663", "basic"),
    ("dewpoint_from_relative_humidity", "OpTdFromRh", ["t", "r"], ["out"], [], False, "666-699", "basic"),
    ("dewpoint_from_specific_humidity", "OpTdFromQ", ["q", "p"], ["out"], [], False, "702-735", "basic"),
    ("virtual_temperature", "OpVirtualT", ["t", "q"], ["out"], [], False, "738-764", "basic"),
    ("virtual_potential_temperature", "OpVirtualTheta", ["t", "q", "p"], ["out"], [], False, "767-798", "basic"),
    ("potential_temperature", "OpTheta", ["t", "p"], ["out"], [], False, "801-829", "basic"),
    ("temperature_from_potential_temperature", "OpTFromTheta", ["th", "p"], ["out"], [], False, "832-858", "basic"),
    ("pressure_on_dry_adiabat", "OpPOnDryAdiabat", ["t", "t_def", "p_def"], ["out"], [], False, "861-889", "basic"),
    ("temperature_on_dry_adiabat", "OpTOnDryAdiabat", ["p", "t_def", "p_def"], ["out"], [], False, "892-920", "basic"),
    ("lcl_temperature", "OpLclT", ["t", "td"], ["out"], [LCL], False, "923-968", "basic"),
    ("lcl", "OpLcl", ["t", "td", "p"], ["t_lcl", "p_lcl"], [LCL], False, "971-1000", "basic"),
    ("ept_from_dewpoint", "OpEptFromTd", ["t", "td", "p"], ["out"], [EPTM], False, "1326-1387,1031-1040,1169-1175,1205-1213,1268-1278", "ept"),
    ("ept_from_specific_humidity", "OpEptFromQ", ["t", "q", "p"], ["out"], [EPTM], False, "1390-1415,1031-1040", "ept"),
    ("saturation_ept", "OpSatEpt", ["t", "p"], ["out"], [EPTM], False, "1418-1469,1042-1045,1177-1182,1215-1224,1280-1295", "ept"),
    ("temperature_on_moist_adiabat", "OpTOnMa", ["ept", "p"], ["out"], [EPT, TM2], False, "1472-1509,1055-1159", "moist"),
    ("wet_bulb_temperature_from_dewpoint", "OpWetBulbFromTd", ["t", "td", "p"], ["out"], [EPT, TM2], False, "1512-1549", "moist"),
    ("wet_bulb_temperature_from_specific_humidity", "OpWetBulbFromQ", ["t", "q", "p"], ["out"], [EPT, TM2], False, "1552-1590", "moist"),
    ("wet_bulb_potential_temperature_from_dewpoint", "OpWbptFromTd", ["t", "td", "p"], ["out"], [EPT, TM3], False, "1593-1634,1047-1053", "wbpt"),
    ("wet_bulb_potential_temperature_from_specific_humidity", "OpWbptFromQ", ["t", "q", "p"], ["out"], [EPT, TM3], False, "1637-1675,1047-1053", "wbpt"),
    ("specific_gas_constant", "OpGasConstant", ["q"], ["out"], [], False, "1678-1707", "basic"),
    # SURVEY.md 8f rank 4 names this free rider on the map skeleton (the only non-thermo entry point)
    ("w_from_omega", "OpWFromOmega", ["omega", "t", "p"], ["out"], [], False, "wind/array/wind.py:192-222", "wind"),
    ("pipeline_svp_td_rh", "OpPipelineSvpTdRh", ["t", "q", "p"], ["es", "td", "rh"], [], False,
     "235-279 + 702-735 + 524-556 fused (SURVEY.md 8a row a13, P3)", "pipeline"),
    ("pipeline_full", "OpPipelineFull", ["t", "q", "p"], ["theta", "es", "rh", "td", "theta_e", "tw"], [], False,
     "801-829 + 235-279 + 524-556 + 702-735 + 1390-1415 + 1552-1590(ifs,newton) fused (SURVEY.md 8a row a13, P5)", "pipeline"),
]

DTYPES = (("f32", "float"), ("f64", "double"))

HEADER_TOP = r'''/* ekm_thermo.h -- C ABI of libekm_thermo.so: MI355X (gfx950) kernels for the
 * earthkit-meteo `thermo` elementwise hot path.
 *
 * GENERATED by tools/gen_abi.py -- edit the table there.
 *
 * Reference interface this replaces: the Python call layer
 * `earthkit.meteo.thermo.<name>(*args, **kwargs)`
 * (/root/reference/src/earthkit/meteo/thermo/thermo.py:13-166, forwarding to
 * thermo/array/thermo.py).  The reference has no FFI of its own: its "backend"
 * is whatever array namespace `array_namespace(*inputs)` returns
 * (thermo/array/thermo.py:826, es_comp.py:73).  Each compute entry point below
 * is what a native backend for one of those functions binds to; the comment on
 * each names the reference lines it implements.
 *
 * Conventions
 *  - plain C types only; every function returns EKM_OK (0) or a negative
 *    EKM_ERR_* code and never throws; ekm_last_error() gives the message of the
 *    calling thread's last failure;
 *  - `dev` is a HIP device ordinal; `stream` is a hipStream_t passed as void*
 *    (NULL = the device's default stream);
 *  - data pointers of compute entry points are DEVICE pointers owned by the
 *    caller; launches are asynchronous on `stream`, allocate nothing, copy
 *    nothing and do not synchronise (graph-capturable);
 *  - an input is described by an ekm_operand: a full field of n values, one
 *    scalar, or a level vector broadcast over the field (see EKM_LEVEL_*), so a
 *    137-level pressure vector is never materialised per grid point;
 *  - outputs are full fields of n values and must not alias inputs of a
 *    different index range;
 *  - `_f32` computes in float with the CDNA4 transcendental unit, `_f64` in
 *    double; NaN/inf results follow the reference (in-band, never an error).
 */
#ifndef EKM_THERMO_H
#define EKM_THERMO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EKM_API __attribute__((visibility("default")))

/* ---- status codes ---- */
#define EKM_OK 0
#define EKM_ERR_HIP (-1)     /* a HIP runtime call failed */
#define EKM_ERR_ARG (-2)     /* bad pointer / size / operand description */
#define EKM_ERR_ENUM (-3)    /* unknown phase / method value */
#define EKM_ERR_NODEV (-4)   /* no such device */

/* ---- enums (fixed values) ---- */
/* phase of saturation_vapour_pressure & co (es_comp.py:22) */
#define EKM_PHASE_MIXED 0
#define EKM_PHASE_WATER 1
#define EKM_PHASE_ICE 2
/* equivalent-potential-temperature method (thermo/array/thermo.py:1319-1323) */
#define EKM_EPT_IFS 0
#define EKM_EPT_BOLTON35 1
#define EKM_EPT_BOLTON39 2
/* moist-adiabat inversion (thermo.py:1504-1509, 1631) */
#define EKM_T_BISECT 0
#define EKM_T_NEWTON 1
#define EKM_T_DIRECT 2
/* lcl_temperature method (thermo.py:960-968) */
#define EKM_LCL_DAVIES 0
#define EKM_LCL_BOLTON 1

/* ---- operand description ---- */
#define EKM_FIELD 0        /* data[i], i < n                                          */
#define EKM_SCALAR 1       /* data[0] for every point                                 */
#define EKM_LEVEL_MAJOR 2  /* data[i / inner]: `len` levels of `inner` points each    */
#define EKM_LEVEL_MINOR 3  /* data[i % len]: the vector runs along the fastest axis   */
#define EKM_HYBRID_FULL 4  /* pressure on hybrid full levels formed in the kernel:
                              data = surface pressure sp (`inner` values), `len` full levels,
                              aux0/aux1 = A/B half-level tables (len+1 values each);
                              value = ph(k) + 0.5*(ph(k+1)-ph(k)), ph(h) = A[h] + B[h]*sp[i % inner],
                              k = i / inner  (vertical/array/vertical.py:670,708).  Last operand only. */

typedef struct ekm_operand {
  const void* data; /* device pointer (float* for _f32, double* for _f64)         */
  int32_t mode;     /* one of the five: EKM_FIELD / _SCALAR / _LEVEL_MAJOR / _LEVEL_MINOR / _HYBRID_FULL */
  int32_t nflat;    /* EKM_HYBRID_FULL: number of LEADING levels k with B[k] = B[k+1] = 0 (pure pressure
                       levels: the upper 53 of the 137 IFS levels), which then run at level-vector
                       speed in a launch of their own; 0 is always valid.  Else 0.            */
  uint64_t len;     /* vector length for the LEVEL modes, else ignored            */
  uint64_t inner;   /* points per level for EKM_LEVEL_MAJOR / EKM_HYBRID_FULL      */
  const void* aux0; /* EKM_HYBRID_FULL: A table (device), else NULL                */
  const void* aux1; /* EKM_HYBRID_FULL: B table (device), else NULL                */
} ekm_operand;

/* ---- ABI version ----
 * Bumped whenever an exported symbol is removed or changes its signature or meaning (history: INTEGRATION.md).  A client
 * built against this header compares EKM_ABI_VERSION with ekm_abi_version() of the library it loaded before any
 * other call (ekm_hip/_ffi.py does); a library older than version 5 does not export the function at all.
 *   5  (round 5) ekm_abi_version added.  Since round 3 (unnumbered "4"): ekm_copy_staged, ekm_host_memcpy,
 *      ekm_host_register, ekm_host_unregister removed; "table_tiles" default 8 -> 0 (= by op); field pointers must be
 *      aligned to their element size; at most 32 KiB (was 64) of staged level vectors per launch.
 *      Added since, without a bump (an addition breaks no client): the vertical interpolation entry points; the ensemble
 *      reductions ekm_efi_*, ekm_sot_*, ekm_sot_func_*, ekm_crps_from_ensemble_*; the per-point quantiles ekm_quantiles_*; the
 *      Crossing Point Forecast ekm_cpf_*; the solar geometry ekm_solar_*; the wind functions
 *      ekm_wind_polar_*, ekm_wind_xy_*, ekm_wind_coriolis_*, ekm_windrose_*; the Gumbel extreme-value fit and its
 *      functions ekm_gumbel_fit_*, ekm_gumbel_cdf_f64, ekm_gumbel_ppf_f64; the reduce family ekm_regimes_project_*,
 *      ekm_regimes_index_*, ekm_pearson_*; the NaN-skipping weighted mean ekm_nanaverage_*, ekm_nanaverage_work_bytes;
 *      the long-axis quantiles ekm_long_quantiles_*; the long-axis reductions ekm_long_efi_*, ekm_long_sot_*,
 *      ekm_long_crps_from_ensemble_*, ekm_long_gumbel_fit_*, ekm_long_cpf_*. */
#define EKM_ABI_VERSION 5
EKM_API int ekm_abi_version(void);              /* EKM_ABI_VERSION of the library as built */

/* ---- lifecycle ---- */
EKM_API int ekm_init(void);                     /* probes the HIP runtime; EKM_ERR_NODEV without a GPU */
EKM_API int ekm_device_count(void);             /* >= 0, or a negative error code */
EKM_API const char* ekm_last_error(void);       /* thread-local, never NULL */
EKM_API const char* ekm_version(void);
EKM_API int ekm_device_name(int dev, char* buf, size_t buflen);
EKM_API int ekm_device_cus(int dev);            /* compute units, or a negative error code */
EKM_API int ekm_mem_info(int dev, size_t* free_bytes, size_t* total_bytes);

/* ---- device memory, streams, events ---- */
EKM_API int ekm_malloc(int dev, size_t bytes, void** out);
EKM_API int ekm_free(int dev, void* ptr);
EKM_API int ekm_host_alloc(size_t bytes, void** out);  /* pinned host memory for fast transfers */
EKM_API int ekm_host_free(void* ptr);
EKM_API int ekm_host_prefault(void* ptr, size_t bytes, int nthreads); /* touch the pages of a fresh host buffer on `nthreads` threads */
EKM_API int ekm_h2d(int dev, void* dst, const void* src, size_t bytes, void* stream);
EKM_API int ekm_d2h(int dev, void* dst, const void* src, size_t bytes, void* stream);
EKM_API int ekm_d2d(int dev, void* dst, const void* src, size_t bytes, void* stream);
EKM_API int ekm_memset(int dev, void* dst, int value, size_t bytes, void* stream);
EKM_API int ekm_fill_u32(int dev, void* dst, uint32_t value, size_t count, void* stream); /* `count` 32-bit words = value (async; a scalar operand's bit pattern without a host buffer) */
EKM_API int ekm_sync(int dev);                  /* hipDeviceSynchronize */
EKM_API int ekm_stream_create(int dev, void** out);
EKM_API int ekm_stream_destroy(int dev, void* stream);
EKM_API int ekm_stream_sync(int dev, void* stream);
EKM_API int ekm_event_create(int dev, void** out);
EKM_API int ekm_event_destroy(int dev, void* event);
EKM_API int ekm_event_record(int dev, void* event, void* stream);
EKM_API int ekm_stream_wait_event(int dev, void* stream, void* event); /* later work on `stream` waits for `event` (no host wait) */
EKM_API int ekm_event_sync(int dev, void* event);
EKM_API int ekm_event_elapsed_ms(int dev, void* start, void* stop, float* ms);
/* HIP graphs: between ekm_graph_begin and ekm_graph_end the launches made on `stream` (from ekm_stream_create; not the
 * default stream) are RECORDED, not run -- every compute entry point only enqueues kernels, so any sequence of them
 * can be recorded; ekm_malloc is allowed meanwhile, copies from pageable host memory and waits are not.
 * ekm_graph_end always ends the recording; it returns the executable graph in *graph_exec (NULL pointer: drop the
 * recording).  ekm_graph_launch replays it on a stream: same kernels, same pointers, one call. */
EKM_API int ekm_graph_begin(int dev, void* stream);
EKM_API int ekm_graph_end(int dev, void* stream, void** graph_exec);
EKM_API int ekm_graph_launch(int dev, void* graph_exec, void* stream);
EKM_API int ekm_graph_destroy(int dev, void* graph_exec);

/* ---- launch tuning (process-wide; defaults are the measured best) ---- */
/* tiles_per_block: consecutive 4-KiB tiles (256 lanes x 16 B) one workgroup streams per field;
 * unroll: tiles in flight per lane per trip (1 or 2; the bisection functions' tree-walk kernels always take 1).  0 keeps a value.
 * The first call that sets either value also switches off, for the rest of the process, the size heuristics that otherwise pick the
 * launch shape of long full-field calls (two tiles in flight for the fp32 Newton kernels, four tiles for the fp64 ones): no call
 * switches them back on, not even ekm_set_tuning(1, 1).  Results do not depend on the launch shape. */
EKM_API int ekm_set_tuning(int tiles_per_block, int unroll);
EKM_API int ekm_get_tuning(int* tiles_per_block, int* unroll);
/* secondary parameters by name (defaults from the environment, in brackets):
 *   "hybrid_band_kb" [EKM_HYBRID_BAND_KB, 8192]  EKM_HYBRID_FULL: KiB of surface pressure per L2-resident band;
 *   "lev_per_wg"     [EKM_LEV_PER_WG, 0]         EKM_HYBRID_FULL, one-in one-out functions only (theta ...): consecutive levels one workgroup walks (0 = 4); no effect on functions with more streams or on the bisection functions;
 *   "table_tiles"    [EKM_TABLE_TILES, 0]        most tiles per workgroup for ops that keep an LDS table (bisection); 0 = by op (8 or 16);
 *   "geo_chunk_levels" [EKM_GEO_CHUNK_LEVELS, all] levels per launch of the geopotential column scan;
 *   "hybrid_rows"      [EKM_HYBRID_ROWS, 1]        pressure_on_hybrid_levels: 1 = one workgroup per (level, tile), every output row
 *                      written in order like a map kernel's stream; 0 = one lane per column walking down the levels; same results;
 *   "f64_plain"        [EKM_F64_PLAIN, 0]          1: the fp64 map kernels redo EVERY lane with the plain-double primitives
 *                      (IEEE special operands fixed up as libm does) instead of only the lanes whose fast first pass
 *                      produced a non-finite output; same results, for tests and A/B timing;
 *   "bisect_exact"     [EKM_BISECT_EXACT, 0]       1: the bisection functions (every method, fp32 and fp64) evaluate the reference's residual (rcp + exp2) at
 *                      EVERY step of their tree walk instead of only where the transcendental-free sign test is within
 *                      rounding of zero; same results, for tests and A/B timing. */
EKM_API int ekm_set_tuning_param(const char* name, int value);
/* The table-driven functions (wet-bulb / moist-adiabat inversion by bisection) read a lookup table that is computed on
 * the device at their first launch there -- asynchronously: no entry point of this library waits on the host.  A
 * launch captured into a HIP graph before the table exists records the fill into that graph.  ekm_prepare_tables(dev)
 * computes every table on `dev` now and WAITS for it (the one synchronising call; not while capturing), so that later
 * launches and captures find them ready. */
EKM_API int ekm_prepare_tables(int dev);

/* ---- synthetic benchmark input, generated on the device (SURVEY.md 8d) ----
 * Fills t, q (and p unless NULL) for points [first, first+n) of a level-major
 * [nlev, inner] grid with the benchmark distribution; counter-based, so any
 * shard of the global index range can be generated independently. */
EKM_API int ekm_synth_fill_f32(int dev, void* stream, float* t, float* q, float* p, uint64_t first, size_t n,
                               uint64_t inner, uint32_t nlev, uint64_t seed);
EKM_API int ekm_synth_fill_f64(int dev, void* stream, double* t, double* q, double* p, uint64_t first, size_t n,
                               uint64_t inner, uint32_t nlev, uint64_t seed);
/* same distribution of t, q around a pressure field that is already on the device (e.g. hybrid levels) */
EKM_API int ekm_synth_fill_given_p_f32(int dev, void* stream, float* t, float* q, const float* p, uint64_t first,
                                       size_t n, uint64_t seed);
EKM_API int ekm_synth_fill_given_p_f64(int dev, void* stream, double* t, double* q, const double* p, uint64_t first,
                                       size_t n, uint64_t seed);
/* The streaming reference of a launch (a benchmark helper like the two above): reads `nin` (0..3) and writes `nout` (1, 2, 3
 * or 6) streams of `bytes` bytes each with the map kernels' launch shape and one add per stream -- what the memory system
 * gives this set of buffers; bench.py times it on the arrays of the launch it has just measured (roofline.stream_ceiling).
 * The outputs are OVERWRITTEN. */
EKM_API int ekm_stream_mix(int dev, void* stream, const void* const* ins, int nin, void* const* outs, int nout, size_t bytes);
EKM_API int ekm_synth_levels_f32(int dev, void* stream, float* p_levels, uint32_t nlev);
EKM_API int ekm_synth_levels_f64(int dev, void* stream, double* p_levels, uint32_t nlev);

/* ---- hybrid model levels: the producer of the pressure field (SURVEY.md 8f rank 1) ----
 * pressure_on_hybrid_levels: reference vertical/array/vertical.py:505-740.
 * A, B: nfull+1 half-level coefficients of the (contiguous) level range, on the device;
 * sp: npts surface pressures; outputs are [rows, npts] level-major, any may be NULL.
 * row_full[k] / row_half[h] give the output row of layer k / half level h, or -1 to skip it
 * (NULL = identity): this is how the reference's `levels=` selection and ordering is expressed.
 * top_is_zero: the reference's any(p_half[0] <= 0.1) (see ekm_any_le_*); alpha_top: log(2) or 1. */
EKM_API int ekm_pressure_on_hybrid_levels_f32(int dev, void* stream, const float* A, const float* B, const float* sp,
                                              size_t npts, uint32_t nfull, const int32_t* row_full,
                                              const int32_t* row_half, int top_is_zero, float alpha_top, float* full,
                                              float* half, float* delta, float* alpha);
EKM_API int ekm_pressure_on_hybrid_levels_f64(int dev, void* stream, const double* A, const double* B, const double* sp,
                                              size_t npts, uint32_t nfull, const int32_t* row_full,
                                              const int32_t* row_half, int top_is_zero, double alpha_top, double* full,
                                              double* half, double* delta, double* alpha);
/* Geopotential chain on hybrid levels, fused with the producer of alpha/delta: reference
 * vertical/array/vertical.py:741-1190 (relative_geopotential_thickness_on_hybrid_levels,
 * geopotential_on_hybrid_levels, height_on_hybrid_levels).  t, q, out: [nfull, npts] level-major;
 * A, B: the nfull+1 half-level coefficients of those levels; zs: surface geopotential (may be NULL
 * for modes 0 and 5).  mode: 0 thickness, 1 geopotential (+zs), 2 geometric height above sea,
 * 3 geopotential height above sea, 4 geometric height above ground, 5 geopotential height above ground. */
EKM_API int ekm_geopotential_on_hybrid_levels_f32(int dev, void* stream, const float* A, const float* B,
                                                  const float* sp, const float* zs, const float* t, const float* q,
                                                  size_t npts, uint32_t nfull, int top_is_zero, float alpha_top,
                                                  int mode, float* out);
EKM_API int ekm_geopotential_on_hybrid_levels_f64(int dev, void* stream, const double* A, const double* B,
                                                  const double* sp, const double* zs, const double* t, const double* q,
                                                  size_t npts, uint32_t nfull, int top_is_zero, double alpha_top,
                                                  int mode, double* out);
/* The same bottom-up scan for callers who already hold alpha and delta (outputs of pressure_on_hybrid_levels):
 * reference vertical/array/vertical.py:741-893 (relative_geopotential_thickness_on_hybrid_levels_from_alpha_delta).
 * t, q, alpha, delta, out: [nfull, npts] level-major; 16 B read + 4 B written per point (fp32). */
EKM_API int ekm_geopotential_thickness_from_alpha_delta_f32(int dev, void* stream, const float* t, const float* q,
                                                            const float* alpha, const float* delta, size_t npts,
                                                            uint32_t nfull, float* out);
EKM_API int ekm_geopotential_thickness_from_alpha_delta_f64(int dev, void* stream, const double* t, const double* q,
                                                            const double* alpha, const double* delta, size_t npts,
                                                            uint32_t nfull, double* out);
/* *flag |= any(a0 + b0*sp[i] <= thresh); *flag must be zeroed by the caller (ekm_memset) */
EKM_API int ekm_any_le_f32(int dev, void* stream, const float* sp, size_t n, float a0, float b0, float thresh,
                           int32_t* flag);
EKM_API int ekm_any_le_f64(int dev, void* stream, const double* sp, size_t n, double a0, double b0, double thresh,
                           int32_t* flag);

/* ---- vertical interpolation from model levels to pressure / height levels ----
 * interpolate_monotonic: reference vertical/array/vertical.py:1616-1719 and vertical/array/monotonic.py:49-370.
 * data: [nlev, npts] level-major; coord: [nlev, npts] (coord_is_field != 0) or [nlev]; target: [ntarget] or
 * [ntarget, npts] (target_is_field != 0); out: [ntarget, npts].  nlev >= 2, ntarget <= 65535.
 * descending: the reference's ordering decision (monotonic.py:82-91: coord[0] >= coord[-1] in the first column),
 *   taken by the caller; nothing is flipped in memory.  A column that is not monotonic gives an unspecified value.
 * mode: EKM_INTERP_LINEAR / _LOG / _NEAREST.
 * aux_*: the optional layers beyond the smallest (min) and the largest (max) coordinate of a column; a layer is
 *   active when both its pointers are given; each is ONE value on the device, or [npts] when its bit of
 *   aux_field_mask is set (bit 0 min_data, 1 min_coord, 2 max_data, 3 max_coord).
 * Like every compute entry point these only enqueue a kernel: nothing waits on the host. */
#define EKM_INTERP_LINEAR 0
#define EKM_INTERP_LOG 1
#define EKM_INTERP_NEAREST 2
EKM_API int ekm_interpolate_monotonic_f32(int dev, void* stream, const float* data, const float* coord,
                                          int coord_is_field, const float* target, int target_is_field,
                                          uint32_t ntarget, size_t npts, uint32_t nlev, int descending, int mode,
                                          const float* aux_min_data, const float* aux_min_coord,
                                          const float* aux_max_data, const float* aux_max_coord,
                                          uint32_t aux_field_mask, float* out);
EKM_API int ekm_interpolate_monotonic_f64(int dev, void* stream, const double* data, const double* coord,
                                          int coord_is_field, const double* target, int target_is_field,
                                          uint32_t ntarget, size_t npts, uint32_t nlev, int descending, int mode,
                                          const double* aux_min_data, const double* aux_min_coord,
                                          const double* aux_max_data, const double* aux_max_coord,
                                          uint32_t aux_field_mask, double* out);
/* The height coordinate of interpolate_pressure_to_height_levels: reference vertical/array/vertical.py:1489-1613
 * (:1593-1601; geopotential_height_from_geopotential :330-345, geometric_height_from_geopotential :472-501).
 * z, out: [nlev, npts] level-major; zs: [npts], read by the "above ground" modes only.  mode as in
 * ekm_geopotential_on_hybrid_levels_*: 2 geometric height above sea, 3 geopotential height above sea, 4 geometric
 * height above ground, 5 geopotential height above ground.  Every operation rounded once, IEEE division. */
EKM_API int ekm_height_from_geopotential_f32(int dev, void* stream, const float* z, const float* zs, size_t npts,
                                             uint32_t nlev, int mode, float* out);
EKM_API int ekm_height_from_geopotential_f64(int dev, void* stream, const double* z, const double* zs, size_t npts,
                                             uint32_t nlev, int mode, double* out);
/* interpolate_hybrid_to_pressure_levels: reference vertical/array/vertical.py:1206-1326, fused with the producer of
 * the pressure (vertical.py:663, 708): the coordinate is p_full formed in the kernel from sp [npts] and the nfull+1
 * half-level coefficients A, B of the data's levels, each operation rounded once in the reference's order; the
 * pressure field is never stored.  aux_min_* is the layer above the model top (the reference's aux_top_*),
 * aux_max_* the one below the lowest level (aux_bottom_*).  nfull <= 2047 (fp64) / 4095 (fp32). */
EKM_API int ekm_interpolate_hybrid_to_pressure_f32(int dev, void* stream, const float* data, const float* A,
                                                   const float* B, const float* sp, const float* target,
                                                   int target_is_field, uint32_t ntarget, size_t npts, uint32_t nfull,
                                                   int descending, int mode, const float* aux_min_data,
                                                   const float* aux_min_coord, const float* aux_max_data,
                                                   const float* aux_max_coord, uint32_t aux_field_mask, float* out);
EKM_API int ekm_interpolate_hybrid_to_pressure_f64(int dev, void* stream, const double* data, const double* A,
                                                   const double* B, const double* sp, const double* target,
                                                   int target_is_field, uint32_t ntarget, size_t npts, uint32_t nfull,
                                                   int descending, int mode, const double* aux_min_data,
                                                   const double* aux_min_coord, const double* aux_max_data,
                                                   const double* aux_max_coord, uint32_t aux_field_mask, double* out);

/* ---- ensemble reductions: Extreme Forecast Index, Shift of Tails, Crossing Point Forecast, CRPS ----
 * One lane per grid point; fields are member-major: clim [nclim, npts], ens / x [nens, npts] (quantiles: any axis).  The point's ensemble is
 * sorted in LDS: nens <= 256 (_f32) / 128 (_f64), more members return EKM_ERR_ARG (cpf: its own limit, below).  Every operation is rounded once in
 * the reference's order and the f64 sums run in its loop order: the results equal the reference's (NumPy) bit for bit.
 * Like every compute entry point these only enqueue a kernel: nothing allocates, copies or waits on the host.
 *
 * efi: reference extreme/array/efi.py:34-89.  clim need not be sorted (the reference counts members <= clim[i]); its
 * rows are streamed once, nclim >= 1 is unbounded.  acosdiff, proddiff, acoef: the nclim-1 float64 coefficients of
 * efi.py:54-60 on the device, computed by the caller (ekm_hip.extreme does it with NumPy as the reference does; no
 * acos is evaluated here).  eps > 0 selects the masked sum divided by max(efimax, eps), eps <= 0 the plain sum * 2/pi.
 * out: float64 [npts] for both input dtypes; NaN where a column of clim or ens holds a NaN. */
EKM_API int ekm_efi_f32(int dev, void* stream, const float* clim, const float* ens, uint32_t nclim, uint32_t nens,
                        size_t npts, double eps, const double* acosdiff, const double* proddiff, const double* acoef,
                        double* out);
EKM_API int ekm_efi_f64(int dev, void* stream, const double* clim, const double* ens, uint32_t nclim, uint32_t nens,
                        size_t npts, double eps, const double* acosdiff, const double* proddiff, const double* acoef,
                        double* out);
/* sot: reference extreme/array/sot.py:51-103.  qc = row `perc` of the climate, qc_tail = row 99 (perc > 50) or row 1
 * (perc < 50): [npts] each, passed as row pointers.  perc in [2, 98], not 50.  The forecast percentile is
 * numpy.percentile's linear method in the input dtype; with eps > 0 members and qc below eps count as 0.  out: [npts]
 * in the input dtype. */
EKM_API int ekm_sot_f32(int dev, void* stream, const float* qc, const float* qc_tail, const float* ens, uint32_t nens,
                        size_t npts, int perc, double eps, float* out);
EKM_API int ekm_sot_f64(int dev, void* stream, const double* qc, const double* qc_tail, const double* ens, uint32_t nens,
                        size_t npts, int perc, double eps, double* out);
/* sot_func: reference extreme/array/sot.py:13-48, elementwise over n points:
 * |qc_tail - qc| > max(eps, 0) ? (qf - qc_tail) / (qc_tail - qc) : NaN, clamped to [lower_bound, upper_bound]. */
EKM_API int ekm_sot_func_f32(int dev, void* stream, const float* qc_tail, const float* qc, const float* qf, size_t n,
                             double eps, double lower_bound, double upper_bound, float* out);
EKM_API int ekm_sot_func_f64(int dev, void* stream, const double* qc_tail, const double* qc, const double* qf, size_t n,
                             double eps, double lower_bound, double upper_bound, double* out);
/* cpf: reference extreme/array/cpf.py:13-155, the Crossing Point Forecast, one launch per call (`symmetric` included).
 * The flags are 0 / non-zero.  sort_clim, sort_ens (cpf.py:140-143): the column is sorted as numpy.sort does, a NaN above
 * every number, else used as given; the inputs are never written.  from_zero (cpf.py:27): the scan starts at member 0,
 * else at nens / 2.  symmetric (cpf.py:145-153): a direct value below 0.5 becomes 1 - (the value of the negated,
 * row-reversed columns); epsilon is then ignored.  use_epsilon, epsilon (cpf.py:86-89): points whose last member is below
 * epsilon (compared in the input dtype) give 0.
 * The ensemble column, and the climate column when sort_clim, are held in LDS:
 * (nens + (sort_clim ? nclim : 0)) * 64 * sizeof(element) <= 160 KiB, i.e. 640 rows (_f32) / 320 rows (_f64); more
 * returns EKM_ERR_ARG and writes nothing.  nclim < 3 gives 0 everywhere.
 * out: float [npts] for both input dtypes (cpf.py:22); _f32 interpolates in float, _f64 in double, rounded on the store. */
EKM_API int ekm_cpf_f32(int dev, void* stream, const float* clim, const float* ens, uint32_t nclim, uint32_t nens,
                        size_t npts, int sort_clim, int sort_ens, int from_zero, int symmetric, int use_epsilon,
                        double epsilon, float* out);
EKM_API int ekm_cpf_f64(int dev, void* stream, const double* clim, const double* ens, uint32_t nclim, uint32_t nens,
                        size_t npts, int sort_clim, int sort_ens, int from_zero, int symmetric, int use_epsilon,
                        double epsilon, float* out);
/* crps_from_ensemble: reference score/array/ensemble.py:34-82.  x: [nens, npts], y: [npts]; p2[i] = (i/nens)^2 and
 * q2[i] = (1 - i/nens)^2, i = 0..nens, float64 on the device (computed by the caller as the reference computes them).
 * out: float64 [npts], NaN where x or y holds a NaN; missing (may be NULL): one byte per point, 1 exactly there -- the
 * reference's isnan_mask, which the NaN of `out` cannot stand for (+-inf input gives NaN without being missing). */
EKM_API int ekm_crps_from_ensemble_f32(int dev, void* stream, const float* x, const float* y, uint32_t nens, size_t npts,
                                       const double* p2, const double* q2, double* out, uint8_t* missing);
EKM_API int ekm_crps_from_ensemble_f64(int dev, void* stream, const double* x, const double* y, uint32_t nens,
                                       size_t npts, const double* p2, const double* q2, double* out, uint8_t* missing);
/* quantiles: reference stats/array/quantiles.py:18-84 (iter_quantiles), all levels of a call in one launch.
 * arr: [outer, m, inner] contiguous, the m samples of point p = o * inner + i at (o * m + j) * inner + i, so the sample
 * axis may be any axis; m <= 256 (f32 data) / 128 (f64 data), more samples return EKM_ERR_ARG.
 * lo, hi, w: the nq position records on the device as float64 vectors, computed by the caller exactly as the reference
 * and numpy.quantile compute them (ekm_hip.stats.quantile_positions; no floor is evaluated here): lo and hi are the two
 * neighbours in the sorted column (whole numbers < m), w the weight.
 * mode: EKM_QUANTILE_SORT, quantiles.py:75-83: s[lo] * (1 - w) + s[hi] * w, each product and the sum rounded once in
 *   float64 (f64 output only: _f64 and _f32_f64); EKM_QUANTILE_LERP, quantiles.py:60-73: numpy.quantile's linear method,
 *   the difference s[hi] - s[lo] in the data's type, then numpy's _lerp in the output type with w as gamma.
 * out: [nq, outer * inner], level-major, float for _f32, double for _f64 and _f32_f64 (f32 data, f64 result: what the
 * reference returns for "sort" and "numpy_bulk").  A column that holds a NaN gives NaN at every level.
 * outer * inner == 0 or nq == 0 returns EKM_OK without a launch. */
#define EKM_QUANTILE_SORT 0
#define EKM_QUANTILE_LERP 1
EKM_API int ekm_quantiles_f32(int dev, void* stream, const float* arr, size_t outer, uint32_t m, size_t inner,
                              const double* lo, const double* hi, const double* w, uint32_t nq, int mode, float* out);
EKM_API int ekm_quantiles_f64(int dev, void* stream, const double* arr, size_t outer, uint32_t m, size_t inner,
                              const double* lo, const double* hi, const double* w, uint32_t nq, int mode, double* out);
EKM_API int ekm_quantiles_f32_f64(int dev, void* stream, const float* arr, size_t outer, uint32_t m, size_t inner,
                                  const double* lo, const double* hi, const double* w, uint32_t nq, int mode, double* out);

/* long_quantiles: the quantiles of ekm_quantiles_* for a LONG sample axis: m <= 16384 (f32 data) / 8192 (f64 data), more
 * samples return EKM_ERR_ARG naming the cap.  Same arguments, same modes, same position records, same output; one
 * workgroup sorts a tile of whole columns in LDS (a bitonic network over the order-preserving whole-number image of the
 * float bits, columns padded to a power of two >= 32) and reads every level off them with the arithmetic of
 * ekm_quantiles_*.  The results are those of ekm_quantiles_* bit for bit for every m both accept, except that a column
 * holding both -0.0 and +0.0 is sorted with -0.0 first (the insertion sort of ekm_quantiles_* keeps their input order), so
 * a level that lands on a zero may differ in the zero's sign.  Short axes are accepted (m >= 1); ekm_quantiles_* is the
 * faster of the two for short ones (ekm_hip/stats.py gives the measured crossover).
 * outer * inner == 0 or nq == 0 returns EKM_OK without a launch. */
EKM_API int ekm_long_quantiles_f32(int dev, void* stream, const float* arr, size_t outer, uint32_t m, size_t inner,
                                   const double* lo, const double* hi, const double* w, uint32_t nq, int mode, float* out);
EKM_API int ekm_long_quantiles_f64(int dev, void* stream, const double* arr, size_t outer, uint32_t m, size_t inner,
                                   const double* lo, const double* hi, const double* w, uint32_t nq, int mode, double* out);
EKM_API int ekm_long_quantiles_f32_f64(int dev, void* stream, const float* arr, size_t outer, uint32_t m, size_t inner,
                                       const double* lo, const double* hi, const double* w, uint32_t nq, int mode,
                                       double* out);

/* The sorted-column reductions for a LONG member or sample axis: up to 16384 values in f32 and 8192 in f64, more return
 * EKM_ERR_ARG naming the cap before anything is read.  Each takes the arguments of its short entry point and gives its
 * results bit for bit for every axis both accept; one workgroup sorts a tile of whole columns in LDS as
 * ekm_long_quantiles_* does (the same keys: a column holding both -0.0 and +0.0 is sorted with -0.0 first, so a result
 * may differ from the short entry point's, and the reference's, in the sign of a zero), then one lane per column runs
 * the short kernel's per-point arithmetic over it.  Short axes are accepted; ekm_hip/extreme.py, score.py and stats.py
 * give the measured crossover.  No points returns EKM_OK without a launch.  Only enqueue a kernel: nothing allocates,
 * copies or waits on the host.
 * ekm_long_efi_*: reference extreme/array/efi.py:34-89, arguments and result as ekm_efi_*; the climate rows are streamed
 *   from global memory, once each.
 * ekm_long_sot_*: reference extreme/array/sot.py:51-103, as ekm_sot_* (members below a positive eps count as 0 before the
 *   sort).
 * ekm_long_crps_from_ensemble_*: reference score/array/ensemble.py:34-82, as ekm_crps_from_ensemble_* (missing may be
 *   NULL).
 * ekm_long_gumbel_fit_*: reference stats/array/extreme_values.py:44-64 with the L-moments of stats/array/_polyfill.py:14-65,
 *   as ekm_gumbel_fit_* ([outer, m, inner], m >= 2; the sums in float64 in the polyfill's order). */
EKM_API int ekm_long_efi_f32(int dev, void* stream, const float* clim, const float* ens, uint32_t nclim, uint32_t nens,
                             size_t npts, double eps, const double* acosdiff, const double* proddiff,
                             const double* acoef, double* out);
EKM_API int ekm_long_efi_f64(int dev, void* stream, const double* clim, const double* ens, uint32_t nclim, uint32_t nens,
                             size_t npts, double eps, const double* acosdiff, const double* proddiff,
                             const double* acoef, double* out);
EKM_API int ekm_long_sot_f32(int dev, void* stream, const float* qc, const float* qc_tail, const float* ens, uint32_t nens,
                             size_t npts, int perc, double eps, float* out);
EKM_API int ekm_long_sot_f64(int dev, void* stream, const double* qc, const double* qc_tail, const double* ens,
                             uint32_t nens, size_t npts, int perc, double eps, double* out);
EKM_API int ekm_long_crps_from_ensemble_f32(int dev, void* stream, const float* x, const float* y, uint32_t nens,
                                            size_t npts, const double* p2, const double* q2, double* out,
                                            uint8_t* missing);
EKM_API int ekm_long_crps_from_ensemble_f64(int dev, void* stream, const double* x, const double* y, uint32_t nens,
                                            size_t npts, const double* p2, const double* q2, double* out,
                                            uint8_t* missing);
EKM_API int ekm_long_gumbel_fit_f32(int dev, void* stream, const float* sample, size_t outer, uint32_t m, size_t inner,
                                    double* mu, double* sigma);
EKM_API int ekm_long_gumbel_fit_f64(int dev, void* stream, const double* sample, size_t outer, uint32_t m, size_t inner,
                                    double* mu, double* sigma);
/* ekm_long_cpf_*: reference extreme/array/cpf.py:13-155, arguments, flags and result as ekm_cpf_* (out: float [npts]), for
 * LONG columns: nens and nclim EACH up to 16384 (_f32) / 8192 (_f64), checked separately; one more returns EKM_ERR_ARG with
 * a message that names the axis, its length and the cap, and writes nothing; nens >= 1 and nclim >= 1.  One workgroup holds
 * a tile of ensemble columns and a tile of climate columns in LDS (each the 16-KiB or the 64-KiB tile, by its own padded
 * column), sorts each where its flag asks for it -- a NaN above every number, as numpy.sort puts it -- or loads it as given,
 * then one lane per point runs the scan of ekm_cpf_* in O(nclim + nens) (cpf_point_running of csrc/ensemble_point.hpp:
 * the bits of ekm_cpf_* on what both take, but for the sign of a zero in a sorted column that holds both zeros). */
EKM_API int ekm_long_cpf_f32(int dev, void* stream, const float* clim, const float* ens, uint32_t nclim, uint32_t nens,
                             size_t npts, int sort_clim, int sort_ens, int from_zero, int symmetric, int use_epsilon,
                             double epsilon, float* out);
EKM_API int ekm_long_cpf_f64(int dev, void* stream, const double* clim, const double* ens, uint32_t nclim, uint32_t nens,
                             size_t npts, int sort_clim, int sort_ens, int from_zero, int symmetric, int use_epsilon,
                             double epsilon, float* out);

/* Gumbel extreme-value statistics: reference stats/array/extreme_values.py:24-155.
 * ekm_gumbel_fit_*: reference extreme_values.py:44-64 (GumbelDistribution.fit) with the L-moments of
 *   stats/array/_polyfill.py:14-65.  sample: [outer, m, inner] contiguous as for ekm_quantiles_* (any sample axis);
 *   2 <= m <= 256 (_f32) / 128 (_f64), more samples return EKM_ERR_ARG.  The column is sorted ascending in LDS, then
 *   s0 = sum x_i, s1 = sum x_i (i - 1) (i = 1..m, in order), b0 = s0 / m, b1 = s1 / (m (m - 1)), l2 = -b0 + 2 b1,
 *   sigma = l2 / log(2), mu = b0 - 0.5772 sigma: all in float64 (an f32 sample is widened on read), every operation
 *   rounded once.  mu, sigma: float64 [outer * inner]; both NaN where the column holds a NaN.
 * ekm_gumbel_cdf_f64: reference extreme_values.py:76-92 (cdf) and :113-133 (value_to_return_period).
 *   out[k * npts + p] = c = 1 - exp(-exp((mu[p] - x[k]) / sigma[p])) for mode EKM_GUMBEL_CDF, freq / c (IEEE division of
 *   that same c) for EKM_GUMBEL_RETURN_PERIOD; plain float64 with the device library's exp.  x: nx levels, float64 on
 *   the device.
 * ekm_gumbel_ppf_f64: reference extreme_values.py:94-110 (ppf) and :136-155 (return_period_to_value).
 *   out[k * npts + p] = mu[p] - sigma[p] * t[k], product and difference rounded once each; t[k] = log(-log(1 - p_k)) is
 *   computed by the caller as the reference computes it (no logarithm is evaluated here).  t: nt values, float64 on the
 *   device.
 * No points or no levels return EKM_OK without a launch.  Only enqueue a kernel: nothing allocates, copies or waits on
 * the host. */
#define EKM_GUMBEL_CDF 0
#define EKM_GUMBEL_RETURN_PERIOD 1
EKM_API int ekm_gumbel_fit_f32(int dev, void* stream, const float* sample, size_t outer, uint32_t m, size_t inner,
                               double* mu, double* sigma);
EKM_API int ekm_gumbel_fit_f64(int dev, void* stream, const double* sample, size_t outer, uint32_t m, size_t inner,
                               double* mu, double* sigma);
EKM_API int ekm_gumbel_cdf_f64(int dev, void* stream, const double* mu, const double* sigma, size_t npts, const double* x,
                               uint32_t nx, double freq, int mode, double* out);
EKM_API int ekm_gumbel_ppf_f64(int dev, void* stream, const double* mu, const double* sigma, size_t npts, const double* t,
                               uint32_t nt, double* out);

/* ---- the reduce family: sums along a long axis, streamed, added across lanes in one fixed order ----
 * ekm_regimes_project_*: reference regimes/array/index.py:10-56 (project).
 *   out[p * nfields + n] = scale[n] * sum_k field[n * k_len + k] * coef[n * coef_stride + p * k_len + k], p < npat.
 *   field: [nfields, k] contiguous.  coef: pattern times normalised weight, formed by the caller in the call's dtype;
 *   coef_stride 0 = the npat rows are shared by all fields ([npat, k]); otherwise every field has its own block of
 *   npat rows, coef_stride >= npat * k elements apart.  scale: [nfields] (the modulator of ModulatedPatterns), or NULL
 *   for none.  One workgroup per field; patterns are taken eight at a time, one launch per eight, and the field is read
 *   once per launch.  Sums are fma chains in the call's dtype (an f32 call accumulates in f32) in a fixed order that
 *   depends on k alone: the same field gives the same bits at any row index and any element-aligned address, and the
 *   same call gives the same bytes twice.  k >= 1; pointers aligned to their element.
 * ekm_regimes_index_*: reference regimes/array/index.py:59-76 (regime_index).
 *   out[i] = (proj[i] - mean_i) / std_i, the difference rounded once and an IEEE division; mean_i = mean[i], or
 *   mean_value where mean is NULL, and std likewise.
 * ekm_pearson_*: reference score/array/deterministic.py:13-37 (pearson_correlation).
 *   x, y: [outer, m, inner] contiguous (any sample axis), out: [outer * inner]; m >= 1 without a cap.  Mean, centring,
 *   norms, normalisation and the sum of products in the call's dtype, three passes over the samples.  inner > 1: one
 *   lane per point adds its samples in order, which is NumPy's order along a non-contiguous axis.  inner == 1: one wave
 *   per row, lane l adds samples l, l + 64, ..., then a butterfly over the 64 lanes.  NaN where a column holds a NaN,
 *   is constant, or m == 1.
 * No fields, no patterns or no points return EKM_OK without a launch.  Only enqueue kernels: nothing allocates, copies
 * or waits on the host. */
EKM_API int ekm_regimes_project_f32(int dev, void* stream, const float* field, size_t nfields, size_t k, const float* coef,
                                    uint32_t npat, size_t coef_stride, const float* scale, float* out);
EKM_API int ekm_regimes_project_f64(int dev, void* stream, const double* field, size_t nfields, size_t k, const double* coef,
                                    uint32_t npat, size_t coef_stride, const double* scale, double* out);
EKM_API int ekm_regimes_index_f32(int dev, void* stream, const float* proj, const float* mean, float mean_value,
                                  const float* std, float std_value, float* out, size_t n);
EKM_API int ekm_regimes_index_f64(int dev, void* stream, const double* proj, const double* mean, double mean_value,
                                  const double* std, double std_value, double* out, size_t n);
EKM_API int ekm_pearson_f32(int dev, void* stream, const float* x, const float* y, size_t outer, size_t m, size_t inner,
                            float* out);
EKM_API int ekm_pearson_f64(int dev, void* stream, const double* x, const double* y, size_t outer, size_t m, size_t inner,
                            double* out);
/* ekm_nanaverage_*: reference stats/array/numpy_extended.py:13-61 (nanaverage).
 *   data: [outer, m, inner] contiguous, out: [outer * inner]: the mean along m of the samples that are not NaN.
 *   weights: NULL for the plain mean (numpy.nanmean), else the weight of data[o, i, j] is
 *   weights[o * wstride_outer + i * wstride_m + j * wstride_inner] (strides in elements, 0 = broadcast); a sample whose
 *   datum or weight is NaN is skipped.  No valid sample: NaN unweighted, 0 weighted (as the reference); m may be 0.
 *   path: 0 = chosen from (outer, m, inner) alone; 1 = points (one lane per output point, samples added in order: NumPy's
 *   order along a non-contiguous axis, the result is the reference's bit for bit; any inner); 2 = rows (one wave per row);
 *   3 = split (one workgroup per chunk of 32768 elements of a row, the chunks' partial pairs added in chunk order by a
 *   second kernel).  2 and 3 need inner == 1 (else EKM_ERR_ARG); another value is EKM_ERR_ENUM.  path 0 takes 1 when
 *   inner > 1, else 3 when m >= 65536 and outer < 2048, else 2.
 *   work: device scratch of the split path, ekm_nanaverage_work_bytes(...) bytes, aligned to the element; may hold
 *   anything on entry and belongs to the call until it has run; NULL / 0 on the other paths.  Too small is EKM_ERR_ARG.
 *   The unweighted sums start at +0 and are divided by the count in double, rounded once.  Weighted: path 1 forms
 *   den = sum w, then sum data * (w / den), as the reference does; paths 2 and 3 form sum data * w and sum w in one pass
 *   and divide once.  No atomics: the same call gives the same bytes, a row the same bits at any row index and address.
 *   Only enqueues kernels: nothing allocates, copies or waits on the host.
 * ekm_nanaverage_work_bytes: reference stats/array/numpy_extended.py:13-61; host only, needs no device: the bytes of
 *   `work` that ekm_nanaverage_* with these arguments needs (0 where it needs none, and for arguments it refuses). */
EKM_API int ekm_nanaverage_f32(int dev, void* stream, const float* data, size_t outer, size_t m, size_t inner,
                               const float* weights, size_t wstride_outer, size_t wstride_m, size_t wstride_inner, int path,
                               void* work, size_t work_bytes, float* out);
EKM_API int ekm_nanaverage_f64(int dev, void* stream, const double* data, size_t outer, size_t m, size_t inner,
                               const double* weights, size_t wstride_outer, size_t wstride_m, size_t wstride_inner, int path,
                               void* work, size_t work_bytes, double* out);
EKM_API size_t ekm_nanaverage_work_bytes(size_t elem_size, size_t outer, size_t m, size_t inner, int weighted, int path);

/* ---- solar geometry: cosine of the solar zenith angle, its time average, top-of-atmosphere incident radiation ----
 * Reference solar/array/solar.py:51-96 (cos_solar_zenith_angle), :99-179 (_integrate), :182-254.  One launch, one lane per
 * point: out[i] = sum over the nnodes time nodes of w * (isr * max0(p * sin(lat) + q * cos(lat) cos(lon) + r * cos(lat) sin(lon))),
 * max0(z) = z < 0 ? 0 : z (a NaN stays).  lat, lon: degrees, each an ekm_operand in mode EKM_FIELD, EKM_SCALAR,
 * EKM_LEVEL_MAJOR or EKM_LEVEL_MINOR (any len >= 1, inner >= 1; len * inner must cover n).  nodes: nnodes records of five
 * float64 on the device, (p, q, r, w, isr) with p = sin(dec), q = cos(dec) cos(a), r = -cos(dec) sin(a), a the node's hour
 * angle plus time correction: the caller computes them as the reference computes its dates, weights, declinations and
 * time corrections (solar.py:27-48, :150-177, :225-229); the instantaneous function is one node with w = isr = 1.
 * All arithmetic is double on the upcast inputs, the result is rounded once: _f32 float in, float out; _f64 double in,
 * double out; _f32_f64 float in, double out.  Only enqueues a kernel: nothing allocates, copies or waits on the host. */
EKM_API int ekm_solar_f32(int dev, void* stream, const ekm_operand* lat, const ekm_operand* lon, const double* nodes,
                          uint32_t nnodes, float* out, size_t n);
EKM_API int ekm_solar_f64(int dev, void* stream, const ekm_operand* lat, const ekm_operand* lon, const double* nodes,
                          uint32_t nnodes, double* out, size_t n);
EKM_API int ekm_solar_f32_f64(int dev, void* stream, const ekm_operand* lat, const ekm_operand* lon, const double* nodes,
                              uint32_t nnodes, double* out, size_t n);

/* ---- wind: speed and direction, polar <-> xy, the Coriolis parameter, the wind rose ----
 * Reference wind/array/wind.py:15-189, :225-328.  The three elementwise entry points take ekm_operands in mode EKM_FIELD,
 * EKM_SCALAR, EKM_LEVEL_MAJOR or EKM_LEVEL_MINOR (as ekm_solar_*), read every operand once and write every output once;
 * the arithmetic is float in the _f32 entry points and double in the _f64 ones.
 *  ekm_wind_polar_*: speed = hypot(u, v) and direction [degrees] from d = atan2(v, u); either output may be NULL and is
 *    then neither computed nor written.  mode 0 (meteo): d <= -pi/2 ? (-pi/2 - d) deg : (1.5 pi - d) deg, deg = 180/pi;
 *    mode 1 (polar, to_positive): d deg, plus 360 where that is negative; mode 2 (polar, signed): d deg.
 *  ekm_wind_xy_*: x = m cos(a), y = m sin(a) with a = 270 - direction degrees (mode 0, meteo) or a = direction (mode 1);
 *    the angle is reduced exactly in degrees.
 *  ekm_wind_coriolis_*: 2 Omega sin(lat degrees), Omega = 7.292115083046062e-05 1/s.
 *  ekm_windrose_*: the two-dimensional histogram np.histogram2d(speed, direction, [speed edges, direction edges]) of n
 *    samples with the last direction column added to the first and dropped.  edges: ns speed edges followed by nd
 *    direction edges, float64 on the device, each non-decreasing (ns >= 2, nd >= 3, ns + nd <= 2048); bin k holds
 *    e[k] <= x < e[k+1], the last bin also x == e[last]; a NaN or a value outside either axis drops the sample.
 *    inv_step: (nd - 1) / (last - first direction edge), a first guess only (any finite value gives the same counts).
 *    table: (ns-1)*(nd-1) 64-bit counters of scratch on the device, zeroed by the call; out: [ns-1][nd-2] float64, the
 *    counts, or with percent != 0 count * 100 / (number of counted samples) (NaN when none).  Enqueues a memset and two kernels.
 * Nothing here allocates, copies or waits on the host. */
EKM_API int ekm_wind_polar_f32(int dev, void* stream, const ekm_operand* u, const ekm_operand* v, int mode, float* speed,
                               float* direction, size_t n);
EKM_API int ekm_wind_xy_f32(int dev, void* stream, const ekm_operand* magnitude, const ekm_operand* direction, int mode,
                            float* x, float* y, size_t n);
EKM_API int ekm_wind_coriolis_f32(int dev, void* stream, const ekm_operand* lat, float* out, size_t n);
EKM_API int ekm_windrose_f32(int dev, void* stream, const float* speed, const float* direction, size_t n, const double* edges,
                             uint32_t ns, uint32_t nd, double inv_step, int percent, unsigned long long* table,
                             double* out);
EKM_API int ekm_wind_polar_f64(int dev, void* stream, const ekm_operand* u, const ekm_operand* v, int mode, double* speed,
                               double* direction, size_t n);
EKM_API int ekm_wind_xy_f64(int dev, void* stream, const ekm_operand* magnitude, const ekm_operand* direction, int mode,
                            double* x, double* y, size_t n);
EKM_API int ekm_wind_coriolis_f64(int dev, void* stream, const ekm_operand* lat, double* out, size_t n);
EKM_API int ekm_windrose_f64(int dev, void* stream, const double* speed, const double* direction, size_t n, const double* edges,
                             uint32_t ns, uint32_t nd, double inv_step, int percent, unsigned long long* table,
                             double* out);

/* ---- thermo entry points ----
 * Argument order: dev, stream, inputs..., enum parameters..., [eps], outputs..., n. */
'''

HEADER_BOTTOM = r'''
#ifdef __cplusplus
}
#endif
#endif /* EKM_THERMO_H */
'''


def proto(name, ins, outs, ints, has_eps, tag, ctype, prefix="ekm_"):
    args = ["int dev", "void* stream"]
    args += [f"const ekm_operand* {i}" for i in ins]
    args += [f"int {p[0]}" for p in ints]
    if has_eps:
        args.append(f"{ctype} eps")
    args += [f"{ctype}* {o}" for o in outs]
    args.append("size_t n")
    return f"int {prefix}{name}_{tag}({', '.join(args)})"


def cite(ref):
    return ref if ("SURVEY" in ref or ".py:" in ref.split(";")[0].split(",")[0] and not ref[0].isdigit()) else f"thermo/array/thermo.py:{ref}"


def gen_header():
    out = [HEADER_TOP]
    for name, functor, ins, outs, ints, has_eps, ref, group in OPS:
        enums = "; ".join(f"{p[0]}: {p[1]}" for p in ints)
        out.append(f"/* {name}: reference {cite(ref)}" + (f" [{enums}]" if enums else "") + " */")
        for tag, ctype in DTYPES:
            out.append("EKM_API " + proto(name, ins, outs, ints, has_eps, tag, ctype) + ";")
        out.append("")
    out.append(HEADER_BOTTOM)
    return "\n".join(out)


def dispatch(functor, ints, call):
    """Nested switch over the enum parameters -> template arguments."""
    if not ints:
        return f"  return {call(functor)};\n"
    if len(ints) == 1:
        (pn, _, cnt), = ints
        s = f"  switch ({pn}) {{\n"
        for v in range(cnt):
            s += f"    case {v}: return {call(f'{functor}<{v}>')};\n"
        s += f'    default: return ekm::set_error(EKM_ERR_ENUM, "{pn}=%d is not a valid value", {pn});\n  }}\n'
        return s
    (p1, _, c1), (p2, _, c2) = ints
    s = f"  switch ({p1} * 8 + {p2}) {{\n"
    for a in range(c1):
        for b in range(c2):
            s += f"    case {a * 8 + b}: return {call(f'{functor}<{a}, {b}>')};\n"
    s += (f'    default: return ekm::set_error(EKM_ERR_ENUM, "{p1}=%d / {p2}=%d is not a valid combination", '
          f"{p1}, {p2});\n  }}\n")
    return s


def gen_entries(group, dtype):
    out = ["// GENERATED by tools/gen_abi.py -- do not edit.\n", '#include "../map_kernel.hpp"\n\n', 'extern "C" {\n\n']
    for name, functor, ins, outs, ints, has_eps, ref, g in OPS:
        if g != group:
            continue
        for tag, ctype in (dtype,):
            out.append(proto(name, ins, outs, ints, has_eps, tag, ctype) + " {\n")
            out.append(f"  const ekm_operand* ins_[] = {{{', '.join(ins)}}};\n")
            out.append(f"  void* outs_[] = {{{', '.join(outs)}}};\n")
            rp = "eps" if has_eps else "0.0"
            if has_eps:
                out.append(f'  if (!(eps > 0)) return ekm::set_error(EKM_ERR_ARG, "{name}(): eps=%g must be > 0", (double)eps);\n')
            out.append(dispatch(functor, ints, lambda f: f"ekm::launch_map<ekm::{f}, {ctype}>(dev, stream, ins_, outs_, n, {rp})"))
            out.append("}\n\n")
    out.append('}  // extern "C"\n')
    return "".join(out)


def gen_host_entries():
    out = ["// GENERATED by tools/gen_abi.py -- do not edit.  Host twin (test infrastructure).\n\n"]
    for name, functor, ins, outs, ints, has_eps, ref, g in OPS:
        for tag, ctype in DTYPES:
            args = [f"const {ctype}* {i}" for i in ins] + [f"int {p[0]}" for p in ints]
            if has_eps:
                args.append(f"{ctype} eps")
            args += [f"{ctype}* {o}" for o in outs] + ["size_t n"]
            out.append(f'extern "C" int ekm_host_{name}_{tag}({", ".join(args)}) {{\n')
            out.append(f"  const {ctype}* ins_[] = {{{', '.join(ins)}}};\n")
            out.append(f"  {ctype}* outs_[] = {{{', '.join(outs)}}};\n")
            rp = "eps" if has_eps else "0.0"
            out.append(dispatch(functor, ints, lambda f: f"host_map<ekm::{f}, {ctype}>(ins_, outs_, n, {rp})").replace(
                "ekm::set_error(EKM_ERR_ENUM, ", "host_bad_enum(").replace("EKM_ERR_ENUM", "-3"))
            out.append("}\n\n")
    return "".join(out)


def gen_optable():
    out = ['"""GENERATED by tools/gen_abi.py -- ctypes signature table of libekm_thermo.so."""\n\n',
           "# name: (inputs, outputs, int parameters, has_eps)\nOPS = {\n"]
    for name, functor, ins, outs, ints, has_eps, ref, g in OPS:
        out.append(f"    {name!r}: ({tuple(ins)!r}, {tuple(outs)!r}, {tuple(p[0] for p in ints)!r}, {has_eps}),\n")
    out.append("}\n")
    return "".join(out)


def write(path, text):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)


def main():
    write(os.path.join(ROOT, "include", "ekm_thermo.h"), gen_header())
    gen = os.path.join(ROOT, "earthkit-meteo_amd", "csrc", "gen")
    for group in sorted({o[7] for o in OPS}):
        for dtype in DTYPES:
            write(os.path.join(gen, f"entries_{group}_{dtype[0]}.hip"), gen_entries(group, dtype))
    write(os.path.join(gen, "host_entries.inc"), gen_host_entries())
    write(os.path.join(ROOT, "earthkit-meteo_amd", "ekm_hip", "_optable.py"), gen_optable())
    print("generated", len(OPS), "ops x", len(DTYPES), "dtypes")


if __name__ == "__main__":
    main()
