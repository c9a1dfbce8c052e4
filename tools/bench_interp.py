#!/usr/bin/env python3
"""Times the vertical interpolation kernels on one GPU and writes profiles/interp_bench.json.

Field: 3600 x 1800 columns x 137 levels (the benchmark field of bench.py), surface pressure 520-1040 hPa, pressure
targets: the 10 mandatory and the 37 standard pressure levels.  How the timings are taken: tools/_benchlib.py.
  fused       ekm_interpolate_hybrid_to_pressure_*: p formed in the kernel;
  two_step    ekm_pressure_on_hybrid_levels_* writing p, then ekm_interpolate_monotonic_* reading it (the sanity
              relation: the fused kernel should beat it);
  generic     ekm_interpolate_monotonic_* alone, the coordinate streamed as a field;
  copy        ekm_stream_mix, one stream in and one out over the bytes of the interpolation's output: the float4-copy
              rate the memory system gives these arrays.
Algorithmic bytes of the fused kernel per output point: 2 data elements read + 1 written, + sp once per column:
  bytes = itemsize * (3 * ntarget * npts + npts);   the generic kernel reads the two bracketing coordinates as well:
  bytes = itemsize * (5 * ntarget * npts)           (its bisection probes are not counted).
`--reference PATH --slab-columns N`: also times the reference's interpolate_hybrid_to_pressure_levels (NumPy) on a slab
of N columns split over `--workers` processes, for the speed-up's denominator; needs the reference checkout.

Usage: python tools/bench_interp.py [--steps 10 --warmup 3 --nx 3600 --ny 1800 --out profiles/interp_bench.json]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

import _benchlib as bl

P10 = [1000, 925, 850, 700, 500, 400, 300, 250, 200, 100]
P37 = [1000, 975, 950, 925, 900, 875, 850, 825, 800, 775, 750, 700, 650, 600, 550, 500, 450, 400, 350, 300, 250, 225, 200,
       175, 150, 125, 100, 70, 50, 30, 20, 10, 7, 5, 3, 2, 1]


def _ref_slab(args):
    path, standin, ncol, seed = args
    sys.path[:0] = [standin, os.path.join(path, "src")]
    from earthkit.meteo.vertical import array as ref

    rng = np.random.default_rng(seed)
    A, B = ref.hybrid_level_parameters(137)
    sp = rng.uniform(52000.0, 104000.0, ncol).astype(np.float32)
    data = rng.uniform(200.0, 300.0, (137, ncol)).astype(np.float32)
    tp = 100.0 * np.asarray(P37, dtype=np.float32)
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        ref.interpolate_hybrid_to_pressure_levels(data, tp, A.astype(np.float32), B.astype(np.float32), sp)
    return time.perf_counter() - t0


def reference_time(path, ncol, workers):
    import multiprocessing as mp

    standin = os.path.join(bl.ROOT, "tests", "golden", "_standin")
    per = ncol // workers
    t0 = time.perf_counter()
    with mp.get_context("spawn").Pool(workers) as pool:
        pool.map(_ref_slab, [(path, standin, per, 0)] * workers)  # import + page faults
        t0 = time.perf_counter()
        legs = pool.map(_ref_slab, [(path, standin, per, i + 1) for i in range(workers)])
        wall = time.perf_counter() - t0
    return dict(columns=per * workers, workers=workers, host_cpus=os.cpu_count(), wall_s=wall, slowest_leg_s=max(legs), points_per_s=per * workers * 37 / wall,
                what="reference interpolate_hybrid_to_pressure_levels, NumPy f32, 37 targets, one slab per process")


def main():
    ap = bl.parser("interp_bench.json")
    ap.add_argument("--nx", type=int, default=3600)
    ap.add_argument("--ny", type=int, default=1800)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--slab-columns", type=int, default=16 * 40500)
    ap.add_argument("--workers", type=int, default=16)
    args = ap.parse_args()

    result = dict(field=[137, args.ny, args.nx], steps=args.steps, warmup=args.warmup, hbm_peak_bytes_per_s=bl.HBM_PEAK, runs=[])
    if args.reference:
        result["reference_numpy"] = reference_time(args.reference, args.slab_columns, args.workers)
        if os.path.exists(args.out):  # keep the GPU numbers of an earlier run
            with open(args.out) as f:
                old = json.load(f)
            old["reference_numpy"] = result["reference_numpy"]
            result = old
        bl.write(args.out, result)
        print(json.dumps(result["reference_numpy"]))
        return

    import ekm_hip
    from ekm_hip import _ffi
    from ekm_hip.vertical import hybrid_level_parameters

    lib, dev, result["device"] = bl.open_device()
    npts, nlev = args.nx * args.ny, 137
    A64, B64 = hybrid_level_parameters(137)
    rng = np.random.default_rng(1)

    def part(nbytes, ms, copy_rate, **more):
        d = bl.derived(ms, nbytes, copy_rate)
        return dict(algorithmic_bytes=nbytes, bytes_per_s=d["bytes_per_s"], frac_hbm_peak=d["frac_hbm_peak"],
                    frac_copy_rate=d["frac_copy_rate"], **more)

    with bl.EventTimer(lib, dev, args.steps, args.warmup) as timer:
        for dtype, targets in ((np.float32, (P10, P37)), (np.float64, (P37,))):
            dt = np.dtype(dtype)
            tag, real = bl.tag(dt), C.c_float if dt == np.float32 else C.c_double
            d_a, d_b = (ekm_hip.DeviceArray.from_host(x.astype(dt)) for x in (A64, B64))
            d_sp = ekm_hip.DeviceArray.from_host(rng.uniform(52000.0, 104000.0, npts).astype(dt))
            data = ekm_hip.DeviceArray.empty((nlev, npts), dt)
            level = rng.uniform(200.0, 300.0, npts).astype(dt)
            for k in range(nlev):  # one random level, shifted per level: the values do not matter to the timing, the bracket does
                data.flat_slice(k * npts, (k + 1) * npts).copy_from_host(level + dt.type(k))
            p = ekm_hip.DeviceArray.empty((nlev, npts), dt)
            for tp in targets:
                nt = len(tp)
                d_t = ekm_hip.DeviceArray.from_host(100.0 * np.asarray(tp, dtype=dt))
                out = ekm_hip.DeviceArray.empty((nt, npts), dt)
                null = None
                fused = lambda: _ffi.check(getattr(lib, f"ekm_interpolate_hybrid_to_pressure_{tag}")(  # noqa: E731
                    dev, None, data.ptr, d_a.ptr, d_b.ptr, d_sp.ptr, d_t.ptr, 0, nt, npts, nlev, 0, 0, null, null, null, null, 0, out.ptr))
                pressure = lambda: _ffi.check(getattr(lib, f"ekm_pressure_on_hybrid_levels_{tag}")(  # noqa: E731
                    dev, None, d_a.ptr, d_b.ptr, d_sp.ptr, npts, nlev, None, None, 1, real(float(np.log(2))), p.ptr, None, None, None))
                generic = lambda: _ffi.check(getattr(lib, f"ekm_interpolate_monotonic_{tag}")(  # noqa: E731
                    dev, None, data.ptr, p.ptr, 1, d_t.ptr, 0, nt, npts, nlev, 0, 0, null, null, null, null, 0, out.ptr))
                pressure()
                ms = dict(fused=timer.mean(fused), generic=timer.mean(generic), two_step=timer.mean(lambda: (pressure(), generic())),
                          copy=timer.copy([data.ptr], [out.ptr], out.nbytes))
                copy_rate = 2 * out.nbytes / (ms["copy"] * 1e-3)
                run = dict(dtype=tag, ntarget=nt, kernel_ms=ms, copy_bytes_per_s=copy_rate,
                           fused=part(dt.itemsize * (3 * nt * npts + npts), ms["fused"], copy_rate,
                                      output_points_per_s=nt * npts / (ms["fused"] * 1e-3)),
                           generic=part(dt.itemsize * 5 * nt * npts, ms["generic"], copy_rate),
                           fused_over_two_step=ms["fused"] / ms["two_step"])
                bl.emit(result, "runs", run)
                out.free(), d_t.free()
            for x in (data, p, d_sp, d_a, d_b):
                x.free()
    bl.write(args.out, result)


if __name__ == "__main__":
    main()
