#!/usr/bin/env python3
"""Times the reduce family (ekm_regimes_project_*, ekm_pearson_*) on one GPU and writes profiles/regimes_bench.json.

project  P = 7 patterns on a 91 x 121 grid (K = 11 011): a batch of 51 x 46 fields (members x steps), and a batch of
         about 1 GiB of fields (the small batch repeated); f32 and f64.  Byte model: the field bytes, read ONCE.
pearson  2 M points x m = 51 with the sample axis not contiguous ([32, 51, 65536]: lane per point), and 32 768 rows x
         m = 4096 with the sample axis contiguous (wave per row); f32 and f64.  Byte model: THREE passes over x and y,
         2 * 3 * m * itemsize per point (passes two and three may hit in cache; the model counts them all the same).
How the GPU timings are taken: tools/_benchlib.py, repeated `--reps` times; min / median / max of the repetitions are
recorded and the median is the headline.  Beside each:
  copy_bytes_per_s   what ekm_stream_mix (one stream in, one out, no arithmetic) reaches on this run's arrays, read plus
                     write, measured the same way; frac_copy_rate = bytes_per_s / copy_bytes_per_s;
  numpy_ms           (project, small batch) the reference's expression, `(field * pattern * weights).sum(axis)` once per
                     pattern, with NumPy on this machine's CPU, and end_to_end_ms, ekm_hip.regimes.project on the same
                     NumPy arrays (upload + kernel + download).

Usage: python tools/bench_regimes.py [--steps 10 --warmup 3 --reps 5 --out profiles/regimes_bench.json]
"""
import os
import statistics
import time

import numpy as np

import _benchlib as bl

PSHAPE, NPAT = (91, 121), 7
K = PSHAPE[0] * PSHAPE[1]
SMALL = 51 * 46


def main():
    ap = bl.parser("regimes_bench.json")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import ekm_hip
    from ekm_hip import _ffi, regimes

    lib, dev, name = bl.open_device()
    result = dict(steps=args.steps, warmup=args.warmup, reps=args.reps, device=name, hbm_peak_bytes_per_s=bl.HBM_PEAK,
                  omp_num_threads=os.environ.get("OMP_NUM_THREADS"), numpy=np.__version__, runs=[])

    with bl.EventTimer(lib, dev, args.steps, args.warmup) as timer:
        def copy_rate(src, dst, nbytes):
            ms = statistics.median(timer.copy([src.ptr], [dst.ptr], nbytes, args.reps))
            return 2 * bl.whole_words(nbytes) / (ms * 1e-3)

        def report(run, times, nbytes, rate):
            ms = statistics.median(times)
            d = bl.derived(ms, nbytes, rate)
            run.update(kernel_ms=ms, kernel_ms_min=min(times), kernel_ms_max=max(times), algorithmic_bytes=nbytes,
                       bytes_per_s=d["bytes_per_s"], copy_bytes_per_s=rate, frac_copy_rate=d["frac_copy_rate"],
                       frac_hbm_peak=d["frac_hbm_peak"])
            bl.emit(result, "runs", run)

        def tiled(block, times):
            """`block` repeated `times` times along a new leading axis, on the device."""
            d_block = ekm_hip.DeviceArray.from_host(block)
            out = ekm_hip.DeviceArray.empty((times,) + block.shape, block.dtype)
            for i in range(times):
                _ffi.check(lib.ekm_d2d(dev, out.ptr + i * block.nbytes, d_block.ptr, block.nbytes, None))
            _ffi.check(lib.ekm_sync(dev))
            d_block.free()
            return out

        rng = np.random.default_rng(1)
        lat = np.cos(np.deg2rad(np.linspace(30.0, 80.0, PSHAPE[0])))[:, None] * np.ones(PSHAPE[1])
        for dtype in (np.float32, np.float64):
            dt = np.dtype(dtype)
            tag = bl.tag(dt)
            fn = getattr(lib, "ekm_regimes_project_" + tag)
            field = rng.normal(0.0, 60.0, (51, 46) + PSHAPE).astype(dt)
            stack = rng.normal(0.0, 1.0, (NPAT,) + PSHAPE).astype(dt)
            weights = lat.astype(dt)
            coef = ekm_hip.DeviceArray.from_host((stack * (weights / weights.sum())).reshape(NPAT, K))
            repeat = max(1, (1 << 30) // field.nbytes)
            for case, nf, d_field in (("project_51x46_fields", SMALL, ekm_hip.DeviceArray.from_host(field)),
                                      ("project_1GiB_of_fields", SMALL * repeat, tiled(field, repeat))):
                out = ekm_hip.DeviceArray.empty((NPAT, nf), dt)
                scratch = ekm_hip.DeviceArray.empty((nf, K), dt)
                rate = copy_rate(d_field, scratch, d_field.nbytes)
                scratch.free()
                times = timer.repeated(lambda: _ffi.check(fn(dev, None, d_field.ptr, nf, K, coef.ptr, NPAT, 0, None, out.ptr)), args.reps)
                run = dict(case=case, dtype=tag, fields=nf, k=K, patterns=NPAT)
                if nf == SMALL:
                    pats = regimes.ConstantPatterns([f"R{i}" for i in range(NPAT)], {"area": [90, 0, 0, 120], "grid": [1, 1]}, stack)
                    wn = weights / weights.sum()
                    t0 = time.perf_counter()
                    for p in range(NPAT):
                        (field * stack[p] * wn).sum(axis=(-2, -1))
                    run["numpy_ms"] = (time.perf_counter() - t0) * 1e3
                    regimes.project(field, pats, weights)  # the first call uploads the coefficients
                    t0 = time.perf_counter()
                    regimes.project(field, pats, weights)
                    run["end_to_end_ms"] = (time.perf_counter() - t0) * 1e3
                report(run, times, d_field.nbytes, rate)
                _ffi.check(lib.ekm_sync(dev))
                d_field.free(), out.free()
            # pearson
            fn = getattr(lib, "ekm_pearson_" + tag)
            for case, block, times_tiled, layout in (("pearson_2M_points_m51_lane_per_point", (51, 65536), 32, (32, 51, 65536)),
                                                     ("pearson_32768_rows_m4096_wave_per_row", (2048, 4096), 16, (32768, 4096, 1))):
                xb = (280.0 + rng.normal(0.0, 5.0, block)).astype(dt)
                yb = (0.5 * (xb - 280.0) + rng.normal(0.0, 1.0, block)).astype(dt)
                x, y = tiled(xb, times_tiled), tiled(yb, times_tiled)
                outer, m, inner = layout
                out = ekm_hip.DeviceArray.empty((outer * inner,), dt)
                rate = copy_rate(x, y, x.nbytes)
                y.free()
                y = tiled(yb, times_tiled)  # (the copy wrote over y)
                times = timer.repeated(lambda: _ffi.check(fn(dev, None, x.ptr, y.ptr, outer, m, inner, out.ptr)), args.reps)
                report(dict(case=case, dtype=tag, points=outer * inner, m=m, passes=3), times, 2 * 3 * m * dt.itemsize * outer * inner, rate)
                _ffi.check(lib.ekm_sync(dev))
                x.free(), y.free(), out.free()
    bl.write(args.out, result)


if __name__ == "__main__":
    main()
