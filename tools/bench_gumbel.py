#!/usr/bin/env python3
"""Times the Gumbel kernels (ekm_gumbel_fit_*, ekm_gumbel_cdf_f64) on one GPU and writes profiles/gumbel_bench.json.

Field: 721 x 1440 points (a 0.25-degree global grid).  `fit` runs on 51 and on 86 annual maxima per point (Gumbel
distributed, from 65 536 distinct columns tiled over the field), sample axis first, f32 and f64; `cdf` on the fitted
parameters at 1 and at 8 levels, as the cdf and as the return period.  How the GPU timings are taken: tools/_benchlib.py.
Beside each time:
  copy_ms_same_bytes   the time ekm_stream_mix (one stream in, one out, no arithmetic) needs for the same number of bytes
                       at the rate it reaches on this run's arrays;
  numpy_ms             the reference's arithmetic with NumPy on the host, once: sort and the two running sums for `fit`
                       (the polyfill's loop without its unused third sum), the two exponentials for `cdf`.
Byte model: fit reads m * itemsize and writes 16 B per point; cdf reads 16 B and writes 8 * nx B per point.

`--long` times GumbelDistribution.long_fit instead and merges two tables into profiles/long_ensemble_bench.json (beside those
of tools/bench_ensemble.py --long), sample axis first:
  fit_crossover    f32 and f64 at 2^20 points, 32 / 51 / 64 / 128 / 256 samples: ekm_long_gumbel_fit_* and ekm_gumbel_fit_* on
                   the same array (the short one refuses 256 samples in f64: null);
  fit_beyond_cap   512 and 1980 samples at 2^16 points: ekm_long_gumbel_fit_*, ekm_long_quantiles_* with one level on the same
                   array (the same load and sort: the difference is the serial read-out), and `numpy_fit` on the host, once.

Usage: python tools/bench_gumbel.py [--steps 10 --warmup 3 --out profiles/gumbel_bench.json]
       python tools/bench_gumbel.py --long [--steps 5 --warmup 2 --out profiles/long_ensemble_bench.json]
"""
import os
import time

import numpy as np

import _benchlib as bl

NPTS, DISTINCT = 721 * 1440, 1 << 16
LN2 = 0.6931471805599453


def numpy_fit(sample):
    s = np.sort(sample, axis=0)
    s0, s1 = np.zeros(s.shape[1:], s.dtype), np.zeros(s.shape[1:], s.dtype)
    for i in range(s.shape[0]):
        s0 = s0 + s[i]
        s1 = s1 + s[i] * i
    n = float(s.shape[0])
    b0, b1 = s0 / n, s1 / (n * (n - 1.0))
    sigma = (-1.0 * b0 + 2.0 * b1) / np.log(2)
    return b0 - sigma * 0.5772, sigma


def long_main(args):
    import ekm_hip
    from ekm_hip import _ffi

    lib, dev, name = bl.open_device()
    result = dict(fit_crossover=[], fit_beyond_cap=[])
    short_cap = {"f32": 256, "f64": 128}
    with bl.EventTimer(lib, dev, args.steps, args.warmup) as timer:
        base = np.random.default_rng(1).gumbel(20.0, 5.0, (1980, DISTINCT))
        for dtype in (np.float32, np.float64):
            dt = np.dtype(dtype)
            tag = bl.tag(dt)
            for key, npts, counts in (("fit_crossover", 1 << 20, (32, 51, 64, 128, 256)), ("fit_beyond_cap", 1 << 16, (512, 1980))):
                sample = bl.tiled_rows(base[:max(counts)], npts, dt)  # m rows: a prefix
                mu, sigma = ekm_hip.DeviceArray.empty((npts,), np.float64), ekm_hip.DeviceArray.empty((npts,), np.float64)
                out = ekm_hip.DeviceArray.empty((npts,), dt)
                for m in counts:
                    def fit(family):
                        fn = getattr(lib, family + tag)
                        return lambda: _ffi.check(fn(dev, None, sample.ptr, 1, m, npts, mu.ptr, sigma.ptr))
                    run = dict(dtype=tag, function="fit", nens=m, npts=npts, long_ms=timer.mean(fit("ekm_long_gumbel_fit_")))
                    if key == "fit_crossover":
                        run["short_ms"] = timer.mean(fit("ekm_gumbel_fit_")) if m <= short_cap[tag] else None
                    else:
                        sort_launch, keep = bl.one_level_long_quantiles(lib, dev, sample, m, npts, out)
                        run["long_quantiles_one_level_ms"] = timer.mean(sort_launch)
                        host = sample.to_host()[:m]
                        t0 = time.perf_counter()
                        numpy_fit(host)
                        run["numpy_ms"] = (time.perf_counter() - t0) * 1e3
                        del keep
                    bl.emit(result, key, run)
                for x in (sample, mu, sigma, out):
                    x.free()
    bl.merge(args.out, result)


def main():
    ap = bl.parser("gumbel_bench.json")
    ap.add_argument("--long", action="store_true", help="time GumbelDistribution.long_fit (module docstring)")
    args = ap.parse_args()
    if args.long:
        if args.out.endswith("gumbel_bench.json"):
            args.out = os.path.join(os.path.dirname(args.out), "long_ensemble_bench.json")
        return long_main(args)

    import ekm_hip
    from ekm_hip import _ffi

    lib, dev, name = bl.open_device()
    result = dict(npts=NPTS, steps=args.steps, warmup=args.warmup, device=name, hbm_peak_bytes_per_s=bl.HBM_PEAK, runs=[])

    with bl.EventTimer(lib, dev, args.steps, args.warmup) as timer:
        def copy_rate(src, dst, nbytes):
            return 2 * nbytes / (timer.copy([src.ptr], [dst.ptr], nbytes) * 1e-3)

        def report(run, ms, nbytes, rate):
            bl.emit(result, "runs", dict(run, kernel_ms=ms, algorithmic_bytes=nbytes, **bl.derived(ms, nbytes, rate, NPTS)))

        rng = np.random.default_rng(1)
        mu = ekm_hip.DeviceArray.empty((NPTS,), np.float64)
        sigma = ekm_hip.DeviceArray.empty((NPTS,), np.float64)
        for m in (51, 86):
            base = rng.gumbel(20.0, 5.0, (m, DISTINCT))
            pick = np.arange(NPTS) % DISTINCT
            for dtype in (np.float32, np.float64):
                dt = np.dtype(dtype)
                tag = bl.tag(dt)
                host = np.ascontiguousarray(base[:, pick].astype(dt))
                sample = ekm_hip.DeviceArray.from_host(host)
                scratch = ekm_hip.DeviceArray.empty((m, NPTS), dt)
                rate = copy_rate(sample, scratch, sample.nbytes)
                fn = getattr(lib, "ekm_gumbel_fit_" + tag)
                ms = timer.mean(lambda: _ffi.check(fn(dev, None, sample.ptr, 1, m, NPTS, mu.ptr, sigma.ptr)))
                t0 = time.perf_counter()
                numpy_fit(host)
                numpy_ms = (time.perf_counter() - t0) * 1e3
                report(dict(case=f"fit_m{m}", dtype=tag, numpy_ms=numpy_ms), ms, (m * dt.itemsize + 16) * NPTS, rate)
                _ffi.check(lib.ekm_sync(dev))
                sample.free(), scratch.free()
        # cdf on the parameters the last fit left (86 samples, f64)
        h_mu, h_sigma = mu.to_host(), sigma.to_host()
        out = ekm_hip.DeviceArray.empty((8, NPTS), np.float64)
        scratch = ekm_hip.DeviceArray.empty((8, NPTS), np.float64)
        rate = copy_rate(out, scratch, out.nbytes)
        for nx in (1, 8):
            levels = np.linspace(25.0, 60.0, nx)
            d_levels = ekm_hip.DeviceArray.from_host(levels)
            t0 = time.perf_counter()
            with np.errstate(all="ignore"):
                1.0 - np.exp(-np.exp((h_mu - levels[:, None]) / h_sigma))
            numpy_ms = (time.perf_counter() - t0) * 1e3
            for what, mode in (("cdf", 0), ("return_period", 1)):
                ms = timer.mean(lambda: _ffi.check(lib.ekm_gumbel_cdf_f64(dev, None, mu.ptr, sigma.ptr, NPTS, d_levels.ptr, nx, 1.0, mode, out.ptr)))
                report(dict(case=f"{what}_nx{nx}", dtype="f64", numpy_ms=numpy_ms), ms, (16 + 8 * nx) * NPTS, rate)
            _ffi.check(lib.ekm_sync(dev))
    bl.write(args.out, result)


if __name__ == "__main__":
    main()
