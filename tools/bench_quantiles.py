#!/usr/bin/env python3
"""Times the per-point quantile kernel (ekm_quantiles_*) on one GPU and writes profiles/quantiles_bench.json.

Field: 51 samples x `--npts` points (default 2^21), zero-clamped gamma data (ties, as precipitation has) from 65 536
distinct columns tiled over the field, once with the sample axis first ([51, npts]) and once with it last ([npts, 51],
the same columns).  How the timings are taken: tools/_benchlib.py.
  first_q101 / first_q5 / first_q1   sample axis first; 101 levels (which=100), five levels (10/25/50/75/90 %), one level;
  last_q101 / last_q5                sample axis last: every lane reads its own contiguous column;
  copy                               ekm_stream_mix, one stream in and one out over the input array: the float4-copy rate
                                     the memory system gives these arrays.
f32 input is timed with method "sort" (f64 result, ekm_quantiles_f32_f64) and, at 101 levels, with "numpy" (f32 result).
Byte model: m * itemsize read and nq * out_itemsize written per point.

Usage: python tools/bench_quantiles.py [--steps 10 --warmup 3 --npts 2097152 --out profiles/quantiles_bench.json]

`--long` times the long-axis kernel (ekm_long_quantiles_*) instead and writes profiles/long_quantiles_bench.json:
m in {256, 512, 1980, 8192} samples, `--gib` GiB of input per case (default 1; a quarter of it at m = 8192), f32 ("sort",
f64 result) and f64, sample axis first and last, which=100; beside each the copy rate of the same array in the same
process, and NumPy's numpy.quantile on one host block of 1024 points.  `crossover`: both kernels on the same arrays at
the short kernel's cap (256 / 128) and below, which is where the advice of ekm_hip/stats.py comes from.
"""
import time

import numpy as np

import _benchlib as bl

M, DISTINCT = 51, 1 << 16
FIVE = [0.1, 0.25, 0.5, 0.75, 0.9]


LONG_MS = (256, 512, 1980, 8192)
CROSS_MS = {"f32": (32, 64, 128, 256), "f64": (32, 64, 128)}
BLOCK = 1024  # distinct columns, tiled over the field; also NumPy's host block


def long_main(args):
    import ekm_hip
    from ekm_hip import _ffi, stats

    lib, dev, name = bl.open_device()
    result = dict(steps=args.steps, warmup=args.warmup, device=name, gib=args.gib, hbm_peak_bytes_per_s=bl.HBM_PEAK, runs=[],
                  crossover=[])
    qs = stats.quantile_levels(100)
    with bl.EventTimer(lib, dev, args.steps, args.warmup) as timer:
        rng = np.random.default_rng(1)
        for dtype in (np.float32, np.float64):
            dt = np.dtype(dtype)
            tag = bl.tag(dt)
            entry = "f64" if tag == "f64" else "f32_f64"
            for m in sorted(set(LONG_MS) | set(CROSS_MS[tag])):
                timed_long = m in LONG_MS and m * dt.itemsize <= 65536
                gib = args.gib * (0.25 if m >= 8192 else 1.0) * (1.0 if timed_long else 0.25)
                npts = max(BLOCK, int(gib * 2 ** 30 / (m * dt.itemsize)) // BLOCK * BLOCK)
                base = np.maximum(rng.gamma(1.5, 2.0, (m, BLOCK)) - 1.0, 0.0).astype(dt)
                host_s = None
                if timed_long:
                    t0 = time.perf_counter()
                    np.quantile(base, qs, axis=0)
                    host_s = time.perf_counter() - t0
                tabs = [ekm_hip.DeviceArray.from_host(t) for t in stats.quantile_positions("sort", m, qs, dt)]
                out = ekm_hip.DeviceArray.empty((101, npts), np.float64)
                scratch = ekm_hip.DeviceArray.empty((m, npts), dt)
                nbytes = (m * dt.itemsize + 101 * 8) * npts
                for layout in ("first", "last"):
                    arr = ekm_hip.DeviceArray.empty((m, npts) if layout == "first" else (npts, m), dt)
                    if layout == "first":
                        row = np.empty(npts, dt)
                        for k in range(m):
                            row.reshape(-1, BLOCK)[:] = base[k]
                            arr.flat_slice(k * npts, (k + 1) * npts).copy_from_host(row)
                    else:
                        block = np.ascontiguousarray(base.T)
                        for r in range(npts // BLOCK):
                            arr.flat_slice(r * block.size, (r + 1) * block.size).copy_from_host(block)
                    outer, inner = (1, npts) if layout == "first" else (npts, 1)
                    copy_rate = 2 * arr.nbytes / (timer.copy([arr.ptr], [scratch.ptr], arr.nbytes) * 1e-3)

                    def launch_of(family):
                        fn = getattr(lib, family + entry)
                        return lambda: _ffi.check(fn(dev, None, arr.ptr, outer, m, inner, tabs[0].ptr, tabs[1].ptr, tabs[2].ptr,
                                                     101, 0, out.ptr))

                    long_ms = timer.mean(launch_of("ekm_long_quantiles_"))
                    if timed_long:
                        bl.emit(result, "runs", dict(dtype=tag, m=m, npts=npts, axis=layout, method="sort", kernel_ms=long_ms,
                                                     algorithmic_bytes=nbytes, numpy_host_s_per_1024_points=host_s,
                                                     **bl.derived(long_ms, nbytes, copy_rate, npts)))
                    if m in CROSS_MS[tag]:
                        short_ms = timer.mean(launch_of("ekm_quantiles_"))
                        bl.emit(result, "crossover", dict(dtype=tag, m=m, npts=npts, axis=layout, long_kernel_ms=long_ms,
                                                          short_kernel_ms=short_ms, long_over_short=long_ms / short_ms))
                    _ffi.check(lib.ekm_sync(dev))
                    arr.free()
                for x in (out, scratch, *tabs):
                    x.free()
    bl.write(args.out, result)


def main():
    ap = bl.parser("quantiles_bench.json")
    ap.add_argument("--npts", type=int, default=1 << 21)
    ap.add_argument("--long", action="store_true", help="the long-axis kernel: writes profiles/long_quantiles_bench.json")
    ap.add_argument("--gib", type=float, default=1.0, help="--long: GiB of input per case")
    args = ap.parse_args()
    if args.long:
        if args.out.endswith("quantiles_bench.json") and not args.out.endswith("long_quantiles_bench.json"):
            args.out = args.out[:-len("quantiles_bench.json")] + "long_quantiles_bench.json"
        return long_main(args)

    import ekm_hip
    from ekm_hip import _ffi, stats

    lib, dev, name = bl.open_device()
    npts = args.npts
    assert npts % DISTINCT == 0, "--npts must be a multiple of 65536"
    reps = npts // DISTINCT
    result = dict(m=M, npts=npts, steps=args.steps, warmup=args.warmup, device=name, hbm_peak_bytes_per_s=bl.HBM_PEAK, runs=[])

    with bl.EventTimer(lib, dev, args.steps, args.warmup) as timer:
        rng = np.random.default_rng(1)
        base = np.maximum(rng.gamma(1.5, 2.0, (M, DISTINCT)) - 1.0, 0.0)

        for dtype in (np.float32, np.float64):
            dt = np.dtype(dtype)
            tag = bl.tag(dt)
            first = ekm_hip.DeviceArray.empty((M, npts), dt)
            for k in range(M):
                first.flat_slice(k * npts, (k + 1) * npts).copy_from_host(np.tile(base[k], reps).astype(dt))
            last = ekm_hip.DeviceArray.empty((npts, M), dt)
            block = np.ascontiguousarray(base.T.astype(dt))
            for r in range(reps):
                last.flat_slice(r * block.size, (r + 1) * block.size).copy_from_host(block)
            scratch = ekm_hip.DeviceArray.empty((M, npts), dt)
            out = ekm_hip.DeviceArray.empty((101, npts), np.float64)

            def tables(method, which):
                qs = stats.quantile_levels(which)
                return [ekm_hip.DeviceArray.from_host(t) for t in stats.quantile_positions(method, M, qs, dt)], int(qs.size)

            def launch_of(arr, outer, inner, method, which):
                tabs, nq = tables(method, which)
                entry = "ekm_quantiles_" + ("f32" if (tag == "f32" and method == "numpy") else "f64" if tag == "f64" else "f32_f64")
                fn, mode = getattr(lib, entry), 0 if method == "sort" else 1
                out_item = 4 if entry.endswith("_f32") else 8
                return (lambda: _ffi.check(fn(dev, None, arr.ptr, outer, M, inner, tabs[0].ptr, tabs[1].ptr, tabs[2].ptr, nq, mode,
                                              out.ptr))), (M * dt.itemsize + nq * out_item) * npts, tabs

            copy_rate = 2 * first.nbytes / (timer.copy([first.ptr], [scratch.ptr], first.nbytes) * 1e-3)

            cases = [("first_q101", first, 1, npts, "sort", 100), ("first_q5", first, 1, npts, "sort", FIVE),
                     ("first_q1", first, 1, npts, "sort", [0.9])]
            if tag == "f32":
                cases.append(("first_q101_numpy", first, 1, npts, "numpy", 100))
            cases += [("last_q101", last, npts, 1, "sort", 100), ("last_q5", last, npts, 1, "sort", FIVE)]
            keep = []
            for what, arr, outer, inner, method, which in cases:
                launch, nbytes, tabs = launch_of(arr, outer, inner, method, which)
                keep.append(tabs)
                ms = timer.mean(launch)
                bl.emit(result, "runs", dict(dtype=tag, case=what, method=method, kernel_ms=ms, algorithmic_bytes=nbytes,
                                             **bl.derived(ms, nbytes, copy_rate, npts)))
            _ffi.check(lib.ekm_sync(dev))
            for x in (first, last, scratch, out):
                x.free()
    bl.write(args.out, result)


if __name__ == "__main__":
    main()
