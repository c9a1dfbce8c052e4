#!/usr/bin/env python3
"""Times ekm_nanaverage_* on one GPU and writes profiles/nanaverage_bench.json.

points  51 x 2 M points, axis 0 ([1, 51, 2097152]: lane per point);
rows    32 768 rows x 4096, the contiguous axis (wave per row);
split   50 rows x 6.5 M (workgroup per chunk of a row, then the chunks in order), the same array with path 2 forced (one
        wave per row: the comparison the split kernel has to win), and axis=None on 1 GiB.
Each in f32 and f64, without weights and with a weight vector along the axis (read through strides, never expanded).
Byte model: the data bytes, read ONCE -- twice by the weighted lane-per-point kernel, which follows the reference's two
passes.  The weight vector and the result are not counted.
How the GPU timings are taken: tools/_benchlib.py, repeated `--reps` times; min / median / max of the repetitions are
recorded and the median is the headline.  Beside each:
  copy_bytes_per_s   what ekm_stream_mix (one stream in, one out, no arithmetic) reaches on this run's array, read plus
                     write, measured the same way; frac_copy_rate = bytes_per_s / copy_bytes_per_s;
  numpy_block_ms     the reference's expressions (numpy.nanmean; ones_like * w, NaN where the datum is NaN, over its
                     nansum, nansum of the products) with NumPy on this machine's CPU on ONE host block, the
                     `numpy_block_fraction`-th part of the device array (the device array is that block repeated).

Usage: python tools/bench_nanaverage.py [--steps 10 --warmup 3 --reps 5 --out profiles/nanaverage_bench.json]
"""
import os
import statistics
import time

import numpy as np

import _benchlib as bl

POINTS, ROWS, SPLIT = 1, 2, 3


def numpy_reference(data, weights, axis):
    with np.errstate(all="ignore"):
        if weights is None:
            return np.nanmean(data, axis=axis)
        tw = np.ones_like(data) * weights
        tw[np.isnan(data)] = np.nan
        den = np.nansum(tw, axis=axis)
        if axis is not None:
            shape = list(tw.shape)
            shape[axis] = 1
            den = den.reshape(shape)
        return np.nansum(data * (tw / den), axis=axis)


def main():
    ap = bl.parser("nanaverage_bench.json")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import ekm_hip
    from ekm_hip import _ffi

    lib, dev, name = bl.open_device()
    result = dict(steps=args.steps, warmup=args.warmup, reps=args.reps, device=name, hbm_peak_bytes_per_s=bl.HBM_PEAK,
                  omp_num_threads=os.environ.get("OMP_NUM_THREADS"), numpy=np.__version__, runs=[])

    with bl.EventTimer(lib, dev, args.steps, args.warmup) as timer:
        def copy_rate(src, dst, nbytes):
            ms = statistics.median(timer.copy([src.ptr], [dst.ptr], nbytes, args.reps))
            return 2 * bl.whole_words(nbytes) / (ms * 1e-3)

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
        # (case, host block, repeats, [outer, m, inner] of the device array, paths, the block's own axis for NumPy)
        shapes = (("points_51_x_2M_axis_0", (51, 1 << 21), 1, (1, 51, 1 << 21), (POINTS,), 0),
                  ("rows_32768_x_4096", (2048, 4096), 16, (32768, 4096, 1), (ROWS,), 1),
                  ("split_50_rows_x_6p5M", (2, 6_500_000), 25, (50, 6_500_000, 1), (SPLIT, ROWS, 0), 1),
                  ("split_axis_none_1GiB", (1 << 24,), None, None, (SPLIT, 0), None))
        for dtype in (np.float32, np.float64):
            dt = np.dtype(dtype)
            tag = bl.tag(dt)
            fn = getattr(lib, "ekm_nanaverage_" + tag)
            for case, bshape, repeat, layout, paths, axis in shapes:
                if repeat is None:  # 1 GiB as one row
                    repeat = (1 << 30) // (bshape[0] * dt.itemsize)
                    layout = (1, bshape[0] * repeat, 1)
                block = (280.0 + rng.normal(0.0, 5.0, bshape)).astype(dt)
                block[rng.uniform(size=bshape) < 0.1] = np.nan
                outer, m, inner = layout
                wvec = np.resize(0.5 + rng.uniform(0.0, 1.0, min(m, 1 << 22)), m).astype(dt)
                data = tiled(block, repeat)
                scratch = ekm_hip.DeviceArray.empty((data.size,), dt)
                rate = copy_rate(data, scratch, data.nbytes)
                scratch.free()
                d_w = ekm_hip.DeviceArray.from_host(wvec)
                out = ekm_hip.DeviceArray.empty((outer * inner,), dt)
                for weighted in (False, True):
                    wb = None
                    if weighted:  # the block's own weights: the part of the vector that lies along the block's axis
                        wb = wvec[:bshape[0], None] if axis == 0 else wvec[:block.shape[-1]]
                    t0 = time.perf_counter()
                    numpy_reference(block, wb, axis)
                    numpy_ms = (time.perf_counter() - t0) * 1e3
                    for path in paths:
                        need = int(lib.ekm_nanaverage_work_bytes(dt.itemsize, outer, m, inner, int(weighted), path))
                        work = ekm_hip.DeviceArray.empty((max(need, 16) // dt.itemsize,), dt)
                        times = timer.repeated(lambda: _ffi.check(fn(dev, None, data.ptr, outer, m, inner, d_w.ptr if weighted else None, 0,
                                                                     1 if weighted else 0, 0, path, work.ptr if need else None, need, out.ptr)),
                                               args.reps)
                        passes = 2 if weighted and inner > 1 else 1
                        ms = statistics.median(times)
                        nbytes = passes * data.nbytes
                        d = bl.derived(ms, nbytes, rate)
                        run = dict(case=case, dtype=tag, weighted=weighted, path=path, outer=outer, m=m, inner=inner, passes=passes,
                                   work_bytes=need, kernel_ms=ms, kernel_ms_min=min(times), kernel_ms_max=max(times), algorithmic_bytes=nbytes,
                                   bytes_per_s=d["bytes_per_s"], copy_bytes_per_s=rate, frac_copy_rate=d["frac_copy_rate"],
                                   frac_hbm_peak=d["frac_hbm_peak"], numpy_block_ms=numpy_ms, numpy_block_fraction=1.0 / repeat)
                        bl.emit(result, "runs", run)
                        _ffi.check(lib.ekm_sync(dev))
                        work.free()
                data.free(), d_w.free(), out.free()
    bl.write(args.out, result)


if __name__ == "__main__":
    main()
