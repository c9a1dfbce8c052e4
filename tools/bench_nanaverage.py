#!/usr/bin/env python3
"""Times ekm_nanaverage_* on one GPU and writes profiles/nanaverage_bench.json.

points  51 x 2 M points, axis 0 ([1, 51, 2097152]: lane per point);
rows    32 768 rows x 4096, the contiguous axis (wave per row);
split   50 rows x 6.5 M (workgroup per chunk of a row, then the chunks in order), the same array with path 2 forced (one
        wave per row: the comparison the split kernel has to win), and axis=None on 1 GiB.
Each in f32 and f64, without weights and with a weight vector along the axis (read through strides, never expanded).
Byte model: the data bytes, read ONCE -- twice by the weighted lane-per-point kernel, which follows the reference's two
passes.  The weight vector and the result are not counted.
Every GPU timing is HIP events around `--steps` launches after `--warmup`, repeated `--reps` times in ONE process on the
same arrays; min / median / max of the repetitions are recorded and the median is the headline.  Beside each:
  copy_bytes_per_s   what ekm_stream_mix (one stream in, one out, no arithmetic) reaches on this run's array, read plus
                     write, measured the same way; frac_copy_rate = bytes_per_s / copy_bytes_per_s;
  numpy_block_ms     the reference's expressions (numpy.nanmean; ones_like * w, NaN where the datum is NaN, over its
                     nansum, nansum of the products) with NumPy on this machine's CPU on ONE host block, the
                     `numpy_block_fraction`-th part of the device array (the device array is that block repeated).

Usage: python tools/bench_nanaverage.py [--steps 10 --warmup 3 --reps 5 --out profiles/nanaverage_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "earthkit-meteo_amd"))

HBM_PEAK = 8.0e12
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nanaverage_bench.json"))
    args = ap.parse_args()

    import ekm_hip
    from ekm_hip import _ffi

    lib, dev = _ffi.lib(), 0
    _ffi.check(lib.ekm_init())
    name = C.create_string_buffer(128)
    lib.ekm_device_name(dev, name, 128)
    result = dict(steps=args.steps, warmup=args.warmup, reps=args.reps, device=name.value.decode(), hbm_peak_bytes_per_s=HBM_PEAK,
                  omp_num_threads=os.environ.get("OMP_NUM_THREADS"), numpy=np.__version__, runs=[])
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _ffi.check(lib.ekm_event_create(dev, C.byref(e)))

    def timed(launch):
        for _ in range(args.warmup):
            launch()
        out = []
        for _ in range(args.reps):
            _ffi.check(lib.ekm_event_record(dev, ev[0], None))
            for _ in range(args.steps):
                launch()
            _ffi.check(lib.ekm_event_record(dev, ev[1], None))
            _ffi.check(lib.ekm_event_sync(dev, ev[1]))
            ms = C.c_float()
            _ffi.check(lib.ekm_event_elapsed_ms(dev, ev[0], ev[1], C.byref(ms)))
            out.append(ms.value / args.steps)
        return out

    def copy_rate(src, dst, nbytes):
        ins, outs = (C.c_void_p * 1)(src.ptr), (C.c_void_p * 1)(dst.ptr)
        nbytes -= nbytes % 16  # ekm_stream_mix copies whole 16-byte words
        ms = statistics.median(timed(lambda: _ffi.check(lib.ekm_stream_mix(dev, None, ins, 1, outs, 1, nbytes))))
        return 2 * nbytes / (ms * 1e-3)

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
        tag = "f32" if dt == np.float32 else "f64"
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
                    times = timed(lambda: _ffi.check(fn(dev, None, data.ptr, outer, m, inner, d_w.ptr if weighted else None, 0,
                                                        1 if weighted else 0, 0, path, work.ptr if need else None, need, out.ptr)))
                    passes = 2 if weighted and inner > 1 else 1
                    ms = statistics.median(times)
                    nbytes = passes * data.nbytes
                    run = dict(case=case, dtype=tag, weighted=weighted, path=path, outer=outer, m=m, inner=inner, passes=passes,
                               work_bytes=need, kernel_ms=ms, kernel_ms_min=min(times), kernel_ms_max=max(times), algorithmic_bytes=nbytes,
                               bytes_per_s=nbytes / (ms * 1e-3), copy_bytes_per_s=rate, frac_copy_rate=nbytes / (ms * 1e-3) / rate,
                               frac_hbm_peak=nbytes / (ms * 1e-3) / HBM_PEAK, numpy_block_ms=numpy_ms, numpy_block_fraction=1.0 / repeat)
                    result["runs"].append(run)
                    print(json.dumps(run), flush=True)
                    _ffi.check(lib.ekm_sync(dev))
                    work.free()
            data.free(), d_w.free(), out.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
