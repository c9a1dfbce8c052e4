#!/usr/bin/env python3
"""Times the per-point quantile kernel (ekm_quantiles_*) on one GPU and writes profiles/quantiles_bench.json.

Field: 51 samples x `--npts` points (default 2^21), zero-clamped gamma data (ties, as precipitation has) from 65 536
distinct columns tiled over the field, once with the sample axis first ([51, npts]) and once with it last ([npts, 51],
the same columns).  Every timing is HIP events around `--steps` launches after `--warmup`, in ONE process on the same
arrays:
  first_q101 / first_q5 / first_q1   sample axis first; 101 levels (which=100), five levels (10/25/50/75/90 %), one level;
  last_q101 / last_q5                sample axis last: every lane reads its own contiguous column;
  copy                               ekm_stream_mix, one stream in and one out over the input array: the float4-copy rate
                                     the memory system gives these arrays.
f32 input is timed with method "sort" (f64 result, ekm_quantiles_f32_f64) and, at 101 levels, with "numpy" (f32 result).
Byte model: m * itemsize read and nq * out_itemsize written per point.

Usage: python tools/bench_quantiles.py [--steps 10 --warmup 3 --npts 2097152 --out profiles/quantiles_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "earthkit-meteo_amd"))

HBM_PEAK = 8.0e12
M, DISTINCT = 51, 1 << 16
FIVE = [0.1, 0.25, 0.5, 0.75, 0.9]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--npts", type=int, default=1 << 21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantiles_bench.json"))
    args = ap.parse_args()

    import ekm_hip
    from ekm_hip import _ffi, stats

    lib, dev = _ffi.lib(), 0
    _ffi.check(lib.ekm_init())
    name = C.create_string_buffer(128)
    lib.ekm_device_name(dev, name, 128)
    npts = args.npts
    assert npts % DISTINCT == 0, "--npts must be a multiple of 65536"
    reps = npts // DISTINCT
    result = dict(m=M, npts=npts, steps=args.steps, warmup=args.warmup, device=name.value.decode(),
                  hbm_peak_bytes_per_s=HBM_PEAK, runs=[])
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        _ffi.check(lib.ekm_event_create(dev, C.byref(e)))

    def timed(launch):
        for _ in range(args.warmup):
            launch()
        _ffi.check(lib.ekm_event_record(dev, ev[0], None))
        for _ in range(args.steps):
            launch()
        _ffi.check(lib.ekm_event_record(dev, ev[1], None))
        _ffi.check(lib.ekm_event_sync(dev, ev[1]))
        ms = C.c_float()
        _ffi.check(lib.ekm_event_elapsed_ms(dev, ev[0], ev[1], C.byref(ms)))
        return ms.value / args.steps

    rng = np.random.default_rng(1)
    base = np.maximum(rng.gamma(1.5, 2.0, (M, DISTINCT)) - 1.0, 0.0)

    for dtype in (np.float32, np.float64):
        dt = np.dtype(dtype)
        tag = "f32" if dt == np.float32 else "f64"
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

        ins, outs = (C.c_void_p * 1)(first.ptr), (C.c_void_p * 1)(scratch.ptr)
        copy_ms = timed(lambda: _ffi.check(lib.ekm_stream_mix(dev, None, ins, 1, outs, 1, first.nbytes)))
        copy_rate = 2 * first.nbytes / (copy_ms * 1e-3)

        cases = [("first_q101", first, 1, npts, "sort", 100), ("first_q5", first, 1, npts, "sort", FIVE),
                 ("first_q1", first, 1, npts, "sort", [0.9])]
        if tag == "f32":
            cases.append(("first_q101_numpy", first, 1, npts, "numpy", 100))
        cases += [("last_q101", last, npts, 1, "sort", 100), ("last_q5", last, npts, 1, "sort", FIVE)]
        keep = []
        for what, arr, outer, inner, method, which in cases:
            launch, nbytes, tabs = launch_of(arr, outer, inner, method, which)
            keep.append(tabs)
            ms = timed(launch)
            rate = nbytes / (ms * 1e-3)
            run = dict(dtype=tag, case=what, method=method, kernel_ms=ms, algorithmic_bytes=nbytes, bytes_per_s=rate,
                       copy_bytes_per_s=copy_rate, copy_ms_same_bytes=nbytes / copy_rate * 1e3,
                       frac_copy_rate=rate / copy_rate, frac_hbm_peak=rate / HBM_PEAK, points_per_s=npts / (ms * 1e-3))
            result["runs"].append(run)
            print(json.dumps(run), flush=True)
        _ffi.check(lib.ekm_sync(dev))
        for x in (first, last, scratch, out):
            x.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
