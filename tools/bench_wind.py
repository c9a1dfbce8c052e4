#!/usr/bin/env python3
"""Times the wind kernels (ekm_wind_*, ekm_windrose_*) on one GPU and writes profiles/wind_bench.json.

Elementwise: speed, direction, xy_to_polar, polar_to_xy and coriolis on full fields of a 0.1-degree global grid
(1801 x 3600 = 6 483 600 points) and of `--big` points (default 2^27), f32 and f64.  How the timings are taken:
tools/_benchlib.py.  Beside each kernel time:
  copy_ms   ekm_stream_mix with as many streams in and out as the call has, of the same size: a no-arithmetic pass;
  ratio     kernel_ms / copy_ms;
  numpy_ms  the same call with NumPy on the host in the same dtype (grid size only), timed once.
Wind rose: 16 sectors x 6 speed bins on the grid's points, on a constant field, a smooth field and a uniform-random
one; np.histogram2d of the same samples beside it.

Usage: python tools/bench_wind.py [--steps 10 --warmup 3 --big 134217728 --out profiles/wind_bench.json]
"""
import ctypes as C
import time

import numpy as np

import _benchlib as bl

GRID = 1801 * 3600
DEG = 180.0 / np.pi


def numpy_call(what, a, b):
    t0 = time.perf_counter()
    if what in ("speed", "xy_to_polar"):
        np.hypot(a, b)
    if what in ("direction", "xy_to_polar"):
        d = np.arctan2(b, a)
        m = d <= -np.pi / 2
        d[m] = (-np.pi / 2 - d[m]) * DEG
        m = ~m
        d[m] = (1.5 * np.pi - d[m]) * DEG
    if what == "polar_to_xy":
        ang = (270.0 - b) / DEG
        a * np.cos(ang), a * np.sin(ang)
    if what == "coriolis":
        1.4584230166092124e-4 * np.sin(a / DEG)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = bl.parser("wind_bench.json")
    ap.add_argument("--big", type=int, default=1 << 27)
    args = ap.parse_args()

    import ekm_hip
    from ekm_hip import _ffi, wind

    lib, dev, name = bl.open_device()
    result = dict(steps=args.steps, warmup=args.warmup, device=name.strip() or "gfx950", elementwise=[], windrose=[])

    with bl.EventTimer(lib, dev, args.steps, args.warmup) as timer:
        rng = np.random.default_rng(1)
        # call -> (entry, inputs, mode, outputs wanted)
        calls = {"speed": ("polar", 2, 0, (1, 0)), "direction": ("polar", 2, 0, (0, 1)), "xy_to_polar": ("polar", 2, 0, (1, 1)),
                 "polar_to_xy": ("xy", 2, 0, (1, 1)), "coriolis": ("coriolis", 1, 0, (1, 0))}
        for npts in (GRID, args.big):
            for dtype in (np.float32, np.float64):
                dt_ = np.dtype(dtype)
                host = [rng.normal(0, 12, npts).astype(dt_), rng.uniform(0, 360, npts).astype(dt_)]
                a, b = (ekm_hip.DeviceArray.from_host(x) for x in host)
                o0, o1 = ekm_hip.DeviceArray.empty((npts,), dt_), ekm_hip.DeviceArray.empty((npts,), dt_)
                ops = [_ffi.Operand(x.ptr, _ffi.FIELD, 0, 0, 0) for x in (a, b)]
                copies = {}
                for what, (entry, nin, mode, wanted) in calls.items():
                    nout = sum(wanted)
                    if (nin, nout) not in copies:
                        copies[nin, nout] = timer.copy([a.ptr, b.ptr][:nin], [o0.ptr, o1.ptr][:nout], a.nbytes)
                    fn = getattr(lib, f"ekm_wind_{entry}_" + bl.tag(dt_))
                    p0, p1 = (o0.ptr if wanted[0] else None), (o1.ptr if wanted[1] else None)
                    if entry == "coriolis":
                        ms = timer.mean(lambda: _ffi.check(fn(dev, None, C.byref(ops[0]), p0, npts)))
                    else:
                        ms = timer.mean(lambda: _ffi.check(fn(dev, None, C.byref(ops[0]), C.byref(ops[1]), mode, p0, p1, npts)))
                    nbytes = npts * dt_.itemsize * (nin + nout)
                    run = dict(call=what, dtype=dt_.name, npts=npts, kernel_ms=ms, copy_ms=copies[nin, nout], ratio=ms / copies[nin, nout],
                               algorithmic_bytes=nbytes, bytes_per_s=nbytes / (ms * 1e-3),
                               numpy_ms=numpy_call(what, host[0], host[1]) if npts == GRID else None)
                    bl.emit(result, "elementwise", run)
                for x in (a, b, o0, o1):
                    x.free()

        bins = [0.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0]
        lon = np.linspace(0, 40 * np.pi, GRID)
        fields = {"constant": (np.full(GRID, 5.0), np.full(GRID, 200.0)),
                  "smooth": (10 + 9 * np.sin(lon), 180 + 170 * np.sin(0.37 * lon)),
                  "random": (rng.uniform(0, 64, GRID), rng.uniform(0, 360, GRID))}
        for dtype in (np.float32, np.float64):
            for fname, (sp, di) in fields.items():
                sp, di = sp.astype(dtype), di.astype(dtype)
                t0 = time.perf_counter()
                np.histogram2d(sp, di, bins=list(wind.rose_edges(np.dtype(dtype), 16, bins)))
                numpy_ms = (time.perf_counter() - t0) * 1e3
                d_sp, d_di = ekm_hip.DeviceArray.from_host(sp), ekm_hip.DeviceArray.from_host(di)
                run = dict(field=fname, dtype=np.dtype(dtype).name, npts=GRID, sectors=16, speed_bins=len(bins), numpy_ms=numpy_ms)
                def go():
                    res, db = wind.windrose(d_sp, d_di, sectors=16, speed_bins=bins)
                    res.free(), db.free()
                run["call_ms"] = timer.mean(go)  # (the whole call: memset, count kernel, finish kernel and the copy of the bins)
                bl.emit(result, "windrose", run)
                d_sp.free(), d_di.free()
    bl.write(args.out, result)


if __name__ == "__main__":
    main()
