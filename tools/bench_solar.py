#!/usr/bin/env python3
"""Times the solar kernel (ekm_solar_*) on one GPU and writes profiles/solar_bench.json.

Points: `--npts` (default 2^21) and a 0.1-degree global grid (1801 x 3600 = 6 483 600 points), random latitudes in
[-90, 90] and longitudes in [-180, 180] as full fields, f32 and f64.  Calls: the instantaneous cosine (one node; f32
input gives f64) and the 24 h average at order 3 (72 nodes; the result in the input dtype).  How the timings are taken:
tools/_benchlib.py.  Beside each kernel time:
  copy_ms   ekm_stream_mix with two streams in and one out of the input arrays' size: a no-arithmetic pass over the
            same arrays (for f32 in -> f64 out the real output is twice that stream);
  numpy_ms  the same call evaluated with plain float64 NumPy on the host, one pass over the points per node as the
            reference evaluates it (`numpy_seconds` below), timed once on the call's own points.

Usage: python tools/bench_solar.py [--steps 10 --warmup 3 --npts 2097152 --out profiles/solar_bench.json]
"""
import ctypes as C
import datetime as dt
import time

import numpy as np

import _benchlib as bl

GRID = 1801 * 3600
DAY = (dt.datetime(2024, 4, 22), dt.datetime(2024, 4, 23))
NOON = dt.datetime(2024, 4, 22, 12)


def numpy_seconds(rec, lat, lon):
    """Plain float64 NumPy, one pass over the points per node, as the reference evaluates it."""
    t0 = time.perf_counter()
    latr = np.deg2rad(lat)
    slat, clat = np.sin(latr), np.cos(latr)
    acc = np.zeros_like(lat)
    for k in range(len(rec["w"])):
        z = rec["sd"][k] * slat + rec["cd"][k] * clat * np.cos(np.deg2rad(rec["h15"][k] + lon + rec["tc"][k]))
        acc += rec["w"][k] * (rec["isr"][k] * np.clip(z, 0.0, None))
    return time.perf_counter() - t0


def main():
    ap = bl.parser("solar_bench.json")
    ap.add_argument("--npts", type=int, default=1 << 21)
    args = ap.parse_args()

    import ekm_hip
    from ekm_hip import _ffi, solar

    lib, dev, name = bl.open_device()
    result = dict(steps=args.steps, warmup=args.warmup, device=name, hbm_peak_bytes_per_s=bl.HBM_PEAK, runs=[])

    with bl.EventTimer(lib, dev, args.steps, args.warmup) as timer:
        dates, weights = solar.node_dates(*DAY)
        records = {"instant": solar.node_records([NOON]), "integrated_24h_order3": solar.node_records(dates, weights)}
        rng = np.random.default_rng(1)

        for npts in (args.npts, GRID):
            lat64, lon64 = rng.uniform(-90, 90, npts), rng.uniform(-180, 180, npts)
            numpy_s = {k: numpy_seconds(r, lat64, lon64) for k, r in records.items()}
            for dtype in (np.float32, np.float64):
                dt_ = np.dtype(dtype)
                lat, lon = ekm_hip.DeviceArray.from_host(lat64.astype(dt_)), ekm_hip.DeviceArray.from_host(lon64.astype(dt_))
                scratch = ekm_hip.DeviceArray.empty((npts,), dt_)
                ops = [_ffi.Operand(a.ptr, _ffi.FIELD, 0, 0, 0) for a in (lat, lon)]
                copy_ms = timer.copy([lat.ptr, lon.ptr], [scratch.ptr], lat.nbytes)
                for what, rec in records.items():
                    out_dt = np.dtype(np.float64) if what == "instant" else dt_
                    entry = "ekm_solar_" + ("f64" if dt_ == np.float64 else "f32_f64" if out_dt == np.float64 else "f32")
                    out = ekm_hip.DeviceArray.empty((npts,), out_dt)
                    nodes = ekm_hip.DeviceArray.from_host(solar.kernel_records(rec))
                    nn = len(rec["w"])
                    fn = getattr(lib, entry)
                    ms = timer.mean(lambda: _ffi.check(fn(dev, None, C.byref(ops[0]), C.byref(ops[1]), nodes.ptr, nn, out.ptr, npts)))
                    nbytes = npts * (2 * dt_.itemsize + out_dt.itemsize)
                    d = bl.derived(ms, nbytes, None, npts)
                    run = dict(dtype=dt_.name, call=what, entry=entry, nnodes=nn, npts=npts, kernel_ms=ms, algorithmic_bytes=nbytes,
                               bytes_per_s=d["bytes_per_s"], frac_hbm_peak=d["frac_hbm_peak"], copy_ms=copy_ms,
                               copy_bytes=3 * lat.nbytes, points_per_s=d["points_per_s"], numpy_ms=numpy_s[what] * 1e3)
                    bl.emit(result, "runs", run)
                    out.free()
                    nodes.free()
                for x in (lat, lon, scratch):
                    x.free()
    bl.write(args.out, result)


if __name__ == "__main__":
    main()
