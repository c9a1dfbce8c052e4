#!/usr/bin/env python3
"""Times the ensemble reduction kernels (efi, sot, crps) on one GPU and writes profiles/ensemble_bench.json.

Field: `--npts` points (default 2^21), 101 climate rows x 51 members, member-major, zero-clamped gamma data (ties, as
precipitation has) from 65 536 distinct columns tiled over the field.  How the timings are taken: tools/_benchlib.py.
  efi    ekm_efi_*            reads (101 + 51) elements, writes 8 B per point (eps <= 0 and eps > 0 arms);
  sot    ekm_sot_*  perc 90   reads 51 + 2 elements, writes one;
  crps   ekm_crps_from_ensemble_*  reads 51 + 1 elements, writes 8 B;
  copy   ekm_stream_mix, one stream in and one out over the ensemble array: the float4-copy rate the memory system
         gives these arrays; `copy_ms_same_bytes` is the time that rate needs for the kernel's algorithmic bytes.

`--long` times the long-axis functions instead (extreme.long_efi, extreme.long_sot, score.long_crps_from_ensemble) and
merges two tables into profiles/long_ensemble_bench.json (tools/bench_gumbel.py --long adds the fit's):
  crossover    f32 and f64 at 2^20 points, 32 / 51 / 64 / 128 / 256 members: the long and the short entry point on the same
               arrays (the short one refuses 256 members in f64: null);
  beyond_cap   512 and 1980 members at 2^16 points: the long entry point, ekm_long_quantiles_* with one level on the same
               ensemble (the same load and sort: the difference is the serial read-out), and the NumPy restatement of
               tests/_ensemble_numpy.py on the host, once.

Usage: python tools/bench_ensemble.py [--steps 10 --warmup 3 --npts 2097152 --out profiles/ensemble_bench.json]
       python tools/bench_ensemble.py --long [--steps 5 --warmup 2 --out profiles/long_ensemble_bench.json]
"""
import os
import sys
import time

import numpy as np

import _benchlib as bl

NCLIM, NENS, DISTINCT = 101, 51, 1 << 16
LONG_CROSSOVER, LONG_BEYOND = (1 << 20, (32, 51, 64, 128, 256)), (1 << 16, (512, 1980))


def long_launches(lib, dev, tag, prefix, clim, ens, y, nens, npts, tabs, wts, out64, out, itemsize):
    """The three launches of family `prefix` ("ekm_" or "ekm_long_") on the first `nens` rows of `ens`."""
    from ekm_hip import _ffi

    row = npts * itemsize
    return dict(
        efi=lambda: _ffi.check(getattr(lib, f"{prefix}efi_{tag}")(dev, None, clim.ptr, ens.ptr, NCLIM, nens, npts, -0.1, tabs[0].ptr,
                                                                 tabs[1].ptr, tabs[2].ptr, out64.ptr)),
        sot=lambda: _ffi.check(getattr(lib, f"{prefix}sot_{tag}")(dev, None, clim.ptr + 90 * row, clim.ptr + 99 * row, ens.ptr, nens,
                                                                 npts, 90, -1e4, out.ptr)),
        crps=lambda: _ffi.check(getattr(lib, f"{prefix}crps_from_ensemble_{tag}")(dev, None, ens.ptr, y.ptr, nens, npts, wts[0].ptr,
                                                                                 wts[1].ptr, out64.ptr, None)))


def long_main(args):
    import ekm_hip
    from ekm_hip import extreme, score

    sys.path.insert(0, os.path.join(bl.ROOT, "tests"))
    import _ensemble_numpy as en  # the restatement the tests hold to the recorded reference

    lib, dev, name = bl.open_device()
    result = dict(device=name, steps=args.steps, warmup=args.warmup, nclim=NCLIM, crossover=[], beyond_cap=[])
    short_cap = {"f32": 256, "f64": 128}
    with bl.EventTimer(lib, dev, args.steps, args.warmup) as timer:
        rng = np.random.default_rng(1)
        base_c = np.sort(np.maximum(rng.gamma(1.5, 2.0, (NCLIM, DISTINCT)) - 1.0, 0.0), axis=0) + np.linspace(0, 0.5, NCLIM)[:, None]
        base_e = np.maximum(rng.gamma(1.5, 2.0, (max(LONG_BEYOND[1]), DISTINCT)) - 1.0, 0.0)
        tabs = [ekm_hip.DeviceArray.from_host(t) for t in extreme.efi_coefficients(NCLIM)]
        for dtype in (np.float32, np.float64):
            dt = np.dtype(dtype)
            tag = bl.tag(dt)
            for key, (npts, members) in (("crossover", LONG_CROSSOVER), ("beyond_cap", LONG_BEYOND)):
                clim, ens = bl.tiled_rows(base_c, npts, dt), bl.tiled_rows(base_e[:max(members)], npts, dt)  # nens rows: a prefix
                y = ekm_hip.DeviceArray.from_host(np.tile(base_e[3], (npts + DISTINCT - 1) // DISTINCT)[:npts].astype(dt))
                out64, out = ekm_hip.DeviceArray.empty((npts,), np.float64), ekm_hip.DeviceArray.empty((npts,), dt)
                for nens in members:
                    wts = [ekm_hip.DeviceArray.from_host(t) for t in score.crps_weights(nens)]
                    common = (clim, ens, y, nens, npts, tabs, wts, out64, out, dt.itemsize)
                    long_ms = {k: timer.mean(f) for k, f in long_launches(lib, dev, tag, "ekm_long_", *common).items()}
                    if key == "crossover":
                        short = long_launches(lib, dev, tag, "ekm_", *common) if nens <= short_cap[tag] else {}
                        for k, ms in long_ms.items():
                            bl.emit(result, key, dict(dtype=tag, function=k, nens=nens, npts=npts, long_ms=ms,
                                                      short_ms=timer.mean(short[k]) if short else None))
                        continue
                    sort_launch, keep = bl.one_level_long_quantiles(lib, dev, ens, nens, npts, out)
                    sort_ms = timer.mean(sort_launch)
                    h_clim, h_ens, h_y = clim.to_host(), ens.to_host()[:nens], y.to_host()
                    host = dict(efi=lambda: en.efi(h_clim, h_ens), sot=lambda: en.sot(h_clim, h_ens, 90), crps=lambda: en.crps(h_ens, h_y))
                    for k, ms in long_ms.items():
                        t0 = time.perf_counter()
                        host[k]()
                        bl.emit(result, key, dict(dtype=tag, function=k, nens=nens, npts=npts, long_ms=ms, long_quantiles_one_level_ms=sort_ms,
                                                  numpy_ms=(time.perf_counter() - t0) * 1e3))
                    del keep
                for x in (clim, ens, y, out64, out):
                    x.free()
    bl.merge(args.out, result)


def main():
    ap = bl.parser("ensemble_bench.json")
    ap.add_argument("--npts", type=int, default=1 << 21)
    ap.add_argument("--long", action="store_true", help="time the long-axis functions (module docstring)")
    args = ap.parse_args()
    if args.long:
        if args.out.endswith("ensemble_bench.json") and not args.out.endswith("long_ensemble_bench.json"):
            args.out = os.path.join(os.path.dirname(args.out), "long_ensemble_bench.json")
        return long_main(args)

    import ekm_hip
    from ekm_hip import _ffi, extreme, score

    lib, dev, name = bl.open_device()
    npts = args.npts
    result = dict(nclim=NCLIM, nens=NENS, npts=npts, steps=args.steps, warmup=args.warmup, device=name,
                  hbm_peak_bytes_per_s=bl.HBM_PEAK, runs=[])

    with bl.EventTimer(lib, dev, args.steps, args.warmup) as timer:
        rng = np.random.default_rng(1)
        base_c = np.sort(np.maximum(rng.gamma(1.5, 2.0, (NCLIM, DISTINCT)) - 1.0, 0.0), axis=0) + np.linspace(0, 0.5, NCLIM)[:, None]
        base_e = np.maximum(rng.gamma(1.5, 2.0, (NENS, DISTINCT)) - 1.0, 0.0)
        reps = (npts + DISTINCT - 1) // DISTINCT
        tabs = [ekm_hip.DeviceArray.from_host(t) for t in extreme.efi_coefficients(NCLIM)]
        wts = [ekm_hip.DeviceArray.from_host(t) for t in score.crps_weights(NENS)]

        for dtype in (np.float32, np.float64):
            dt = np.dtype(dtype)
            tag = bl.tag(dt)

            def field(base, rows):
                d = ekm_hip.DeviceArray.empty((rows, npts), dt)
                for k in range(rows):
                    d.flat_slice(k * npts, (k + 1) * npts).copy_from_host(np.tile(base[k], reps)[:npts].astype(dt))
                return d

            clim, ens = field(base_c, NCLIM), field(base_e, NENS)
            y = ekm_hip.DeviceArray.from_host(np.tile(base_e[3], reps)[:npts].astype(dt))
            scratch = ekm_hip.DeviceArray.empty((NENS, npts), dt)
            out64 = ekm_hip.DeviceArray.empty((npts,), np.float64)
            out = ekm_hip.DeviceArray.empty((npts,), dt)
            row = npts * dt.itemsize
            launches = dict(
                efi=lambda: _ffi.check(getattr(lib, f"ekm_efi_{tag}")(dev, None, clim.ptr, ens.ptr, NCLIM, NENS, npts, -0.1,
                                                                    tabs[0].ptr, tabs[1].ptr, tabs[2].ptr, out64.ptr)),
                efi_eps=lambda: _ffi.check(getattr(lib, f"ekm_efi_{tag}")(dev, None, clim.ptr, ens.ptr, NCLIM, NENS, npts, 1e-4,
                                                                        tabs[0].ptr, tabs[1].ptr, tabs[2].ptr, out64.ptr)),
                sot=lambda: _ffi.check(getattr(lib, f"ekm_sot_{tag}")(dev, None, clim.ptr + 90 * row, clim.ptr + 99 * row, ens.ptr,
                                                                    NENS, npts, 90, -1e4, out.ptr)),
                crps=lambda: _ffi.check(getattr(lib, f"ekm_crps_from_ensemble_{tag}")(dev, None, ens.ptr, y.ptr, NENS, npts,
                                                                                    wts[0].ptr, wts[1].ptr, out64.ptr, None)))
            nbytes = dict(efi=(NCLIM + NENS) * dt.itemsize * npts + 8 * npts, efi_eps=(NCLIM + NENS) * dt.itemsize * npts + 8 * npts,
                          sot=(NENS + 3) * dt.itemsize * npts, crps=(NENS + 1) * dt.itemsize * npts + 8 * npts)
            copy_rate = 2 * ens.nbytes / (timer.copy([ens.ptr], [scratch.ptr], ens.nbytes) * 1e-3)
            for what, launch in launches.items():
                ms = timer.mean(launch)
                bl.emit(result, "runs", dict(dtype=tag, kernel=what, kernel_ms=ms, algorithmic_bytes=nbytes[what],
                                             **bl.derived(ms, nbytes[what], copy_rate, npts)))
            for x in (clim, ens, y, scratch, out64, out):
                x.free()
    bl.write(args.out, result)


if __name__ == "__main__":
    main()
