#!/usr/bin/env python3
"""Times the Crossing Point Forecast kernel (cpf) on one GPU beside efi and writes profiles/cpf_bench.json.

Field: `--npts` points (default 2^21), 101 climate rows x 51 members, member-major: a N(0, 3) climate (sorted) against
a forecast of the same spread shifted per point by N(0, 2), on a 1/16 grid, from 65 536 distinct columns tiled over the
field.  How the timings are taken: tools/_benchlib.py.
  cpf            ekm_cpf_*, both sorts on (the default call): reads (101 + 51) elements, writes 4 B per point;
  cpf_symmetric  the same with symmetric: the reversed scan runs in the same launch;
  cpf_from_zero  the scan starts at member 0;
  cpf_clim_given sort_clim off: the climate streams from global memory, only the ensemble is in LDS;
  efi            ekm_efi_* on the same arrays: reads the same elements, writes 8 B;
  copy           ekm_stream_mix, one stream in and one out over the ensemble array: the float4-copy rate the memory
                 system gives these arrays; `copy_ms_same_bytes` is the time that rate needs for the kernel's bytes.

`--long` times extreme.long_cpf instead and writes profiles/long_cpf_bench.json:
  crossover    f32 and f64 at 2^20 points, 101 climate rows, 32 / 51 / 64 / 128 / 256 members: ekm_long_cpf_* and ekm_cpf_*
               on the same arrays under the default options, `symmetric`, `from_zero` and sort_clim off (null where the
               short entry point refuses the shape), and ekm_long_quantiles_* with one level on the ensemble array: the
               load and sort of one tile with the cheapest read-out there is;
  beyond_cap   (nclim, nens) = (101, 1980), (1980, 51), (1980, 1980) at 2^16 points: the long entry point and the same
               one-level long_quantiles; the climate is then a raw sample, unsorted.

Usage: python tools/bench_cpf.py [--steps 10 --warmup 3 --npts 2097152 --out profiles/cpf_bench.json]
       python tools/bench_cpf.py --long [--steps 5 --warmup 2 --out profiles/long_cpf_bench.json]
"""
import os

import numpy as np

import _benchlib as bl

NCLIM, NENS, DISTINCT = 101, 51, 1 << 16


LONG_OPTIONS = dict(default=(1, 0, 0), symmetric=(1, 0, 1), from_zero=(1, 1, 0), clim_given=(0, 0, 0))  # sort_clim, from_zero, symmetric


def long_main(args):
    import ekm_hip
    from ekm_hip import _ffi

    lib, dev, name = bl.open_device()
    result = dict(steps=args.steps, warmup=args.warmup, device=name, crossover=[], beyond_cap=[])

    def launch_of(prefix, tag, clim, ens, nclim, nens, npts, out, option):
        """A launch of family `prefix` on the first `nens` rows of `ens`, or None where the entry point refuses the shape."""
        fn, (sort_clim, from_zero, symmetric) = getattr(lib, f"{prefix}cpf_{tag}"), LONG_OPTIONS[option]
        call = lambda: fn(dev, None, clim.ptr, ens.ptr, nclim, nens, npts, sort_clim, 1, from_zero, symmetric, 0, 0.0, out.ptr)  # noqa: E731
        if call() == _ffi.EKM_ERR_ARG:
            return None
        return lambda: _ffi.check(call())

    with bl.EventTimer(lib, dev, args.steps, args.warmup) as timer:
        rng = np.random.default_rng(1)
        for key, npts, distinct, shapes in (("crossover", 1 << 20, 1 << 14, [(NCLIM, m) for m in (32, 51, 64, 128, 256)]),
                                            ("beyond_cap", 1 << 16, 1 << 12, [(101, 1980), (1980, 51), (1980, 1980)])):
            rows_c, rows_e = max(c for c, _ in shapes), max(e for _, e in shapes)
            base_c = np.round(rng.normal(0, 3, (rows_c, distinct)) * 16) / 16 + 0.0
            base_e = np.round((rng.normal(0, 3, (rows_e, distinct)) + rng.normal(0, 2, distinct)) * 16) / 16 + 0.0
            if key == "crossover":
                base_c = np.sort(base_c, axis=0)
            for dtype in (np.float32, np.float64):
                dt = np.dtype(dtype)
                tag = bl.tag(dt)
                clim, ens = bl.tiled_rows(base_c, npts, dt), bl.tiled_rows(base_e, npts, dt)
                out, qout = ekm_hip.DeviceArray.empty((npts,), np.float32), ekm_hip.DeviceArray.empty((npts,), dt)
                for nclim, nens in shapes:
                    sort_launch, keep = bl.one_level_long_quantiles(lib, dev, ens, nens, npts, qout)
                    sort_ms = timer.mean(sort_launch)
                    for option in (LONG_OPTIONS if key == "crossover" else ("default", "symmetric")):
                        common = (tag, clim, ens, nclim, nens, npts, out, option)
                        run = dict(dtype=tag, nclim=nclim, nens=nens, npts=npts, options=option,
                                   long_ms=timer.mean(launch_of("ekm_long_", *common)), long_quantiles_one_level_ms=sort_ms)
                        if key == "crossover":
                            short = launch_of("ekm_", *common)
                            run["short_ms"] = timer.mean(short) if short else None
                        bl.emit(result, key, run)
                    del keep
                for x in (clim, ens, out, qout):
                    x.free()
    bl.write(args.out, result)


def main():
    ap = bl.parser("cpf_bench.json")
    ap.add_argument("--npts", type=int, default=1 << 21)
    ap.add_argument("--long", action="store_true", help="time extreme.long_cpf beside cpf (module docstring)")
    args = ap.parse_args()
    if args.long:
        if args.out.endswith("cpf_bench.json") and not args.out.endswith("long_cpf_bench.json"):
            args.out = os.path.join(os.path.dirname(args.out), "long_cpf_bench.json")
        return long_main(args)

    import ekm_hip
    from ekm_hip import _ffi, extreme

    lib, dev, name = bl.open_device()
    npts = args.npts
    result = dict(nclim=NCLIM, nens=NENS, npts=npts, steps=args.steps, warmup=args.warmup, device=name,
                  hbm_peak_bytes_per_s=bl.HBM_PEAK, runs=[])

    with bl.EventTimer(lib, dev, args.steps, args.warmup) as timer:
        rng = np.random.default_rng(1)
        base_c = np.sort(np.round(rng.normal(0, 3, (NCLIM, DISTINCT)) * 16) / 16 + 0.0, axis=0)
        base_e = np.round((rng.normal(0, 3, (NENS, DISTINCT)) + rng.normal(0, 2, DISTINCT)) * 16) / 16 + 0.0
        reps = (npts + DISTINCT - 1) // DISTINCT
        tabs = [ekm_hip.DeviceArray.from_host(t) for t in extreme.efi_coefficients(NCLIM)]

        for dtype in (np.float32, np.float64):
            dt = np.dtype(dtype)
            tag = bl.tag(dt)

            def field(base, rows):
                d = ekm_hip.DeviceArray.empty((rows, npts), dt)
                for k in range(rows):
                    d.flat_slice(k * npts, (k + 1) * npts).copy_from_host(np.tile(base[k], reps)[:npts].astype(dt))
                return d

            clim, ens = field(base_c, NCLIM), field(base_e, NENS)
            scratch = ekm_hip.DeviceArray.empty((NENS, npts), dt)
            out64 = ekm_hip.DeviceArray.empty((npts,), np.float64)
            out = ekm_hip.DeviceArray.empty((npts,), np.float32)

            def cpf(sort_clim=1, from_zero=0, symmetric=0):
                fn = getattr(lib, f"ekm_cpf_{tag}")
                return lambda: _ffi.check(fn(dev, None, clim.ptr, ens.ptr, NCLIM, NENS, npts, sort_clim, 1, from_zero, symmetric, 0, 0.0,
                                             out.ptr))

            launches = dict(
                cpf=cpf(), cpf_symmetric=cpf(symmetric=1), cpf_from_zero=cpf(from_zero=1), cpf_clim_given=cpf(sort_clim=0),
                efi=lambda: _ffi.check(getattr(lib, f"ekm_efi_{tag}")(dev, None, clim.ptr, ens.ptr, NCLIM, NENS, npts, -0.1,
                                                                    tabs[0].ptr, tabs[1].ptr, tabs[2].ptr, out64.ptr)))
            nbytes = {k: (NCLIM + NENS) * dt.itemsize * npts + (8 if k == "efi" else 4) * npts for k in launches}
            copy_rate = 2 * ens.nbytes / (timer.copy([ens.ptr], [scratch.ptr], ens.nbytes) * 1e-3)
            for what, launch in launches.items():
                ms = timer.mean(launch)
                bl.emit(result, "runs", dict(dtype=tag, kernel=what, kernel_ms=ms, algorithmic_bytes=nbytes[what],
                                             **bl.derived(ms, nbytes[what], copy_rate, npts)))
            for x in (clim, ens, scratch, out64, out):
                x.free()
    bl.write(args.out, result)


if __name__ == "__main__":
    main()
