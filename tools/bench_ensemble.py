#!/usr/bin/env python3
"""Times the ensemble reduction kernels (efi, sot, crps) on one GPU and writes profiles/ensemble_bench.json.

Field: `--npts` points (default 2^21), 101 climate rows x 51 members, member-major, zero-clamped gamma data (ties, as
precipitation has) from 65 536 distinct columns tiled over the field.  How the timings are taken: tools/_benchlib.py.
  efi    ekm_efi_*            reads (101 + 51) elements, writes 8 B per point (eps <= 0 and eps > 0 arms);
  sot    ekm_sot_*  perc 90   reads 51 + 2 elements, writes one;
  crps   ekm_crps_from_ensemble_*  reads 51 + 1 elements, writes 8 B;
  copy   ekm_stream_mix, one stream in and one out over the ensemble array: the float4-copy rate the memory system
         gives these arrays; `copy_ms_same_bytes` is the time that rate needs for the kernel's algorithmic bytes.

Usage: python tools/bench_ensemble.py [--steps 10 --warmup 3 --npts 2097152 --out profiles/ensemble_bench.json]
"""
import numpy as np

import _benchlib as bl

NCLIM, NENS, DISTINCT = 101, 51, 1 << 16


def main():
    ap = bl.parser("ensemble_bench.json")
    ap.add_argument("--npts", type=int, default=1 << 21)
    args = ap.parse_args()

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
