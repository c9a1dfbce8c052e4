#!/usr/bin/env python3
"""Times the ensemble reduction kernels (efi, sot, crps) on one GPU and writes profiles/ensemble_bench.json.

Field: `--npts` points (default 2^21), 101 climate rows x 51 members, member-major, zero-clamped gamma data (ties, as
precipitation has) from 65 536 distinct columns tiled over the field.  Every timing is HIP events around `--steps`
launches after `--warmup`, in ONE process on the same arrays:
  efi    ekm_efi_*            reads (101 + 51) elements, writes 8 B per point (eps <= 0 and eps > 0 arms);
  sot    ekm_sot_*  perc 90   reads 51 + 2 elements, writes one;
  crps   ekm_crps_from_ensemble_*  reads 51 + 1 elements, writes 8 B;
  copy   ekm_stream_mix, one stream in and one out over the ensemble array: the float4-copy rate the memory system
         gives these arrays; `copy_ms_same_bytes` is the time that rate needs for the kernel's algorithmic bytes.

Usage: python tools/bench_ensemble.py [--steps 10 --warmup 3 --npts 2097152 --out profiles/ensemble_bench.json]
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
NCLIM, NENS, DISTINCT = 101, 51, 1 << 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--npts", type=int, default=1 << 21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_bench.json"))
    args = ap.parse_args()

    import ekm_hip
    from ekm_hip import _ffi, extreme, score

    lib, dev = _ffi.lib(), 0
    _ffi.check(lib.ekm_init())
    name = C.create_string_buffer(128)
    lib.ekm_device_name(dev, name, 128)
    npts = args.npts
    result = dict(nclim=NCLIM, nens=NENS, npts=npts, steps=args.steps, warmup=args.warmup, device=name.value.decode(),
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
    base_c = np.sort(np.maximum(rng.gamma(1.5, 2.0, (NCLIM, DISTINCT)) - 1.0, 0.0), axis=0) + np.linspace(0, 0.5, NCLIM)[:, None]
    base_e = np.maximum(rng.gamma(1.5, 2.0, (NENS, DISTINCT)) - 1.0, 0.0)
    reps = (npts + DISTINCT - 1) // DISTINCT
    tabs = [ekm_hip.DeviceArray.from_host(t) for t in extreme.efi_coefficients(NCLIM)]
    wts = [ekm_hip.DeviceArray.from_host(t) for t in score.crps_weights(NENS)]

    for dtype in (np.float32, np.float64):
        dt = np.dtype(dtype)
        tag = "f32" if dt == np.float32 else "f64"

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
        ins, outs = (C.c_void_p * 1)(ens.ptr), (C.c_void_p * 1)(scratch.ptr)
        copy_ms = timed(lambda: _ffi.check(lib.ekm_stream_mix(dev, None, ins, 1, outs, 1, ens.nbytes)))
        copy_rate = 2 * ens.nbytes / (copy_ms * 1e-3)
        for what, launch in launches.items():
            ms = timed(launch)
            rate = nbytes[what] / (ms * 1e-3)
            run = dict(dtype=tag, kernel=what, kernel_ms=ms, algorithmic_bytes=nbytes[what], bytes_per_s=rate,
                       copy_bytes_per_s=copy_rate, copy_ms_same_bytes=nbytes[what] / copy_rate * 1e3,
                       frac_copy_rate=rate / copy_rate, frac_hbm_peak=rate / HBM_PEAK, points_per_s=npts / (ms * 1e-3))
            result["runs"].append(run)
            print(json.dumps(run), flush=True)
        for x in (clim, ens, y, scratch, out64, out):
            x.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
