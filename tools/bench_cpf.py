#!/usr/bin/env python3
"""Times the Crossing Point Forecast kernel (cpf) on one GPU beside efi and writes profiles/cpf_bench.json.

Field: `--npts` points (default 2^21), 101 climate rows x 51 members, member-major: a N(0, 3) climate (sorted) against
a forecast of the same spread shifted per point by N(0, 2), on a 1/16 grid, from 65 536 distinct columns tiled over the
field.  Every timing is HIP events around `--steps` launches after `--warmup`, in ONE process on the same arrays:
  cpf            ekm_cpf_*, both sorts on (the default call): reads (101 + 51) elements, writes 4 B per point;
  cpf_symmetric  the same with symmetric: the reversed scan runs in the same launch;
  cpf_from_zero  the scan starts at member 0;
  cpf_clim_given sort_clim off: the climate streams from global memory, only the ensemble is in LDS;
  efi            ekm_efi_* on the same arrays: reads the same elements, writes 8 B;
  copy           ekm_stream_mix, one stream in and one out over the ensemble array: the float4-copy rate the memory
                 system gives these arrays; `copy_ms_same_bytes` is the time that rate needs for the kernel's bytes.

Usage: python tools/bench_cpf.py [--steps 10 --warmup 3 --npts 2097152 --out profiles/cpf_bench.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cpf_bench.json"))
    args = ap.parse_args()

    import ekm_hip
    from ekm_hip import _ffi, extreme

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
    base_c = np.sort(np.round(rng.normal(0, 3, (NCLIM, DISTINCT)) * 16) / 16 + 0.0, axis=0)
    base_e = np.round((rng.normal(0, 3, (NENS, DISTINCT)) + rng.normal(0, 2, DISTINCT)) * 16) / 16 + 0.0
    reps = (npts + DISTINCT - 1) // DISTINCT
    tabs = [ekm_hip.DeviceArray.from_host(t) for t in extreme.efi_coefficients(NCLIM)]

    for dtype in (np.float32, np.float64):
        dt = np.dtype(dtype)
        tag = "f32" if dt == np.float32 else "f64"

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
        for x in (clim, ens, scratch, out64, out):
            x.free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
