#!/usr/bin/env python3
"""Golden vectors for extreme.long_efi, extreme.long_sot, score.long_crps_from_ensemble and
stats.GumbelDistribution.long_fit: the REFERENCE's efi, sot, crps_from_ensemble and Gumbel fit on member / sample axes
beyond the 256 / 128 values the short kernels take, recorded the way gen_golden_ensemble.py and gen_golden_gumbel.py
record the short ones (their loaders of the reference, `write_npz` and `bare_signature` are imported, not restated; build
container only).

Writes tests/golden/long_ensemble_golden.npz: for every case the arguments of one call and what the reference returned,
a JSON manifest with the NumPy version that computed them and the recorded signatures, and the EFI coefficient tables as
this host's libm computes them.  Data only; arrays are stored
once and shared between cases (one ensemble per dtype and member count serves every function); the file regenerates byte
for byte.

Cases (24 points each): f32 and f64, m in {257, 300, 512, 513, 1980};
  efi   eps -0.1 and 0.5, against a sorted and an unsorted 101-row climate;
  sot   perc 10 and 90, eps -1e4 (the default) and 0.75 (members and climate below it count as 0);
  crps_from_ensemble   nan_policy "propagate";
  fit   entry (c) of gen_golden_gumbel.py: the reference's polyfill on the sample widened to float64.
Columns of every ensemble: 0-9 smooth, 10-19 tie-heavy (clamped precipitation rounded to 1/4), 20 one NaN member, 21 one
+inf, 22 one -inf, 23 all equal.  The climate's columns are of the same kinds (10-14 with a ramp added, so that its rows
lie further apart than sot's positive eps; 20-23: smooth).  No column mixes -0.0 and +0.0 (NumPy's sort does not define
their order).  To keep the file small the smooth data is rounded to 2**-10 (f32) /
2**-24 (f64): still all distinct in a column of these lengths but for chance, with short mantissas that compress.
"""
import json
import os

import numpy as np

import gen_golden_gumbel as gg
from gen_golden_ensemble import F32, F64, FUNCS, HERE, bare_signature, write_npz

NPTS = 24
MS = (257, 300, 512, 513, 1980)
NCLIM = 101


def smooth(rng, rows, npts, dt):
    grid = 2.0 ** (10 if dt is F32 else 24)
    return (np.round((280.0 + 12.0 * rng.normal(0, 1, (rows, npts))) * grid) / grid).astype(dt)


def ties(rng, rows, npts, dt, shift=1.5, grid=8):
    a = np.maximum(rng.gamma(1.5, 2.0, (rows, npts)) - shift, 0.0)
    return (np.round(a * grid) / grid).astype(dt)


def ensemble(rng, m, dt):
    a = smooth(rng, m, NPTS, dt)
    a[:, 10:20] = ties(rng, m, 10, dt, 0.25, 4)      # the low percentiles lie between 0 and sot's positive eps
    a[m // 2, 20] = np.nan
    a[m // 3, 21] = np.inf
    a[m // 3, 22] = -np.inf
    a[:, 23] = dt(281.25)
    return a


def climate(rng, dt):
    c = smooth(rng, NCLIM, NPTS, dt)
    c[:, 10:20] = ties(rng, NCLIM, 10, dt)
    c[:, 10:15] += np.linspace(0, 20, NCLIM, dtype=dt)[:, None]  # rows well apart: sot's denominator is above its positive eps
    c = np.sort(c, axis=0)
    unsorted = np.stack([rng.permutation(c[:, j]) for j in range(NPTS)], axis=1)
    return c, unsorted


def analysis(rng, ens, dt):
    """One value per point near the middle of its column; a NaN at point 9."""
    y = np.nanmedian(np.where(np.isfinite(ens), ens, np.nan).astype(F64), axis=0) + rng.normal(0, 2, NPTS)
    y[9] = np.nan
    return y.astype(dt)


class Recorder:
    def __init__(self):
        self.store, self.manifest, self.seen = {}, [], {}

    def put(self, v):
        v = np.asarray(v)
        key = (v.dtype.str, v.shape, v.tobytes())
        if key not in self.seen:
            self.seen[key] = f"a{len(self.seen):04d}"
            self.store[self.seen[key]] = v
        return self.seen[key]

    def add(self, func, note, arrays, plain, out):
        """out: {name: array} -- "out" for the functions that return one array, "mu" and "sigma" for the fit."""
        self.manifest.append(dict(id=f"c{len(self.manifest):04d}", func=func, note=note,
                                  arrays={k: self.put(v) for k, v in arrays.items()}, plain=plain,
                                  out={k: self.put(v) for k, v in out.items()}))

    def call(self, func, note, arrays, plain):
        before = {k: v.copy() for k, v in arrays.items()}
        out = np.asarray(FUNCS[func](**{k: v.copy() for k, v in arrays.items()}, **plain))
        assert all(before[k].tobytes() == arrays[k].tobytes() for k in arrays)
        self.add(func, note, arrays, plain, dict(out=out))

    def fit(self, note, sample):
        gg.ref.lmoment = gg.poly.lmoment
        try:
            dist = gg.ref.GumbelDistribution.fit(sample.astype(F64), axis=0)
        finally:
            gg.ref.lmoment = gg.NATIVE_LMOMENT
        self.add("fit", note, dict(sample=sample), dict(axis=0), dict(mu=np.asarray(dist.mu), sigma=np.asarray(dist.sigma)))


def main():
    rec = Recorder()
    rng = np.random.default_rng(20261022)
    for dt, tag in ((F64, "f64"), (F32, "f32")):
        clim, unsorted = climate(rng, dt)
        for m in MS:
            ens = ensemble(rng, m, dt)
            for eps in (-0.1, 0.5):
                rec.call("efi", f"{tag} m {m} sorted clim eps {eps}", dict(clim=clim, ens=ens), dict(eps=eps))
                rec.call("efi", f"{tag} m {m} unsorted clim eps {eps}", dict(clim=unsorted, ens=ens), dict(eps=eps))
            for perc in (10, 90):
                for eps in (-1e4, 0.75):
                    rec.call("sot", f"{tag} m {m} perc {perc} eps {eps}", dict(clim=clim, ens=ens), dict(perc=perc, eps=eps))
            rec.call("crps_from_ensemble", f"{tag} m {m}", dict(x=ens, y=analysis(rng, ens, dt)), dict(nan_policy="propagate"))
            rec.fit(f"{tag} m {m}", ens)
    sigs = {f: bare_signature(FUNCS[f]) for f in ("efi", "sot", "crps_from_ensemble")}
    sigs["fit"] = bare_signature(gg.ref.GumbelDistribution.fit)
    p = np.linspace(0.0, 1.0, NCLIM)  # the EFI coefficient tables as this host's libm computes them (gen_golden_ensemble.py)
    acosdiff, proddiff = np.diff(np.acos(np.sqrt(p))), np.diff(np.sqrt(p * (1.0 - p)))
    tables = [rec.put(t) for t in (acosdiff, proddiff, (1.0 - 2.0 * p[:-1]) * acosdiff + proddiff)]
    meta = dict(cases=rec.manifest, numpy=np.__version__, signatures=sigs, efi_tables=tables)
    rec.store["manifest"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "long_ensemble_golden.npz")
    write_npz(path, rec.store)
    print(len(rec.manifest), "cases,", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
