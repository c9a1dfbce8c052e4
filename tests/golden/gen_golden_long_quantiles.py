#!/usr/bin/env python3
"""Golden vectors for stats.long_quantiles: the REFERENCE's iter_quantiles on sample axes beyond the 256 / 128 values the
short kernel takes, recorded the way gen_golden_quantiles.py records the short ones (its Recorder, data makers and
loader of the reference are imported, not restated; build container only).

Writes tests/golden/long_quantiles_golden.npz: for every case the arguments of one call and the stacked rows the reference
yielded, and a JSON manifest with the NumPy version that computed them and the recorded signature.  Data only; arrays are
stored once and shared between cases; the file regenerates byte for byte.

Cases (8 points each): f32 and f64, the three methods, m in {257, 300, 512, 513, 1980}, `which` in
{100, [0.9, 0.0, 0.33], 1}, tie-heavy data (rounded to 1/8) and smooth data; and one 300-sample array with special columns
(all-equal, a NaN, +inf on top, -inf at the bottom) laid out with the sample axis first, last and in the middle.  No
column mixes -0.0 and +0.0 (NumPy's sort does not define their order).  To keep the file small the smooth data is
rounded to 2**-10 (f32) / 2**-24 (f64): still all distinct in a column of these lengths but for chance, with short
mantissas that compress.
"""
import json
import os

import numpy as np

from gen_golden_quantiles import METHODS, F32, F64, HERE, Recorder, bare_signature, precip, ref, smooth, write_npz

NPTS = 8
MS = (257, 300, 512, 513, 1980)
WHICH = (100, [0.9, 0.0, 0.33], 1)


def smooth_short(rng, rows, npts, dt):
    grid = 2.0 ** (10 if dt is F32 else 24)
    return (np.round(smooth(rng, rows, npts, F64) * grid) / grid).astype(dt)


def special(rng, m, dt):
    a = smooth_short(rng, m, NPTS, dt)
    a[:, 0] = dt(3.25)          # all-equal
    a[m // 2, 1] = np.nan       # a NaN member
    a[m // 3, 2] = np.inf       # +inf on top
    a[m // 3, 3] = -np.inf      # -inf at the bottom
    a[:, 4:6] = precip(rng, m, 2, dt)
    return a


def main():
    rec = Recorder()
    rng = np.random.default_rng(20261021)
    for dt, tag in ((F64, "f64"), (F32, "f32")):
        for m in MS:
            for kind, make in (("ties", precip), ("smooth", smooth_short)):
                arr = make(rng, m, NPTS, dt)
                for method in METHODS:
                    for which in WHICH:
                        rec.add(f"{tag} m {m} {kind} {method} which {which}", arr, which=which, method=method)
        first = special(rng, 300, dt)
        layouts = (("first", first, 0), ("last", np.ascontiguousarray(first.T), -1),
                   ("middle", np.ascontiguousarray(first.reshape(300, 2, 4).transpose(1, 0, 2)), 1))
        for where, arr, axis in layouts:
            for method in METHODS:
                for which in WHICH:
                    rec.add(f"{tag} m 300 special axis {where} {method} which {which}", arr, which=which, axis=axis, method=method)
    for entry in rec.manifest:
        assert entry["raises"] is None, entry
    meta = dict(cases=rec.manifest, numpy=np.__version__, signatures={"iter_quantiles": bare_signature(ref.iter_quantiles)})
    rec.store["manifest"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "long_quantiles_golden.npz")
    write_npz(path, rec.store)
    print(len(rec.manifest), "cases,", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
