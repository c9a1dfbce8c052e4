#!/usr/bin/env python3
"""Golden vectors for extreme.long_cpf: the REFERENCE's extreme.array.cpf on columns the short `cpf` refuses
(nens + nclim > 640, so neither the f32 nor the f64 short path sorts them), recorded the way gen_golden_cpf.py records
the short ones (its loader of the reference, `write_npz` and `bare_signature` are imported, not restated; build
container only).

Writes tests/golden/long_cpf_golden.npz: a JSON manifest and, per case, what the reference returned (float32).  Data
only.  To keep the file small every input is stored ONCE, in float32, on a grid of 1/16 (exact in both dtypes): a case
names its climate (stored sorted), its ensemble (stored unsorted), the dtype the reference was given them in, and how
the call's arrays derive from the stored ones -- `perm` (a row permutation of the climate: the unsorted climate) and
`presort_ens` (the ensemble sorted before the call).  tests/_long_cpf.py rebuilds the arrays the same way.  The file
regenerates byte for byte.

Cases: (nclim, nens) in SHAPES, f32 and f64, the 12 option sets of cpf_golden.npz; 24 points each:
  0-7   normal climate, a narrower ensemble shifted per point;   8-11  zero-clamped gamma (heavy ties, only +0.0);
  12    every value equal, climate = ensemble;   13  a climate of zeros;   14 / 15  ensemble wholly below / above;
  16    a NaN in one climate row;   17  a NaN in one member;   18 / 19  a +inf / -inf member;
  20    climate from -inf to +inf;   21  the ensemble runs over the climate's range;
  22    the two lowest members inside the low climate rows (the lower-tail interpolation, with from_zero);
  23    the ensemble high in the climate (the upper-tail interpolation).
No column mixes -0.0 and +0.0 (NumPy's sort does not define their order)."""
import json
import os
import sys

import numpy as np

from gen_golden_cpf import F32, F64, HERE, bare_signature, ref_extreme, write_npz

sys.path.insert(0, os.path.dirname(HERE))
import _cpf_numpy as cn  # noqa: E402
from _long_ensemble import no_column_mixes_the_zeros  # noqa: E402

NPTS = 24
SHAPES = ((101, 700), (700, 51), (513, 257), (1980, 51), (101, 1980), (700, 700))
OPTIONS = (  # (note, options, unsorted climate, ensemble sorted first): the 12 option sets of gen_golden_cpf.option_cases
    ("default", {}, False, False),
    ("from_zero", dict(from_zero=True), False, False),
    ("symmetric", dict(symmetric=True), False, False),
    ("symmetric from_zero", dict(symmetric=True, from_zero=True), False, False),
    ("epsilon 0.5", dict(epsilon=0.5), False, False),
    ("epsilon 0.5 symmetric", dict(epsilon=0.5, symmetric=True), False, False),
    ("sorts off presorted", dict(sort_clim=False, sort_ens=False), False, True),
    ("sorts off unsorted", dict(sort_clim=False, sort_ens=False), True, False),
    ("sorts off unsorted symmetric from_zero", dict(sort_clim=False, sort_ens=False, symmetric=True, from_zero=True), True, False),
    ("sorts off unsorted epsilon 0.5", dict(sort_clim=False, sort_ens=False, epsilon=0.5), True, False),
    ("sort_clim off", dict(sort_clim=False, from_zero=True), False, False),
    ("sort_ens off", dict(sort_ens=False, from_zero=True), True, False),
)


def grid(a):
    return np.round(a * 16) / 16 + 0.0  # (adding 0.0 turns -0.0 into 0.0)


def fields(rng, nclim, nens):
    """(climate sorted, ensemble unsorted), float32 values on the 1/16 grid."""
    clim = grid(rng.normal(0, 3, (nclim, NPTS)))
    ens = grid(rng.normal(0, 1.5, (nens, NPTS)) + rng.normal(0, 3, NPTS))
    clim[:, 8:12] = grid(np.maximum(rng.gamma(1.5, 2.0, (nclim, 4)) - 1.5, 0.0))
    ens[:, 8:12] = grid(np.maximum(rng.gamma(1.5, 2.0, (nens, 4)) * rng.uniform(0.3, 2.5, 4) - 1.5, 0.0))
    clim = np.sort(clim, axis=0)
    clim[:, 12], ens[:, 12] = 3.25, 3.25
    clim[:, 13] = 0.0
    clim[:, 14] += 1000.0
    clim[:, 15] -= 1000.0
    clim[nclim // 2, 16] = np.nan
    ens[nens // 2, 17] = np.nan
    ens[0, 18], ens[nens - 1, 19] = np.inf, -np.inf
    clim[0, 20], clim[-1, 20] = -np.inf, np.inf
    ens[:, 21] = grid(rng.permutation(np.linspace(clim[0, 21], clim[-1, 21], nens)))
    # 22: with from_zero member 1 is the crossing member for the rows r with (nclim-1)/(nens+1) < r <= 2 (nclim-1)/(nens+1);
    # the two lowest members sit on one of them, the others above the climate's middle
    r = max(1, int(1.5 * (nclim - 1) / (nens + 1)))
    ens[:, 22] = np.abs(ens[:, 22]) + clim[nclim // 2, 22]
    ens[nens // 3, 22] = ens[2 * nens // 3, 22] = clim[r, 22]
    # 23: a narrow ensemble between the climate's 90 % row and its top
    lo, hi = clim[(9 * nclim) // 10, 23], clim[-1, 23]
    ens[:, 23] = grid(rng.uniform(lo, max(hi - 0.0625, lo), nens))
    clim = np.sort(clim, axis=0)  # NaN last, as the stored climate is the sorted one
    clim, ens = clim.astype(F32), ens.astype(F32)
    assert np.array_equal(clim.astype(F64).astype(F32), clim, equal_nan=True)
    assert no_column_mixes_the_zeros(clim) and no_column_mixes_the_zeros(ens)
    return clim, ens


def main():
    store, manifest, kinds, reversed_used = {}, [], set(), False
    rng = np.random.default_rng(20261023)
    for nclim, nens in SHAPES:
        assert nclim + nens > 640 and nclim * nens <= 500000
        clim, ens = fields(rng, nclim, nens)
        perm = rng.permutation(nclim).astype(np.uint16)
        assert not (np.diff(clim[perm][:, :12], axis=0) >= 0).all(axis=0).any()
        head = f"{nclim}x{nens}"
        store[f"clim_{head}"], store[f"ens_{head}"], store[f"perm_{head}"] = clim, ens, perm
        for dt, tag in ((F32, "f32"), (F64, "f64")):
            for note, options, unsorted, presort in OPTIONS:
                c = (clim[perm] if unsorted else clim).astype(dt)
                e = (np.sort(ens, axis=0) if presort else ens).astype(dt)
                before = c.copy(), e.copy()
                out = np.asarray(ref_extreme.cpf(clim=c, ens=e, **options))
                assert out.dtype == F32 and out.shape == (NPTS,)
                assert before[0].tobytes() == c.tobytes() and before[1].tobytes() == e.tobytes()
                restated, kind, rev = cn.cpf_with_kinds(c, e, **options)
                assert restated.tobytes() == out.tobytes(), (head, tag, note)  # the restatement tells the writes apart
                kinds |= {(int(k), bool(options.get("from_zero"))) for k in kind}
                reversed_used = reversed_used or bool(rev.any())
                key = f"out_{len(manifest):04d}"
                store[key] = out
                manifest.append(dict(id=f"c{len(manifest):04d}", note=f"{tag} {head} {note}", dtype=tag, nclim=nclim, nens=nens,
                                     clim=f"clim_{head}", ens=f"ens_{head}", perm=f"perm_{head}" if unsorted else None,
                                     presort_ens=presort, plain=options, out=key))
                print(manifest[-1]["note"], flush=True)
    # every kind of write decides a point somewhere; the lower-tail interpolation needs from_zero
    assert {k for k, _ in kinds} == {cn.NONE, cn.LOWER, cn.PLAIN, cn.UPPER}, kinds
    assert (cn.LOWER, True) in kinds and reversed_used
    meta = dict(cases=manifest, numpy=np.__version__, signature=bare_signature(ref_extreme.cpf))
    store["manifest"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "long_cpf_golden.npz")
    write_npz(path, store)
    print(len(manifest), "cases,", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
