"""An independent NumPy restatement of the Crossing Point Forecast (reference extreme/array/cpf.py), the bound of its
one documented deviation, and access to tests/golden/cpf_golden.npz -- TEST INFRASTRUCTURE.

Written from the algorithm, one column of state per quantity and `numpy.where` for every conditional write (no boolean
fancy indexing, no early exit; the members that only prime a row are compared in one step): which (climate row,
member) steps happen depends only on nclim, nens and from_zero, and per point the state is the value so far, `done`
and `primed`.  It also reports WHICH write decided each point, which the
census uses to show that its field exercises all three."""
import functools
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cpf_golden.npz")
F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
U32 = 2.0 ** -24  # unit roundoff of f32
NONE, LOWER, PLAIN, UPPER = 0, 1, 2, 3  # the write that decided a point


def arith_dtype(*arrays):
    return F32 if all(np.asarray(a).dtype == F32 for a in arrays) else F64


def _scan(clim, ens, T, from_zero):
    """One scan over columns that are used as given.  Levels are Python floats: compared as such, and brought to T where
    they meet the fields (NumPy 2 treats a Python float beside an f32 array as an f32 scalar)."""
    nclim, npts = clim.shape
    nens = ens.shape[0]
    value, kind = np.zeros(npts, F32), np.zeros(npts, np.int8)
    done, primed = np.zeros(npts, bool), np.zeros(npts, bool)
    start = 0 if from_zero else nens // 2

    def intersection(lev, lev2, qc, qc2, qf):
        return (T.type(lev) * (qc2 - qf) + T.type(lev2) * (qf - qc)) / (qc2 - qc)

    with np.errstate(all="ignore"):
        for icl in range(1, nclim - 1):
            row_level = icl / (nclim - 1.0)
            qc = clim[icl]
            # the members below the row's level prime; nothing is written while they do, so they are taken together
            iq = start
            while iq < nens and (iq + 1.0) / (nens + 1.0) < row_level:
                iq += 1
            if iq > start:
                primed = primed | ((ens[start:iq] >= qc).any(axis=0) & ~done)
            if iq == nens:
                continue  # no member reaches this row's level
            member_level = (iq + 1.0) / (nens + 1.0)
            qf = ens[iq]
            if iq < 2:
                qc2 = clim[icl - 1]
                hit = (qf < qc) & (qc2 < qc) & primed
                x = np.maximum(intersection(row_level, (icl - 1) / (nclim - 1), qc, qc2, qf).astype(F64), 0.0)
                value, kind = np.where(hit, x.astype(F32), value), np.where(hit, LOWER, kind)
                done = done | hit
            hit = (qf < qc) & ~done & primed
            value, kind = np.where(hit, F32.type(member_level), value), np.where(hit, PLAIN, kind)
            done = done | hit
            if iq == nens - 1:
                top = clim[nclim - 1]
                hit = (qf > qc) & (top > qc) & ~done & primed
                x = np.minimum(intersection(row_level, 1.0, qc, top, qf).astype(F64), 1.0)
                value, kind = np.where(hit, x.astype(F32), value), np.where(hit, UPPER, kind)
    return value.astype(F32), kind.astype(np.int8)


def cpf_with_kinds(clim, ens, sort_clim=True, sort_ens=True, epsilon=None, symmetric=False, from_zero=False, dtype=None):
    """(cpf, kind of the write that decided the direct scan, "the reversed scan was used")."""
    clim, ens = np.asarray(clim), np.asarray(ens)
    if clim.ndim != 2 or ens.ndim != 2:
        raise ValueError("cpf: clim and ens must be 2-D")
    assert clim.shape[1] == ens.shape[1]
    T = np.dtype(dtype) if dtype is not None else arith_dtype(clim, ens)
    clim, ens = clim.astype(T), ens.astype(T)
    if sort_clim:
        clim = np.sort(clim, axis=0)  # NaN last
    if sort_ens:
        ens = np.sort(ens, axis=0)
    value, kind = _scan(clim, ens, T, from_zero)
    reversed_used = np.zeros(value.shape, bool)
    if symmetric:
        rev, _ = _scan(-clim[::-1], -ens[::-1], T, from_zero)
        reversed_used = value < F32.type(0.5)
        value = np.where(reversed_used, F32.type(1) - rev, value).astype(F32)
    elif epsilon is not None:
        value = np.where(ens[-1] < T.type(epsilon), F32.type(0), value).astype(F32)
    return value, kind, reversed_used


def cpf(clim, ens, sort_clim=True, sort_ens=True, epsilon=None, symmetric=False, from_zero=False, dtype=None):
    return cpf_with_kinds(clim, ens, sort_clim, sort_ens, epsilon, symmetric, from_zero, dtype)[0]


def mixed_cpf_bound(clim, ens, **options):
    """|reference - product| per point when only `clim` is f32 (the product computes in f64 on the upcast columns).

    The reference lets NumPy promote operation by operation.  Every comparison then mixes f32 with f64 and runs in f64,
    exactly, as in the product; so both take the same writes at the same members, and a level written by the plain
    crossing is the same number.  In an interpolation (t (c2 - f) + t2 (f - c)) / (c2 - c) the numerator's differences
    involve f (f64) and are formed in f64 as in the product, but the denominator c2 - c is a difference of two f32 climate
    rows and is rounded to f32: relative error at most u = 2^-24.  So the reference's f64 quotient is the product's times
    (1 + d), |d| <= u (1 + 2^-20) (the f64 roundings of the quotient and of the exact-in-f64 denominator, 2^-53 each, are
    covered by the factor).  Clamping to [0, 1] does not widen a difference, and each side is then rounded to f32 once:
    half an ulp, at most u |x| each.  Together |reference - product| <= 3 u |x| (1 + 2^-20) at an interpolated point
    and 0 elsewhere.  With `symmetric` the same holds for the reversed scan, and 1 - r adds its own rounding to f32 on
    each side, u |1 - r| each: 3 u |r| + 2 u |1 - r| <= 3 u there (r in [0, 1]), provided the direct value is on the same
    side of 0.5 in both, which the plain-crossing levels and any interpolated value further than the bound from 0.5 are.
    `epsilon` compares the last member (f64 in both) and adds nothing."""
    c64, e64 = np.asarray(clim, F64), np.asarray(ens, F64)
    value, kind, reversed_used = cpf_with_kinds(c64, e64, **options)
    interpolated = (kind == LOWER) | (kind == UPPER)
    bound = np.where(interpolated, 3 * U32 * np.abs(value.astype(F64)), 0.0)
    if options.get("symmetric"):
        bound = np.where(reversed_used, 3 * U32, bound)
    return np.where(np.isnan(bound), 0.0, bound) * (1 + 2.0 ** -20)


# ---- golden file ----
@functools.lru_cache(maxsize=1)
def _load():
    with np.load(PATH) as f:
        meta = json.loads(bytes(f["manifest"]).decode())
        arrays = {k: f[k] for k in f.files if k != "manifest"}
    return meta, arrays


def signature():
    return _load()[0]["signature"]


def cases():
    return list(_load()[0]["cases"])


def kwargs_of(case):
    arrays = _load()[1]
    kw = dict(case["plain"])
    kw.update({k: arrays[key] for k, key in case["arrays"].items()})
    return kw


def expected_of(case):
    return _load()[1][case["out"]]


def case_id(case):
    return f"{case['id']}-{case['note'].replace(' ', '_')}"


def is_mixed_clim_f32(case):
    """The documented deviation: only clim is f32, so the reference rounds the climate-row differences to f32."""
    kw = kwargs_of(case)
    return kw["clim"].dtype == F32 and kw["ens"].dtype == F64


def options_of(case):
    return {k: v for k, v in kwargs_of(case).items() if k not in ("clim", "ens")}
