"""An independent NumPy restatement of the ensemble reductions (EFI, SOT, CRPS), the judges the ensemble tests share
and access to tests/golden/ensemble_golden.npz -- TEST INFRASTRUCTURE.

The restatement is vectorised over points and explicit about every rounding: each step names its dtype, the sums over
climate rows and members run one row at a time in float64.  It states what the kernels are meant to compute (and what
the reference computes: the golden cases hold it to the recorded results bit for bit), without calling the reference's
code paths (no numpy.percentile, no numpy.sum over the member axis)."""
import functools
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ensemble_golden.npz")
F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
U32 = 2.0 ** -24  # unit roundoff of f32


def arith_dtype(*arrays):
    return F32 if all(np.asarray(a).dtype == F32 for a in arrays) else F64


def efi_tables(nclim):
    p = np.linspace(0.0, 1.0, nclim)
    acosdiff = np.diff(np.arccos(np.sqrt(p)))
    proddiff = np.diff(np.sqrt(p * (1.0 - p)))
    return acosdiff, proddiff, (1.0 - 2.0 * p[:-1]) * acosdiff + proddiff


def _frac(clim_row, ens, T):
    count = np.zeros(ens.shape[1], np.int64)
    for m in range(ens.shape[0]):
        count += ens[m] <= clim_row
    return count.astype(T) / T.type(ens.shape[0])


def efi(clim, ens, eps=-0.1, tables=None, dtype=None):
    clim, ens = np.asarray(clim), np.asarray(ens)
    T = np.dtype(dtype) if dtype is not None else arith_dtype(clim, ens)
    clim, ens = clim.astype(T), ens.astype(T)
    nclim, npts = clim.shape
    acosdiff, proddiff, acoef = tables if tables is not None else efi_tables(nclim)
    missing = np.isnan(clim).any(axis=0) | np.isnan(ens).any(axis=0)
    scale, teps = T.type(nclim - 1), T.type(eps)
    total, totmax = np.zeros(npts, F64), np.zeros(npts, F64)
    with np.errstate(all="ignore"):
        f0 = _frac(clim[0], ens, T)
        for icl in range(nclim - 1):
            f1 = _frac(clim[icl + 1], ens, T)
            dfdp = ((f1 - f0) * scale).astype(F64)
            a = (T.type(2) * f0 - T.type(1)).astype(F64)
            d = a * acosdiff[icl] + acoef[icl] * dfdp - proddiff[icl]
            if eps > 0:
                m = clim[icl + 1] > teps
                total = total + np.where(m, d, 0.0)
                totmax = totmax + np.where(m, -acosdiff[icl] - proddiff[icl], 0.0)
            else:
                total = total + d
            f0 = f1
        if eps > 0:
            total = total / np.maximum(totmax, eps)
        else:
            total = total * (2.0 / np.pi)
    total[missing] = np.nan
    return total


def mixed_efi_bound(clim, ens, eps=-0.1):
    """|efi with frac in f32 (the reference when only clim is f32) - efi with frac in f64 (the product for mixed dtypes)|
    per point, from the term magnitudes.  frac = k/n rounded to f32 is off by at most u|frac| <= u (u = 2^-24), so
    2 frac - 1 by at most 2u + u|2 frac - 1| <= 3u, and dFdp = fl(fl(f1 - f0) (nclim-1)) by at most
    (nclim-1)(2u + u|f1 - f0|) + u|dFdp|.  The term (2 frac - 1) acosdiff + acoef dFdp - proddiff therefore moves by at
    most 3u|acosdiff| + |acoef| ((nclim-1)(2u + u|df|) + u|dFdp|); the sum over the rows, times 2/pi resp. divided by
    max(efimax, eps), is the bound (the f64 roundings, 2^-53 relative, are covered by the factor 1 + 2^-20).
    Measured on 20 000 gamma-distributed points at 101 x 51: 2.1e-8 absolute at most, against a bound of 1.0e-6."""
    clim, ens = np.asarray(clim, F64), np.asarray(ens, F64)
    nclim, npts = clim.shape
    acosdiff, proddiff, acoef = efi_tables(nclim)
    bound, totmax = np.zeros(npts), np.zeros(npts)
    f0 = _frac(clim[0], ens, F64)
    for icl in range(nclim - 1):
        f1 = _frac(clim[icl + 1], ens, F64)
        df = np.abs(f1 - f0)
        term = 3 * U32 * abs(acosdiff[icl]) + abs(acoef[icl]) * ((nclim - 1) * (2 * U32 + U32 * df) + U32 * df * (nclim - 1))
        m = clim[icl + 1] > eps if eps > 0 else np.ones(npts, bool)
        bound += np.where(m, term, 0.0)
        totmax += np.where(m, -acosdiff[icl] - proddiff[icl], 0.0)
        f0 = f1
    scale = 1.0 / np.maximum(totmax, eps) if eps > 0 else 2.0 / np.pi
    return bound * scale * (1 + 2.0 ** -20)


def percentile_position(nens, perc, T):
    """numpy.percentile's linear method for a Python int `perc` on data of dtype T: everything in T."""
    q = T.type(perc) / T.type(100)
    vi = T.type(nens - 1) * q
    if vi >= nens - 1:
        return nens - 1, nens - 1, vi - T.type(-1)
    lo = int(np.floor(vi))
    return lo, lo + 1, vi - T.type(lo)


def sot_func(qc_tail, qc, qf, eps=-1e-4, lower_bound=-10, upper_bound=10, dtype=None):
    qc_tail, qc, qf = (np.asarray(a) for a in (qc_tail, qc, qf))
    T = np.dtype(dtype) if dtype is not None else arith_dtype(qc_tail, qc, qf)
    qc_tail, qc, qf = np.broadcast_arrays(qc_tail.astype(T), qc.astype(T), qf.astype(T))
    with np.errstate(all="ignore"):
        den = qc_tail - qc
        r = np.where(np.abs(den) > T.type(max(eps, 0)), (qf - qc_tail) / den, T.type(np.nan))
        r = np.where(r < T.type(lower_bound), T.type(lower_bound), r)
        r = np.where(r > T.type(upper_bound), T.type(upper_bound), r)
    return r.astype(T)


def sot(clim, ens, perc, eps=-1e4, dtype=None):
    clim, ens = np.asarray(clim), np.asarray(ens)
    T = np.dtype(dtype) if dtype is not None else arith_dtype(clim, ens)
    pts = clim.shape[1:]
    clim, ens = clim.astype(T).reshape(clim.shape[0], -1), ens.astype(T).reshape(ens.shape[0], -1)
    qc, qc_tail = clim[perc], clim[99 if perc > 50 else 1]
    if eps > 0:
        ens = np.where(ens < T.type(eps), T.type(0), ens)
        qc = np.where(qc < T.type(eps), T.type(0), qc)
    s = np.sort(ens, axis=0)
    lo, hi, gamma = percentile_position(ens.shape[0], perc, T)
    with np.errstate(all="ignore"):
        diff = s[hi] - s[lo]
        qf = s[hi] - diff * (T.type(1) - gamma) if gamma >= 0.5 else s[lo] + diff * gamma
    qf = np.where(np.isnan(ens).any(axis=0), T.type(np.nan), qf).astype(T)
    return sot_func(qc_tail, qc, qf, eps=eps, dtype=T).reshape(pts)


def crps(x, y, dtype=None):
    """(crps with NaN at the missing points, the missing mask); `nan_policy` is applied by the caller."""
    x, y = np.asarray(x), np.asarray(y)
    T = np.dtype(dtype) if dtype is not None else arith_dtype(x, y)
    pts = y.shape
    x, y = x.astype(T).reshape(x.shape[0], -1), y.astype(T).reshape(-1)
    n = x.shape[0]
    missing = np.isnan(x).any(axis=0) | np.isnan(y)
    s = np.sort(x, axis=0)
    p = np.arange(n + 1) / float(n)
    p2, q2 = p**2, (1 - p) ** 2
    zero = np.zeros(y.shape, F64)
    with np.errstate(all="ignore"):
        total = None
        for i in range(n + 1):
            if i == 0:
                alpha, beta = zero, np.maximum((s[0] - y).astype(F64), 0.0)
            elif i == n:
                alpha, beta = np.maximum(-(s[n - 1] - y).astype(F64), 0.0), zero
            else:
                dxx = (s[i] - s[i - 1]).astype(F64)
                alpha = np.minimum(dxx, np.maximum(-(s[i - 1] - y).astype(F64), 0.0))
                beta = np.minimum(dxx, np.maximum((s[i] - y).astype(F64), 0.0))
            term = alpha * p2[i] + beta * q2[i]
            total = term if total is None else total + term
    total = np.where(missing, np.nan, total)
    return total.reshape(pts), missing.reshape(pts)


def crps_from_ensemble(x, y, nan_policy="propagate", dtype=None):
    total, missing = crps(x, y, dtype)
    if nan_policy == "omit":
        return total.reshape(-1)[~missing.reshape(-1)]
    return total


RESTATEMENT = {"efi": efi, "sot": sot, "sot_func": sot_func, "crps_from_ensemble": crps_from_ensemble}


# ---- golden file ----
@functools.lru_cache(maxsize=1)
def _load():
    with np.load(PATH) as f:
        meta = json.loads(bytes(f["manifest"]).decode())
        arrays = {k: f[k] for k in f.files if k != "manifest"}
    return meta, arrays


def signatures():
    return _load()[0]["signatures"]


def recorded_tables(nclim):
    meta, arrays = _load()
    return tuple(arrays[k] for k in meta["efi_tables"][str(nclim)])


def cases(func=None):
    return [c for c in _load()[0]["cases"] if func is None or c["func"] == func]


def kwargs_of(case):
    arrays = _load()[1]
    kw = dict(case["plain"])
    kw.update({k: arrays[key] for k, key in case["arrays"].items()})
    return kw


def expected_of(case):
    return _load()[1][case["out"]]


def case_id(case):
    return f"{case['id']}-{case['func']}-{case['note'].replace(' ', '_')}"


# ---- judges ----
class Mismatch(AssertionError):
    pass


def judge_exact(got, want, what=""):
    """dtype, shape, NaN positions, and every other value bit for bit (the sign of a zero included)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        raise Mismatch(f"{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}")
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        raise Mismatch(f"{what}: NaN pattern differs at {int(np.sum(np.isnan(got) != np.isnan(want)))} points")
    ok = np.isnan(want) | ((got == want) & (np.signbit(got) == np.signbit(want)))
    if not ok.all():
        i = np.flatnonzero(~ok.reshape(-1))[0]
        raise Mismatch(f"{what}: {int((~ok).sum())} of {ok.size} values differ, first at {i}: {got.reshape(-1)[i]!r} against {want.reshape(-1)[i]!r}")


def judge_bound(got, want, bound, what="", ledger=None):
    """|got - want| <= bound at every point, the same NaN pattern; used/allowed goes to the ledger."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        raise Mismatch(f"{what}: shape {got.shape} against {want.shape}")
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        raise Mismatch(f"{what}: NaN pattern differs")
    err = np.where(np.isnan(want), 0.0, np.abs(got.astype(F64) - want.astype(F64)))
    if ledger is not None:
        ledger.append((what, "efi mixed-dtype bound", float(np.max(err / np.maximum(bound, 1e-300), initial=0.0)), 1.0, err.size))
    if not (err <= bound).all():
        i = int(np.argmax(err - bound))
        raise Mismatch(f"{what}: |{got.reshape(-1)[i]!r} - {want.reshape(-1)[i]!r}| = {err.reshape(-1)[i]:.3e} > {np.reshape(bound, -1)[i]:.3e}")


def equal_bits(a, b):
    """Number of points at which a and b agree (NaN with NaN, else value and sign)."""
    a, b = np.asarray(a), np.asarray(b)
    return int(np.sum((np.isnan(a) & np.isnan(b)) | ((a == b) & (np.signbit(a) == np.signbit(b)))))


def is_mixed_efi(case):
    """The documented deviation: only clim is f32, so the reference forms frac in f32 and the product in f64."""
    if case["func"] != "efi":
        return False
    kw = kwargs_of(case)
    return kw["clim"].dtype == F32 and kw["ens"].dtype != F32


def judge_case(case, got, what, ledger=None):
    want = expected_of(case)
    if is_mixed_efi(case):
        kw = kwargs_of(case)
        return judge_bound(got, want, mixed_efi_bound(kw["clim"], kw["ens"], kw.get("eps", -0.1)), what, ledger)
    return judge_exact(got, want, what)
