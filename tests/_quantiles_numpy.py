"""An independent NumPy restatement of stats.iter_quantiles' three methods, and access to
tests/golden/quantiles_golden.npz -- TEST INFRASTRUCTURE.  The judges are those of _ensemble_numpy (bit for bit).

Vectorised over points and explicit about every rounding; numpy.quantile is not called.  The golden cases hold it to the
recorded reference bit for bit, the GPU census then uses it as the reference for fields no recording covers.
  sort        f = (m-1) q, j = int(f), x = f - j in float64; s[j] (1-x) + s[min(j+1, m-1)] x, every operation in float64;
  numpy_bulk  numpy's linear method with float64 levels: virtual index, floor and gamma in float64; the difference of
              the two neighbours in the DATA's dtype, then numpy's _lerp in float64;
  numpy       the same with the level cast to the data's dtype first: everything in the data's dtype.
"""
import functools
import json
import os

import numpy as np

from _ensemble_numpy import F32, F64, Mismatch, equal_bits, judge_exact  # noqa: F401

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quantiles_golden.npz")
METHODS = ("sort", "numpy_bulk", "numpy")


def arith_dtype(arr):
    return F32 if np.asarray(arr).dtype == F32 else F64


def levels(which):
    return np.linspace(0.0, 1.0, which + 1) if isinstance(which, int) else np.asarray(which, dtype=F64)


def positions(method, m, q, T):
    """(lo, hi, weight) of ONE level q (a float64 scalar), in Python scalars of the dtype each method works in."""
    if method == "sort":
        f = np.float64(m - 1) * np.float64(q)
        j = int(f)
        return j, min(j + 1, m - 1), f - np.float64(j)
    W = T if method == "numpy" else F64
    vi = W.type(m - 1) * W.type(q)
    if vi >= m - 1:
        return m - 1, m - 1, vi + W.type(1)
    lo = int(np.floor(vi))
    return lo, lo + 1, vi - W.type(lo)


def quantiles(arr, which=100, axis=0, method="sort"):
    """The stacked rows [nq, ...] of iter_quantiles(arr, which, axis, method)."""
    arr = np.asarray(arr)
    T = arith_dtype(arr)
    s = np.sort(np.moveaxis(arr.astype(T), axis, 0), axis=0)
    m = s.shape[0]
    missing = np.isnan(s).any(axis=0)
    out_dtype = T if method == "numpy" else F64
    rows = []
    with np.errstate(all="ignore"):
        for q in levels(which):
            lo, hi, w = positions(method, m, q, T)
            if method == "sort":
                row = s[lo].astype(F64) * (np.float64(1) - w)
                row = row + s[hi].astype(F64) * w
            else:
                W = out_dtype
                diff = (s[hi] - s[lo]).astype(W)  # formed in T
                a, b = s[lo].astype(W), s[hi].astype(W)
                row = b - diff * (W.type(1) - w) if w >= 0.5 else a + diff * w
            rows.append(np.where(missing, out_dtype.type(np.nan), row).astype(out_dtype))
    return np.stack(rows) if rows else np.empty((0,) + s.shape[1:], out_dtype)


# ---- golden file ----
@functools.lru_cache(maxsize=1)
def _load():
    with np.load(PATH) as f:
        meta = json.loads(bytes(f["manifest"]).decode())
        arrays = {k: f[k] for k in f.files if k != "manifest"}
    return meta, arrays


def signatures():
    return _load()[0]["signatures"]


def recorded_numpy_version():
    return _load()[0]["numpy"]


def cases():
    return _load()[0]["cases"]


def value_cases():
    return [c for c in cases() if not c["raises"] and "deviation" not in c]


def kwargs_of(case):
    kw = dict(case["plain"])
    kw["arr"] = _load()[1][case["arrays"]["arr"]]
    return kw


def expected_of(case):
    """The stacked rows the reference yielded; None when it yielded none (`which=[]`)."""
    return _load()[1][case["out"]] if case["out"] else None


def case_id(case):
    return f"{case['id']}-{case['note'].replace(' ', '_')}"


def judge_case(case, got, what=""):
    """got: the stacked result of the case.  Row count, dtype, shape, NaN pattern and every bit."""
    got, want = np.asarray(got), expected_of(case)
    if want is None:
        if got.shape[0] != 0:
            raise Mismatch(f"{what}: {got.shape[0]} rows where the reference yields none")
        return
    judge_exact(got, want, what)
