"""An independent NumPy restatement of stats.GumbelDistribution (fit, cdf, ppf) and the two return-period functions,
their judges, and access to tests/golden/gumbel_golden.npz -- TEST INFRASTRUCTURE.

The restatement is vectorised over points and explicit about every rounding (csrc/ensemble_point.hpp, gumbel_*_point):
  fit   the column sorted ascending in its own dtype, widened to float64; s0 = s0 + x_i and s1 = s1 + x_i * (i - 1) one
        sample at a time; b0 = s0 / n, b1 = s1 / (n * (n - 1)), l2 = -1 * b0 + 2 * b1, sigma = l2 / log(2),
        mu = b0 - sigma * 0.5772; a column that holds a NaN gives NaN twice;
  cdf   1 - exp(-exp((mu - x) / sigma)) in float64, the levels on leading axes;
  ppf   mu - sigma * log(-log(1 - p)) in float64.
The golden cases hold `fit` to recording (c) (the reference's polyfill on the sample widened to float64) and `ppf` to
the recorded reference bit for bit.

Bounds (each judge prints, and files in the ledger, the largest share of its bound that was used):
  * recordings (a) and (b) of `fit` (the reference on the sample's own dtype, through SciPy and through its polyfill)
    against (c): 2 n (eps_ref + 2^-52) max|x| per all-finite column, eps_ref = 2^-23 for an f32 sample and 2^-52 for f64:
    the forward-error bound of a length-n recursive sum whose weights sum to at most 1, carried through / ln 2 and
    - 0.5772 sigma (a factor under 2);
  * cdf: |got - ref| <= 8 * 2^-53: the rounding of the quotient, of both exponentials and of the subtraction, with
    e exp(-e) (1 + |ln e|) < 1;
  * return period: |got - ref| <= |ref| (8 * 2^-53 / cdf_ref + 4 * 2^-53); where cdf_ref == 0 the reference gives inf and
    the result must be inf or at least freq / (8 * 2^-53).
"""
import datetime
import functools
import json
import os

import numpy as np

from _ensemble_numpy import F32, F64, Mismatch, equal_bits, judge_exact  # noqa: F401

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gumbel_golden.npz")
LN2 = 0.6931471805599453
U = 2.0 ** -53
CDF_BOUND = 8 * U
FIT_KIND = "gumbel fit: reference paths against the float64 polyfill (tests/_gumbel_numpy.py)"
CDF_KIND = "gumbel cdf: 8 * 2^-53 absolute (tests/_gumbel_numpy.py)"
RP_KIND = "gumbel return period: |ref| (8 * 2^-53 / cdf + 4 * 2^-53) (tests/_gumbel_numpy.py)"


def arith_dtype(arr):
    return F32 if np.asarray(arr).dtype == F32 else F64


# ---- the restatement ----
def fit(sample, axis=0):
    """(mu, sigma) as float64 arrays of `sample`'s shape without `axis`."""
    sample = np.asarray(sample)
    T = arith_dtype(sample)
    s = np.sort(np.moveaxis(sample.astype(T), axis, 0), axis=0)
    n = s.shape[0]
    missing = np.isnan(s).any(axis=0)
    s = s.astype(F64)
    s0, s1 = np.zeros(s.shape[1:], F64), np.zeros(s.shape[1:], F64)
    with np.errstate(all="ignore"):
        for i in range(n):
            s0 = s0 + s[i]
            s1 = s1 + s[i] * np.float64(i)
        b0 = s0 / np.float64(n)
        b1 = s1 / (np.float64(n) * np.float64(n - 1))
        l2 = np.float64(-1.0) * b0 + np.float64(2.0) * b1
        sigma = l2 / np.float64(LN2)
        mu = b0 - sigma * np.float64(0.5772)
    return np.where(missing, np.nan, mu), np.where(missing, np.nan, sigma)


def _expand(levels, ndim):
    levels = np.asarray(levels, dtype=F64)
    return levels.reshape(levels.shape + (1,) * ndim)


def _params(mu, sigma):
    mu, sigma = np.broadcast_arrays(np.asarray(mu, dtype=F64), np.asarray(sigma, dtype=F64))
    return mu, sigma


def cdf(mu, sigma, x):
    mu, sigma = _params(mu, sigma)
    with np.errstate(all="ignore"):
        return np.asarray(1.0 - np.exp(-np.exp((mu - _expand(x, mu.ndim)) / sigma)))


def ppf(mu, sigma, p):
    mu, sigma = _params(mu, sigma)
    with np.errstate(all="ignore"):
        return np.asarray(mu - sigma * np.log(-np.log(1.0 - _expand(p, mu.ndim))))


def value_to_return_period(mu, sigma, freq, value):
    with np.errstate(all="ignore"):
        return np.asarray((1.0 if freq is None else float(freq)) / cdf(mu, sigma, value))


def return_period_to_value(mu, sigma, freq, return_period):
    with np.errstate(all="ignore"):
        return ppf(mu, sigma, (1.0 if freq is None else float(freq)) / np.asarray(return_period, dtype=F64))


# ---- judges ----
def _same_layout(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        raise Mismatch(f"{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}")
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        raise Mismatch(f"{what}: NaN pattern differs at {int(np.sum(np.isnan(got) != np.isnan(want)))} points")
    return got, want


def _file(ledger, what, kind, used, n):
    print(f"{what}: {used:.3f} of its bound used ({n} values)")
    if ledger is not None:
        ledger.append((what, kind, used, 1.0, n))
    return used


def judge_fit_exact(got, want, what=""):
    """(mu, sigma) pairs, bit for bit with the same NaN pattern."""
    judge_exact(got[0], want[0], what + " mu")
    judge_exact(got[1], want[1], what + " sigma")


def judge_fit_bound(got, want, sample_first, nonfinite, what="", ledger=None):
    """got: (mu, sigma) of a reference path on the sample's own dtype; want: recording (c); sample_first: the sample
    with its axis first.  Every all-finite column is compared, mu and sigma each, within
    2 n (eps_ref + 2^-52) max|x|; `nonfinite` (the generator's list) marks the columns left out."""
    sample_first = np.asarray(sample_first)
    n = sample_first.shape[0]
    eps_ref = 2.0 ** -23 if sample_first.dtype == F32 else 2.0 ** -52
    finite = ~np.asarray(nonfinite, bool)
    assert np.array_equal(finite, np.isfinite(sample_first.astype(F64)).all(axis=0)), "the generator's list is not the non-finite columns"
    bound = 2.0 * n * (eps_ref + 2.0 ** -52) * np.max(np.abs(sample_first.astype(F64)), axis=0, initial=0.0, where=np.isfinite(sample_first.astype(F64)))
    used = 0.0
    for name, g, w in (("mu", got[0], want[0]), ("sigma", got[1], want[1])):
        g, w = np.asarray(g, F64), np.asarray(w, F64)
        if g.shape != w.shape:
            raise Mismatch(f"{what} {name}: shape {g.shape} against {w.shape}")
        if np.isnan(g[finite]).any() or np.isnan(w[finite]).any():
            raise Mismatch(f"{what} {name}: NaN in an all-finite column")
        err = np.abs(g[finite] - w[finite])
        if not (err <= bound[finite]).all():
            i = int(np.argmax(err - bound[finite]))
            raise Mismatch(f"{what} {name}: |{g[finite][i]!r} - {w[finite][i]!r}| = {err[i]:.3e} > {bound[finite][i]:.3e}")
        used = max(used, float(np.max(np.where(bound[finite] > 0, err / np.maximum(bound[finite], 1e-300), 0.0), initial=0.0)))
    return _file(ledger, what, FIT_KIND, used, 2 * int(finite.sum()))


def judge_cdf(got, want, what="", ledger=None):
    got, want = _same_layout(got, want, what)
    err = np.where(np.isnan(want), 0.0, np.abs(got - want))
    if not (err <= CDF_BOUND).all():
        i = int(np.argmax(err))
        raise Mismatch(f"{what}: |{got.reshape(-1)[i]!r} - {want.reshape(-1)[i]!r}| = {err.reshape(-1)[i]:.3e} > {CDF_BOUND:.3e}")
    return _file(ledger, what, CDF_KIND, float(np.max(err, initial=0.0)) / CDF_BOUND, err.size)


def judge_return_period(got, want, cdf_ref, freq, what="", ledger=None):
    """want = freq / cdf_ref, the reference's; cdf_ref the reference's cdf at the same points."""
    got, want = _same_layout(got, want, what)
    cdf_ref = np.broadcast_to(np.asarray(cdf_ref, F64), want.shape)
    freq = 1.0 if freq is None else float(freq)
    zero = cdf_ref == 0
    with np.errstate(all="ignore"):
        ok_zero = np.isinf(got) | (got >= freq / CDF_BOUND)
        bound = np.abs(want) * (CDF_BOUND / cdf_ref + 4 * U)
        err = np.abs(got - want)
    rest = ~zero & ~np.isnan(want)
    if not ok_zero[zero].all():
        i = int(np.flatnonzero(zero.reshape(-1) & ~ok_zero.reshape(-1))[0])
        raise Mismatch(f"{what}: {got.reshape(-1)[i]!r} where the reference's cdf is 0 (needs inf or >= {freq / CDF_BOUND:.3e})")
    bad = rest & ~(err <= bound)
    if bad.any():
        i = int(np.flatnonzero(bad.reshape(-1))[0])
        raise Mismatch(f"{what}: |{got.reshape(-1)[i]!r} - {want.reshape(-1)[i]!r}| = {err.reshape(-1)[i]:.3e} > {bound.reshape(-1)[i]:.3e}")
    with np.errstate(all="ignore"):
        used = float(np.max(np.where(rest & (bound > 0), err / bound, 0.0), initial=0.0))
    return _file(ledger, what, RP_KIND, used, int(rest.sum()))


# ---- golden file ----
@functools.lru_cache(maxsize=1)
def _load():
    with np.load(PATH) as f:
        meta = json.loads(bytes(f["manifest"]).decode())
        arrays = {k: f[k] for k in f.files if k != "manifest"}
    return meta, arrays


def meta():
    return _load()[0]


def signatures():
    return _load()[0]["signatures"]


def cases(func=None):
    return [c for c in _load()[0]["cases"] if func is None or c["func"] == func]


def fit_cases():
    """The fit cases the reference computes (not the error cases)."""
    return [c for c in cases("fit") if not c["note"].startswith("error")]


def fit_error_cases():
    return [c for c in cases("fit") if c["note"].startswith("error")]


def call_cases(*funcs):
    return [c for c in _load()[0]["cases"] if c["func"] in funcs]


def case_id(case):
    return f"{case['id']}-{case['func']}-{case['note'].replace(' ', '_')}"


def sample_of(case):
    return _load()[1][case["arrays"]["sample"]]


def recorded_fit(case, which):
    """(mu, sigma) of recording "a", "b" or "c"; None where the reference raised."""
    r = case[which]
    return None if r["raises"] else (_load()[1][r["mu"]], _load()[1][r["sigma"]])


def nonfinite_of(case):
    return _load()[1][case["nonfinite"]]


def _plain(v):
    return datetime.timedelta(seconds=v[1]) if isinstance(v, list) and v and v[0] == "timedelta" else v


def call_args(case):
    """dict(mu, sigma, freq, arg) of a cdf / ppf / return-period case."""
    arrays = _load()[1]
    arg = arrays[case["arrays"]["arg"]] if "arg" in case["arrays"] else _plain(case["plain"]["arg"])
    return dict(mu=arrays[case["arrays"]["mu"]], sigma=arrays[case["arrays"]["sigma"]], freq=_plain(case["plain"]["freq"]), arg=arg)


def expected_of(case):
    return _load()[1][case["out"]] if case["out"] else None


def is_timedelta_case(case):
    return isinstance(case["plain"]["freq"], list)


def judge_call(case, got, what="", ledger=None):
    """A cdf / ppf / return-period result against the recorded reference, by the rule of its function.  The reference
    result of f32 parameters is float64 here as well (the recorded levels are float64)."""
    want = expected_of(case)
    func = case["func"]
    if func in ("ppf", "return_period_to_value"):
        return judge_exact(got, want, what)
    if func == "cdf":
        return judge_cdf(got, want, what, ledger)
    return judge_return_period(got, want, recorded_cdf_of(case), call_args(case)["freq"], what, ledger)


def _levels_key(case):
    return (case["arrays"]["mu"], case["arrays"]["sigma"], case["arrays"].get("arg"), json.dumps(case["plain"].get("arg")))


def recorded_cdf_of(case):
    """The reference's cdf recorded for the distribution and the levels of a value_to_return_period case."""
    twin = next(c for c in cases("cdf") if _levels_key(c) == _levels_key(case))
    return expected_of(twin)
