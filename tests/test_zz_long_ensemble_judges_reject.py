"""The judges of the long-axis ensemble tests reject what a defect would produce: `_long_ensemble.judge_case` (every
function's recorded cases; for the fit both of its arrays) and `judge_exact` as the GPU tests call it directly.  Each must
raise on a change of one ulp, on a NaN that moved, on a wrong dtype, on a wrong shape and on the other zero, and accept
the recorded result itself.  No GPU involved."""
import numpy as np
import pytest

import _long_ensemble as le


def _arrays(want):
    return list(want) if isinstance(want, tuple) else [want]


def _with(want, k, array):
    """`want` with its k-th array replaced."""
    if not isinstance(want, tuple):
        return array
    out = list(want)
    out[k] = array
    return tuple(out)


def _one_ulp(a):
    """`a` with its first finite non-zero value moved to its neighbour."""
    b = a.copy().reshape(-1)
    i = int(np.flatnonzero(np.isfinite(b) & (b != 0))[0])
    b[i] = np.nextafter(b[i], b.dtype.type(np.inf))
    assert b[i] != a.reshape(-1)[i]
    return b.reshape(a.shape)


def _moved_nan(a):
    """`a` with a NaN taken from one point and put on a point that had a number."""
    b = a.copy().reshape(-1)
    nan, num = np.flatnonzero(np.isnan(b)), np.flatnonzero(np.isfinite(b))
    b[nan[0]], b[num[0]] = b[num[0]], np.nan
    assert int(np.isnan(b).sum()) == int(np.isnan(a).sum())
    return b.reshape(a.shape)


@pytest.mark.parametrize("func", le.FUNCS)
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_judge_case_rejects_one_ulp_a_moved_nan_and_a_wrong_dtype(func, tag):
    case = next(c for c in le.cases(func, tag) if " m 300" in c["note"])
    want = le.expected_of(case)
    le.judge_case(case, want)  # the recorded result itself passes, so what follows is rejected for the defect alone
    for k, a in enumerate(_arrays(want)):
        assert np.isnan(a).any() and np.isfinite(a).any()
        other = np.float32 if a.dtype == np.float64 else np.float64
        zeroed = a.copy()
        zeroed[np.flatnonzero(np.isfinite(a))[0]] = 0.0
        for name, bad in (("one ulp", _one_ulp(a)), ("moved NaN", _moved_nan(a)), ("dtype", a.astype(other)), ("shape", a[:-1]),
                          ("no NaN", np.where(np.isnan(a), 0, a).astype(a.dtype)), ("all NaN", np.full_like(a, np.nan))):
            with pytest.raises(le.Mismatch):
                le.judge_case(case, _with(want, k, bad), name)
        le.judge_exact(zeroed, zeroed)
        with pytest.raises(le.Mismatch):  # the sign of a zero counts
            le.judge_exact(-zeroed, np.where(zeroed == 0, 0.0, -zeroed).astype(a.dtype), "the other zero")


@pytest.mark.parametrize("T", [le.F32, le.F64], ids=["f32", "f64"])
def test_judge_exact_rejects_one_ulp_a_moved_nan_and_a_wrong_dtype(T):
    want = np.array([1.5, -2.25, np.nan, 0.0, np.inf, 3.0], T)
    le.judge_exact(want.copy(), want)
    other = np.float32 if T == le.F64 else np.float64
    minus_zero = want.copy()
    minus_zero[3] = -0.0
    for bad in (_one_ulp(want), _moved_nan(want), want.astype(other), want[:-1], minus_zero):
        with pytest.raises(le.Mismatch):
            le.judge_exact(bad, want)


def test_a_fit_result_is_judged_through_its_attributes_too():
    """The GPU tests hand `judge_case` a distribution: an object with .mu and .sigma."""
    case = le.cases("fit", "f64")[0]
    mu, sigma = le.expected_of(case)

    class Dist:
        pass

    d = Dist()
    d.mu, d.sigma = mu, sigma
    le.judge_case(case, d)
    d.sigma = _one_ulp(sigma)
    with pytest.raises(le.Mismatch):
        le.judge_case(case, d)
