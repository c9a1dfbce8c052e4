"""stats.GumbelDistribution and the return-period functions without a GPU: the independent NumPy restatement and the
host twin of the kernels' per-point routines (gumbel_fit_point, gumbel_cdf_point, gumbel_ppf_point,
csrc/ensemble_point.hpp) against the results recorded from the reference (tests/golden/gumbel_golden.npz), the public
signatures, the error conventions and the host-side half of the class.

Parity (tests/_gumbel_numpy.py states the bounds and where they come from):
  * fit: bit for bit against recording (c), the reference's polyfill on the sample widened to float64, with the same NaN
    pattern; recordings (a) and (b), the reference on the sample's own dtype through SciPy and through its polyfill, lie
    within 2 n (eps_ref + 2^-52) max|x| of (c) on every all-finite column.  The polyfill refuses 2 and 3 values, so
    there is no (c) for those: the twin equals the restatement bit for bit and (a), where SciPy computes it, is held to
    the restatement by the same bound;
  * ppf and return_period_to_value: bit for bit against the recorded reference;
  * cdf: within 8 * 2^-53; value_to_return_period: within |ref| (8 * 2^-53 / cdf_ref + 4 * 2^-53)."""
import ctypes as C
import datetime
import inspect

import numpy as np
import pytest

import _compare
import _gumbel_numpy as gn
import _hosttwin
from ekm_hip import stats
from ekm_hip.stats import GumbelDistribution  # the class under test: absent before this feature

FIT_CASES = gn.fit_cases()
NUMERIC_CALLS = [c for c in gn.call_cases("cdf", "ppf", "value_to_return_period", "return_period_to_value")
                 if not gn.is_timedelta_case(c)]
TIMEDELTA_CALLS = [c for c in gn.call_cases("value_to_return_period", "return_period_to_value") if gn.is_timedelta_case(c)]


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def twin_fit(sample, axis=0):
    sample = np.asarray(sample)
    T = gn.arith_dtype(sample)
    a = np.ascontiguousarray(sample, T)
    axis %= a.ndim
    m, rest = a.shape[axis], a.shape[:axis] + a.shape[axis + 1:]
    outer, inner = int(np.prod(a.shape[:axis], dtype=np.int64)), int(np.prod(a.shape[axis + 1:], dtype=np.int64))
    mu, sigma = np.full(rest, 7.0), np.full(rest, 7.0)
    fn = getattr(_hosttwin.lib(), "ekm_host_gumbel_fit_" + ("f32" if T == gn.F32 else "f64"))
    fn.restype = C.c_int
    assert fn(_vp(a), C.c_size_t(outer), C.c_uint(m), C.c_size_t(inner), _vp(mu), _vp(sigma)) == 0
    return mu, sigma


def _twin_outer(name, mu, sigma, levels, *extra):
    mu, sigma = (np.array(a, order="C") for a in np.broadcast_arrays(np.asarray(mu, gn.F64), np.asarray(sigma, gn.F64)))
    levels = np.array(levels, gn.F64, order="C")
    out = np.full(levels.shape + mu.shape, 7.0)
    fn = getattr(_hosttwin.lib(), name)
    fn.restype = C.c_int
    assert fn(_vp(mu), _vp(sigma), C.c_size_t(mu.size), _vp(levels), C.c_uint(levels.size), *extra, _vp(out)) == 0
    return out


def twin_call(case):
    kw = gn.call_args(case)
    freq = 1.0 if kw["freq"] is None else float(kw["freq"])
    with np.errstate(all="ignore"):
        if case["func"] == "cdf":
            return _twin_outer("ekm_host_gumbel_cdf_f64", kw["mu"], kw["sigma"], kw["arg"], C.c_double(1.0), C.c_int(0))
        if case["func"] == "value_to_return_period":
            return _twin_outer("ekm_host_gumbel_cdf_f64", kw["mu"], kw["sigma"], kw["arg"], C.c_double(freq), C.c_int(1))
        p = np.asarray(kw["arg"], gn.F64) if case["func"] == "ppf" else freq / np.asarray(kw["arg"], gn.F64)
        return _twin_outer("ekm_host_gumbel_ppf_f64", kw["mu"], kw["sigma"], np.log(-np.log(1.0 - p)))


def restated_call(case):
    kw = gn.call_args(case)
    if case["func"] in ("cdf", "ppf"):
        return getattr(gn, case["func"])(kw["mu"], kw["sigma"], kw["arg"])
    return getattr(gn, case["func"])(kw["mu"], kw["sigma"], kw["freq"], kw["arg"])


# ---- fit ----
@pytest.mark.parametrize("case", FIT_CASES, ids=gn.case_id)
def test_fit_restatement_and_host_twin_against_the_float64_polyfill(case):
    sample, axis = gn.sample_of(case), case["plain"]["axis"]
    restated, twin = gn.fit(sample, axis), twin_fit(sample, axis)
    gn.judge_fit_exact(twin, restated, "host twin against the restatement " + case["note"])
    want = gn.recorded_fit(case, "c")
    if want is None:  # 2 or 3 values: the polyfill refuses them
        assert sample.shape[axis] < 4 and case["c"]["raises"][0] == "ValueError"
        return
    gn.judge_fit_exact(restated, want, "restatement " + case["note"])
    gn.judge_fit_exact(twin, want, "host twin " + case["note"])


@pytest.mark.parametrize("case", FIT_CASES, ids=gn.case_id)
def test_fit_reference_paths_lie_within_the_summation_bound(case):
    sample, axis = gn.sample_of(case), case["plain"]["axis"]
    first = np.moveaxis(sample, axis, 0)
    first = first.astype(gn.arith_dtype(first))
    want = gn.recorded_fit(case, "c") or gn.fit(sample, axis)
    judged = 0
    for which in ("a", "b"):
        got = gn.recorded_fit(case, which)
        if which == "b" and sample.dtype.kind in "iu":
            # the polyfill's sums are zeros_like(sample): on an integer sample they are integers and every quotient is
            # truncated on the store, so (b) is no floating-point sum and the bound's derivation does not cover it
            # (23.1 against 24.3 in the recorded case).  The product computes an integer sample as float64: (c).
            assert got is not None and not np.array_equal(got[0], want[0])
            continue
        if got is not None:
            assert got[0].dtype == got[1].dtype == gn.F64  # float64 either way: numpy.log(2) is a float64 scalar
            gn.judge_fit_bound(got, want, first, gn.nonfinite_of(case), f"recording ({which}) {case['note']}", _compare.LEDGER)
            judged += 1
    assert judged >= 1
    # on the columns left out the product follows recording (c): NaN where it has NaN
    if gn.recorded_fit(case, "c") is not None:
        out = gn.nonfinite_of(case).astype(bool)
        gn.judge_exact(gn.fit(sample, axis)[0][out], want[0][out], "left-out columns " + case["note"])


def test_every_case_the_issue_names_is_recorded():
    notes = [c["note"] for c in gn.cases()]
    for tag, ns in (("f32", (2, 3, 4, 9, 51, 128, 256)), ("f64", (2, 3, 4, 9, 51, 128))):
        for n in ns:
            for kind in ("gumbel", "narrow", "precip"):
                assert f"{tag} n {n} {kind}" in notes
        for axis in (0, 1, 2, -1):
            assert f"{tag} cube axis {axis}" in notes
        assert f"{tag} n 51 special" in notes
    assert "integer input" in notes and len(gn.fit_error_cases()) == 3
    for func in ("cdf", "ppf", "value_to_return_period", "return_period_to_value"):
        assert any("odd sigma" in c["note"] for c in gn.cases(func))
    assert TIMEDELTA_CALLS and any(c["out"] for c in TIMEDELTA_CALLS)
    case = next(c for c in gn.cases("cdf") if c["note"] == "plain levels 1-d")
    kw = gn.call_args(case)
    z = (kw["mu"] - kw["arg"][:, None]) / kw["sigma"]
    assert z.min() < -40 and z.max() > 4
    assert list(gn.call_args(next(c for c in gn.cases("ppf") if c["note"] == "plain p 1-d"))["arg"]) == [0, 1e-12, 0.5, 1 - 1e-12, 1]
    print("recorded with NumPy", gn.meta()["numpy"], "SciPy", gn.meta()["scipy"], "lmoment of", gn.meta()["native_lmoment"])


def test_the_special_columns_hold_what_they_are_meant_to():
    case = next(c for c in FIT_CASES if c["note"] == "f64 n 9 special")
    sample, (mu, sigma) = gn.sample_of(case), gn.recorded_fit(case, "c")
    assert mu[0] == 3.25 and sigma[0] == 0.0                      # all equal
    assert np.isnan(sample[:, 2]).any() and np.isnan(mu[2]) and np.isnan(sigma[2])
    assert np.isinf(sample[:, 4]).any() and np.isnan(sigma[4])    # +inf: inf - inf
    assert np.isinf(sample[:, 5]).any() and np.isnan(mu[5])       # a leading -inf: -inf * 0
    assert list(np.flatnonzero(gn.nonfinite_of(case))) == [2, 3, 4, 5, 6, 7]
    precip = next(c for c in FIT_CASES if c["note"] == "f32 n 51 precip")
    assert (gn.sample_of(precip)[:, 1:3] == 0).all() and (gn.recorded_fit(precip, "c")[1][1:3] == 0).all()


# ---- cdf, ppf and the return periods ----
@pytest.mark.parametrize("case", NUMERIC_CALLS, ids=gn.case_id)
def test_restatement_and_host_twin_against_the_recorded_reference(case):
    assert case["raises"] is None
    gn.judge_call(case, restated_call(case), "restatement " + gn.case_id(case), _compare.LEDGER)
    got = twin_call(case)
    gn.judge_call(case, got, "host twin " + gn.case_id(case), _compare.LEDGER)
    if case["func"] == "value_to_return_period":  # freq / cdf of the same call, bit for bit
        kw = gn.call_args(case)
        cdf = _twin_outer("ekm_host_gumbel_cdf_f64", kw["mu"], kw["sigma"], kw["arg"], C.c_double(1.0), C.c_int(0))
        with np.errstate(all="ignore"):
            gn.judge_exact(got, (1.0 if kw["freq"] is None else float(kw["freq"])) / cdf, "freq / cdf")


def test_twin_refuses_a_bad_mode():
    one = np.ones(1)
    fn = _hosttwin.lib().ekm_host_gumbel_cdf_f64
    fn.restype = C.c_int
    assert fn(_vp(one), _vp(one), C.c_size_t(1), _vp(one), C.c_uint(1), C.c_double(1.0), C.c_int(2), _vp(one)) == -3


# ---- the public interface: what needs no GPU ----
def test_signatures_are_the_references():
    sig = gn.signatures()
    assert str(inspect.signature(GumbelDistribution.__init__)) == sig["GumbelDistribution"]
    assert str(inspect.signature(GumbelDistribution.fit)) == sig["fit"]
    assert str(inspect.signature(GumbelDistribution.cdf)) == sig["cdf"]
    assert str(inspect.signature(GumbelDistribution.ppf)) == sig["ppf"]
    assert str(inspect.signature(stats.value_to_return_period)) == sig["value_to_return_period"]
    assert str(inspect.signature(stats.return_period_to_value)) == sig["return_period_to_value"]


def test_distribution_holds_float64_numpy_arrays_for_numpy_input():
    d = GumbelDistribution(np.arange(6, dtype=np.float32).reshape(2, 3), np.array([1.0, 2.0, 3.0], np.float32), freq=2)
    assert d.shape == (2, 3) and d.ndim == 2 and d.freq == 2
    assert isinstance(d.mu, np.ndarray) and d.mu.dtype == d.sigma.dtype == np.float64 and d.sigma.shape == (2, 3)
    assert np.array_equal(d.sigma, np.broadcast_to([1.0, 2.0, 3.0], (2, 3)))
    s = GumbelDistribution(21, 4.5)
    assert s.shape == () and s.ndim == 0 and s.freq is None and s.mu.dtype == np.float64
    with pytest.raises(ValueError):
        GumbelDistribution(np.zeros(3), np.zeros(4))


@pytest.mark.parametrize("case", gn.fit_error_cases(), ids=gn.case_id)
def test_fit_error_conventions(case):
    """Before any device work: these raise on a machine without a GPU as well, with the exception class the reference
    raises (numpy.exceptions.AxisError is a ValueError)."""
    assert any(case[w]["raises"] and case[w]["raises"][0] in ("ValueError", "AxisError") for w in "abc")
    with pytest.raises(ValueError):
        GumbelDistribution.fit(gn.sample_of(case), axis=case["plain"]["axis"])


def test_fit_without_points_needs_no_device():
    d = GumbelDistribution.fit(np.zeros((5, 0), np.float32), freq=3.0)
    assert d.shape == (0,) and d.mu.dtype == np.float64 and d.freq == 3.0
    assert d.cdf([1.0, 2.0]).shape == (2, 0) and d.ppf(np.zeros((2, 3))).shape == (2, 3, 0)
    assert stats.value_to_return_period(d, 1.0).shape == (0,)
    assert GumbelDistribution(np.ones(4), 2.0).cdf([]).shape == (0, 4)


def test_freq_must_be_none_a_number_or_a_timedelta():
    d = GumbelDistribution(np.ones(0), 1.0, freq="yearly")
    with pytest.raises(TypeError):
        stats.value_to_return_period(d, 1.0)
    with pytest.raises(TypeError):
        stats.return_period_to_value(d, 10.0)
    assert stats.return_period_to_value(GumbelDistribution(np.ones(0), 1.0, freq=datetime.timedelta(days=1)),
                                        datetime.timedelta(days=10)).shape == (0,)
