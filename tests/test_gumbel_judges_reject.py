"""The Gumbel judges of tests/_gumbel_numpy.py must reject what they exist to catch: each case below hands a judge a
result that is wrong in one way and expects `Mismatch` (after the right result has passed)."""
import numpy as np
import pytest

import _gumbel_numpy as gn

MU = np.array([20.0, 18.5, 23.25, 21.0, 19.0, 22.0])
SIGMA = np.array([5.0, 4.5, 6.0, 5.5, 4.0, 5.25])
X = np.array([10.0, 31.5, 60.0])


def _ulp(a, i):
    b = np.array(a, copy=True)
    b.reshape(-1).view(np.uint64)[i] += 1
    return b


def _sample():
    return np.random.default_rng(4).gumbel(20, 5, (51, 6))


def test_one_ulp_where_bits_are_required():
    fit = gn.fit(_sample())
    gn.judge_fit_exact(fit, fit, "the same")
    with pytest.raises(gn.Mismatch):
        gn.judge_fit_exact((_ulp(fit[0], 2), fit[1]), fit, "mu one ulp off")
    with pytest.raises(gn.Mismatch):
        gn.judge_fit_exact((fit[0], _ulp(fit[1], 5)), fit, "sigma one ulp off")
    ppf = gn.ppf(MU, SIGMA, [0.5, 0.99])
    gn.judge_exact(ppf, ppf, "the same")
    with pytest.raises(gn.Mismatch):
        gn.judge_exact(_ulp(ppf, 7), ppf, "ppf one ulp off")
    case = next(c for c in gn.cases("return_period_to_value") if c["note"] == "plain return period 1-d freq 0.5")
    want = gn.expected_of(case)
    gn.judge_call(case, want, "the same")
    with pytest.raises(gn.Mismatch):
        gn.judge_call(case, _ulp(want, 30), "return_period_to_value one ulp off")
    with pytest.raises(gn.Mismatch):
        gn.judge_call(case, want.astype(np.float32), "another dtype")


def test_a_cdf_off_by_1e_12():
    want = gn.cdf(MU, SIGMA, X)
    gn.judge_cdf(want + 4 * gn.U, want, "half the bound")
    bad = want.copy()
    bad[1, 3] += 1e-12
    with pytest.raises(gn.Mismatch):
        gn.judge_cdf(bad, want, "off by 1e-12")
    case = next(c for c in gn.cases("cdf") if c["note"] == "plain levels 1-d")
    bad = gn.expected_of(case).copy()
    bad[0, 0] += 1e-12  # where the cdf itself is below 1e-12
    with pytest.raises(gn.Mismatch):
        gn.judge_call(case, bad, "off by 1e-12 in the far tail")


def test_a_return_period_off_by_4e_11_on_a_cdf_of_1e_9():
    """What an exponential good to 4e-11 relative would give: the subtraction from 1 makes that absolute."""
    mu, sigma = np.array([20.0]), np.array([5.0])
    x = mu - sigma * np.log(1e-9)  # exp((mu - x) / sigma) = 1e-9, so the cdf is 1e-9
    cdf = gn.cdf(mu, sigma, x)
    assert abs(cdf[0, 0] - 1e-9) < 1e-15
    want = gn.value_to_return_period(mu, sigma, 2.0, x)
    gn.judge_return_period(want, want, cdf, 2.0, "the same")
    gn.judge_return_period(2.0 / (cdf + 4 * gn.U), want, cdf, 2.0, "half the bound")
    with pytest.raises(gn.Mismatch):
        gn.judge_return_period(2.0 / (cdf + 4e-11), want, cdf, 2.0, "a cdf off by 4e-11")
    with pytest.raises(gn.Mismatch):
        gn.judge_return_period(2.0 / (cdf - 4e-11), want, cdf, 2.0, "a cdf off by -4e-11")
    # where the reference's cdf is 0 its return period is inf: inf or beyond freq / (8 * 2^-53) passes, less does not
    zero, inf = np.zeros((1, 1)), np.full((1, 1), np.inf)
    gn.judge_return_period(inf, inf, zero, 2.0, "inf")
    gn.judge_return_period(np.full((1, 1), 2.0 / (4 * gn.U)), inf, zero, 2.0, "a cdf of half the bound")
    with pytest.raises(gn.Mismatch):
        gn.judge_return_period(np.full((1, 1), 2.0 / 1e-12), inf, zero, 2.0, "a cdf of 1e-12 where the reference has 0")


def test_mu_and_sigma_swapped():
    fit = gn.fit(_sample())
    with pytest.raises(gn.Mismatch):
        gn.judge_fit_exact((fit[1], fit[0]), fit, "swapped")
    sample = _sample()
    nonfinite = np.zeros(6, np.uint8)
    gn.judge_fit_bound(fit, fit, sample, nonfinite, "the same")
    with pytest.raises(gn.Mismatch):
        gn.judge_fit_bound((fit[1], fit[0]), fit, sample, nonfinite, "swapped, against the bound")
    want = gn.cdf(MU, SIGMA, X)
    with pytest.raises(gn.Mismatch):
        gn.judge_cdf(gn.cdf(SIGMA, MU, X), want, "cdf of the swapped parameters")
    with pytest.raises(gn.Mismatch):
        gn.judge_exact(gn.ppf(SIGMA, MU, [0.5, 0.99]), gn.ppf(MU, SIGMA, [0.5, 0.99]), "ppf of the swapped parameters")


def test_a_fit_beyond_the_summation_bound():
    sample = _sample().astype(np.float32)
    fit = gn.fit(sample)
    nonfinite = np.zeros(6, np.uint8)
    bound = 2 * 51 * (2.0 ** -23 + 2.0 ** -52) * np.abs(sample).max(axis=0)
    gn.judge_fit_bound((fit[0] + 0.5 * bound, fit[1]), fit, sample, nonfinite, "half the bound")
    with pytest.raises(gn.Mismatch):
        gn.judge_fit_bound((fit[0] + 2 * bound, fit[1]), fit, sample, nonfinite, "twice the bound")
    with pytest.raises(AssertionError):
        gn.judge_fit_bound(fit, fit, sample, np.array([0, 1, 0, 0, 0, 0], np.uint8), "a finite column listed as left out")


def test_a_nan_moved_to_another_point():
    sample = _sample()
    sample[7, 2] = np.nan
    fit = gn.fit(sample)
    assert np.isnan(fit[0][2]) and np.isnan(fit[1][2])
    moved = fit[0].copy()
    moved[2], moved[3] = fit[0][3], np.nan
    with pytest.raises(gn.Mismatch):
        gn.judge_fit_exact((moved, fit[1]), fit, "a NaN moved")
    mu = MU.copy()
    mu[1] = np.nan
    want = gn.cdf(mu, SIGMA, X)
    got = want.copy()
    got[:, 1], got[:, 4] = want[:, 4], np.nan
    with pytest.raises(gn.Mismatch):
        gn.judge_cdf(got, want, "cdf: a NaN moved")
    rp = gn.value_to_return_period(mu, SIGMA, 1.0, X)
    got = rp.copy()
    got[:, 1], got[:, 4] = rp[:, 4], np.nan
    with pytest.raises(gn.Mismatch):
        gn.judge_return_period(got, rp, want, 1.0, "return period: a NaN moved")
    with pytest.raises(gn.Mismatch):
        gn.judge_exact(got, rp, "bits: a NaN moved")
