"""Negative tests of the judge in tests/_nanaverage_numpy.py: along the contiguous axis it must reject a result that is
wrong in a way an average can be wrong -- one valid element dropped, one NaN counted as a sample, divided by m instead of
the valid count, unnormalised weights, NaN in place of the weighted all-NaN 0.0 -- and accept the correct one.  The data
is temperature-like (280 +- 5) with m >= 9, so each of those errors is many times the bar."""
import numpy as np
import pytest

import _nanaverage_numpy as nn


# (f32 at m = 257: the bar, 0.017 K, is no longer many times below the effect of one dropped element, 0.04 K)
CASES = [(nn.F32, 9), (nn.F32, 51), (nn.F64, 9), (nn.F64, 51), (nn.F64, 257)]


def _data(T, m, rows=4, seed=0):
    rng = np.random.default_rng(seed + m)
    x = (280 + rng.normal(0, 5, (rows, m))).astype(T)
    x[:, 0] = 290.0  # the element the tests drop: two standard deviations off the mean
    x[:, 2] = np.nan
    x[1, 5] = np.nan
    w = (0.5 + rng.uniform(0, 1, m)).astype(T)
    return x, w


def test_judge_rejects_wrong_averages():
    for T, m in CASES:
        _unweighted(T, m)
        _weighted(T, m)


def _unweighted(T, m):
    x, _ = _data(T, m)
    good = nn.numpy_formula(x, axis=1)
    assert nn.judge(x, None, 1, good, good, "the correct result passes") <= 1.0
    valid = ~np.isnan(x)
    dropped = x.copy()
    dropped[:, 0] = np.nan  # element 0 is valid in every row
    wrong = {
        "one valid element dropped": nn.numpy_formula(dropped, axis=1),
        "one NaN counted as a sample": (np.nansum(x, axis=1) / (valid.sum(axis=1) + 1)).astype(T),
        "divided by m": (np.nansum(x, axis=1) / m).astype(T),
    }
    for what, got in wrong.items():
        with pytest.raises(nn.Mismatch, match="bar"):
            nn.judge(x, None, 1, got.astype(T), good, what)
    moved = good.copy()
    moved[0] = np.nan
    with pytest.raises(nn.Mismatch, match="NaN pattern"):
        nn.judge(x, None, 1, moved, good, "a NaN moved")
    with pytest.raises(nn.Mismatch):
        nn.judge(x, None, 1, good.astype(nn.F64 if T == nn.F32 else nn.F32), good, "dtype")
    with pytest.raises(nn.Mismatch):
        nn.judge(x, None, 1, good[:-1], good, "shape")


def _weighted(T, m):
    x, w = _data(T, m)
    x[3] = np.nan  # an all-NaN row: 0.0 with weights
    good = nn.numpy_formula(x, w, axis=1)
    assert good[3] == 0.0
    assert nn.judge(x, w, 1, good, good, "the correct result passes") <= 1.0
    valid = ~np.isnan(x)
    dropped = x.copy()
    dropped[:, 0] = np.nan
    wsum = np.where(valid, w, 0).sum(axis=1)
    wrong = {
        "one valid element dropped": nn.numpy_formula(dropped, w, axis=1),
        "one NaN counted as a sample": np.nansum(x * w, axis=1) / np.where(wsum == 0, 1, wsum + w[2]),
        "divided by the sum of all weights": np.nansum(x * w, axis=1) / w.sum(),
        "unnormalised weights": np.nansum(x * w, axis=1),
    }
    for what, got in wrong.items():
        with pytest.raises(nn.Mismatch, match="bar"):
            nn.judge(x, w, 1, got.astype(T), good, what)
    nan_for_zero = good.copy()
    nan_for_zero[3] = np.nan
    with pytest.raises(nn.Mismatch, match="NaN pattern"):
        nn.judge(x, w, 1, nan_for_zero, good, "NaN in place of the weighted all-NaN 0.0")


def test_infinities_the_bit_for_bit_path_and_cancelling_weights(capsys):
    x, w = _data(nn.F64, 9)
    x[0, 0] = np.inf
    good = nn.numpy_formula(x, w, axis=1)
    nn.judge(x, w, 1, good, good, "an infinite mean passes")
    lost = good.copy()
    lost[0] = 1e300
    with pytest.raises(nn.Mismatch):
        nn.judge(x, w, 1, lost, good, "an infinity lost")
    flipped = -good
    with pytest.raises(nn.Mismatch):
        nn.judge(x, w, 1, flipped, good, "the other infinity")
    # inner > 1: one flipped bit is a mismatch
    xt = np.ascontiguousarray(x[1:].T)
    want = nn.numpy_formula(xt, axis=0)
    nn.judge(xt, None, 0, want, want, "the recording passes")
    off = want.copy()
    off.view(np.uint64)[0] ^= 1
    with pytest.raises(nn.Mismatch, match="values differ"):
        nn.judge(xt, None, 0, off, want, "one bit")
    # cancelling weights are reported as not judged
    capsys.readouterr()
    x = np.array([[280.0, 281.0, 279.0, 282.0]])
    w = np.array([1.0, -1.0, 2.0, -2.0])
    _, _, judged = nn.exact_and_bar(x, w, 1, nn.F64)
    assert not judged.any()
    nn.judge(x, w, 1, np.array([np.inf]), np.array([np.nan]), "cancelling weights")
    assert "not judged" in capsys.readouterr().out
    _, bar, judged = nn.exact_and_bar(x, np.array([1.0, -0.5, 2.0, 0.25]), 1, nn.F64)
    assert judged.all() and bar[0] > 0
