"""Negative tests of the judges in tests/_regimes_numpy.py: each must reject a result that is wrong in the way it is
there to catch -- off by twice the bar, a NaN moved, an infinity lost, one flipped bit on the bit-for-bit paths, a wrong
dtype, shape or label order -- and accept the recorded reference."""
import numpy as np
import pytest

import _regimes_numpy as rn


def _case(func, needle):
    return next(c for c in rn.cases(func) if needle in c["note"] and not c["raises"])


def _flip_lowest_bit(a, at=0):
    a = np.array(a, copy=True)
    raw = a.reshape(-1).view(f"u{a.dtype.itemsize}")
    raw[at] ^= 1
    return a


PROJECT = [_case("project", n) for n in ("constant (5, 13) fields (5,)", "modulated (5, 13) fields (5,)", "perfield (5, 13)", "a field with NaN float32",
                                         "a field with inf float64")]


@pytest.mark.parametrize("case", PROJECT, ids=rn.case_id)
def test_project_judge_rejects(case):
    want = {k: np.array(v, copy=True) for k, v in rn.recorded(case).items()}
    rn.judge_project(case, want, "the reference passes")
    exact, bar = rn.project_exact_and_bar(case)
    label = case["plain"]["labels"][-1]
    T = want[label].dtype
    fin = np.flatnonzero(np.isfinite(exact[label].reshape(-1)))
    i = int(fin[0])

    def broken(change):
        got = {k: v.copy() for k, v in want.items()}
        change(got)
        return got

    def off_by_twice_the_bar(got):
        got[label].reshape(-1)[i] = (exact[label].reshape(-1)[i] + 2 * bar[label].reshape(-1)[i] + np.spacing(np.abs(exact[label].reshape(-1)[i]).astype(T))).astype(T)

    def nan_moved(got):
        got[label].reshape(-1)[i] = np.nan

    for change in (off_by_twice_the_bar, nan_moved):
        with pytest.raises(rn.Mismatch):
            rn.judge_project(case, broken(change), change.__name__)
    with pytest.raises(rn.Mismatch, match="result is"):
        rn.judge_project(case, {k: v.astype(np.float64 if T == np.float32 else np.float32) for k, v in want.items()}, "dtype")
    with pytest.raises(rn.Mismatch, match="shape"):
        rn.judge_project(case, {k: v.reshape(-1)[:-1] for k, v in want.items()}, "shape")
    if len(want) > 1:
        with pytest.raises(rn.Mismatch, match="labels"):
            rn.judge_project(case, dict(reversed(list(want.items()))), "label order")
    notfin = np.flatnonzero(~np.isfinite(exact[label].reshape(-1)))
    if notfin.size:  # a NaN or an infinity replaced by a number
        def made_finite(got):
            got[label].reshape(-1)[notfin[0]] = 1.0
        with pytest.raises(rn.Mismatch):
            rn.judge_project(case, broken(made_finite), "made finite")


@pytest.mark.parametrize("needle", ["float32 (51, 63) axis 0", "float64 (9, 65) axis 0", "float64 (3, 9, 63) axis 1", "float32 special columns axis 0"])
def test_pearson_bit_for_bit_judge_rejects_one_flipped_bit(needle):
    case = _case("pearson_correlation", needle)
    a, axis, want = rn.arrays_of(case), case["plain"]["axis"], rn.recorded(case)
    rn.judge_pearson(a["x"], a["y"], axis, want, want, "the reference passes")
    at = int(np.flatnonzero(np.isfinite(want.reshape(-1)))[-1])
    with pytest.raises(rn.Mismatch, match="values differ"):
        rn.judge_pearson(a["x"], a["y"], axis, _flip_lowest_bit(want, at), want, "one bit")
    moved = want.copy()
    moved.reshape(-1)[at] = np.nan
    with pytest.raises(rn.Mismatch, match="NaN pattern"):
        rn.judge_pearson(a["x"], a["y"], axis, moved, want, "a NaN moved")
    with pytest.raises(rn.Mismatch):
        rn.judge_pearson(a["x"], a["y"], axis, want.astype(np.float64 if want.dtype == np.float32 else np.float32), want, "dtype")


@pytest.mark.parametrize("needle", ["float32 (3, 257) axis -1", "float64 (3, 51) axis -1", "float32 (2, 2, 257) axis -1", "float64 special columns axis -1"])
def test_pearson_bar_judge_rejects(needle):
    case = _case("pearson_correlation", needle)
    a, axis, want = rn.arrays_of(case), case["plain"]["axis"], rn.recorded(case)
    _, m, inner = rn.layout(a["x"].shape, axis)
    assert inner == 1
    assert rn.judge_pearson(a["x"], a["y"], axis, want, want, "the reference passes") <= 1.0
    at = int(np.flatnonzero(np.isfinite(want.reshape(-1)))[0])
    exact = rn.pearson_exact(a["x"], a["y"], axis).reshape(-1)[at]
    off = want.copy()
    off.reshape(-1)[at] = want.dtype.type(exact + 2 * rn.pearson_bar(m, want.dtype) + np.finfo(want.dtype).eps)
    with pytest.raises(rn.Mismatch, match="bar"):
        rn.judge_pearson(a["x"], a["y"], axis, off, want, "off by twice the bar")
    moved = want.copy()
    moved.reshape(-1)[at] = np.nan
    with pytest.raises(rn.Mismatch, match="NaN pattern"):
        rn.judge_pearson(a["x"], a["y"], axis, moved, want, "a NaN moved")
    with pytest.raises(rn.Mismatch):
        rn.judge_pearson(a["x"], a["y"], axis, want.reshape(-1)[:-1], want, "shape")


@pytest.mark.parametrize("needle", ["float32 array mean and std", "float64 std of 0"])
def test_regime_index_judge_rejects_one_flipped_bit(needle):
    case = _case("regime_index", needle)
    want = rn.recorded(case)
    rn.judge_index(want, want, "the reference passes")
    label = case["plain"]["labels"][0]
    at = int(np.flatnonzero(np.isfinite(want[label].reshape(-1)))[0])
    with pytest.raises(rn.Mismatch, match="values differ"):
        rn.judge_index({**want, label: _flip_lowest_bit(want[label], at)}, want, "one bit")
    moved = want[label].copy()
    moved.reshape(-1)[at] = np.nan
    with pytest.raises(rn.Mismatch, match="NaN pattern"):
        rn.judge_index({**want, label: moved}, want, "a NaN moved")
    with pytest.raises(rn.Mismatch, match="labels"):
        rn.judge_index(dict(reversed(list(want.items()))), want, "label order")
