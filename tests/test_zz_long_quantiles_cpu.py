"""stats.long_quantiles without a GPU: the host twin of the kernel (std::sort on the kernel's whole-number keys, then
quantile_point of csrc/ensemble_point.hpp) and the NumPy restatement `_quantiles_numpy.quantiles`, imported unchanged,
against the rows recorded from the reference on sample axes of 257 to 1980 values
(tests/golden/long_quantiles_golden.npz); the order of the keys; the public signatures and the errors that need no device.

Parity: bit for bit, with identical NaN pattern and result dtype, no point excluded, all three methods, f32 and f64."""
import inspect

import numpy as np
import pytest

import _long_quantiles as lq
from ekm_hip import stats

CASES = lq.cases()
GROUPS = [f"{tag} {method}" for tag in ("f32", "f64") for method in lq.METHODS]  # 39 recorded cases each


@pytest.mark.parametrize("group", GROUPS)
def test_host_twin_against_the_recorded_reference(group):
    cases = lq.cases_of(group)
    assert len(cases) == 39
    for case in cases:
        lq.judge_case(case, lq.twin(**lq.kwargs_of(case)), "twin " + lq.case_id(case))


@pytest.mark.parametrize("group", GROUPS)
def test_restatement_against_the_recorded_reference(group):
    """This is what makes `_quantiles_numpy.quantiles` the reference of the GPU census at 1980 samples."""
    for case in lq.cases_of(group):
        lq.judge_case(case, lq.quantiles(**lq.kwargs_of(case)), "restatement " + lq.case_id(case))


def test_every_case_the_issue_names_is_recorded():
    notes = [c["note"] for c in CASES]
    for tag in ("f32", "f64"):
        for method in lq.METHODS:
            for which in (100, [0.9, 0.0, 0.33], 1):
                for m in (257, 300, 512, 513, 1980):
                    for kind in ("ties", "smooth"):
                        assert f"{tag} m {m} {kind} {method} which {which}" in notes
                for where in ("first", "last", "middle"):
                    assert f"{tag} m 300 special axis {where} {method} which {which}" in notes
    assert all(lq.kwargs_of(c)["arr"].shape[c["plain"].get("axis", 0)] > 256 for c in CASES)
    case = next(c for c in CASES if c["note"] == "f64 m 300 special axis first sort which 100")
    arr, want = lq.kwargs_of(case)["arr"], lq.expected_of(case)
    assert (arr[:, 0] == arr[0, 0]).all() and np.isnan(arr[:, 1]).any() and arr[:, 2].max() == np.inf and arr[:, 3].min() == -np.inf
    assert np.isnan(want[:, 1]).all() and want[0, 3] == -np.inf
    assert np.isnan(want[100, 2]) and np.isfinite(want[99, 2])  # "sort": inf * 0 at the top level, as in the reference
    for c in CASES:  # no column mixes the two zeros
        a = lq.kwargs_of(c)["arr"]
        a = np.moveaxis(a, c["plain"].get("axis", 0), 0).reshape(a.shape[c["plain"].get("axis", 0)], -1)
        neg, pos = (a == 0) & np.signbit(a), (a == 0) & ~np.signbit(a)
        assert not (neg.any(axis=0) & pos.any(axis=0)).any()


@pytest.mark.parametrize("T", [lq.F32, lq.F64], ids=["f32", "f64"])
def test_the_keys_put_minus_zero_before_plus_zero_and_keep_the_order_of_the_numbers(T):
    rng = np.random.default_rng(4)
    x = np.concatenate([rng.normal(0, 1, 200), [0.0, -0.0, 0.0, -0.0, -0.0, np.inf, -np.inf], np.ldexp(1.0, [-140, -1060][T == lq.F64]) * np.array([1, -1])])
    x = rng.permutation(x).astype(T)
    s = lq.sort_by_key(x)
    assert np.array_equal(s, np.sort(x))  # as values (the two zeros compare equal)
    zeros = s[s == 0]
    assert zeros.size == 5 and np.signbit(zeros[:3]).all() and not np.signbit(zeros[3:]).any()
    # through the entry point, "sort": level 0 is s[0] * 1 + s[1] * 0, which is -0.0 only when BOTH are -0.0; the levels
    # that touch the +0.0 in third place give +0.0 -- in whatever order the three come in
    for perm in ([0.0, -0.0, -0.0], [-0.0, 0.0, -0.0], [-0.0, -0.0, 0.0]):
        got = lq.twin(np.array(perm, T), [0.0, 0.5, 1.0], 0, "sort")
        assert np.signbit(got).tolist() == [True, False, False]
    y = np.concatenate([x, [np.nan]]).astype(T)
    assert np.isnan(lq.sort_by_key(y)[-1])  # a NaN takes the largest key


def test_signatures_are_the_references():
    assert str(inspect.signature(stats.long_quantiles)) == lq.signature()
    assert str(inspect.signature(stats.iter_long_quantiles)) == lq.signature()
    assert inspect.isgeneratorfunction(stats.iter_long_quantiles) and not inspect.isgeneratorfunction(stats.long_quantiles)


def test_argument_errors_need_no_device():
    arr = np.zeros((300, 2))
    gen = stats.iter_long_quantiles(arr, method="bogus")  # nothing runs yet, as in the reference
    with pytest.raises(ValueError, match="Invalid method 'bogus', expected 'sort', 'numpy_bulk', or 'numpy'"):
        next(gen)
    for fn in (stats.long_quantiles, lambda *a, **k: list(stats.iter_long_quantiles(*a, **k))):
        with pytest.raises(ValueError, match="Invalid method"):
            fn(arr, method="median")
        for levels in ([0.5, 1.5], [-0.25, 0.5], [0.5, float("nan")]):
            for method in lq.METHODS:
                with pytest.raises(ValueError, match=r"Quantiles must be in the range \[0, 1\]"):
                    fn(arr, levels, 0, method)
        with pytest.raises(np.exceptions.AxisError):
            fn(arr, axis=2)
        with pytest.raises(np.exceptions.AxisError):
            fn(arr, axis=-3)
        with pytest.raises(ValueError):
            fn(np.zeros((0, 2)))
        with pytest.raises(ValueError):
            fn(np.float64(1.0))
        with pytest.raises(ValueError):
            fn(arr, which=[[0.5]])


def test_no_result_without_work_needs_no_device():
    got = stats.long_quantiles(np.zeros((700, 3), np.float32), which=[], method="numpy")
    assert got.shape == (0, 3) and got.dtype == np.float32
    assert stats.long_quantiles(np.zeros((700, 0)), which=4).shape == (5, 0)
    assert list(stats.iter_long_quantiles(np.zeros((700, 3)), [], axis=0)) == []


def test_long_and_short_share_their_host_code(monkeypatch):
    """One body: the two public functions differ in the family of entry points they name, nothing else."""
    seen = []
    monkeypatch.setattr(stats, "_quantiles", lambda *a: seen.append(a) or "r")
    a = np.zeros((3, 2))
    assert stats.quantiles(a, 4, 1, "numpy") == "r" and stats.long_quantiles(a, 4, 1, "numpy") == "r"
    assert seen[0][1:] == (4, 1, "numpy", "ekm_quantiles_") and seen[1][1:] == (4, 1, "numpy", "ekm_long_quantiles_")
