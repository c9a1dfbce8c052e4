"""stats.iter_quantiles without a GPU: the independent NumPy restatement and the host twin of the kernel's per-point
routine (quantile_point, csrc/ensemble_point.hpp) against the rows recorded from the reference
(tests/golden/quantiles_golden.npz), the public signature and error conventions, the position tables, and the judge.

Parity: bit for bit, with identical NaN pattern and result dtype, no point excluded, all three methods, f32 and f64."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

import _quantiles_numpy as qn
from ekm_hip import stats  # noqa: F401  (the module under test: absent before this feature)
import _hosttwin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUE_CASES = qn.value_cases()
ERROR_CASES = [c for c in qn.cases() if c["raises"] or "deviation" in c]


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def twin(arr, which=100, axis=0, method="sort"):
    """One call through the host twin: the argument handling of ekm_hip.stats restated for the twin's C entry points
    (dtype choice, [outer, m, inner] view of the array, position tables from the restatement's scalar expression)."""
    arr = np.asarray(arr)
    T = qn.arith_dtype(arr)
    out_dtype = T if method == "numpy" else qn.F64
    a = np.ascontiguousarray(arr, T)
    axis %= a.ndim
    m, rest = a.shape[axis], a.shape[:axis] + a.shape[axis + 1:]
    outer, inner = int(np.prod(a.shape[:axis], dtype=np.int64)), int(np.prod(a.shape[axis + 1:], dtype=np.int64))
    pos = [qn.positions(method, m, q, T) for q in qn.levels(which)]
    nq = len(pos)
    lo, hi, w = (np.array([float(p[k]) for p in pos] + [0.0]) for k in range(3))
    out = np.full((nq,) + rest, 7, out_dtype)
    tag = "f32" if out_dtype == qn.F32 else "f64" if T == qn.F64 else "f32_f64"
    fn = getattr(_hosttwin.lib(), f"ekm_host_quantiles_{tag}")
    fn.restype = C.c_int
    rc = fn(_vp(a), C.c_size_t(outer), C.c_uint(m), C.c_size_t(inner), _vp(lo), _vp(hi), _vp(w), C.c_uint(nq),
            C.c_int(0 if method == "sort" else 1), _vp(out))
    assert rc == 0
    return out


@pytest.mark.parametrize("case", VALUE_CASES, ids=qn.case_id)
def test_restatement_against_the_recorded_reference(case):
    qn.judge_case(case, qn.quantiles(**qn.kwargs_of(case)), qn.case_id(case))


@pytest.mark.parametrize("case", VALUE_CASES, ids=qn.case_id)
def test_host_twin_against_the_recorded_reference(case):
    qn.judge_case(case, twin(**qn.kwargs_of(case)), qn.case_id(case))


def test_every_case_the_issue_names_is_recorded():
    notes = [c["note"] for c in qn.cases()]
    for tag, ms in (("f32", (1, 2, 7, 8, 9, 51, 128, 256)), ("f64", (1, 2, 7, 8, 9, 51, 128))):
        for m in ms:
            for kind in ("ties", "smooth"):
                for method in qn.METHODS:
                    for which in (0, 1, 4, 100, [0.1, 0.5, 1.0], [0.9, 0.0, 0.33], []):
                        assert f"{tag} m {m} {kind} {method} which {which}" in notes
        for axis in (0, 1, 2, -1):
            assert any(n.startswith(f"{tag} cube axis {axis} ") for n in notes)
        assert any(n.startswith(f"{tag} m 51 special") for n in notes)
    assert any(n.startswith("integer input") for n in notes)
    assert all(c["arrays"]["arr"] for c in qn.cases())
    print("recorded with NumPy", qn.recorded_numpy_version(), "- this host has", np.__version__)
    assert qn.recorded_numpy_version()


def test_the_special_columns_hold_what_they_are_meant_to():
    """x == 0 meeting an infinity gives the reference's NaN in "sort" (and only a NaN member does in every level)."""
    case = next(c for c in VALUE_CASES if c["note"] == "f64 m 9 special sort which 4")
    arr, want = qn.kwargs_of(case)["arr"], qn.expected_of(case)
    assert np.isnan(arr[:, 2]).any() and np.isnan(want[:, 2]).all()
    assert np.isinf(np.sort(arr[:, 7])[-2:]).all() and np.isnan(want[3, 7]) and not np.isnan(want[2, 7])
    for col in range(arr.shape[1]):  # no column mixes the two zeros
        z = arr[:, col][arr[:, col] == 0]
        assert z.size == 0 or np.signbit(z).all() or not np.signbit(z).any()


# ---- the public interface: signatures and errors, no GPU involved ----
def test_signatures_are_the_references():
    assert str(inspect.signature(stats.iter_quantiles)) == qn.signatures()["iter_quantiles"]
    assert str(inspect.signature(stats.quantiles)) == qn.signatures()["iter_quantiles"]
    assert inspect.isgeneratorfunction(stats.iter_quantiles)


@pytest.mark.parametrize("case", ERROR_CASES, ids=qn.case_id)
def test_error_conventions(case):
    """Before any device work: these raise on a machine without a GPU as well."""
    kw = qn.kwargs_of(case)
    if "deviation" in case:  # "sort" with a level outside [0, 1] or NaN: IndexError / wrap-around / int(NaN) there
        kind, message = "ValueError", "Quantiles must be in the range [0, 1]"
    else:
        kind, message = case["raises"]
    for fn in (lambda: list(stats.iter_quantiles(**kw)), lambda: stats.quantiles(**kw)):
        with pytest.raises(ValueError) as info:
            fn()
        assert type(info.value).__name__ == kind and str(info.value) == message


def test_iter_quantiles_raises_at_the_first_step_like_a_generator():
    gen = stats.iter_quantiles(np.zeros((3, 2)), method="bogus")  # nothing runs yet, as in the reference
    with pytest.raises(ValueError, match="Invalid method 'bogus', expected 'sort', 'numpy_bulk', or 'numpy'"):
        next(gen)
    with pytest.raises(ValueError):
        stats.quantiles(np.zeros((3, 2)), axis=2)
    with pytest.raises(ValueError):
        stats.quantiles(np.zeros((0, 2)))
    with pytest.raises(ValueError):
        stats.quantiles(np.zeros((3, 2)), which=[[0.5]])


def test_quantiles_equals_the_stacked_generator(monkeypatch):
    """quantiles() is the stacked generator: iter_quantiles yields row k of the one result, whatever computed it."""
    calls = []

    def fake(arr, which=100, axis=0, method="sort"):
        calls.append((which, axis, method))
        return qn.quantiles(arr, which, axis, method)

    monkeypatch.setattr(stats, "quantiles", fake)
    arr = np.random.default_rng(5).normal(0, 1, (4, 7, 5))
    for method in qn.METHODS:
        rows = list(stats.iter_quantiles(arr, [0.9, 0.0, 0.33], axis=1, method=method))
        assert len(rows) == 3 and all(r.shape == (4, 5) for r in rows)
        qn.judge_exact(np.stack(rows), qn.quantiles(arr, [0.9, 0.0, 0.33], 1, method))
    assert len(calls) == 3  # one computation (one launch) for all levels
    assert list(stats.iter_quantiles(arr, [], axis=-1)) == []


def test_no_result_without_work_needs_no_device():
    got = stats.quantiles(np.zeros((7, 3), np.float32), which=[], method="numpy")
    assert got.shape == (0, 3) and got.dtype == np.float32
    assert stats.quantiles(np.zeros((7, 0)), which=4).shape == (5, 0)


def test_product_position_tables_are_the_references_expression():
    """ekm_hip.stats.quantile_positions (vectorised, what the kernel is given) against the scalar expressions of the
    reference's loop and of numpy.quantile, for every sample count and level set of the recording."""
    for T in (qn.F32, qn.F64):
        for m in (1, 2, 7, 8, 9, 51, 128, 256):
            for which in (0, 1, 4, 100, [0.1, 0.5, 1.0], [0.9, 0.0, 0.33]):
                qs = stats.quantile_levels(which)
                assert np.array_equal(qs, qn.levels(which)) and qs.dtype == np.float64
                for method in qn.METHODS:
                    lo, hi, w = stats.quantile_positions(method, m, qs, T)
                    assert lo.dtype == hi.dtype == w.dtype == np.float64
                    for k, q in enumerate(qs):
                        want = qn.positions(method, m, q, T)
                        assert (lo[k], hi[k]) == want[:2] and w[k] == np.float64(want[2]), (T, m, which, method, k)
                        assert 0 <= lo[k] < m and 0 <= hi[k] < m
    # numpy's clipping at the last sample: both neighbours the last one, gamma = the virtual index + 1
    lo, hi, w = stats.quantile_positions("numpy", 51, np.array([1.0]), qn.F32)
    assert (lo[0], hi[0], w[0]) == (50, 50, 51)


# ---- the judge rejects what it must ----
def _flip(a, i):
    b = np.array(a, copy=True)
    b.reshape(-1).view(np.uint32 if b.dtype == qn.F32 else np.uint64)[i] ^= 1
    return b


@pytest.mark.parametrize("note", ["f32 m 51 special numpy which 100", "f64 m 51 special sort which 100",
                                  "f32 m 51 special numpy_bulk which 4"])
def test_judge_rejects_a_flipped_bit_a_wrong_nan_and_a_wrong_dtype(note):
    case = next(c for c in VALUE_CASES if c["note"] == note)
    want = qn.expected_of(case)
    qn.judge_case(case, want)
    level = want.shape[0] // 2
    i = level * want.shape[1] + int(np.flatnonzero(~np.isnan(want[level]))[-1])
    with pytest.raises(qn.Mismatch):
        qn.judge_case(case, _flip(want, i))  # one low bit in one level
    bad = want.copy()
    bad.reshape(-1)[i] = np.nan
    with pytest.raises(qn.Mismatch):
        qn.judge_case(case, bad)             # a NaN where the reference has a number
    bad = want.copy()
    bad[level, 2] = 1.0
    with pytest.raises(qn.Mismatch):
        qn.judge_case(case, bad)             # a number where the reference has a NaN
    with pytest.raises(qn.Mismatch):
        qn.judge_case(case, want.astype(np.float32 if want.dtype == qn.F64 else np.float64))
    with pytest.raises(qn.Mismatch):
        qn.judge_case(case, want[:-1])       # a level missing


def test_judge_rejects_sorts_values_offered_for_numpy_on_f64_input():
    """The two formulae differ in the last bit on a few per cent of values: the case is checked to differ."""
    case = next(c for c in VALUE_CASES if c["note"] == "f64 m 51 smooth numpy which 100")
    kw = qn.kwargs_of(case)
    as_sort = qn.quantiles(kw["arr"], 100, 0, "sort")
    want = qn.expected_of(case)
    differ = int(np.sum(as_sort != want))
    assert as_sort.dtype == want.dtype and 0 < differ < want.size // 4, differ
    assert np.max(np.abs(as_sort - want) / np.abs(want)) < 4 * 2.0 ** -53  # the last bits only
    with pytest.raises(qn.Mismatch):
        qn.judge_case(case, as_sort)
    empty = next(c for c in VALUE_CASES if c["note"] == "f64 m 51 smooth numpy which []")
    with pytest.raises(qn.Mismatch):
        qn.judge_case(empty, want)           # rows where the reference yields none
