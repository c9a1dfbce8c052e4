"""regimes.project, regimes.regime_index and score.pearson_correlation without a GPU: the NumPy restatement and the host
twin of the kernels (csrc/reduce_point.hpp through csrc/host_twin.cpp) against the results recorded from the reference
(tests/golden/regimes_golden.npz), the reference's own results against the same bars, the public signatures, the
argument checks, the dtype table and the zero-size results that need no device.

Parity (tests/_regimes_numpy.py states the bars and derives them):
  * project: within (K + 4) eps sum |f p w| of the exact sum (+ eps |exact| with a modulator);
  * pearson along a non-contiguous axis (inner > 1): bit for bit; along the contiguous axis: within (2 m + 16) eps;
  * regime_index: bit for bit."""
import inspect

import numpy as np
import pytest

import _compare
import _regimes_numpy as rn
import _regimes_twin as twin
from ekm_hip import regimes, score
from ekm_hip.score import pearson_correlation  # noqa: F401  (absent before this feature)

PROJECT = [c for c in rn.cases("project") if not c["raises"]]
PROJECT_ERRORS = [c for c in rn.cases("project") if c["raises"]]
INDEX = rn.cases("regime_index")
PEARSON = [c for c in rn.cases("pearson_correlation") if not c["raises"]]
PEARSON_ERRORS = [c for c in rn.cases("pearson_correlation") if c["raises"]]


def test_the_golden_file_holds_the_cases_the_tests_rely_on():
    assert len(PROJECT) >= 35 and len(PROJECT_ERRORS) == 5 and len(INDEX) >= 12 and len(PEARSON) >= 60
    kinds = {c["plain"]["kind"] for c in PROJECT}
    assert kinds == {"constant", "modulated", "perfield"}
    assert {len(c["plain"]["labels"]) for c in PROJECT} >= {1, 3, 8, 9}
    assert any(tuple(c["plain"]["pshape"]) == (91, 121) for c in PROJECT)
    layouts = {rn.layout(rn.arrays_of(c)["x"].shape, c["plain"]["axis"]) for c in PEARSON}
    assert {i for _, _, i in layouts} >= {1, 2, 63, 64, 65, 1000} and {m for _, m, _ in layouts} >= {1, 2, 3, 9, 51, 257}
    assert {o for o, _, _ in layouts} >= {1, 3}


def test_signatures_are_the_reference_s():
    sigs = rn.signatures()
    assert str(inspect.signature(regimes.project)) == sigs["project"]
    assert str(inspect.signature(regimes.regime_index)) == sigs["regime_index"]
    assert str(inspect.signature(score.pearson_correlation)) == sigs["pearson_correlation"]
    assert str(inspect.signature(regimes.ConstantPatterns.__init__)) == sigs["ConstantPatterns"]
    assert str(inspect.signature(regimes.ModulatedPatterns.__init__)) == sigs["ModulatedPatterns"]
    # Patterns: the reference's `xp` has no default; ours is accepted and ignored, so it may be left out
    assert str(inspect.signature(regimes.Patterns.__init__)) == sigs["Patterns"].replace("xp)", "xp=None)")


# ---- project ----
@pytest.mark.parametrize("case", PROJECT, ids=rn.case_id)
def test_project_reference_restatement_and_host_twin_within_the_bar(case):
    want = rn.recorded(case)
    for label, w in want.items():
        assert w.dtype == rn.project_dtype(case), "the dtype rule is the reference's"
    rn.judge_project(case, want, "reference " + case["note"], _compare.LEDGER)  # if this fails the case is wrong, not the bar
    rn.judge_project(case, rn.project(case), "restatement " + case["note"], _compare.LEDGER)
    rn.judge_project(case, twin.project(case), "host twin " + case["note"], _compare.LEDGER)


def test_project_twin_gives_the_same_bits_at_any_row_and_address():
    rng = np.random.default_rng(5)
    for T in (rn.F32, rn.F64):
        for k in (1, 3, 63, 65, 257, 1025):
            coef = rng.normal(0, 1, (9, k)).astype(T)
            row = rng.normal(0, 50, k).astype(T)
            batch = rng.normal(0, 50, (5, k)).astype(T)
            first = twin.project_raw(row[None], coef.reshape(-1), 9)
            for at in (0, 2, 4):
                batch[at] = row
                rn.judge_exact(twin.project_raw(batch, coef.reshape(-1), 9)[:, at], first[:, 0], f"row {at} k {k}")
            shifted = np.empty(5 * k + 3, T)
            shifted[3:] = batch.reshape(-1)
            rn.judge_exact(twin.project_raw(shifted[3:].reshape(5, k), coef.reshape(-1), 9), twin.project_raw(batch, coef.reshape(-1), 9), "shifted")


@pytest.mark.parametrize("case", PROJECT_ERRORS, ids=rn.case_id)
def test_project_errors_are_the_reference_s(case):
    patterns, extra = rn.build_patterns(case, regimes)
    a = rn.arrays_of(case)
    with pytest.raises(Exception) as info:
        regimes.project(a["field"], patterns, a.get("weights"), **extra)
    assert [type(info.value).__name__, str(info.value)] == case["raises"]


def test_project_refuses_patterns_of_another_shape_and_a_modulator_that_does_not_fit():
    grid = rn.grid_of((5, 13))

    class Odd(regimes.Patterns):
        def patterns(self):
            return {"a": np.zeros((4, 13))}

    with pytest.raises(ValueError, match=r"pattern 'a' evaluates to shape \(4, 13\).*\(5, 13\).*\(2, 5, 13\)"):
        regimes.project(np.zeros((2, 5, 13)), Odd(["a"], grid), np.ones((5, 13)))
    mod = regimes.ModulatedPatterns(["a"], grid, np.zeros((1, 5, 13)), lambda step: step)
    with pytest.raises(ValueError, match=r"modulator values of shape \(3,\) do not fit the fields \(2,\)"):
        regimes.project(np.zeros((2, 5, 13)), mod, np.ones((5, 13)), step=np.ones(3))


def test_pattern_classes_keep_the_reference_s_bookkeeping():
    grid = {"area": [90, -90, 20, 30], "grid": [2.5, 5]}
    stack = np.arange(2 * 29 * 25, dtype=np.float32).reshape(2, 29, 25)
    c = regimes.ConstantPatterns(["NAO+", "BL"], grid, stack, xp="ignored")
    assert c.labels == ("NAO+", "BL") and c.grid is grid and c.shape == (29, 25) and c.size == 725 and c.ndim == 2
    assert list(c.patterns()) == ["NAO+", "BL"] and np.array_equal(c.patterns()["BL"], stack[1])
    assert repr(c) == "ConstantPatterns('NAO+', 'BL')"
    with pytest.raises(ValueError, match="exactly one label axis"):
        regimes.ConstantPatterns(["a"], grid, stack[0])
    with pytest.raises(ValueError, match="number of labels"):
        regimes.ConstantPatterns(["a"], grid, stack)
    with pytest.raises(ValueError, match="modulator must be callable"):
        regimes.ModulatedPatterns(["a", "b"], grid, stack, 3.0)
    m = regimes.ModulatedPatterns(["a", "b"], grid, stack, lambda day: np.cos(day))
    got = m.patterns(day=np.array([0.0, 1.0, 2.0]))
    assert list(got) == ["a", "b"] and got["b"].shape == (3, 29, 25)
    assert np.array_equal(got["b"], np.cos(np.array([0.0, 1.0, 2.0]))[:, None, None] * stack[1])
    with pytest.raises(TypeError):
        regimes.Patterns(["a"], grid)  # abstract


def test_zero_size_results_need_no_device():
    c = regimes.ConstantPatterns(["a", "b"], rn.grid_of((5, 13)), np.zeros((2, 5, 13), np.float32))
    out = regimes.project(np.zeros((0, 5, 13), np.float32), c, np.ones((5, 13), np.float32))
    assert list(out) == ["a", "b"] and out["a"].shape == (0,) and out["a"].dtype == np.float32
    out = regimes.project(np.zeros((3, 0, 5, 13)), c, np.ones((5, 13), np.float32))
    assert out["b"].shape == (3, 0) and out["b"].dtype == np.float64
    idx = regimes.regime_index({"a": np.zeros((0, 4), np.float32)}, {"a": 1.0}, {"a": np.zeros((0, 4))})
    assert idx["a"].shape == (0, 4) and idx["a"].dtype == np.float64
    r = score.pearson_correlation(np.zeros((7, 0), np.float32), np.zeros((7, 0), np.float32), axis=0)
    assert r.shape == (0,) and r.dtype == np.float32
    assert score.pearson_correlation(np.zeros((0, 7), np.int32), np.zeros((0, 7)), axis=1).shape == (0,)


# ---- regime_index ----
@pytest.mark.parametrize("case", INDEX, ids=rn.case_id)
def test_regime_index_host_twin_equals_the_reference(case):
    proj, mean, std = rn.index_args(case)
    want = rn.recorded(case)
    got = {}
    for label in proj:
        arrays = [proj[label]] + [v for v in (mean[label], std[label]) if isinstance(v, np.ndarray)]
        T = rn.arith_dtype(*arrays)
        got[label] = twin.index_raw(proj[label].astype(T), mean[label], std[label])
    rn.judge_index(got, want, "host twin " + case["note"])


def test_regime_index_checks_shapes():
    with pytest.raises(ValueError, match=r"mean of shape \(3,\) must have the projection's shape \(4,\)"):
        regimes.regime_index({"a": np.zeros(4)}, {"a": np.zeros(3)}, {"a": 1.0})
    with pytest.raises(KeyError):
        regimes.regime_index({"a": np.zeros(4)}, {}, {"a": 1.0})


# ---- pearson ----
@pytest.mark.parametrize("case", PEARSON, ids=rn.case_id)
def test_pearson_restatement_and_host_twin_against_the_reference(case):
    a, axis, want = rn.arrays_of(case), case["plain"]["axis"], rn.recorded(case)
    x, y = a["x"], a["y"]
    T = rn.arith_dtype(x, y)
    assert want.dtype == T, "the dtype rule is the reference's"
    _, m, inner = rn.layout(x.shape, axis)
    if inner == 1:
        so = second_order_term(x, y, axis, T)
        assert not (so >= 1.0).any(), f"case data: the second-order centring term reaches {np.nanmax(so):.3g} eps"
        used = rn.judge_pearson(x, y, axis, want, want, "reference " + case["note"], _compare.LEDGER)  # the reference alone
        assert used <= 1.0
    restated = rn.pearson(x, y, axis)
    rn.judge_pearson(x, y, axis, restated, want, "restatement " + case["note"], _compare.LEDGER)
    rn.judge_pearson(x, y, axis, twin.pearson(x, y, axis), want, "host twin " + case["note"], _compare.LEDGER)
    if inner > 1:
        rn.judge_exact(twin.pearson(x, y, axis), restated, "host twin against the restatement")
    if case["plain"]["r"] is not None:
        assert np.allclose(want, case["plain"]["r"], rtol=0, atol=1e-5 if T == rn.F32 else 1e-13)


def second_order_term(x, y, axis, T):
    so = np.maximum(rn.second_order_term(x, axis, T), rn.second_order_term(y, axis, T))
    return so[np.isfinite(so)]


def test_pearson_argument_errors():
    with pytest.raises(ValueError, match=r"shapes of x \(9, 6\) and y \(9, 5\) must match"):
        score.pearson_correlation(np.zeros((9, 6)), np.zeros((9, 5)))
    for axis in (2, -3):
        with pytest.raises(np.exceptions.AxisError):
            score.pearson_correlation(np.zeros((9, 6)), np.zeros((9, 6)), axis=axis)
    assert {c["raises"][0] for c in PEARSON_ERRORS} == {"AssertionError", "AxisError"}  # the reference asserts; we raise


def test_dtype_table():
    """f32 only when every array of the call is f32; everything else is f64."""
    from ekm_hip import _ensemble as e

    f32, f64, i32 = np.zeros(2, np.float32), np.zeros(2), np.zeros(2, np.int32)
    assert e.arith_dtype(f32, f32, f32) == np.float32
    for mix in ((f32, f64, f32), (f64, f64, f64), (f32, f32, i32), (np.zeros(2, np.float16), f32, f32)):
        assert e.arith_dtype(*mix) == np.float64
    for case in PROJECT + PEARSON:
        want = rn.recorded(case)
        want = next(iter(want.values())) if isinstance(want, dict) else want
        a = rn.arrays_of(case)
        assert want.dtype == e.arith_dtype(*a.values()), case["note"]
