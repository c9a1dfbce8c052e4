"""stats.nanaverage without a GPU: the NumPy restatement and the host twin of the kernels (csrc/reduce_point.hpp through
csrc/host_twin.cpp) against the results recorded from the reference (tests/golden/nanaverage_golden.npz), the reference's
own results against the same bar, the public signature, the argument checks and the results that need no device.

Parity (tests/_nanaverage_numpy.py states the bar and derives it): bit for bit where the averaged axis is not the
contiguous one (path 1 of the twin); within (n + 4 + n kappa) eps sum |d w| / |sum w| of the exact mean along the
contiguous axis, for the reference and for paths 1, 2 and 3 of the twin alike.

The golden cases are walked inside a test, not parametrised (the GPU suite has one test per case): a failure names its
case in the judge's message."""
import inspect

import numpy as np
import pytest

import _compare
import _nanaverage_numpy as nn
import _nanaverage_twin as twin
from ekm_hip import stats
from ekm_hip.stats import nanaverage  # noqa: F401  (absent before this feature)

VALID = [c for c in nn.cases() if not c["raises"] and not c["product_raises"]]
REFUSED = [c for c in nn.cases() if c["product_raises"]]


def _layout(case):
    d, _, kw = nn.call_of(case)
    return nn.layout(d.shape, kw.get("axis"))


def test_every_case_the_issue_names_is_recorded():
    notes = [c["note"] for c in nn.cases()]

    def has(*needles):
        return any(all(n in note for n in needles) for note in notes)

    for dt in ("float32", "float64"):
        for axis in ("axis 0", "axis 1", "axis 2", "axis -1", "axis None", "axis (0, 1)", "axis (-2, -1)", "axis (0, 2)"):
            assert has(dt, axis), (dt, axis)
        for what in ("keepdims", "scalar weight", "weights vector", "full weights", "weights [m, 1]", "cos-latitude", "a NaN weight",
                     "weights summing to 0", "weights all zero", "weights of mixed sign", "special columns", "an all-NaN array", "m 0",
                     "an empty result", "does not collapse"):
            assert has(dt, what), (dt, what)
    assert has("integer data") and has("float32 data float64 weights") and has("error a tuple of axes with weights")
    layouts = {_layout(c) for c in VALID}
    assert {m for _, m, _ in layouts} >= {0, 1, 2, 3, 9, 51, 257}
    assert {i for _, _, i in layouts} >= {1, 5, 7, 63} and {o for o, _, _ in layouts} >= {1, 3, 5}
    special = nn.arrays_of(next(c for c in VALID if c["note"] == "float32 special columns axis 0"))["data"]
    assert np.isnan(special[:, 1]).all() and np.signbit(special[:, 2]).all() and np.isposinf(special).any() and np.isneginf(special).any()
    raised = {c["note"]: (c["raises"][0] if c["raises"] else None, c["product_raises"]) for c in REFUSED}
    assert raised["error a tuple of axes with weights"] == ("TypeError", "TypeError")
    assert raised["error axis out of range"] == ("AxisError", "AxisError")
    assert raised["error weights enlarge the shape"] == ("IndexError", "ValueError")
    assert raised["float64 (3, 9, 7) axis (0, 2) not adjacent"] == (None, "ValueError")
    assert raised["error the keyword dtype"] == (None, "TypeError")
    assert len(VALID) >= 140 and len(REFUSED) >= 10
    assert str(inspect.signature(stats.nanaverage)) == nn.signatures()["nanaverage"], "the signature is the reference's"


def test_restatement_and_host_twin_against_the_reference():
    """Every valid golden case (one test: the judges name the case in what they raise)."""
    for case in VALID:
        _restatement_and_host_twin(case)
    for T in (nn.F32, nn.F64):  # rows around the split chunk, weights by stride, a row at another index and address
        _twin_long_rows(T)


def _restatement_and_host_twin(case):
    d, w, kw = nn.call_of(case)
    axis, keepdims, want = kw.get("axis"), kw.get("keepdims", False), nn.recorded(case)
    T = nn.arith_dtype(d) if w is None else nn.arith_dtype(d, w)
    assert want.dtype == T, "the dtype rule is the reference's"
    assert want.shape == nn.result_shape(d.shape, axis, keepdims)
    outer, m, inner = nn.layout(d.shape, axis)
    if outer * inner == 0:
        return
    judge = lambda got, what, **k: nn.judge(d, w, axis, got, want, f"{what} {case['note']}", _compare.LEDGER, keepdims, **k)  # noqa: E731
    if inner == 1:
        assert judge(want, "reference") <= 1.0  # if this fails the bar is too tight, not the reference wrong
    judge(nn.restated(d, w, axis, keepdims), "restatement")
    judge(twin.nanaverage(d, w, axis, keepdims, nn.POINTS), "twin path 1")
    judge(twin.nanaverage(d, w, axis, keepdims, 0), "twin path 0")
    if inner > 1:
        judge(nn.numpy_formula(d, w, **kw), "numpy formula")
        nn.judge_exact(twin.nanaverage(d, w, axis, keepdims, 0), nn.restated(d, w, axis, keepdims), "twin against the restatement")
    else:
        judge(twin.nanaverage(d, w, axis, keepdims, nn.ROWS), "twin path 2")
        judge(twin.nanaverage(d, w, axis, keepdims, nn.SPLIT), "twin path 3")


def _twin_long_rows(T):
    rng = np.random.default_rng(4)
    c = nn.SPLIT_CHUNK
    for m in (c - 1, c, c + 1, 3 * c + 5):
        x = (280 + rng.normal(0, 5, (3, m))).astype(T)
        x[rng.uniform(size=x.shape) < 0.1] = np.nan
        x[1, 0], x[1, -1] = np.nan, np.nan
        w = (0.5 + rng.uniform(0, 1, m)).astype(T)
        want = nn.numpy_formula(x, axis=1)
        wantw = nn.numpy_formula(x, w, axis=1)
        for path in (nn.ROWS, nn.SPLIT, 0):
            got = twin.raw(x.reshape(-1), 3, m, 1, path=path)
            nn.judge(x, None, 1, got, want, f"twin path {path} m {m}", _compare.LEDGER)
            gw = twin.raw(x.reshape(-1), 3, m, 1, w, (0, 1, 0), path)  # one weight vector, shared by the rows through stride 0
            nn.judge(x, w, 1, gw, wantw, f"twin path {path} m {m} weighted", _compare.LEDGER)
            nn.judge_exact(gw, twin.nanaverage(x, w, 1, path=path), "weights by stride against expanded weights")
            # the same row at another row index and address gives the same bits
            moved = np.concatenate([np.zeros(1, T), x[2], x[0], x[2]])[1:]
            again = twin.raw(moved, 3, m, 1, path=path)
            nn.judge_exact(again[[0, 2]], got[[2, 2]], "a row at another index")
    assert twin.raw(np.zeros(4 * c, T), 1, 4 * c, 1, path=0).shape == (1,)


def _path_rule_and_weight_strides():
    from ekm_hip import _ffi

    wb = _ffi.lib().ekm_nanaverage_work_bytes
    c = nn.SPLIT_CHUNK
    assert wb(4, 1, 2 * c, 1, 0, 0) == 2 * 2 * 4 and wb(8, 50, 6_500_000, 1, 1, 0) == 50 * 199 * 2 * 8  # split
    assert wb(4, 1, 2 * c - 1, 1, 0, 0) == 0 and wb(4, 2048, 2 * c, 1, 0, 0) == 0 and wb(4, 2047, 2 * c, 1, 0, 0) > 0  # rows
    assert wb(4, 50, 6_500_000, 2, 0, 0) == 0 and wb(4, 3, 9, 1, 0, 3) == 3 * 2 * 4 and wb(4, 3, 0, 1, 0, 3) == 3 * 2 * 4
    assert wb(4, 3, 9, 2, 0, 3) == 0 and wb(4, 3, 9, 1, 0, 4) == 0 and wb(2, 3, 9, 1, 0, 3) == 0  # refused arguments
    _weight_strides_collapse_or_expand()


def test_argument_errors_are_raised_before_any_device_is_asked_for(monkeypatch):
    from ekm_hip import _ensemble, device

    def no_device(*a, **k):
        raise AssertionError("a device was asked for")

    monkeypatch.setattr(device.DeviceArray, "empty", no_device)
    monkeypatch.setattr(_ensemble, "upload", no_device)
    for case in REFUSED:
        _refused(case)
    _more_argument_errors()


def _refused(case):
    d, w, kw = nn.call_of(case)
    with pytest.raises(Exception) as info:
        stats.nanaverage(d, w, **kw)
    assert type(info.value).__name__ == case["product_raises"], info.value
    if case["note"] == "error a tuple of axes with weights":
        assert "with weights, axis must be None or an int" in str(info.value)
    if "not adjacent" in case["note"]:
        assert "(0, 2)" in str(info.value) and "adjacent" in str(info.value)
    if "keyword" in case["note"]:
        assert ("'dtype'" if "dtype" in case["note"] else "'initial'") in str(info.value)


def _more_argument_errors():
    x = np.zeros((3, 4, 5))
    for kw in (dict(out=None), dict(where=True)):
        with pytest.raises(TypeError, match=next(iter(kw))):
            stats.nanaverage(x, **kw)
    for axis in ((), (0, 0), (2, 0), [0, 1]):
        with pytest.raises((ValueError, TypeError)):
            stats.nanaverage(x, axis=axis)
    with pytest.raises(np.exceptions.AxisError):
        stats.nanaverage(np.float64(1.0), axis=0)
    with pytest.raises(ValueError, match=r"weights of shape \(4,\) do not broadcast against the data's shape \(3, 4, 5\)"):
        stats.nanaverage(x, np.ones(4))


def test_what_needs_no_device_and_a_valid_call_without_one_raises():
    """The path rule and the weight strides (functions of the shape), empty results; then a valid call with no GPU."""
    import ekm_hip
    from ekm_hip import _ffi

    _path_rule_and_weight_strides()

    for case in VALID:
        d, w, kw = nn.call_of(case)
        outer, _, inner = _layout(case)
        if outer * inner:
            continue
        got = stats.nanaverage(d, w, **kw)
        want = nn.recorded(case)
        assert isinstance(got, np.ndarray) and got.shape == want.shape and got.dtype == want.dtype, case["note"]
    assert stats.nanaverage(np.zeros((4, 0), np.int32), axis=0, keepdims=True).shape == (1, 0)
    if _ffi.lib().ekm_device_count() <= 0:  # no silent CPU path: without a device a valid call raises
        with pytest.raises(ekm_hip.EkmError):
            stats.nanaverage(np.ones((3, 4), np.float32), axis=0)


def _weight_strides_collapse_or_expand():
    f = stats._nanaverage_weight_strides
    assert f((), (3, 9, 7), 1, 1) == (0, 0, 0)                 # a scalar
    assert f((9, 1), (3, 9, 7), 1, 1) == (0, 1, 0)             # [m, 1]
    assert f((7,), (3, 9, 7), 2, 2) == (0, 1, 0)               # a vector along the last axis
    assert f((3, 9, 7), (3, 9, 7), 1, 1) == (63, 7, 1)         # a full array
    assert f((3, 9, 7), (3, 9, 7), 0, 2) == (0, 1, 0)          # ... for axis=None
    assert f((9, 1), (5, 9, 7), 0, 0) is None                  # [lat, 1] in the inner group: lat and lon do not collapse
    assert f((3, 1, 1), (3, 9, 7), 0, 0) == (0, 1, 0)
    assert f((3, 1, 7), (3, 9, 7), 1, 1) == (7, 0, 1)          # broadcast along the averaged axis
    assert f((9, 1), (3, 9, 7), 0, 2) is None                  # axis=None: [9, 1] against (3, 9, 7) does not collapse
    assert f((1, 9, 7), (3, 9, 7), 1, 2) == (0, 1, 0)          # a tuple run (weights are refused earlier; the rule is general)
