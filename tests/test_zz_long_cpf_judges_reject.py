"""The judge of the long_cpf tests rejects what a defect would produce: `_long_cpf.judge_case` (the recorded cases) and
`judge_exact` as the GPU tests call it against the host twin.  Each must raise on one point moved by one ulp of float32,
on a crossing level (iq + 1) / (nens + 1) replaced by its neighbour's, on a clamped 0 given as -0.0, and on the outputs of
two adjacent points swapped, and accept the recorded result itself.  No GPU involved."""
import numpy as np
import pytest

import _cpf_numpy as cn
import _long_cpf as lc

F32 = np.float32


def _case(tag, shape, option):
    return next(c for c in lc.cases(tag) if c["note"] == f"{tag} {shape} {option}")


def _plain_crossings(case):
    """(indices of the points a plain crossing decided, the member index iq of each)."""
    kw = lc.kwargs_of(case)
    value, kind, rev = cn.cpf_with_kinds(**kw)
    idx = np.flatnonzero((kind == cn.PLAIN) & ~rev)
    nens = kw["ens"].shape[0]
    iq = np.rint(value[idx].astype(np.float64) * (nens + 1)).astype(int) - 1
    assert idx.size and all(F32((i + 1.0) / (nens + 1.0)) == v for i, v in zip(iq, value[idx]))
    return idx, iq, nens


@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("shape", ["1980x51", "101x1980", "700x700"])
def test_one_ulp_a_neighbouring_level_and_a_swap_are_rejected(tag, shape):
    case = _case(tag, shape, "default")
    want = lc.expected_of(case)
    lc.judge_case(case, want.copy())  # the recorded result itself passes, so what follows is rejected for the defect alone
    moved = np.flatnonzero(np.isfinite(want) & (want != 0))
    assert moved.size
    for i in moved:  # one ulp of float32, either way, at every point that holds a number
        for towards in (np.inf, -np.inf):
            bad = want.copy()
            bad[i] = np.nextafter(bad[i], F32(towards))
            with pytest.raises(lc.Mismatch):
                lc.judge_case(case, bad, f"one ulp at {i}")
    idx, iq, nens = _plain_crossings(case)
    for i, q in zip(idx, iq):  # the level of the member before, and of the member after
        for other in (q - 1, q + 1):
            bad = want.copy()
            bad[i] = F32((other + 1.0) / (nens + 1.0))
            assert bad[i] != want[i]
            with pytest.raises(lc.Mismatch):
                lc.judge_case(case, bad, f"level of member {other} for member {q}")
    swapped = 0
    for i in range(want.size - 1):  # two adjacent points swapped, wherever that changes anything
        if want[i].tobytes() != want[i + 1].tobytes():
            bad = want.copy()
            bad[i], bad[i + 1] = want[i + 1], want[i]
            with pytest.raises(lc.Mismatch):
                lc.judge_case(case, bad, f"points {i} and {i + 1} swapped")
            swapped += 1
    assert swapped >= 8


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_the_other_zero_is_rejected(tag):
    """The lower-tail interpolation clamps at 0 (numpy.maximum(x, 0) gives +0.0): -0.0 in its place is another result."""
    zeros = 0
    for case in lc.cases(tag):
        want = lc.expected_of(case)
        for i in np.flatnonzero(want == 0):
            assert not np.signbit(want[i])
            bad = want.copy()
            bad[i] = F32(-0.0)
            with pytest.raises(lc.Mismatch):
                lc.judge_case(case, bad, "the other zero")
            zeros += 1
    assert zeros > 100
    with pytest.raises(lc.Mismatch):
        lc.judge_exact(np.array([-0.0, 0.5], F32), np.array([0.0, 0.5], F32))


def test_wrong_dtype_shape_and_nan_are_rejected():
    case = _case("f32", "513x257", "symmetric from_zero")
    want = lc.expected_of(case)
    lc.judge_case(case, want)
    nan_at = want.copy()
    nan_at[3] = np.nan
    for bad in (want.astype(np.float64), want[:-1], nan_at, np.zeros_like(want)):
        with pytest.raises(lc.Mismatch):
            lc.judge_case(case, bad)
    got = lc.twin(**lc.kwargs_of(case))
    lc.judge_exact(got, want)
    got[5] = np.nextafter(got[5], F32(2)) if got[5] != 0 else F32(1e-45)
    with pytest.raises(lc.Mismatch):
        lc.judge_exact(got, want, "the twin's output moved by one ulp")
