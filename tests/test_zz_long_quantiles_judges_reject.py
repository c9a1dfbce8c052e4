"""The judge of the long-axis quantile tests rejects what a broken sorting network would produce: for a recorded case of
300 samples, the rows computed from a column with two neighbouring sorted samples swapped, with a padding value in place
of the largest sample, and numbers where a NaN column must give NaN.  No GPU involved: the wrong rows are computed here
from a deliberately wrong "sorted" column, with the restatement's own position records and arithmetic."""
import numpy as np
import pytest

import _long_quantiles as lq


def _rows_from_sorted(s, which, method, T):
    """The rows of `_quantiles_numpy.quantiles` from a column array `s` [m, npts] taken AS IF sorted (no NaN handling)."""
    out_dtype = T if method == "numpy" else lq.F64
    rows = []
    with np.errstate(all="ignore"):
        for q in lq.qn.levels(which):
            lo, hi, w = lq.qn.positions(method, s.shape[0], q, T)
            if method == "sort":
                row = s[lo].astype(lq.F64) * (np.float64(1) - w) + s[hi].astype(lq.F64) * w
            else:
                diff = (s[hi] - s[lo]).astype(out_dtype)
                a, b = s[lo].astype(out_dtype), s[hi].astype(out_dtype)
                row = b - diff * (out_dtype.type(1) - w) if w >= 0.5 else a + diff * w
            rows.append(row.astype(out_dtype))
    return np.stack(rows)


@pytest.mark.parametrize("note", ["f32 m 300 smooth numpy which 100", "f64 m 300 smooth sort which 100",
                                  "f32 m 300 smooth numpy_bulk which 100", "f64 m 300 special axis first sort which 100"])
def test_judge_rejects_what_a_broken_network_gives(note):
    case = next(c for c in lq.cases() if c["note"] == note)
    kw = lq.kwargs_of(case)
    arr, method = kw["arr"], kw["method"]
    T = arr.dtype
    want = lq.expected_of(case)
    nan_cols = np.isnan(arr).any(axis=0)
    s = np.sort(arr, axis=0)
    right = _rows_from_sorted(s, 100, method, T)
    right[:, nan_cols] = np.nan
    lq.judge_case(case, right)  # the helper itself is right, so what follows is rejected for the defect alone
    lq.judge_case(case, want)

    col = int(np.flatnonzero(~nan_cols & np.isfinite(arr).all(axis=0) & (s[150] != s[151]))[-1])
    swapped = s.copy()
    swapped[[150, 151], col] = s[[151, 150], col]  # two neighbouring sorted samples swapped
    bad = _rows_from_sorted(swapped, 100, method, T)
    bad[:, nan_cols] = np.nan
    assert 0 < lq.qn.equal_bits(bad, want) < want.size and np.sum(bad[:, col] != want[:, col]) <= 4
    with pytest.raises(lq.Mismatch):
        lq.judge_case(case, bad)

    for pad in (np.inf, np.nan):  # the padding's key read as a value in the top slot: +inf, or the NaN the largest key decodes to
        leaked = s.copy()
        leaked[-1, col] = pad
        bad = _rows_from_sorted(leaked, 100, method, T)
        bad[:, nan_cols] = np.nan
        assert np.array_equal(bad[:-2], want[:-2], equal_nan=True)  # only the top levels see it
        with pytest.raises(lq.Mismatch):
            lq.judge_case(case, bad)

    if nan_cols.any():  # a NaN column answered with numbers (the NaN sorted as the maximum and read as one)
        bad = right.copy()
        numbers = _rows_from_sorted(np.where(np.isnan(s), np.inf, s), 100, method, T)
        bad[:50, nan_cols] = numbers[:50, nan_cols]
        assert np.isfinite(bad[:50, nan_cols]).all()
        with pytest.raises(lq.Mismatch):
            lq.judge_case(case, bad)
    else:
        bad = want.copy()
        bad[:, col] = np.nan  # and the other way round: NaN where the reference has numbers
        with pytest.raises(lq.Mismatch):
            lq.judge_case(case, bad)


def test_the_nan_column_case_is_among_them():
    case = next(c for c in lq.cases() if c["note"] == "f64 m 300 special axis first sort which 100")
    assert np.isnan(lq.kwargs_of(case)["arr"]).any(axis=0).sum() == 1
