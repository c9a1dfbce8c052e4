"""An independent NumPy restatement of stats.nanaverage, its judges, and access to tests/golden/nanaverage_golden.npz --
TEST INFRASTRUCTURE.

The restatement (`restated`): the averaged run of axes moved to the front and flattened, ONE ROW AFTER THE OTHER in the
call's dtype from an accumulator that starts at +0.  Unweighted: the sum of `isnan(d) ? 0 : d` divided by the count of
the others in float64 and rounded once.  Weighted: den = the sum of w where neither d nor w is NaN, then the sum of
d * (w / den) with NaN products as 0.  This is what NumPy does when the averaged axis is not the contiguous one.

The parity claims:

  inner > 1 (the averaged axis is not the contiguous one): bit for bit with the recording, the sign of zero included.

  inner == 1 (the contiguous axis, axis=None): NumPy adds pairwise, the kernels lane by lane, chunk by chunk: no fixed
  order gives NumPy's bits, so the result is held to a bound on |got - exact| that is valid for a sum of the valid terms
  in ANY order.  `exact` is the reference's formula in numpy.longdouble on the inputs widened.  With u = eps / 2 the unit
  roundoff, n the number of valid terms, N = sum d w, D = sum w (w = 1 and D = n exactly without weights):
    * every product d w is rounded once and a sum of n terms in any order adds at most n - 1 roundings to each:
      |N^ - N| <= ((1 + u)^n - 1) sum |d w|, and likewise |D^ - D| <= ((1 + u)^(n-1) - 1) sum |w|;
    * the quotient is rounded once: got = (N^ / D^) (1 + delta), |delta| <= u;
    * first order: got - N / D = (N^ - N) / D - (N / D) (D^ - D) / D + delta N / D, and |N / D| <= sum |d w| / |D|, so
      |got - exact| <= (n u + (n - 1) u kappa + u) sum |d w| / |D| with kappa = sum |w| / |D| >= 1, the condition of the
      weight sum (1 for weights of one sign, and the term is absent without weights: the count is exact).
    The reference's own order (every weight divided by D^ first, then d times that, then the sum) has the same count: two
    roundings per term, n - 1 from the sum, and the error of D^ shared by all terms.
    The bar doubles that (eps in place of u), which covers every second-order term while n eps kappa < 0.1:
        bar = (n + 4 + [weighted] n kappa) eps sum |d w| / |sum w|.
    Where n eps kappa >= 0.1 -- weights of mixed sign that cancel, sum w = 0 with some w != 0 -- no bound of this kind
    exists: such points are NOT JUDGED on the contiguous paths (their number is printed); the goldens keep them on the
    bit-for-bit path.  Where `exact` is not finite the result must be the same infinity, or NaN with it.
  None of the constants is taken from a run; each judge prints, and files in the ledger, the largest share of the bar used.
"""
import functools
import json
import os

import numpy as np

from _ensemble_numpy import F32, F64, Mismatch, equal_bits, judge_exact  # noqa: F401
from _regimes_numpy import judge_bar

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nanaverage_golden.npz")
KIND = "nanaverage along the contiguous axis: (n + 4 + n kappa) eps sum |d w| / |sum w| (tests/_nanaverage_numpy.py)"
LD = np.longdouble
POINTS, ROWS, SPLIT = 1, 2, 3
SPLIT_CHUNK = 32768  # csrc/reduce_point.hpp: kNanSplitChunk


def arith_dtype(*arrays):
    return F32 if all(np.asarray(a).dtype == F32 for a in arrays) else F64


# ---- golden file ----
@functools.lru_cache(maxsize=1)
def _load():
    with np.load(PATH) as f:
        meta = json.loads(bytes(f["manifest"]).decode())
        arrays = {k: f[k] for k in f.files if k != "manifest"}
    for a in arrays.values():
        a.setflags(write=False)
    return meta, arrays


def signatures():
    return _load()[0]["signatures"]


def cases():
    return _load()[0]["cases"]


def arrays_of(case):
    return {k: _load()[1][key] for k, key in case["arrays"].items()}


def recorded(case):
    return None if case["out"] is None else _load()[1][case["out"]]


def case_id(case):
    return f"{case['id']}-{case['note'].replace(' ', '_')}"


def call_of(case):
    """(data, weights or None, kwargs) as the recording was called."""
    a = arrays_of(case)
    kwargs = dict(case["plain"]["kwargs"])
    if case["plain"]["axis_is_tuple"]:
        kwargs["axis"] = tuple(kwargs["axis"])
    return a["data"], a.get("weights"), kwargs


# ---- layout ----
def run_of(shape, axis):
    """(first, last) of the averaged run of dimensions."""
    nd = len(shape)
    if axis is None:
        return 0, nd - 1
    named = sorted(a % nd for a in (axis if isinstance(axis, tuple) else (axis,)))
    assert named == list(range(named[0], named[-1] + 1)), "not one run of adjacent axes"
    return named[0], named[-1]


def layout(shape, axis):
    first, last = run_of(shape, axis)
    prod = lambda s: int(np.prod(s, dtype=np.int64))  # noqa: E731
    return prod(shape[:first]), prod(shape[first:last + 1]), prod(shape[last + 1:])


def _rows_first(data, weights, axis, T):
    """(d [m, outer, inner], w of the same shape or None) in dtype T."""
    data = np.asarray(data)
    outer, m, inner = layout(data.shape, axis)
    d = np.moveaxis(data.astype(T).reshape(outer, m, inner), 1, 0)
    if weights is None:
        return d, None
    w = np.broadcast_to(np.asarray(weights).astype(T), data.shape).reshape(outer, m, inner)
    return d, np.moveaxis(w, 1, 0)


def result_shape(shape, axis, keepdims=False):
    first, last = run_of(shape, axis)
    return tuple(shape[:first]) + ((1,) * (last - first + 1) if keepdims else ()) + tuple(shape[last + 1:])


# ---- the restatement ----
def restated(data, weights=None, axis=None, keepdims=False):
    data = np.asarray(data)
    T = arith_dtype(data) if weights is None else arith_dtype(data, weights)
    d, w = _rows_first(data, weights, axis, T)
    m = d.shape[0]
    zero, z = np.zeros(d.shape[1:], T), np.dtype(T).type(0)
    with np.errstate(all="ignore"):
        if w is None:
            acc, cnt = zero.copy(), np.zeros(d.shape[1:], np.int64)
            for i in range(m):
                nan = np.isnan(d[i])
                acc = acc + np.where(nan, z, d[i])
                cnt += ~nan
            res = (acc.astype(F64) / cnt.astype(F64)).astype(T)
        else:
            den = zero.copy()
            for i in range(m):
                den = den + np.where(np.isnan(d[i]) | np.isnan(w[i]), z, w[i])
            res = zero.copy()
            for i in range(m):
                p = d[i] * (w[i] / den)
                res = res + np.where(np.isnan(p), z, p)
    return np.asarray(res, dtype=T).reshape(result_shape(data.shape, axis, keepdims))


def numpy_formula(data, weights=None, **kwargs):
    """What the reference computes, with NumPy's own reductions (numpy.nanmean; ones_like * w, NaN where the datum is
    NaN, divided by its nansum, nansum of the products)."""
    data = np.asarray(data)
    with np.errstate(all="ignore"):
        if weights is None:
            import warnings

            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return np.nanmean(data, **kwargs)
        tw = np.ones_like(data) * np.asarray(weights)
        tw[np.isnan(data)] = np.nan
        den = np.nansum(tw, **kwargs)
        if kwargs.get("axis") is not None:
            shape = list(tw.shape)
            shape[kwargs["axis"]] = 1
            den = den.reshape(shape)
        return np.nansum(data * (tw / den), **kwargs)


# ---- exact value and bar ----
def exact_and_bar(data, weights, axis, dtype, keepdims=False):
    """(exact in longdouble, bar, judged) in the result's shape.  judged: False where no bound exists (docstring)."""
    data = np.asarray(data)
    d, w = _rows_first(data, weights, axis, LD)
    eps = LD(np.finfo(dtype).eps)
    with np.errstate(all="ignore"):
        if w is None:
            valid = ~np.isnan(d)
            n = valid.sum(axis=0)
            exact = np.where(valid, d, LD(0)).sum(axis=0) / n.astype(LD)
            bar = (n + 4) * eps * np.where(valid, np.abs(d), LD(0)).sum(axis=0) / np.maximum(n, 1)
            judged = np.ones(n.shape, bool)
        else:
            valid = ~(np.isnan(d) | np.isnan(w))
            n = valid.sum(axis=0)
            wv = np.where(valid, w, LD(0))
            den = wv.sum(axis=0)
            terms = d * (np.where(valid, w, LD(np.nan)) / den)
            exact = np.where(np.isnan(terms), LD(0), terms).sum(axis=0)
            prod = np.where(valid, np.abs(d * w), LD(0))
            prod = np.where(np.isnan(prod), LD(0), prod)  # inf * 0 enters as 0, as in the sum
            sw = np.abs(wv).sum(axis=0)
            kappa = np.where(den != 0, sw / np.abs(den), np.where(sw == 0, LD(1), LD(np.inf)))
            bar = (n + 4 + n * kappa) * eps * prod.sum(axis=0) / np.where(den != 0, np.abs(den), LD(1))
            judged = n * eps * kappa < LD(0.1)
    shape = result_shape(data.shape, axis, keepdims)
    return exact.reshape(shape), np.asarray(bar, dtype=LD).reshape(shape), judged.reshape(shape)


def judge(data, weights, axis, got, want, what, ledger=None, keepdims=False, bit_for_bit=None):
    """inner > 1 (or bit_for_bit=True): `got` equals `want` bit for bit.  Otherwise `got` has want's dtype and shape and
    lies within the bar of the exact value.  Returns the share of the bar used (0 on the bit-for-bit path)."""
    data = np.asarray(data)
    _, _, inner = layout(data.shape, axis)
    if inner > 1 if bit_for_bit is None else bit_for_bit:
        judge_exact(got, want, what)
        return 0.0
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        raise Mismatch(f"{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}")
    exact, bar, judged = exact_and_bar(data, weights, axis, got.dtype, keepdims)
    if not judged.all():
        print(f"{what}: {int((~judged).sum())} of {judged.size} points have no bound (cancelling weights) and are not judged")
        got, exact = np.where(judged, got, got.dtype.type(0)), np.where(judged, exact, LD(0))
    return judge_bar(got, exact, bar, what, KIND, ledger)
