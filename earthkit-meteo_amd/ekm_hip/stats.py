"""`earthkit.meteo.stats.iter_quantiles` on MI355X: the quantiles of a sample axis at every point of an array (reference
stats/array/quantiles.py:18-84; kernel `quantile_points` in csrc/ensemble.hip).

`iter_quantiles` keeps the reference's name, argument order, defaults and its being a generator; `quantiles` is this
project's addition and returns the same rows stacked.  All levels of a call are computed by ONE launch: the point's
samples are sorted once in LDS and every level is read off the sorted column.  NumPy in -> NumPy out; `DeviceArray` in
-> `DeviceArray` out (the yielded rows are views of one allocation); device tensors of another ROCm library are taken
over through DLPack and handed back in that library's type.  The input is never modified (the reference's docstring says
"in place", its code copies).

The three methods do not give the same bits, and each is reproduced bit for bit:
  "sort"        s[j] * (1 - x) + s[min(j + 1, m - 1)] * x with f = (m - 1) * q, j = int(f), x = f - j: positions, products
                and sum in float64, so the result is float64 for f32 input too.  No shortcut for x == 0: an infinite
                s[j + 1] there gives NaN, as in the reference;
  "numpy_bulk"  numpy.quantile with float64 levels: float64 result;
  "numpy"       numpy.quantile with each level cast to the array's dtype: the result has the array's dtype.
f32 and f64 arrays are computed as they are; every other dtype (integer, f16) is computed as f64.  A column that holds a
NaN gives NaN at every level.

Limits and deviations:
  * the sample axis holds at most 256 values in f32 and 128 in f64 (the sorted columns of 64 points fill 64 KiB of LDS);
    more raises `EkmError`;
  * a level outside [0, 1] or NaN raises `ValueError` in every method.  For "sort" the reference raises `IndexError`
    above 1 and silently wraps around to the largest samples below 0;
  * the levels are read as float64 (a list, as the reference documents it); an integer array computed by "numpy" gets
    numpy.quantile on f64 data (the reference casts each level to the integer dtype, i.e. to 0 or 1).
The first use of a (method, sample count, levels) uploads its position table, which cannot be recorded: call once outside
an `ekm_hip.graph()` block before recording.
"""
import math

import numpy as np

from . import _ensemble as _e
from ._ffi import QUANTILE_LERP, QUANTILE_SORT
from .device import DeviceArray, current_stream
from .vertical import _foreign_aware

_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)
_METHODS = ("sort", "numpy_bulk", "numpy")


def quantile_levels(which):
    """The float64 levels of `which` (quantiles.py:54-58): an int n gives linspace(0, 1, n + 1), a list its own order."""
    if isinstance(which, int):
        qs = np.linspace(0.0, 1.0, which + 1)
    else:
        qs = np.asarray(which, dtype=np.float64)
        if qs.ndim != 1:
            raise ValueError(f"iter_quantiles: which must be an int or a list of levels, got an array of shape {qs.shape}")
    if qs.size and not (qs.min() >= 0.0 and qs.max() <= 1.0):  # a NaN fails both comparisons
        raise ValueError("Quantiles must be in the range [0, 1]")
    return qs


def quantile_positions(method, m, qs, dtype):
    """The position records (lo, hi, w) of the levels `qs` in a sorted column of `m` samples, as float64 vectors, computed
    with NumPy exactly as the reference ("sort", quantiles.py:76-81) and numpy.quantile's linear method ("numpy_bulk" with
    float64 levels, "numpy" with the levels in `dtype`) compute them; the kernel evaluates no floor of its own."""
    qs, m = np.asarray(qs, dtype=np.float64), int(m)
    if method == "sort":
        f = (m - 1) * qs
        j = f.astype(np.int64)  # int(f): the levels are >= 0
        return j.astype(np.float64), np.minimum(j + 1, m - 1).astype(np.float64), f - j
    q = qs.astype(dtype) if method == "numpy" else qs
    vi = (m - 1) * q  # numpy's virtual index, in the dtype of the levels
    prev = np.floor(vi)
    nxt = prev + 1
    above = vi >= m - 1  # numpy clips both neighbours to the last sample and keeps -1 as the "previous index"
    prev[above], nxt[above] = -1, -1
    prev, nxt = prev.astype(np.intp), nxt.astype(np.intp)
    gamma = np.asarray(vi - prev, dtype=vi.dtype)
    return (prev % m).astype(np.float64), (nxt % m).astype(np.float64), gamma.astype(np.float64)


@_foreign_aware("arr")
def quantiles(arr, which=100, axis=0, method="sort"):
    """Every level of `iter_quantiles(arr, which, axis, method)` stacked along a new leading axis: [nq, ...] with `axis`
    removed from `arr`'s shape.  The reference has no such function; with `which=100` on an ensemble or a climate sample
    this is the `clim` that `extreme.sot` and `extreme.efi` take."""
    if method not in _METHODS:
        raise ValueError(f"Invalid method {method!r}, expected 'sort', 'numpy_bulk', or 'numpy'")
    arr = _e.as_input(arr)
    qs = quantile_levels(which)
    shape = tuple(int(v) for v in arr.shape)
    if not shape:
        raise ValueError("iter_quantiles: arr must have at least one dimension")
    if not -len(shape) <= axis < len(shape):
        raise np.exceptions.AxisError(axis, len(shape))
    axis = int(axis) % len(shape)
    m, outer, inner = shape[axis], math.prod(shape[:axis]), math.prod(shape[axis + 1:])
    rest = shape[:axis] + shape[axis + 1:]
    if m < 1:
        raise ValueError("iter_quantiles: the sample axis is empty")
    dtype = _e.arith_dtype(arr)
    out_dtype = _F32 if dtype == _F32 and method == "numpy" else _F64
    nq = int(qs.size)
    if (nq == 0 or outer * inner == 0) and not _e.on_device(arr):
        return np.empty((nq,) + rest, out_dtype)  # no work: no device is asked for
    device, stream, keep = _e.device_of(arr), current_stream(), []
    if nq == 0 or outer * inner == 0:
        return DeviceArray.empty((nq,) + rest, out_dtype, device)
    _, tabs = _e.table(("quantiles", method, dtype.str, qs.tobytes()), m, device,
                       lambda: quantile_positions(method, m, qs, dtype))
    d_arr = _e.upload(arr, dtype, device, stream, keep)
    out = DeviceArray.empty((nq,) + rest, out_dtype, device)
    entry = "ekm_quantiles_" + ("f32" if out_dtype == _F32 else "f64" if dtype == _F64 else "f32_f64")
    _e._ffi.check(getattr(_e.lib(), entry)(
        device, stream, d_arr.ptr, outer, m, inner, tabs[0].on(stream), tabs[1].on(stream), tabs[2].on(stream), nq,
        QUANTILE_SORT if method == "sort" else QUANTILE_LERP, out.on(stream)))
    return _e.finish(out, _e.on_device(arr))


def iter_quantiles(arr, which=100, axis=0, method="sort"):
    """Iterate over the quantiles of `arr` along `axis` (quantiles.py:18-84).  which: an int n for the n + 1 evenly
    spaced levels linspace(0, 1, n + 1), or a list of levels in [0, 1], yielded in the caller's order.  method: 'sort',
    'numpy_bulk' or 'numpy' (module docstring).  One launch computes all levels; level k is then yielded as row k of
    the result, with `arr`'s shape without `axis`."""
    res = quantiles(arr, which, axis, method)
    if isinstance(res, DeviceArray):
        n = math.prod(res.shape[1:])
        for k in range(res.shape[0]):
            yield res.flat_slice(k * n, (k + 1) * n).reshape(res.shape[1:])
    else:
        yield from res
