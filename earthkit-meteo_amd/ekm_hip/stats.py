"""`earthkit.meteo.stats.iter_quantiles` on MI355X: the quantiles of a sample axis at every point of an array (reference
stats/array/quantiles.py:18-84; kernel `quantile_points` in csrc/ensemble.hip, and `long_quantile_tiles` in
csrc/long_quantiles.hip for sample axes beyond 256 / 128 values: `long_quantiles`, below).

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

`long_quantiles` / `iter_long_quantiles` (kernel `long_quantile_tiles` in csrc/long_quantiles.hip) are `quantiles` /
`iter_quantiles` for LONG sample axes: up to 16384 values in f32 and 8192 in f64 (one column, padded to a power of two,
in 64 KiB of LDS; more raises `EkmError` naming the cap).  Everything above holds for them -- the three methods bit for
bit, the dtype rules, NaN columns, the input and output types, the errors, the graph rule; the two pairs share one host
body and one set of position tables.  One workgroup sorts a tile of whole columns with a bitonic network over the
order-preserving whole-number image of the float bits, then reads every level off the sorted columns with the
arithmetic of `quantiles`.  Those keys order -0.0 before +0.0, which NumPy's sort leaves open (and the insertion sort of
`quantiles` keeps as the input has them): in a column that holds both zeros, a level that lands on a zero may differ
from the reference, and from `quantiles`, in the zero's sign -- the one place where the results are not the reference's
bits.  Short axes are accepted and give the bits of `quantiles`.
Which to call: `iter_quantiles` / `quantiles` are the reference's names and stay as they are (their cap is an error, not a
fallback); for speed, the two kernels are level at 32 samples and `long_quantiles` is the faster from 64 samples up,
because the per-lane insertion sort is O(m^2): measured on one MI355X at 101 levels (profiles/long_quantiles_bench.json,
`crossover`), f32 long / short = 0.70 / 0.71 ms at 32 samples (sample axis last; 0.79 / 0.70 ms with it first), 0.49 /
1.86 ms at 64, 0.48 / 6.8 ms at 128 and 1.85 / 100 ms at 256; f64 0.44 / 0.64 ms at 32 and 0.44 / 6.9 ms at 128.

`GumbelDistribution`, `value_to_return_period` and `return_period_to_value` (reference stats/array/extreme_values.py:24-155;
kernels `gumbel_fit_points`, `gumbel_cdf_points`, `gumbel_ppf_points` in csrc/ensemble.hip) keep the reference's names,
argument order and defaults.  `fit` sorts the sample axis of every point in LDS and forms the first two L-moments as the
reference's own `lmoment` (stats/array/_polyfill.py) forms them; `cdf` and `ppf` are outer products of the levels and the
points, shape `x.shape + dist.shape`.  `mu` and `sigma` are NumPy arrays for NumPy input, `DeviceArray`s for device input
and tensors of the caller's library for its device tensors, and so are the results.  `ppf` and `return_period_to_value`
equal the reference bit for bit (the host forms log(-log(1 - p)) with NumPy, the kernel one product and one difference);
`fit` equals the reference's polyfill on the sample widened to float64 bit for bit; `cdf` is within 8 * 2**-53 absolute
of the reference (two exponentials of the device library), and the return period is `freq / cdf` of that cdf.

Deviations of the Gumbel functions:
  * mu, sigma and every result are float64.  The reference gives f32 when mu, sigma and x are all f32; levels,
    probabilities and return periods are read as float64 on the host;
  * the sample axis holds at most 256 values in f32 and 128 in f64; more raises `EkmError`;
  * samples of 2 and 3 values are accepted in every build.  The reference's polyfill refuses fewer than 4 (SciPy's
    `lmoment`, which the reference uses where SciPy >= 1.15 is installed, takes 3);
  * an f32 sample is sorted as f32 and summed in float64.  Both reference paths sum it in f32, so this is the more
    accurate result: the difference is bounded by 2 n (2**-23 + 2**-52) max|x| per column;
  * a `timedelta` freq works for NumPy distributions only (the host forms `freq / cdf` and `freq / return_period` as the
    reference does); for a device distribution it raises `TypeError`.
The first use of a set of levels uploads it, which cannot be recorded: call once outside an `ekm_hip.graph()` block.

`GumbelDistribution.long_fit` (kernel `long_gumbel_fit_tiles` in csrc/long_ensemble.hip) is `fit` for LONG sample axes: up to
16384 values in f32 and 8192 in f64 (more raises `EkmError` naming the cap), any axis.  Same arguments, dtype rules, errors,
input and output types; it returns the same class, so `cdf`, `ppf`, `value_to_return_period` and `return_period_to_value`
work on it unchanged, and the two share one host body.  One workgroup sorts a tile of whole columns with the network of
`long_quantiles`, then one lane per column forms the two sums in float64 in the polyfill's order.  As for `long_quantiles`
the keys order -0.0 before +0.0: in a column that holds both zeros mu and sigma may differ from `fit`'s in the sign of a
zero (a sum of zeros); nowhere else.  Short axes are accepted and give the bits of `fit`.
Which to call: `fit` stays as it is (its cap is an error, not a fallback); for speed `long_fit` is the faster at every
sample count measured, from 32 up: on one MI355X at 2^20 points, sample axis first (profiles/long_ensemble_bench.json,
`fit_crossover`), f32 long / short = 0.13 / 0.31 ms at 32 samples, 0.30 / 1.01 at 51, 0.31 / 1.93 at 64, 0.83 / 15.3 at
128 and 2.1 / 117 at 256; f64 0.23 / 0.53 at 32, 0.61 / 1.78 at 51 and 1.62 / 30.0 at 128.  Beyond the short cap, at 2^16
points: f32 0.43 ms at 512 samples and 2.8 ms at 1980 (f64 0.79 and 5.3 ms; NumPy on the host: 0.47 s and 2.2 s).

`nanaverage(data, weights=None, **kwargs)` (reference stats/array/numpy_extended.py:13-61; kernels `nanavg_points`,
`nanavg_rows`, `nanavg_split` in csrc/reduce.hip) is the NaN-skipping, optionally weighted mean along one axis, a run of
adjacent axes or the whole array.  The data is read once (twice by the weighted mean along a non-contiguous axis) and
nothing is stored but the result; weights that broadcast (a vector along the axis, `[lat, 1]`, a scalar) are read through
strides, never expanded.  Nothing is uploaded but the operands, so a device-resident call can be recorded into a graph.
Its docstring lists the deviations.
"""
import datetime
import math
import numbers
import operator

import numpy as np

from . import _ensemble as _e
from ._ffi import GUMBEL_CDF, GUMBEL_RETURN_PERIOD, QUANTILE_LERP, QUANTILE_SORT
from .device import DeviceArray, _Allocation, current_stream
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


def _quantiles(arr, which, axis, method, family):
    """What `quantiles` (family "ekm_quantiles_") and `long_quantiles` ("ekm_long_quantiles_") share: everything but the
    kernel and its cap."""
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
    entry = family + ("f32" if out_dtype == _F32 else "f64" if dtype == _F64 else "f32_f64")
    _e._ffi.check(getattr(_e.lib(), entry)(
        device, stream, d_arr.ptr, outer, m, inner, tabs[0].on(stream), tabs[1].on(stream), tabs[2].on(stream), nq,
        QUANTILE_SORT if method == "sort" else QUANTILE_LERP, out.on(stream)))
    return _e.finish(out, _e.on_device(arr))


@_foreign_aware("arr")
def quantiles(arr, which=100, axis=0, method="sort"):
    """Every level of `iter_quantiles(arr, which, axis, method)` stacked along a new leading axis: [nq, ...] with `axis`
    removed from `arr`'s shape.  The reference has no such function; with `which=100` on an ensemble or a climate sample
    this is the `clim` that `extreme.sot` and `extreme.efi` take."""
    return _quantiles(arr, which, axis, method, "ekm_quantiles_")


@_foreign_aware("arr")
def long_quantiles(arr, which=100, axis=0, method="sort"):
    """`quantiles` for a long sample axis: up to 16384 values in f32 and 8192 in f64 (more raises `EkmError`), sorted by
    one workgroup per tile of columns (kernel `long_quantile_tiles`).  Same arguments, methods, dtypes, levels, errors and
    results; for a sample axis both functions take, the bits are the same, except for the sign of a zero result in a
    column that holds both -0.0 and +0.0 (module docstring).  With `which=100` on a model-climate sample (say 20 years x
    9 dates x 11 members = 1980 values) this is the `clim` of `extreme.efi`, `extreme.sot` and `extreme.cpf`."""
    return _quantiles(arr, which, axis, method, "ekm_long_quantiles_")


def _nanaverage_run(axis, ndim, weighted):
    """(first, last) of the run of adjacent dimensions that `axis` names, or None for all of them."""
    if axis is None:
        return None
    if isinstance(axis, tuple):
        if weighted:  # the reference fails on `reshape[axis] = 1` with a list-index TypeError
            raise TypeError(f"nanaverage: with weights, axis must be None or an int, not the tuple {axis}")
        named = []
        for a in axis:
            a = operator.index(a)
            if not -ndim <= a < ndim:
                raise np.exceptions.AxisError(a, ndim)
            named.append(a % ndim)
        run = sorted(named)
        if not run or len(set(run)) != len(run) or run != list(range(run[0], run[-1] + 1)):
            raise ValueError(f"nanaverage: axis={axis} must name distinct adjacent dimensions (one run, such as (-2, -1)); "
                             f"of {ndim} dimensions it names {tuple(named)}")
        return run[0], run[-1]
    a = operator.index(axis)
    if not -ndim <= a < ndim:
        raise np.exceptions.AxisError(a, ndim)
    return a % ndim, a % ndim


def _nanaverage_weight_strides(wshape, shape, first, last):
    """The element strides (outer, m, inner) under which C-contiguous weights of `wshape`, broadcast against `shape`, are
    read on the [outer, m, inner] view (0 = broadcast), or None when a group of dimensions does not collapse to one."""
    nd = len(shape)
    w = (1,) * (nd - len(wshape)) + tuple(wshape)
    strides, acc = [0] * nd, 1
    for k in reversed(range(nd)):
        strides[k] = 0 if w[k] == 1 else acc
        acc *= w[k]
    out = []
    for lo, hi in ((0, first), (first, last + 1), (last + 1, nd)):
        stride = expect = None
        for k in reversed(range(lo, hi)):
            if shape[k] == 1:
                continue
            if stride is None:
                stride = strides[k]
            elif strides[k] != expect:
                return None
            expect = strides[k] * shape[k]
        out.append(stride or 0)
    return tuple(out)


@_foreign_aware("data", "weights")
def nanaverage(data, weights=None, **kwargs):
    """A merge of the functionality of np.nanmean and np.average (numpy_extended.py:13-61): the mean of `data` along
    `axis` where NaN values are ignored and `weights` are applied if given.

    weights: anything NumPy broadcasts against data's shape; normalised by the sum of the valid weights of every slice.  A
    sample whose weight is NaN is skipped like one whose datum is NaN.
    kwargs: axis (None: the whole array; an int; for the unweighted mean also a tuple of adjacent axes) and keepdims.

    The result is float32 only when every array given is float32, float64 otherwise.  Along an axis that is not the
    contiguous one the result is the reference's bit for bit; along the contiguous axis (and for axis=None) NumPy adds
    pairwise and the kernels lane by lane, so the result is within a rounding bound of the exact mean
    (tests/_nanaverage_numpy.py).  An all-NaN slice gives NaN without weights and 0.0 with them, as in the reference.

    Deviations: a tuple of axes must name one run of adjacent dimensions (ValueError otherwise); the other keywords of
    numpy.nansum / numpy.nanmean (dtype, out, where, initial) raise TypeError; weights that would enlarge data's shape
    raise ValueError (the reference fails later, with a boolean-index error); no RuntimeWarning is issued for an empty
    slice; float16 input is computed and returned as float64; integer data with integer weights is computed in float64 (the
    reference fails there, writing NaN into an integer array)."""
    for key in kwargs:
        if key not in ("axis", "keepdims"):
            raise TypeError(f"nanaverage: the keyword {key!r} is not supported (axis and keepdims are)")
    axis, keepdims = kwargs.get("axis"), bool(kwargs.get("keepdims", False))
    data = _e.as_input(data)
    weighted = weights is not None
    if weighted:
        weights = _e.as_input(weights)
    shape = tuple(int(v) for v in data.shape)
    nd = len(shape)
    run = _nanaverage_run(axis, nd, weighted)
    first, last = (0, nd - 1) if run is None else run
    outer, m, inner = math.prod(shape[:first]), math.prod(shape[first:last + 1]), math.prod(shape[last + 1:])
    rest = shape[:first] + ((1,) * (last - first + 1) if keepdims else ()) + shape[last + 1:]
    wstrides = (0, 0, 0)
    if weighted:
        wshape = tuple(int(v) for v in weights.shape)
        try:
            fits = np.broadcast_shapes(wshape, shape) == shape
        except ValueError:
            fits = False
        if not fits:
            raise ValueError(f"nanaverage: weights of shape {wshape} do not broadcast against the data's shape {shape}")
        wstrides = _nanaverage_weight_strides(wshape, shape, first, last)
    dtype = _e.arith_dtype(data, weights) if weighted else _e.arith_dtype(data)
    device_result = _e.on_device(data, weights) if weighted else _e.on_device(data)
    if outer * inner == 0 and not device_result:
        return np.empty(rest, dtype)  # no work: no device is asked for
    device, stream, keep = (_e.device_of(data, weights) if weighted else _e.device_of(data)), current_stream(), []
    out = DeviceArray.empty(rest, dtype, device)
    if outer * inner == 0:
        return out
    d_data = _e.upload(data, dtype, device, stream, keep)
    d_w = None
    if weighted:
        if wstrides is None:  # the broadcast does not collapse onto [outer, m, inner]: expanded once, on the host
            host = weights.to_host() if isinstance(weights, DeviceArray) else weights
            weights, wstrides = np.ascontiguousarray(np.broadcast_to(host, shape)), (m * inner, inner, 1)
        d_w = _e.upload(weights, dtype, device, stream, keep)
    lib = _e.lib()
    need = int(lib.ekm_nanaverage_work_bytes(dtype.itemsize, outer, m, inner, int(weighted), 0))
    work = None
    if need:  # the split path's partial sums: the block belongs to this call (and to the graph that records it)
        work = _Allocation(need, device)
        work.touch(stream)
    _e._ffi.check(getattr(lib, "ekm_nanaverage_" + _e.tag_of(dtype))(
        device, stream, d_data.ptr, outer, m, inner, d_w.ptr if weighted else None, *wstrides, 0,
        work.ptr if work is not None else None, need, out.on(stream)))
    if work is not None:
        work.free()  # back to the block cache of this stream: a later user is ordered after the kernels
    return out if device_result else _e.finish(out, False)[()]


def iter_quantiles(arr, which=100, axis=0, method="sort"):
    """Iterate over the quantiles of `arr` along `axis` (quantiles.py:18-84).  which: an int n for the n + 1 evenly
    spaced levels linspace(0, 1, n + 1), or a list of levels in [0, 1], yielded in the caller's order.  method: 'sort',
    'numpy_bulk' or 'numpy' (module docstring).  One launch computes all levels; level k is then yielded as row k of
    the result, with `arr`'s shape without `axis`."""
    yield from _rows(quantiles(arr, which, axis, method))


def iter_long_quantiles(arr, which=100, axis=0, method="sort"):
    """`iter_quantiles` for a long sample axis (`long_quantiles`): one launch computes all levels, level k is yielded as
    row k of the one result."""
    yield from _rows(long_quantiles(arr, which, axis, method))


def _rows(res):
    """The rows of a stacked result: views of the one allocation for a `DeviceArray`."""
    if isinstance(res, DeviceArray):
        n = math.prod(res.shape[1:])
        for k in range(res.shape[0]):
            yield res.flat_slice(k * n, (k + 1) * n).reshape(res.shape[1:])
    else:
        yield from res


def _as_f64_device(a, shape, device):
    """`a` (DeviceArray or NumPy) as a float64 DeviceArray of `shape`; another dtype or shape goes through the host."""
    if isinstance(a, DeviceArray) and a.dtype == _F64 and tuple(a.shape) == shape:
        return a
    host = a.to_host() if isinstance(a, DeviceArray) else np.asarray(a)
    return DeviceArray.from_host(np.ascontiguousarray(np.broadcast_to(host.astype(np.float64), shape)), device).reshape(shape)


def _is_timedelta(freq):
    return isinstance(freq, (datetime.timedelta, np.timedelta64))


def _numeric_freq(freq):
    if freq is None:
        return 1.0
    if isinstance(freq, (numbers.Real, np.number)) and not isinstance(freq, bool):
        return float(freq)
    raise TypeError(f"freq must be None, a number or a timedelta, got {type(freq).__name__}")


class GumbelDistribution:
    """Gumbel distribution for extreme value statistics (extreme_values.py:24-110).

    mu, sigma: offset and scale, numbers or arrays, broadcast against each other and held as float64.
    freq: None, a number or a timedelta: the duration between the values of the represented data; scales the return
    periods computed from the distribution."""

    def __init__(self, mu, sigma, freq=None):
        from . import _engine

        (mu, sigma), self._foreign = _engine._adopt_foreign([mu, sigma])
        self._handed = None
        self.freq = freq
        if _e.on_device(mu, sigma):
            device = _e.device_of(mu, sigma)
            shape = np.broadcast_shapes(tuple(np.shape(mu)), tuple(np.shape(sigma)))
            self._mu, self._sigma = _as_f64_device(mu, shape, device), _as_f64_device(sigma, shape, device)
        else:
            mu, sigma = np.broadcast_arrays(np.asarray(mu), np.asarray(sigma))
            self._mu, self._sigma = mu.astype(np.float64, copy=False), sigma.astype(np.float64, copy=False)

    @classmethod
    def fit(cls, sample, axis=0, freq=None):
        """Gumbel distribution with parameters fitted to a sample of values along `axis` by the method of L-moments
        (extreme_values.py:44-64).  One launch: every point's samples are sorted in LDS, then summed in float64."""
        return cls._fit(sample, axis, freq, "ekm_gumbel_fit_")

    @classmethod
    def long_fit(cls, sample, axis=0, freq=None):
        """`fit` for a long sample axis: up to 16384 values in f32 and 8192 in f64 (more raises `EkmError` naming the cap),
        sorted by one workgroup per tile of columns (kernel `long_gumbel_fit_tiles`), then summed in float64 in the same
        order.  Same arguments, dtypes, errors and results, the same class; for a sample axis both take, the bits are
        the same (module docstring: the sign of a zero)."""
        return cls._fit(sample, axis, freq, "ekm_long_gumbel_fit_")

    @classmethod
    def _fit(cls, sample, axis, freq, family):
        """What `fit` (family "ekm_gumbel_fit_") and `long_fit` ("ekm_long_gumbel_fit_") share: everything but the kernel
        and its cap."""
        from . import _engine

        (sample,), foreign = _engine._adopt_foreign([sample])
        sample = _e.as_input(sample)
        shape = tuple(int(v) for v in sample.shape)
        if not shape:
            raise ValueError("GumbelDistribution.fit: sample must have at least one dimension")
        if not -len(shape) <= axis < len(shape):
            raise np.exceptions.AxisError(axis, len(shape))
        axis = int(axis) % len(shape)
        m, outer, inner = shape[axis], math.prod(shape[:axis]), math.prod(shape[axis + 1:])
        rest = shape[:axis] + shape[axis + 1:]
        if m < 2:
            raise ValueError("GumbelDistribution.fit: at least two values are needed along the sample axis")
        dtype = _e.arith_dtype(sample)
        if outer * inner == 0 and not _e.on_device(sample):
            return cls(np.empty(rest), np.empty(rest), freq=freq)  # no work: no device is asked for
        device, stream, keep = _e.device_of(sample), current_stream(), []
        mu, sigma = DeviceArray.empty(rest, _F64, device), DeviceArray.empty(rest, _F64, device)
        if outer * inner:
            d_sample = _e.upload(sample, dtype, device, stream, keep)
            _e._ffi.check(getattr(_e.lib(), family + _e.tag_of(dtype))(
                device, stream, d_sample.ptr, outer, m, inner, mu.on(stream), sigma.on(stream)))
        on_device = _e.on_device(sample)
        dist = cls(_e.finish(mu, on_device), _e.finish(sigma, on_device), freq=freq)
        dist._foreign = foreign
        return dist

    def _hand(self):
        if self._handed is None:
            from . import _engine

            self._handed = _engine._hand_back((self._mu, self._sigma), self._foreign) if self._foreign else (self._mu, self._sigma)
        return self._handed

    @property
    def mu(self):
        return self._hand()[0]

    @property
    def sigma(self):
        return self._hand()[1]

    @property
    def shape(self):
        """Tuple of dimensions."""
        return tuple(self._mu.shape)

    @property
    def ndim(self):
        """Number of dimensions."""
        return len(self._mu.shape)

    @property
    def _on_device(self):
        return isinstance(self._mu, DeviceArray)

    def _outer(self, what, levels, freq=1.0, mode=None):
        """out[k, p] of the `levels` (a float64 array of any shape) and the points: one launch of gumbel_cdf_points
        (mode given) or gumbel_ppf_points."""
        levels = np.asarray(levels, dtype=np.float64, order="C")  # (ascontiguousarray would make a number 1-D)
        shape = tuple(levels.shape) + self.shape
        npts, nlev = math.prod(self.shape), int(levels.size)
        if npts == 0 or nlev == 0:
            res = DeviceArray.empty(shape, _F64, self._mu.device) if self._on_device else np.empty(shape)
        else:
            device, stream, keep = _e.device_of(self._mu), current_stream(), []
            _, (d_levels,) = _e.table(("gumbel", what, levels.tobytes()), nlev, device, lambda: (levels.reshape(-1),))
            mu, sigma = _e.upload(self._mu, _F64, device, stream, keep), _e.upload(self._sigma, _F64, device, stream, keep)
            out = DeviceArray.empty(shape, _F64, device)
            if mode is None:
                rc = _e.lib().ekm_gumbel_ppf_f64(device, stream, mu.ptr, sigma.ptr, npts, d_levels.on(stream), nlev, out.on(stream))
            else:
                rc = _e.lib().ekm_gumbel_cdf_f64(device, stream, mu.ptr, sigma.ptr, npts, d_levels.on(stream), nlev, float(freq),
                                                 mode, out.on(stream))
            _e._ffi.check(rc)
            res = _e.finish(out, self._on_device)
        if self._foreign:
            from . import _engine

            res = _engine._hand_back((res,), self._foreign)[0]
        return res

    def cdf(self, x):
        """The probability that a random variable from the distribution is less than or equal to x
        (extreme_values.py:76-92): 1 - exp(-exp((mu - x) / sigma)), shape x.shape + dist.shape."""
        return self._outer("cdf", x, 1.0, GUMBEL_CDF)

    def ppf(self, p):
        """The percent point function (inverse cdf) of the probability p in [0, 1] (extreme_values.py:94-110):
        mu - sigma * log(-log(1 - p)), shape p.shape + dist.shape."""
        with np.errstate(all="ignore"):
            t = np.log(-np.log(1.0 - np.asarray(p, dtype=np.float64)))
        return self._outer("ppf", t)


def value_to_return_period(dist, value):
    """Return period of a value given a distribution of extremes (extreme_values.py:113-133): freq / dist.cdf(value),
    with freq = 1 when the distribution has none.  A numeric freq is divided in the kernel."""
    if _is_timedelta(dist.freq):
        if dist._on_device:
            raise TypeError("value_to_return_period: a timedelta freq needs a NumPy distribution (the device result is float64)")
        with np.errstate(all="ignore"):
            return dist.freq / dist.cdf(value)
    return dist._outer("return_period", value, _numeric_freq(dist.freq), GUMBEL_RETURN_PERIOD)


def return_period_to_value(dist, return_period):
    """Value for a given return period of a distribution of extremes (extreme_values.py:136-155):
    dist.ppf(freq / return_period), with freq = 1 when the distribution has none."""
    if _is_timedelta(dist.freq):
        if dist._on_device:
            raise TypeError("return_period_to_value: a timedelta freq needs a NumPy distribution")
        return dist.ppf(dist.freq / return_period)
    with np.errstate(all="ignore"):
        return dist.ppf(_numeric_freq(dist.freq) / np.asarray(return_period, dtype=np.float64))
