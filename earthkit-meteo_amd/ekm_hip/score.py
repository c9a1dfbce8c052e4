"""`earthkit.meteo.score` on MI355X: `crps_from_ensemble` (reference score/array/ensemble.py; kernel csrc/ensemble.hip)
and `pearson_correlation` (reference score/array/deterministic.py; kernels csrc/reduce.hip).

Same name, argument order, default and error conventions as the reference.  NumPy in -> NumPy out; `DeviceArray` in ->
`DeviceArray` out; device tensors of another ROCm library go through DLPack.  `x` is member-major (n_ens, ...), `y` has
the points' shape; trailing dimensions are flattened to points.  At most 256 members in f32 and 128 in f64.  The
differences are formed in f32 when x and y are both f32 and in f64 otherwise; the result is float64 and equals the
reference's bit for bit.

nan_policy: "propagate" leaves NaN at points where x or y holds a NaN.  "raise" and "omit" read the kernel's one-byte
"missing" flags back to the host, so they wait for the device (and cannot be recorded into a graph); "omit" returns the
1-D result of the remaining points, compacted on the host also for DeviceArray input (then uploaded again).

`long_crps_from_ensemble` (kernel `long_crps_tiles` in csrc/long_ensemble.hip) is `crps_from_ensemble` for LONG member
axes: up to 16384 members in f32 and 8192 in f64 (more raises `EkmError` naming the cap).  Same arguments, dtype rule,
policies, errors, input and output types and graph rule; the two share one host body and one set of weight tables.  One
workgroup sorts a tile of whole columns with the bitonic network of `stats.long_quantiles`, then one lane per column walks
the sorted column with the arithmetic of `crps_from_ensemble`, the sum in the same serial order.  The keys of that sort
order -0.0 before +0.0, which NumPy's sort leaves open: in a column that holds both zeros a result may differ from the
reference, and from `crps_from_ensemble`, in the sign of a zero -- the one place where the results are not the reference's
bits.  Short axes are accepted and give the bits of `crps_from_ensemble`.
Which to call: `crps_from_ensemble` is the reference's name and stays as it is (its cap is an error, not a fallback); for
speed the long form is the faster at every member count measured, from 32 up, because the per-lane insertion sort is
O(nens^2): on one MI355X at 2^20 points (profiles/long_ensemble_bench.json, `crossover`), f32 long / short = 0.14 / 0.30 ms
at 32 members, 0.30 / 0.99 at 51, 0.31 / 1.86 at 64, 0.82 / 14.0 at 128 and 2.3 / 104 at 256; f64 0.24 / 0.53 at 32,
0.60 / 1.73 at 51 and 1.63 / 27.5 at 128.  Beyond the short cap, at 2^16 points: f32 0.59 ms at 512 members and 6.0 ms at
1980 (f64 1.1 and 12.1 ms; the NumPy restatement on the host: 0.57 s and 2.6 s) -- at 1980 members the serial walk of one
lane per column costs three times the sort.

`pearson_correlation(x, y, axis=0)`: the correlation of x and y along `axis`, any axis and any length of it (the kernels
stream the axis; nothing is uploaded but the operands, so the call can be recorded into a graph).  f32 when x and y are
both f32, otherwise f64 (integers included), the result in that dtype (the reference works in place on x, so for an
f32 x with an f64 y it returns f32; here that pair is computed and returned in f64).  No NaN policy, as in the
reference: a NaN in a column, a constant column and a sample axis of length 1 give NaN.  Mean, centring, norms, normalisation and the sum of
products are formed in the reference's order, in three passes over the samples (2 * 3 * m values read per point):
  * `axis` is not the last axis with more than one element (inner > 1): one lane per point adds its samples one after
    the other, which is what NumPy does along such an axis: the result equals the reference's bit for bit;
  * the samples of a point are contiguous (inner == 1): one wave per point, lane l adds samples l, l + 64, ..., then a
    fixed butterfly over the lanes.  NumPy adds such rows pairwise, so the bits differ: |got - exact| <= (2 m + 16) eps
    (tests/_regimes_numpy.py).  The same call gives the same bytes every time.
"""
import math

import numpy as np

from . import _ensemble as _e
from .device import DeviceArray, _Allocation, current_stream
from .vertical import _foreign_aware


def crps_weights(n_ens):
    """(p**2, (1 - p)**2) for p = arange(n_ens + 1) / n_ens (ensemble.py:76-77), as the reference computes them."""
    p = np.arange(n_ens + 1) / float(n_ens)
    return p**2, (1 - p) ** 2


def _crps_from_ensemble(x, y, nan_policy, family):
    """What `crps_from_ensemble` (family "ekm_crps_from_ensemble_") and `long_crps_from_ensemble`
    ("ekm_long_crps_from_ensemble_") share: everything but the kernel and its cap."""
    if nan_policy not in ["raise", "propagate", "omit"]:
        raise ValueError("Invalid argument: nan_policy must be 'raise', 'propagate', or 'omit'.")
    x, y = _e.as_input(x), _e.as_input(y)
    if len(x.shape) < 1 or tuple(x.shape[1:]) != tuple(y.shape):
        raise ValueError(f"crps_from_ensemble: x {tuple(x.shape)} must be (n_ens,) + the shape of y {tuple(y.shape)}")
    pts = tuple(int(v) for v in y.shape)
    npts, nens = _e.npoints(pts), int(x.shape[0])
    if nens < 1:
        raise ValueError("crps_from_ensemble: x needs at least one member")
    device_result = _e.on_device(x, y)
    if nan_policy == "raise" and not device_result:
        # the reference's test on the host input, before any GPU work (ensemble.py:44-47)
        if bool(np.any(np.isnan(x))) or bool(np.any(np.isnan(y))):
            raise ValueError(f"Missing values present in input and nan_policy={nan_policy}")
    dtype = _e.arith_dtype(x, y)
    device, stream, keep = _e.device_of(x, y), current_stream(), []
    _, tabs = _e.table("crps", nens, device, lambda: crps_weights(nens))
    d_x = _e.upload(x, dtype, device, stream, keep)
    d_y = _e.upload(y, dtype, device, stream, keep)
    out = DeviceArray.empty(pts, np.float64, device)
    flags = None
    if nan_policy != "propagate":
        flags = _Allocation(max(npts, 16), device)
        flags.touch(stream)
    _e._ffi.check(getattr(_e.lib(), family + _e.tag_of(dtype))(
        device, stream, d_x.ptr, d_y.ptr, nens, npts, tabs[0].on(stream), tabs[1].on(stream), out.on(stream),
        flags.ptr if flags is not None else None))
    if flags is None:
        return _e.finish(out, device_result)
    missing = np.zeros(max(npts, 1), np.uint8)
    lib = _e.lib()
    _e._ffi.check(lib.ekm_d2h(device, missing.ctypes.data, flags.ptr, npts, stream))
    _e._ffi.check(lib.ekm_stream_sync(device, stream))
    flags.free()
    missing = missing[:npts].astype(bool)
    if nan_policy == "raise":
        if missing.any():
            raise ValueError(f"Missing values present in input and nan_policy={nan_policy}")
        return _e.finish(out, device_result)
    res = _e.finish(out, False).reshape(-1)[~missing]
    return DeviceArray.from_host(res, device) if device_result else res


@_foreign_aware("x", "y")
def crps_from_ensemble(x, y, nan_policy="propagate"):
    """Continuous Ranked Probability Score of the ensemble x (n_ens, n_points) against y (n_points), Hersbach (2000)
    (ensemble.py:13-82).  Returns float64 with y's shape ("omit": 1-D, the points without missing values)."""
    return _crps_from_ensemble(x, y, nan_policy, "ekm_crps_from_ensemble_")


@_foreign_aware("x", "y")
def long_crps_from_ensemble(x, y, nan_policy="propagate"):
    """`crps_from_ensemble` for a long member axis: up to 16384 members in f32 and 8192 in f64 (more raises `EkmError`
    naming the cap), sorted by one workgroup per tile of columns (kernel `long_crps_tiles`).  Same arguments, dtypes,
    policies, errors and results; for a member count both functions take, the bits are the same (module docstring: the
    sign of a zero)."""
    return _crps_from_ensemble(x, y, nan_policy, "ekm_long_crps_from_ensemble_")


@_foreign_aware("x", "y")
def pearson_correlation(x, y, axis=0):
    """Pearson correlation coefficient of x and y along `axis` (deterministic.py:13-37).  The shapes must match; the
    result has x's shape with `axis` removed."""
    x, y = _e.as_input(x), _e.as_input(y)
    shape = tuple(int(v) for v in x.shape)
    if shape != tuple(int(v) for v in y.shape):
        raise ValueError(f"pearson_correlation: the shapes of x {shape} and y {tuple(y.shape)} must match")
    if not shape:
        raise np.exceptions.AxisError(axis, 0)
    if not -len(shape) <= axis < len(shape):
        raise np.exceptions.AxisError(axis, len(shape))
    axis = int(axis) % len(shape)
    m, outer, inner = shape[axis], math.prod(shape[:axis]), math.prod(shape[axis + 1:])
    rest = shape[:axis] + shape[axis + 1:]
    dtype = _e.arith_dtype(x, y)
    device_result = _e.on_device(x, y)
    if outer * inner == 0 and not device_result:
        return np.empty(rest, dtype)  # no work: no device is asked for
    if m == 0 and not device_result:  # the reference: every array is empty along the axis and the sum of nothing is 0
        return np.zeros(rest, dtype)[()]
    device, stream, keep = _e.device_of(x, y), current_stream(), []
    if m == 0:
        return DeviceArray.from_host(np.zeros(rest, dtype), device).reshape(rest)
    out = DeviceArray.empty(rest, dtype, device)
    if outer * inner == 0:
        return out
    d_x, d_y = _e.upload(x, dtype, device, stream, keep), _e.upload(y, dtype, device, stream, keep)
    _e._ffi.check(getattr(_e.lib(), "ekm_pearson_" + _e.tag_of(dtype))(
        device, stream, d_x.ptr, d_y.ptr, outer, m, inner, out.on(stream)))
    return out if device_result else _e.finish(out, False)[()]
