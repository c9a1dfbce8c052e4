"""`earthkit.meteo.extreme` on MI355X: Extreme Forecast Index, Shift of Tails and Crossing Point Forecast of an
ensemble against a model climate (reference extreme/array/efi.py, extreme/array/sot.py, extreme/array/cpf.py; kernels
csrc/ensemble.hip).

Same names, argument order, defaults and error conventions as the reference.  NumPy in -> NumPy out; `DeviceArray` in
-> `DeviceArray` out; device tensors of another ROCm library are taken over through DLPack and handed back in that
library's type.  Fields are member-major: `clim` [nclim, npoints], `ens` [nens, npoints]; at most 256 members in f32 and
128 in f64 (more raises `EkmError`).  `cpf` has its own limit: the members, plus the climate rows when `sort_clim`, may
number 640 in f32 and 320 in f64.

The arithmetic runs in f32 when every array argument is f32 and in f64 otherwise (f64, mixed, integer).  In f32 and in
f64 the results equal the reference's bit for bit.  Deviation: with mixed dtypes the reference's `efi` forms `frac` in
`clim`'s dtype (so in f32 when only `clim` is f32) while this computes in f64; the two differ by the rounding of `frac`
and `dFdp` to f32 (about 1e-8 absolute on the index, see tests/_ensemble_numpy.py::mixed_efi_bound).

`cpf` (marked experimental in the reference) returns float32 for every input dtype, as the reference does, and keeps
the reference's oddities: a column with a NaN does not give NaN (numpy.sort puts the NaN last and the scan compares as
usual), the lower-tail interpolation overwrites a crossing that is already written, the upper-tail one may be
overwritten by a later row.  Deviation: with mixed dtypes `cpf` computes in f64 on the upcast columns, while the
reference lets NumPy promote operation by operation, so with `clim` f32 and `ens` f64 it forms the differences of two
climate rows in f32 (the denominator of both interpolations).  Only interpolated values can differ, by at most
3 * 2^-24 relative (derived in tests/_cpf_numpy.py::mixed_cpf_bound; on the recorded mixed cases no point differs);
levels written by a plain crossing are equal.  With `clim` f64 and `ens` f32 the reference's arithmetic is f64 as here,
except that it compares `epsilon` rounded to f32.

`sot_unsorted` (raises on every call in the reference) is not provided.

`long_efi` / `long_sot` (kernels `long_efi_tiles`, `long_sot_tiles` in csrc/long_ensemble.hip) are `efi` / `sot` for LONG
member axes: up to 16384 members in f32 and 8192 in f64 (one column, padded to a power of two, in 64 KiB of LDS; more
raises `EkmError` naming the cap).  Everything above holds for them -- arguments, dtype rules, the mixed-dtype deviation,
errors, input and output types, the graph rule; each pair shares one host body and one set of coefficient tables.  One
workgroup sorts a tile of whole columns with the bitonic network of `stats.long_quantiles`, then one lane per column runs
the arithmetic of `efi` / `sot` over the sorted column (efi streams its climate rows from global memory, once each).  The
keys of that sort order -0.0 before +0.0, which NumPy's sort leaves open (and the insertion sort of `efi` / `sot` keeps as
the input has them): in a column that holds both zeros a result may differ from the reference, and from the short
function, in the sign of a zero -- the one place where the results are not the reference's bits.  Short axes are accepted
and give the bits of `efi` / `sot`.
`long_cpf` (kernel `long_cpf_tiles`, same file) is `cpf` for long columns: up to 16384 members AND up to 16384 climate rows
in f32, 8192 each in f64, checked separately and whether or not they are sorted (`EkmError` naming the axis and the cap),
so a raw model-climate sample (the 1980 values `stats.long_quantiles` was built for) is a legitimate `clim`.  Everything
said of `cpf` holds -- arguments, dtype rules, the mixed-dtype deviation, the float32 result, errors, input and output
types, the graph rule; the two share one host body.  One workgroup holds a tile of ensemble columns and a tile of climate
columns, sorts each where its flag asks for it (a NaN last, as numpy.sort puts it) or loads it as given, then one lane per
point scans them in O(nclim + nens) with a running maximum in place of `cpf`'s O(nclim * nens) priming loop: the same
writes at the same members, so the bits of `cpf` and of the reference.  The zero-sign exception stated for `long_efi`
applies to a SORTED column that holds both zeros (the key sort orders -0.0 before +0.0): an interpolated value may then
differ in the sign of a zero.
Which to call: `efi` / `sot` are the reference's names and stay as they are (their cap is an error, not a fallback); for
speed the long forms are the faster at every member count measured, from 32 up, because the per-lane insertion sort is
O(nens^2): on one MI355X at 2^20 points and 101 climate rows (profiles/long_ensemble_bench.json, `crossover`), f32 long /
short efi = 0.54 / 0.66 ms at 32 members, 0.96 / 1.53 at 51, 1.02 / 2.55 at 64, 2.2 / 15.6 at 128 and 5.1 / 108 at 256;
sot 0.12 / 0.28 at 32, 0.28 / 0.95 at 51, 0.72 / 13.7 at 128 and 1.75 / 103 at 256; f64 efi 0.94 / 1.21 at 32, 1.81 / 2.72
at 51 and 4.3 / 30.7 at 128, sot 0.54 / 1.65 at 51 and 1.42 / 26.7 at 128.  Beyond the short cap, at 2^16 points: f32 efi
1.0 ms at 512 members and 5.6 ms at 1980, sot 0.31 and 1.6 ms (the NumPy restatement on the host: 1.3 s and 4.7 s for efi).
`cpf` or `long_cpf`: `cpf` is the reference's name and stays as it is.  For speed, at 2^20 points and 101 sorted climate
rows (profiles/long_cpf_bench.json, `crossover`; long / short ms) the long form wins from 51 members up under every
option set -- f32 default 2.42 / 4.00 at 51, 2.50 / 10.8 at 64, 2.75 / 34.2 at 128, 6.19 / 248 at 256; f64 4.71 / 7.93 at
51, 5.35 / 68.6 at 128 -- ties at 32 (f32 2.32 / 2.32) and LOSES at 32 members with `sort_clim=False` (f32 1.81 / 1.36, f64
3.30 / 1.38; at 51 it wins again, 1.90 / 2.26): the short kernel then streams the climate with every lane busy, while the
long one runs its scan on the 32 (f64 16) lanes of 256 that have a column.  Beyond `cpf`'s cap, at 2^16 points with an
unsorted climate sample: f32 6.7 ms at 101 x 1980, 21.8 at 1980 x 51, 26.5 at 1980 x 1980 (f64 13.5, 42.3, 52.9).
"""
import numpy as np

from . import _ensemble as _e
from .device import DeviceArray, current_stream
from .vertical import _foreign_aware

_F32 = np.dtype(np.float32)


def efi_coefficients(nclim):
    """(acosdiff, proddiff, acoef) of efi.py:54-60, computed with NumPy as the reference computes them: the kernel takes
    them as tables and evaluates no acos."""
    p = np.linspace(0.0, 1.0, nclim)
    acosdiff = np.diff(np.acos(np.sqrt(p)))
    proddiff = np.diff(np.sqrt(p * (1.0 - p)))
    acoef = (1.0 - 2.0 * p[:-1]) * acosdiff + proddiff
    return acosdiff, proddiff, acoef


def _efi(clim, ens, eps, family):
    """What `efi` (family "ekm_efi_") and `long_efi` ("ekm_long_efi_") share: everything but the kernel and its cap."""
    clim, ens = _e.as_input(clim), _e.as_input(ens)
    if len(clim.shape) != 2 or len(ens.shape) != 2:
        raise ValueError(f"efi: clim and ens must be 2-D (nclim, npoints) and (nens, npoints), got {tuple(clim.shape)} and {tuple(ens.shape)}")
    nclim, npts = (int(v) for v in clim.shape)
    nens, npts_ens = (int(v) for v in ens.shape)
    assert npts == npts_ens  # efi.py:45
    eps = float(eps)
    dtype = _e.arith_dtype(clim, ens)
    device, stream, keep = _e.device_of(clim, ens), current_stream(), []
    if nens < 1 or nclim < 1:
        raise ValueError("efi: clim and ens need at least one row each")
    _, tabs = _e.table("efi", nclim, device, lambda: efi_coefficients(nclim))
    d_clim = _e.upload(clim, dtype, device, stream, keep)
    d_ens = _e.upload(ens, dtype, device, stream, keep)
    out = DeviceArray.empty((npts,), np.float64, device)
    _e._ffi.check(getattr(_e.lib(), family + _e.tag_of(dtype))(
        device, stream, d_clim.ptr, d_ens.ptr, nclim, nens, npts, eps, tabs[0].on(stream), tabs[1].on(stream),
        tabs[2].on(stream), out.on(stream)))
    return _e.finish(out, _e.on_device(clim, ens))


@_foreign_aware("clim", "ens")
def efi(clim, ens, eps=-0.1):
    """Extreme Forecast Index (efi.py:16-89).  clim: (nclim, npoints) per-point climatology, sorted or not; ens:
    (nens, npoints).  Returns float64 (npoints) for f32 and f64 input, NaN where a column of clim or ens holds a NaN."""
    return _efi(clim, ens, eps, "ekm_efi_")


@_foreign_aware("clim", "ens")
def long_efi(clim, ens, eps=-0.1):
    """`efi` for a long member axis: up to 16384 members in f32 and 8192 in f64 (more raises `EkmError` naming the cap),
    sorted by one workgroup per tile of columns (kernel `long_efi_tiles`).  Same arguments, dtypes, errors and results;
    for a member count both functions take, the bits are the same (module docstring: the sign of a zero)."""
    return _efi(clim, ens, eps, "ekm_long_efi_")


def _cpf(clim, ens, sort_clim, sort_ens, epsilon, symmetric, from_zero, family):
    """What `cpf` (family "ekm_cpf_") and `long_cpf` ("ekm_long_cpf_") share: everything but the kernel and its caps."""
    clim, ens = _e.as_input(clim), _e.as_input(ens)
    if len(clim.shape) != 2 or len(ens.shape) != 2:
        raise ValueError(f"cpf: clim and ens must be 2-D (nclim, npoints) and (nens, npoints), got {tuple(clim.shape)} and {tuple(ens.shape)}")
    nclim, npts = (int(v) for v in clim.shape)
    nens, npts_ens = (int(v) for v in ens.shape)
    assert npts == npts_ens  # cpf.py:138
    if nens < 1 or nclim < 1:
        raise ValueError("cpf: clim and ens need at least one row each")
    use_epsilon = epsilon is not None and not symmetric  # cpf.py:145-146
    dtype = _e.arith_dtype(clim, ens)
    device, stream, keep = _e.device_of(clim, ens), current_stream(), []
    d_clim = _e.upload(clim, dtype, device, stream, keep)
    d_ens = _e.upload(ens, dtype, device, stream, keep)
    out = DeviceArray.empty((npts,), _F32, device)
    _e._ffi.check(getattr(_e.lib(), family + _e.tag_of(dtype))(
        device, stream, d_clim.ptr, d_ens.ptr, nclim, nens, npts, int(bool(sort_clim)), int(bool(sort_ens)),
        int(bool(from_zero)), int(bool(symmetric)), int(use_epsilon), float(epsilon) if use_epsilon else 0.0,
        out.on(stream)))
    return _e.finish(out, _e.on_device(clim, ens))


@_foreign_aware("clim", "ens")
def cpf(clim, ens, sort_clim=True, sort_ens=True, epsilon=None, symmetric=False, from_zero=False):
    """Crossing Point Forecast (cpf.py:94-155).  clim: (nclim, npoints) per-point climatology; ens: (nens, npoints).
    sort_clim / sort_ens: sort the columns first (a NaN goes last, as numpy.sort puts it), else they are used as given.
    epsilon: points whose last member is below it give 0; ignored when `symmetric`.  symmetric: values below 0.5 become
    1 - (the CPF of the negated fields).  from_zero: look for the crossing from the lowest member, not from the median.
    Returns float32 (npoints); one kernel launch per call.  The inputs are never written."""
    return _cpf(clim, ens, sort_clim, sort_ens, epsilon, symmetric, from_zero, "ekm_cpf_")


@_foreign_aware("clim", "ens")
def long_cpf(clim, ens, sort_clim=True, sort_ens=True, epsilon=None, symmetric=False, from_zero=False):
    """`cpf` for long columns: up to 16384 members AND up to 16384 climate rows in f32, 8192 each in f64, whether they
    are sorted or not (one more of either raises `EkmError` naming the axis and the cap) -- a raw model-climate sample
    is a legitimate `clim`.  One workgroup sorts a tile of ensemble columns and a tile of climate columns (kernel
    `long_cpf_tiles`), then one lane per point scans them in O(nclim + nens).  Same arguments, dtypes, errors and
    results; for columns both functions take, the bits are the same (module docstring: the sign of a zero)."""
    return _cpf(clim, ens, sort_clim, sort_ens, epsilon, symmetric, from_zero, "ekm_long_cpf_")


def _points_shape(a, b, what):
    if len(a.shape) < 1 or len(b.shape) < 1 or tuple(a.shape[1:]) != tuple(b.shape[1:]):
        raise ValueError(f"{what}: the point dimensions differ: {tuple(a.shape)} against {tuple(b.shape)}")
    return tuple(int(v) for v in a.shape[1:])


def _sot(clim, ens, perc, eps, family):
    """What `sot` (family "ekm_sot_") and `long_sot` ("ekm_long_sot_") share: everything but the kernel and its cap."""
    clim, ens = _e.as_input(clim), _e.as_input(ens)
    if not (isinstance(perc, int) or isinstance(perc, np.int64)) or (perc < 2 or perc > 98):
        raise Exception("Percentile value should be and Integer between 2 and 98, is {}".format(perc))
    if clim.shape[0] != 101:
        raise Exception("Climatology array should contain 101 percentiles, it has {} values".format(tuple(clim.shape)))
    if perc == 50:
        raise Exception("Percentile value to be computed cannot be 50 for sot, has to be in the upper or lower half")
    pts = _points_shape(clim, ens, "sot")
    npts, nens, perc, eps = _e.npoints(pts), int(ens.shape[0]), int(perc), float(eps)
    if nens < 1:
        raise ValueError("sot: ens needs at least one member")
    tail = 99 if perc > 50 else 1
    dtype = _e.arith_dtype(clim, ens)
    device, stream, keep = _e.device_of(clim, ens), current_stream(), []
    if isinstance(clim, DeviceArray):
        d_clim = _e.upload(clim, dtype, device, stream, keep)
        row = npts * dtype.itemsize
        p_qc, p_tail = d_clim.ptr + perc * row, d_clim.ptr + tail * row
    else:  # only the two rows the result depends on travel
        d_rows = _e.upload(np.stack([clim[perc].reshape(-1), clim[tail].reshape(-1)]), dtype, device, stream, keep)
        p_qc, p_tail = d_rows.ptr, d_rows.ptr + npts * dtype.itemsize
    d_ens = _e.upload(ens, dtype, device, stream, keep)
    out = DeviceArray.empty(pts, dtype, device)
    _e._ffi.check(getattr(_e.lib(), family + _e.tag_of(dtype))(
        device, stream, p_qc, p_tail, d_ens.ptr, nens, npts, perc, eps, out.on(stream)))
    return _e.finish(out, _e.on_device(clim, ens))


@_foreign_aware("clim", "ens")
def sot(clim, ens, perc, eps=-1e4):
    """Shift of Tails (sot.py:51-103) from the 101 climate percentiles `clim` (101, ...) and the unsorted ensemble `ens`
    (nens, ...); trailing dimensions are flattened to points.  `perc`: an int in [2, 98], not 50.  The result has the
    points' shape, in the arithmetic dtype."""
    return _sot(clim, ens, perc, eps, "ekm_sot_")


@_foreign_aware("clim", "ens")
def long_sot(clim, ens, perc, eps=-1e4):
    """`sot` for a long member axis: up to 16384 members in f32 and 8192 in f64 (more raises `EkmError` naming the cap),
    sorted by one workgroup per tile of columns (kernel `long_sot_tiles`).  Same arguments, dtypes, errors and results;
    for a member count both functions take, the bits are the same (module docstring: the sign of a zero)."""
    return _sot(clim, ens, perc, eps, "ekm_long_sot_")


@_foreign_aware("qc_tail", "qc", "qf")
def sot_func(qc_tail, qc, qf, eps=-1e-4, lower_bound=-10, upper_bound=10):
    """Shift of Tails from percentiles that are computed already (sot.py:13-48): NaN where |qc_tail - qc| does not
    exceed max(eps, 0), clamped to [lower_bound, upper_bound].  NumPy arguments broadcast; DeviceArrays must agree in
    shape."""
    args = [_e.as_input(x) for x in (qc_tail, qc, qf)]
    device_result = _e.on_device(*args)
    if device_result:
        shape = tuple(next(a.shape for a in args if isinstance(a, DeviceArray)))
        if any(tuple(a.shape) != shape for a in args):
            raise ValueError(f"sot_func: DeviceArray arguments must have one shape, got {[tuple(a.shape) for a in args]}")
    else:
        args = list(np.broadcast_arrays(*args))
        shape = args[0].shape
    dtype = _e.arith_dtype(*args)
    device, stream, keep = _e.device_of(*args), current_stream(), []
    d = [_e.upload(a, dtype, device, stream, keep) for a in args]
    out = DeviceArray.empty(shape, dtype, device)
    _e._ffi.check(getattr(_e.lib(), f"ekm_sot_func_{_e.tag_of(dtype)}")(
        device, stream, d[0].ptr, d[1].ptr, d[2].ptr, _e.npoints(shape), float(eps), float(lower_bound),
        float(upper_bound), out.on(stream)))
    return _e.finish(out, device_result)
