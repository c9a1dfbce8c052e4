"""`earthkit.meteo.regimes` on MI355X: projection of fields onto weather-regime patterns and the regime index
(reference regimes/array/index.py, regimes/patterns.py; kernels `project_fields` and `standardise` in csrc/reduce.hip,
arithmetic csrc/reduce_point.hpp).

Same names, argument order and error conventions as the reference.  NumPy in -> NumPy out; `DeviceArray` in ->
`DeviceArray` out (the per-label results are views of one allocation); a device tensor of another ROCm library is taken
over through DLPack and the results go back in that library's type.  Inputs are never modified; there is no CPU fallback.

`project` reads every field ONCE per eight patterns: the host forms the coefficient matrix C[p] = pattern_p * weights_n
(weights normalised with NumPy, `weights / weights.sum()`, as the reference does), uploads it, and one launch gives all
projections.  Three kinds of evaluated patterns are taken:
  * shared: every evaluated pattern has `patterns.shape` (`ConstantPatterns`, any subclass that returns such arrays);
  * `ModulatedPatterns`: C comes from the base patterns and the modulator's value of each field multiplies the finished
    sum.  The reference multiplies every grid point by it instead; the results differ by one more rounding;
  * per field: an evaluated pattern has the field's full shape.  One launch per label with a per-field coefficient block
    (pattern * weights formed on the host: one host pass and one upload of the field's size per label).
Anything else raises `ValueError` naming the shapes.

The arithmetic is f32 only when field, patterns (and modulator values) and weights are all f32, otherwise f64; the result
has that dtype, as in the reference.  An f32 call accumulates in f32: products and sums are fused multiply-adds in a fixed
order (256 lanes stride the grid points, a butterfly over each wave, the four waves in order), so a call gives the same
bytes every time and a field gives the same bits wherever it lies in the batch.  The order is not NumPy's (pairwise
over the flattened pattern axes), so results are not the reference's bit for bit: |got - exact| <= (K + 4) eps sum_k
|f_k p_k w_k| for K grid points, which is the bound of any summation order (tests/_regimes_numpy.py).

The coefficient matrix of a `ConstantPatterns` or `ModulatedPatterns` object is kept on the device per (object, weights,
dtype, device); its first use uploads, which cannot be recorded: call once outside an `ekm_hip.graph()` block before
recording.  Modulator values, per-field patterns and the patterns of other subclasses are uploaded by every call, so
such calls cannot be recorded at all.

`regime_index` is `(projection - mean[label]) / std[label]` per label: one elementwise kernel, the difference and an IEEE
division, bit for bit with the reference.  `mean` and `std` hold Python numbers or arrays of the projection's shape.

Not ported: the xarray layer.  The `xp` argument of the pattern classes is accepted and ignored: pattern arrays are held
as NumPy arrays on the host.
"""
import abc
import math
import numbers
import weakref

import numpy as np

from . import _ensemble as _e
from .device import DeviceArray, current_stream

_coef_cache = weakref.WeakKeyDictionary()


class Patterns(abc.ABC):
    """A labelled set of patterns on a regular grid (patterns.py:17-111).

    labels: one name per pattern, in output order.  grid: {"area": [lat0, lon0, lat1, lon1], "grid": [dlat, dlon]}.
    xp: ignored."""

    def __init__(self, labels, grid, xp=None):
        self._labels = tuple(labels)
        self._grid = grid
        self._xp = xp

    @property
    def labels(self):
        """Labels of the patterns."""
        return self._labels

    @property
    def grid(self):
        """The grid on which the patterns live."""
        return self._grid

    @property
    def shape(self):
        """Shape of a single pattern: the points of the area at the grid's spacing, both ends counted."""
        north, west, south, east = self.grid["area"]
        dlat, dlon = self.grid["grid"]
        return (int(abs(north - south) / dlat) + 1, int(abs(west - east) / dlon) + 1)

    @property
    def size(self):
        """Number of grid points in a single pattern."""
        return math.prod(self.shape)

    @property
    def ndim(self):
        """Number of axes of a single pattern."""
        return len(self.shape)

    @property
    def xp(self):
        return self._xp

    @abc.abstractmethod
    def patterns(self, **patterns_extra_coords):
        """Mapping label -> pattern, evaluated for the given coordinates (if any)."""

    def __repr__(self):
        return f"{type(self).__name__}{self.labels}"


def _stacked(patterns, owner):
    stack = np.asarray(patterns)
    if stack.ndim != 1 + len(owner.shape):
        raise ValueError("must have exactly one label axis in the patterns")
    if len(owner.labels) != stack.shape[0]:
        raise ValueError("number of labels does not match number of patterns")
    return stack


class ConstantPatterns(Patterns):
    """Fixed patterns, one per label, stacked along the first axis of `patterns` (patterns.py:140-174)."""

    def __init__(self, labels, grid, patterns, xp=None):
        super().__init__(labels, grid, xp)
        self._patterns = _stacked(patterns, self)

    def patterns(self):
        return dict(zip(self._labels, self._patterns))


class ModulatedPatterns(Patterns):
    """Base patterns scaled by a scalar function of extra coordinates, e.g. of the date (patterns.py:177-230).

    modulator: called with the keyword arguments that `project` receives as `patterns_extra_coords`; returns one
    factor per field."""

    def __init__(self, labels, grid, base_patterns, modulator, xp=None):
        super().__init__(labels, grid, xp)
        self._base_patterns = _stacked(base_patterns, self)
        if not callable(modulator):
            raise ValueError("modulator must be callable")
        self._modulator = modulator

    def modulation(self, **patterns_extra_coords):
        """The modulator's values for the given coordinates, as a NumPy array."""
        return np.asarray(self._modulator(**patterns_extra_coords))

    def patterns(self, **patterns_extra_coords):
        factor = self.modulation(**patterns_extra_coords)
        factor = factor.reshape(factor.shape + (1,) * self.ndim)
        return {label: factor * base for label, base in zip(self._labels, self._base_patterns)}


def _host(a):
    return a.to_host() if isinstance(a, DeviceArray) else np.asarray(a)


def _adopt(arrays):
    from . import _engine

    return _engine._adopt_foreign(list(arrays))


def _hand_back_dict(res, foreign):
    if foreign is None:
        return res
    from . import _engine

    return dict(zip(res, _engine._hand_back(tuple(res.values()), foreign)))


def _coefficients(patterns, stack, wn, dtype, device, cached):
    """The (P, K) matrix pattern_p * weights_n in `dtype` on the device; kept per Patterns object when `cached`."""
    key = (wn.dtype.str, wn.tobytes(), dtype.str, int(device))
    per_object = _coef_cache.setdefault(patterns, {}) if cached else {}
    if key not in per_object:
        coef = stack.astype(dtype, copy=False).reshape(stack.shape[0], -1) * wn.astype(dtype, copy=False).reshape(-1)
        per_object[key] = DeviceArray.from_host(np.ascontiguousarray(coef), device)
    return per_object[key]


def project(field, patterns, weights, **patterns_extra_coords):
    """Project onto the given regime patterns (index.py:10-56).

    field: the field(s); the patterns are projected onto its trailing axes.  weights: summation weights of the
    patterns' shape, normalised to a sum of 1 before use.  patterns_extra_coords: keyword arguments of the pattern
    generation (the dates of date-modulated patterns), of the field's shape without the pattern axes.

    Returns {label: array of shape field.shape[:-patterns.ndim]}."""
    (field,), foreign = _adopt([field])
    (weights,), _ = _adopt([weights])
    field = _e.as_input(field)
    pshape = tuple(patterns.shape)
    nd = len(pshape)
    fshape = tuple(int(v) for v in field.shape)
    if fshape[-nd:] != pshape:
        raise ValueError(f"shape of input fields {fshape} incompatible with shape of patterns {pshape}")
    if weights is None:
        raise NotImplementedError("automatic generation of weights")
    weights = _host(weights)
    if tuple(weights.shape) != pshape:
        raise ValueError(f"shape of weights {tuple(weights.shape)} must match shape of patterns {pshape}")
    with np.errstate(all="ignore"):
        wn = np.ascontiguousarray(weights / weights.sum())
    nshape = fshape[:-nd]
    nfields, k = math.prod(nshape), math.prod(pshape)

    scale = None
    known = type(patterns) in (ConstantPatterns, ModulatedPatterns)
    if isinstance(patterns, ModulatedPatterns) and type(patterns).patterns is ModulatedPatterns.patterns:
        labels, shared = patterns.labels, patterns._base_patterns
        scale = patterns.modulation(**patterns_extra_coords)
        try:
            fits = np.broadcast_shapes(scale.shape, nshape) == nshape
        except ValueError:
            fits = False
        if not fits:
            raise ValueError(f"modulator values of shape {scale.shape} do not fit the fields {nshape} of the input {fshape}")
        dtype = _e.arith_dtype(field, shared, wn, scale)
    else:
        evaluated = {label: np.asarray(p) for label, p in patterns.patterns(**patterns_extra_coords).items()}
        labels = tuple(evaluated)
        for label, p in evaluated.items():
            if p.shape != pshape and p.shape != fshape:
                raise ValueError(f"pattern {label!r} evaluates to shape {p.shape}: neither the shape of a pattern {pshape} nor "
                                 f"that of the input fields {fshape}")
        dtype = _e.arith_dtype(field, wn, *evaluated.values())
        shared = None
        if all(p.shape == pshape for p in evaluated.values()):
            shared = patterns._patterns if type(patterns) is ConstantPatterns else np.stack(list(evaluated.values())) if evaluated else np.empty((0,) + pshape)
    npat = len(labels)
    device_result = _e.on_device(field)
    if (nfields == 0 or npat == 0) and not device_result:
        return {label: np.empty(nshape, dtype) for label in labels}  # no work: no device is asked for
    device, stream, keep = _e.device_of(field), current_stream(), []
    out = DeviceArray.empty((max(npat, 1), max(nfields, 1)), dtype, device)
    if nfields and npat:
        entry = getattr(_e.lib(), "ekm_regimes_project_" + _e.tag_of(dtype))
        d_field = _e.upload(field, dtype, device, stream, keep)
        if shared is not None:
            d_coef = _coefficients(patterns, shared, wn, dtype, device, known)
            d_scale = None
            if scale is not None:
                d_scale = _e.upload(np.ascontiguousarray(np.broadcast_to(scale, nshape), dtype=dtype).reshape(-1), dtype, device, stream, keep)
            _e._ffi.check(entry(device, stream, d_field.ptr, nfields, k, d_coef.on(stream), npat, 0,
                                d_scale.ptr if d_scale is not None else None, out.on(stream)))
        else:
            w = wn.astype(dtype, copy=False)
            for row, p in enumerate(evaluated.values()):
                per_field = p.shape == fshape
                coef = np.ascontiguousarray(p.astype(dtype, copy=False) * w)
                d_coef = _e.upload(coef.reshape(-1), dtype, device, stream, keep)
                _e._ffi.check(entry(device, stream, d_field.ptr, nfields, k, d_coef.ptr, 1, k if per_field else 0, None,
                                    out.on(stream) + row * nfields * dtype.itemsize))
    if device_result:
        res = {label: out.flat_slice(row * nfields, (row + 1) * nfields).reshape(nshape) for row, label in enumerate(labels)}
        return _hand_back_dict(res, foreign)
    host = _e.finish(out, False)
    return {label: host[row, :nfields].reshape(nshape)[()] for row, label in enumerate(labels)}


def _operand(value, shape, what):
    """A `mean` or `std` entry: (array or None, number or None, the dtype it brings into the promotion or None)."""
    if isinstance(value, numbers.Real) and not isinstance(value, np.generic):
        return None, float(value), None  # a Python number takes the projection's dtype
    if isinstance(value, DeviceArray):
        if tuple(value.shape) != shape:
            raise ValueError(f"regime_index: {what} of shape {tuple(value.shape)} must have the projection's shape {shape}")
        return value, None, value.dtype
    a = np.asarray(value)
    if a.ndim == 0:
        return None, a, a.dtype
    try:
        fits = np.broadcast_shapes(a.shape, shape) == shape
    except ValueError:
        fits = False
    if not fits:
        raise ValueError(f"regime_index: {what} of shape {a.shape} must have the projection's shape {shape}")
    return np.broadcast_to(a, shape), None, a.dtype


class _Dt:
    def __init__(self, dtype):
        self.dtype = dtype


def regime_index(projections, mean, std):
    """Regime index by standardisation of projections onto patterns (index.py:59-76):
    {label: (projection - mean[label]) / std[label]}."""
    labels = list(projections)
    adopted, foreign = _adopt([projections[label] for label in labels])
    res = {}
    for label, proj in zip(labels, adopted):
        proj = _e.as_input(proj)
        shape = tuple(int(v) for v in proj.shape)
        (m_arr, m_val, m_dt), (s_arr, s_val, s_dt) = _operand(mean[label], shape, "mean"), _operand(std[label], shape, "std")
        dtype = _e.arith_dtype(proj, *(_Dt(d) for d in (m_dt, s_dt) if d is not None))
        device_result = _e.on_device(proj)
        n = math.prod(shape)
        if n == 0 and not device_result:
            res[label] = np.empty(shape, dtype)  # no work: no device is asked for
            continue
        device, stream, keep = _e.device_of(proj, m_arr, s_arr), current_stream(), []
        out = DeviceArray.empty(shape, dtype, device)
        if n:
            real = dtype.type
            d_proj = _e.upload(proj, dtype, device, stream, keep)
            d_mean = _e.upload(m_arr, dtype, device, stream, keep) if m_arr is not None else None
            d_std = _e.upload(s_arr, dtype, device, stream, keep) if s_arr is not None else None
            _e._ffi.check(getattr(_e.lib(), "ekm_regimes_index_" + _e.tag_of(dtype))(
                device, stream, d_proj.ptr, d_mean.ptr if d_mean is not None else None, real(0 if m_val is None else m_val),
                d_std.ptr if d_std is not None else None, real(0 if s_val is None else s_val), out.on(stream), n))
        res[label] = out if device_result else _e.finish(out, False)[()]
    return _hand_back_dict(res, foreign)
