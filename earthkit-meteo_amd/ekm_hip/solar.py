"""`earthkit.meteo.solar` on MI355X: cosine of the solar zenith angle, its average over a time interval and the
top-of-atmosphere incident solar radiation at every grid point (reference solar/array/solar.py; kernel `solar_points` in
csrc/solar.hip, per-point arithmetic csrc/solar_point.hpp).

Same names, argument order, keyword-only arguments, defaults and errors as the reference.  NumPy in -> NumPy out;
`DeviceArray` in -> `DeviceArray` out; device tensors of another ROCm library are taken over through DLPack and handed
back in that library's type.  `julian_day`, `solar_declination_angle` and `incoming_solar_radiation` are host scalars,
computed with NumPy exactly as the reference computes them.

The three array functions are ONE launch each.  They are the same sum over time nodes -- the instantaneous function has
one node, the integrated ones the Gauss-Legendre nodes of every sub-interval -- and everything that depends on the date
is made on the host, operation for operation as the reference makes it (`node_records`): `linspace` time steps, weights,
`begin_date + timedelta(hours=float(t))`, declination and time correction from that date's `julian_day`, and the hour
angle from the date's INTEGER hour (a step function within the hour, as in the reference).  The kernel reads latitude
and longitude once, takes one sine / cosine pair of each and keeps the accumulator in a register through all nodes.
Each operand may be a full field, a scalar, or a vector along the leading or the trailing axes of the result
(`lat[:, None]`, `lon[None, :]`): those are indexed by the kernel, any other broadcast pattern is expanded first.

Result types, as recorded from the reference (tests/golden/solar_golden.npz):
  cos_solar_zenith_angle             float64 for f32 and f64 (and integer) input, shape = broadcast(lat, lon); Python
                                     scalars give a NumPy float64 scalar;
  cos_solar_zenith_angle_integrated,
  toa_incident_solar_radiation       dtype and shape of `latitudes`; `longitudes` must broadcast TO that shape
                                     (ValueError), integer latitudes raise TypeError (the reference: NumPy's
                                     UFuncTypeError, a subclass), dtypes other than f32 / f64 raise TypeError.
`integration_order` outside 1-4 raises ValueError; `intervals_per_hour <= 0`, `end_date <= begin_date` and an interval
that rounds to no sub-interval raise AssertionError.

Arithmetic and deviations.  All arithmetic is float64 on the (upcast) inputs and the result is rounded once.  For f64
input the result is within 1e-13 absolute of the reference's cosine (tests/test_gpu_solar.py derives the bound from the
operation count; times max(isr) for the radiation).  For f32 input the reference takes sin / cos of the latitude in f32,
adds the hour angle to the longitude in f32 and, in the integrated functions, rounds its f32 accumulator after every
node; this computes in double and rounds once, so it is closer to the reference's own f64 run on the upcast inputs than
the reference's f32 run is (the two differ by 1.0e-7 instantaneous and 1.7e-7 over 24 h at order 3, measured on 1 M
random points).  The sign of a zero result is not specified.  Degrees are reduced modulo 360 exactly before the
conversion to radians, so at |longitude| of many turns this is more accurate than the reference, whose `deg2rad`
rounds the unreduced angle.

The node records (five float64 per node, at most a few KiB) are uploaded on the current stream at the first call with a
given set of dates and kept in a small least-recently-used cache per device (16 entries).  Inside an
`ekm_hip.graph()` block nothing can be uploaded: make the same call once before the block, so that its records are
cached; the recorded graph then keeps them alive, and the dates are constants of the graph.
"""
import collections as _collections
import ctypes as _C
import datetime
import math
import sys as _sys
import threading as _threading

import numpy as np

from . import _engine, _ffi
from .device import DeviceArray, _no_capture, current_device, current_stream
from .vertical import _foreign_aware, _to_device

DAYS_PER_YEAR = 365.25
_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)


# ---- host scalars ----
# The reference's formulas (solar.py:18-48, 225-229) are truncated Fourier series in the year angle.  They are stated here
# as coefficient tables and evaluated term by term in the reference's order of operations, so the values are its values
# bit for bit (tests/test_solar_cpu.py compares them with recorded ones).
_DECLINATION = (0.396372, ((1, -22.91327, 4.025430), (2, -0.387205, 0.051967), (3, -0.154527, 0.084798)))  # degrees
_TIME_CORRECTION = (0.004297, ((1, 0.107029, -1.837877), (2, -0.837378, -2.340475)))                      # h.degrees
_RADIATION_MEAN, _RADIATION_AMPLITUDE = 4892416.0, 165120.0


def julian_day(date):
    """Days since 1 January 00:00 of `date`'s year, in `date`'s own time zone if it has one, with the time of day as a
    fraction of whole seconds."""
    new_year = date.replace(month=1, day=1, hour=0, minute=0, second=0, microsecond=0, fold=0)
    since = date - new_year
    return since.days + since.seconds / 86400.0


def _year_angle(date):
    return julian_day(date) / DAYS_PER_YEAR * np.pi * 2


def _series(angle, constant, harmonics):
    """constant + sum over (k, c, s) of c cos(k angle) + s sin(k angle), added left to right."""
    total = constant
    for k, c, s in harmonics:
        phase = angle if k == 1 else k * angle
        total = total + c * np.cos(phase)
        total = total + s * np.sin(phase)
    return float(total)


def solar_declination_angle(date):
    """(declination [degrees], time correction [h.degrees]) of `date`, as Python floats."""
    angle = _year_angle(date)
    return _series(angle, *_DECLINATION), _series(angle, *_TIME_CORRECTION)


def incoming_solar_radiation(date):
    """Solar radiation arriving at the top of the atmosphere on `date`: an annual cosine about its mean."""
    return np.cos(_year_angle(date)) * _RADIATION_AMPLITUDE + _RADIATION_MEAN


# ---- time nodes ----
def _quadrature_rule(order):
    """(abscissae, weights) on [-1, 1] for 1 to 4 nodes per sub-interval, with the values the reference uses
    (solar.py:113-145): its three-node rule has the abscissa sqrt(5/9), not Gauss-Legendre's sqrt(3/5), and that is kept."""
    if order == 1:
        return np.array([0.0]), np.array([2.0])
    if order == 2:
        root3 = np.sqrt(np.float64(3.0))
        return np.array([-1.0 / root3, 1.0 / root3]), np.array([1.0, 1.0])
    if order == 3:
        x = np.sqrt(np.float64(5.0 / 9.0))
        return np.array([-x, 0.0, x]), np.array([5.0 / 9.0, 8.0 / 9.0, 5.0 / 9.0])
    if order == 4:
        spread, root30 = 2.0 / 7.0 * np.sqrt(np.float64(6.0 / 5.0)), np.sqrt(np.float64(30))
        outer, inner = np.sqrt(3.0 / 7.0 + spread), np.sqrt(3.0 / 7.0 - spread)
        light, heavy = (18 - root30) / 36, (18 + root30) / 36
        return np.array([-outer, -inner, inner, outer]), np.array([light, heavy, heavy, light])
    raise ValueError(f"integration_order must be 1, 2, 3 or 4, not {order!r}")


def node_dates(begin_date, end_date, intervals_per_hour=1, integration_order=3):
    """(dates, weights) of the quadrature over [begin_date, end_date]: one datetime and one float64 weight per node,
    sub-interval by sub-interval; the weights sum to 1 up to rounding.  All sub-intervals are formed at once, with
    the reference's operations element by element (solar.py:147-177): half-widths from the `linspace` edges, weights
    half * W / hours, offsets half * E + midpoint, each offset added to `begin_date` as a `timedelta` of float hours."""
    abscissae, rule_weights = _quadrature_rule(integration_order)
    assert intervals_per_hour > 0
    assert end_date > begin_date
    hours = (end_date - begin_date).total_seconds() / 3600.0
    pieces = int(hours * intervals_per_hour + 0.5)
    assert pieces > 0
    edges = np.linspace(0, hours, num=pieces + 1)
    lower, upper = edges[:-1, None], edges[1:, None]
    half = (upper - lower) / 2.0
    weights = (half * rule_weights[None, :] / hours).ravel()
    offsets = (half * abscissae[None, :] + (upper + lower) / 2.0).ravel()
    return [begin_date + datetime.timedelta(hours=float(t)) for t in offsets], weights


def node_records(dates, weights=None, radiation=False):
    """The per-node float64 vectors the sum is made of, as a dict: `sd`, `cd` (sine and cosine of the node date's
    declination), `h15` ((hour - 12) * 15 of the node date: its integer hour only), `tc` (its time correction), `w`
    (1 when `weights` is None) and `isr` (`incoming_solar_radiation` of the node date when `radiation`, else 1)."""
    n = len(dates)
    rec = {k: np.empty(n, np.float64) for k in ("sd", "cd", "h15", "tc", "w", "isr")}
    for k, date in enumerate(dates):
        declination, time_correction = solar_declination_angle(date)
        declination = np.deg2rad(np.asarray(declination))
        rec["sd"][k], rec["cd"][k] = np.sin(declination), np.cos(declination)
        rec["h15"][k] = (date.hour - 12) * 15
        rec["tc"][k] = time_correction
        rec["isr"][k] = incoming_solar_radiation(date) if radiation else 1.0
    rec["w"][:] = 1.0 if weights is None else weights
    return rec


def kernel_records(rec):
    """[nnodes, 5] float64 for ekm_solar_*: (p, q, r, w, isr) with p = sd, q = cd cos(a), r = -cd sin(a) and
    a = h15 + tc, the node's angle, which the kernel applies to the longitude by angle addition."""
    a = np.deg2rad(np.fmod(rec["h15"] + rec["tc"], 360.0))
    return np.ascontiguousarray(np.stack([rec["sd"], rec["cd"] * np.cos(a), -(rec["cd"] * np.sin(a)), rec["w"], rec["isr"]], axis=1))


_records = _collections.OrderedDict()  # (device, bytes of the records) -> (host array, DeviceArray)
_records_lock = _threading.Lock()      # lookup, eviction, upload and insert of one call are one step for other threads
_RECORDS_MAX = 16


def _records_on_device(host, device, stream):
    key = (int(device), host.tobytes())
    with _records_lock:
        hit = _records.get(key)
        if hit is not None:
            _records.move_to_end(key)
            return hit[1]
        _no_capture("the upload of the time-node records of an ekm_hip.solar call that has not been made before the block")
        while len(_records) >= _RECORDS_MAX:
            _, (_, old) = _records.popitem(last=False)
            old.free()  # stream-ordered: the block goes back behind the kernels that read it
        d = DeviceArray.empty(host.shape, _F64, device)
        _ffi.check(_ffi.lib().ekm_h2d(device, d.on(stream), host.ctypes.data, host.nbytes, stream))
        _records[key] = (host, d)  # `host` stays alive with the entry
        return d


# ---- launch ----
def _as_operand(x):
    if isinstance(x, DeviceArray):
        return x
    x = np.asarray(x)
    if x.dtype.kind not in "fiub":
        raise TypeError(f"ekm_hip.solar: unsupported dtype {x.dtype}")
    return x


def _launch(rec, lat, lon, shape, dtype, out_dtype):
    """One launch over `shape`: lat and lon in `dtype`, the result in `out_dtype`, as a DeviceArray."""
    device = next((a.device for a in (lat, lon) if isinstance(a, DeviceArray)), current_device())
    stream, n = current_stream(), int(math.prod(shape))
    out = DeviceArray.empty(shape, out_dtype, device)
    if n == 0:
        return out
    temps, operands = [], []
    for a in (lat, lon):
        cls = _engine.classify(tuple(a.shape), shape)
        if cls is None:
            host = a.to_host() if isinstance(a, DeviceArray) else a
            a = np.broadcast_to(host.reshape((1,) * (len(shape) - host.ndim) + tuple(host.shape)), shape)
            cls = (_ffi.FIELD, 0, 0)
        d = _to_device(a, dtype, device)
        if d is not a:
            temps.append(d)
        operands.append(_ffi.Operand(d.on(stream), cls[0], 0, cls[1], cls[2]))
    nodes = _records_on_device(kernel_records(rec), device, stream)
    entry = "ekm_solar_" + ("f32_f64" if (dtype, out_dtype) == (_F32, _F64) else "f32" if dtype == _F32 else "f64")
    _ffi.check(getattr(_ffi.lib(), entry)(device, stream, _C.byref(operands[0]), _C.byref(operands[1]), nodes.on(stream), len(rec["w"]),
                                          out.on(stream), n))
    for t in temps:
        t.free()
    return out


def _float_dtype(a):
    return np.dtype(a.dtype) if np.dtype(a.dtype) in (_F32, _F64) else _F64


def _finish(out, device_result, dtype=None):
    if dtype is not None and out.dtype != dtype:  # mixed input dtypes: computed in f64, returned in latitudes' dtype
        host = out.to_host().astype(dtype)
        out.free()
        return DeviceArray.from_host(host, out.device) if device_result else host
    if device_result:
        return out
    host = out.to_host()
    out.free()
    return host


@_foreign_aware("latitudes", "longitudes")
def cos_solar_zenith_angle(date, latitudes, longitudes):
    """Cosine of the solar zenith angle at `date` (solar.py:51-96), negative values clipped to 0.  latitudes,
    longitudes: degrees, mutually broadcastable.  Returns float64 of the broadcast shape (a NumPy float64 scalar for
    Python scalars); NaN where either coordinate is NaN or infinite."""
    lat, lon = _as_operand(latitudes), _as_operand(longitudes)
    device_result = isinstance(lat, DeviceArray) or isinstance(lon, DeviceArray)
    shape = tuple(np.broadcast_shapes(tuple(lat.shape), tuple(lon.shape)))
    dtype = _F32 if _float_dtype(lat) == _F32 and _float_dtype(lon) == _F32 else _F64
    rec = node_records([date])
    if not device_result and math.prod(shape) == 0:
        return np.zeros(shape, _F64)
    res = _finish(_launch(rec, lat, lon, shape, dtype, _F64), device_result)
    return res[()] if not device_result and not shape else res


def _integrated(radiation, begin_date, end_date, latitudes, longitudes, intervals_per_hour, integration_order):
    lat, lon = _as_operand(latitudes), _as_operand(longitudes)
    dates, weights = node_dates(begin_date, end_date, intervals_per_hour, integration_order)
    if np.dtype(lat.dtype).kind in "iub":
        raise TypeError(f"Cannot cast the float64 integrand to latitudes' dtype {lat.dtype}: the result has the dtype of "
                        "latitudes, which must be float32 or float64")
    if np.dtype(lat.dtype) not in (_F32, _F64):
        raise TypeError(f"latitudes must be float32 or float64, not {lat.dtype}")
    shape = tuple(lat.shape)
    if tuple(np.broadcast_shapes(shape, tuple(lon.shape))) != shape:  # raises ValueError itself if they do not broadcast
        raise ValueError(f"longitudes of shape {tuple(lon.shape)} do not broadcast to the shape of latitudes {shape}")
    device_result = isinstance(lat, DeviceArray) or isinstance(lon, DeviceArray)
    out_dtype = np.dtype(lat.dtype)
    dtype = out_dtype if _float_dtype(lon) == out_dtype and np.dtype(lon.dtype).kind == "f" else _F64
    rec = node_records(dates, weights, radiation)
    if not device_result and math.prod(shape) == 0:
        return np.zeros(shape, out_dtype)
    return _finish(_launch(rec, lat, lon, shape, dtype, out_dtype if dtype == out_dtype else _F64), device_result, out_dtype)


@_foreign_aware("latitudes", "longitudes")
def cos_solar_zenith_angle_integrated(begin_date, end_date, latitudes, longitudes, *, intervals_per_hour=1, integration_order=3):
    """Average of the cosine of the solar zenith angle over [begin_date, end_date] by Gauss-Legendre quadrature on
    `intervals_per_hour` sub-intervals per hour (solar.py:182-222).  integration_order: 1, 2, 3 or 4 nodes per
    sub-interval.  The result has the dtype and shape of `latitudes`."""
    return _integrated(False, begin_date, end_date, latitudes, longitudes, intervals_per_hour, integration_order)


@_foreign_aware("latitudes", "longitudes")
def toa_incident_solar_radiation(begin_date, end_date, latitudes, longitudes, *, intervals_per_hour=1, integration_order=3):
    """Top-of-atmosphere incident solar radiation averaged over [begin_date, end_date] (solar.py:232-254): the same
    quadrature with every node weighted by `incoming_solar_radiation` of its date.  Dtype and shape of `latitudes`."""
    return _integrated(True, begin_date, end_date, latitudes, longitudes, intervals_per_hour, integration_order)


# `earthkit.meteo.solar.array.<name>` is how the reference reaches the array-level functions
array = _sys.modules[__name__]
