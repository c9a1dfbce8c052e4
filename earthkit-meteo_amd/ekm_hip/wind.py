"""`earthkit.meteo.wind` on MI355X: wind speed and direction, the polar / xy conversions, the Coriolis parameter, the
wind rose and the hydrostatic vertical velocity (reference wind/array/wind.py; kernels in csrc/wind.hip, per-point
arithmetic csrc/wind_point.hpp; `w_from_omega` is a map kernel of the thermo family).

Same names, argument order, defaults, error types and messages as the reference.  NumPy in -> NumPy out; `DeviceArray`
in -> `DeviceArray` out; device tensors of another ROCm library are taken over through DLPack and handed back in that
library's type.  Python scalars give what the reference gives (NumPy float64 scalars; a 0-d array from `direction` where
the reference assigns through a mask).  float32 input gives float32, anything else -- integers, bools, a float32 beside a
float64 -- is computed and returned as float64.  Operands broadcast against each other: a full field, a scalar, or a
vector along the leading or the trailing axes of the result are indexed by the kernel, any other pattern is expanded on
the host first.

`speed`, `direction` and `xy_to_polar` are ONE launch of one kernel that reads `u` and `v` once and writes the speed,
the direction or both; `polar_to_xy` and `coriolis` are one launch each.  float32 fields are computed in float32
arithmetic, everything else in float64; the inverse tangent, the hypotenuse and the sine / cosine are the project's own
(no math library on the device).  The direction follows the reference's arithmetic from d = atan2(v, u):
meteo d <= -pi/2 ? (-pi/2 - d) deg : (1.5 pi - d) deg; polar d deg, plus 360 where negative if `to_positive`.  At the
branch point of the meteo direction (v < 0, |u| within a few eps of 0) a result may be 360 where the reference has 0
or the reverse: the same direction.  `polar_to_xy` reduces the angle exactly in degrees, so at exact multiples of 90
degrees a component is an exact zero where the reference has +-1.8e-16 |m|; with an infinite magnitude such an element
is NaN where the reference has +-inf (the one deviation: INTEGRATION.md).

`windrose` is a memset and two kernels and does not wait on the host.  The edges are built here by the reference's own
NumPy expressions in the dtype of `speed` (its quirks included: `linspace(int(-step/2), int(360+step/2),
int(360/step)+2)`), uploaded once as float64 and kept in a small least-recently-used cache per device (16 entries);
inside an `ekm_hip.graph()` block nothing can be uploaded, so make the same call once before the block.  A recorded
graph reads the cached block at every replay: it must be replayed before 16 OTHER sets of edges have been used on that
device, after which the block is evicted and freed.  Samples are
compared with the edges in float64, which is exact.  Counts and percentages are bit for bit the reference's.
Deviations from the reference: the exact zeros of `polar_to_xy` above, and a limit of 2048 edges (speed
+ direction together: `sectors` above about 2000 raise ValueError where the reference works).  Integer `speed` beside a
DeviceArray `direction` gives a DeviceArray histogram and the (integer) direction bins as a NumPy array.
"""
import collections as _collections
import ctypes as _C
import math as _math
import sys as _sys
import threading as _threading

import numpy as np

from . import _engine, _ffi
from .device import DeviceArray, _no_capture, current_device, current_stream
from .vertical import _foreign_aware, _to_device

_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)
_METEO, _POLAR_POSITIVE, _POLAR_SIGNED = 0, 1, 2
MAX_EDGES = 2048  # csrc/wind.hip: kRoseMaxEdges


def w_from_omega(omega, t, p):
    """Hydrostatic vertical velocity (m/s) from pressure velocity omega (Pa/s), temperature t (K) and
    pressure p (Pa): w = -(omega * t * Rd) / (p * g), evaluated as (-Rd/g) * (omega * t / p) (wind.py:222)."""
    return _engine.run("w_from_omega", (omega, t, p))[0]


# ---- the elementwise family ----
def _as_operand(x):
    if isinstance(x, DeviceArray):
        return x
    x = np.asarray(x)
    if x.dtype.kind not in "iub" and x.dtype not in (_F32, _F64):
        raise TypeError(f"ekm_hip.wind: unsupported dtype {x.dtype}")
    return x


def _elementwise(entry, operands, mode, wanted):
    """One launch of ekm_wind_<entry>_*: `wanted` says which of the two outputs exist.  Returns the results in the
    caller's array type: a tuple with None where an output was not wanted."""
    ops = [_as_operand(x) for x in operands]
    device_result = any(isinstance(a, DeviceArray) for a in ops)
    shape = tuple(np.broadcast_shapes(*[tuple(a.shape) for a in ops]))
    dtype = _F32 if all(np.dtype(a.dtype) == _F32 for a in ops) else _F64
    n = int(_math.prod(shape))
    if n == 0 and not device_result:
        return tuple(np.zeros(shape, dtype) if w else None for w in wanted), False
    device = next((a.device for a in ops if isinstance(a, DeviceArray)), current_device())
    stream = current_stream()
    outs = [DeviceArray.empty(shape, dtype, device) if w else None for w in wanted]
    if n:
        temps, cops = [], []
        for a in ops:
            cls = _engine.classify(tuple(a.shape), shape)
            if cls is None:
                host = a.to_host() if isinstance(a, DeviceArray) else a
                a = np.broadcast_to(host.reshape((1,) * (len(shape) - host.ndim) + tuple(host.shape)), shape)
                cls = (_ffi.FIELD, 0, 0)
            d = _to_device(a, dtype, device)
            if d is not a:
                temps.append(d)
            cops.append(_ffi.Operand(d.on(stream), cls[0], 0, cls[1], cls[2]))
        fn = getattr(_ffi.lib(), f"ekm_wind_{entry}_" + ("f32" if dtype == _F32 else "f64"))
        ptrs = [o.on(stream) if o is not None else None for o in outs]
        if entry == "coriolis":
            _ffi.check(fn(device, stream, _C.byref(cops[0]), ptrs[0], n))
        else:
            _ffi.check(fn(device, stream, _C.byref(cops[0]), _C.byref(cops[1]), mode, ptrs[0], ptrs[1], n))
        for t in temps:
            t.free()
    if device_result:
        return tuple(outs), False
    res = []
    for o in outs:
        res.append(None if o is None else o.to_host())
        if o is not None:
            o.free()
    return tuple(res), not shape


def _direction_mode(convention, to_positive, who):
    if convention == "meteo":
        return _METEO
    if convention == "polar":
        return _POLAR_POSITIVE if to_positive else _POLAR_SIGNED
    raise ValueError(f"{who}(): invalid convention={convention}!")


@_foreign_aware("u", "v")
def speed(u, v):
    """Wind speed / vector magnitude hypot(u, v) (wind.py:15-34), without overflow or underflow in between."""
    (s, _), scalar = _elementwise("polar", (u, v), _METEO, (True, False))
    return s[()] if scalar else s


@_foreign_aware("u", "v")
def direction(u, v, convention="meteo", to_positive=True):
    """Direction [degrees] of the vector (u, v) (wind.py:37-104).  convention "meteo": where the wind blows from,
    clockwise from North; "polar": anti-clockwise from the x axis, in [0, 360] if `to_positive`, else [-180, 180]."""
    mode = _direction_mode(convention, to_positive, "direction")
    (_, d), scalar = _elementwise("polar", (u, v), mode, (False, True))
    return d[()] if scalar and mode == _POLAR_SIGNED else d  # (the reference's masked assignment leaves a 0-d array)


@_foreign_aware("x", "y")
def xy_to_polar(x, y, convention="meteo"):
    """(magnitude, direction [degrees]) of the vector (x, y) in one pass over x and y (wind.py:107-135)."""
    mode = _direction_mode(convention, True, "direction")
    (s, d), scalar = _elementwise("polar", (x, y), mode, (True, True))
    return (s[()] if scalar else s), d


@_foreign_aware("magnitude", "direction")
def polar_to_xy(magnitude, direction, convention="meteo"):
    """(x, y) components from magnitude and direction [degrees] (wind.py:138-189)."""
    if convention not in ("meteo", "polar"):
        raise ValueError(f"polar_to_xy(): invalid convention={convention}!")
    (x, y), scalar = _elementwise("xy", (magnitude, direction), _METEO if convention == "meteo" else _POLAR_POSITIVE, (True, True))
    return (x[()], y[()]) if scalar else (x, y)


@_foreign_aware("lat")
def coriolis(lat):
    """Coriolis parameter 2 Omega sin(lat) [1/s], lat in degrees (wind.py:225-251)."""
    (f, _), scalar = _elementwise("coriolis", (lat,), 0, (True, False))
    return f[()] if scalar else f


# ---- wind rose ----
def rose_edges(speed_dtype, sectors, speed_bins):
    """(speed edges, direction edges) in the dtype of `speed`, by the reference's own expressions (wind.py:308-312)."""
    dir_step = 360.0 / sectors
    dir_bins = np.linspace(int(-dir_step / 2), int(360 + dir_step / 2), int(360 / dir_step) + 2, dtype=speed_dtype)
    return np.asarray(speed_bins, dtype=speed_dtype), dir_bins


_edges = _collections.OrderedDict()  # (device, bytes of the edges, dtype of dir_bins) -> (host edges, DeviceArray, dir_bins DeviceArray)
_edges_lock = _threading.Lock()
_EDGES_MAX = 16


def _edges_on_device(host, dir_bins, device, stream):
    key = (int(device), host.tobytes(), dir_bins.dtype.str)
    with _edges_lock:
        hit = _edges.get(key)
        if hit is not None:
            _edges.move_to_end(key)
            return hit[1], hit[2]
        _no_capture("the upload of the bin edges of an ekm_hip.wind.windrose call that has not been made before the block")
        while len(_edges) >= _EDGES_MAX:
            _, (_, old, old_bins) = _edges.popitem(last=False)
            old.free()  # stream-ordered: the block goes back behind the kernels that read it
            if old_bins is not None:
                old_bins.free()
        d = DeviceArray.empty(host.shape, _F64, device)
        _ffi.check(_ffi.lib().ekm_h2d(device, d.on(stream), host.ctypes.data, host.nbytes, stream))
        bins = np.ascontiguousarray(dir_bins[:-1])
        b = None  # (integer samples are host arrays: their direction bins are handed back from the host)
        if bins.dtype in (_F32, _F64):
            b = DeviceArray.empty(bins.shape, bins.dtype, device)
            _ffi.check(_ffi.lib().ekm_h2d(device, b.on(stream), bins.ctypes.data, bins.nbytes, stream))
        _edges[key] = ((host, bins), d, b)  # the host arrays stay alive with the entry
        return d, b


@_foreign_aware("speed", "direction")
def windrose(speed, direction, sectors=16, speed_bins=None, percent=True):
    """Wind rose (wind.py:254-328): the histogram of `speed` over `speed_bins` (first axis) and of the meteorological
    `direction` [degrees, 0 to 360] over `sectors` sectors shifted by half a sector (second axis), as counts or, with
    `percent`, as percentages of the counted samples; and the lower edges of the sectors.  float64 [len(speed_bins)-1,
    sectors] and the edges in the dtype of `speed`."""
    speed_bins = speed_bins if speed_bins is not None else []
    if len(speed_bins) < 2:
        raise ValueError("windrose(): speed_bins must have at least 2 elements!")
    sectors = int(sectors)
    if sectors < 1:
        raise ValueError("windrose(): sectors must be greater than 1!")
    sp, di = _as_operand(speed), _as_operand(direction)
    device_result = isinstance(sp, DeviceArray) or isinstance(di, DeviceArray)
    if len(sp.shape) > 1 or len(di.shape) > 1:
        raise ValueError("windrose(): speed and direction must be one-dimensional")
    n = int(_math.prod(sp.shape))
    if n != int(_math.prod(di.shape)):
        raise ValueError(f"windrose(): speed has {n} samples, direction {int(_math.prod(di.shape))}")
    sdt = np.dtype(sp.dtype)
    se, de = rose_edges(sdt, sectors, speed_bins)
    if se.ndim != 1:
        raise ValueError("windrose(): speed_bins must be one-dimensional")
    for k, e in enumerate((se, de)):
        if np.any(e[:-1] > e[1:]):
            raise ValueError(f"`bins[{k}]` must be monotonically increasing, when an array")
    ns, nd = len(se), len(de)
    if ns + nd > MAX_EDGES:
        raise ValueError(f"windrose(): {ns} speed edges and {nd} direction edges: at most {MAX_EDGES} together are supported")
    edges = np.ascontiguousarray(np.concatenate([se.astype(_F64), de.astype(_F64)]))
    span = float(edges[-1] - edges[ns])
    inv_step = (nd - 1) / span if span > 0 and _math.isfinite(span) else 0.0
    dtype = _F32 if sdt == _F32 and np.dtype(di.dtype) == _F32 else _F64
    device = next((a.device for a in (sp, di) if isinstance(a, DeviceArray)), current_device())
    stream = current_stream()
    dev_edges, dev_bins = _edges_on_device(edges, de, device, stream)
    temps, ptrs = [], []
    for a in (sp, di):
        if n == 0:
            ptrs.append(None)
            continue
        d = _to_device(a if isinstance(a, DeviceArray) else a.reshape(n), dtype, device)
        if d is not a:
            temps.append(d)
        ptrs.append(d.on(stream))
    table = DeviceArray.empty(((ns - 1) * (nd - 1),), _F64, device)  # 64-bit counters, zeroed by the call
    out = DeviceArray.empty((ns - 1, nd - 2), _F64, device)
    fn = getattr(_ffi.lib(), "ekm_windrose_" + ("f32" if dtype == _F32 else "f64"))
    _ffi.check(fn(device, stream, ptrs[0], ptrs[1], n, dev_edges.on(stream), ns, nd, inv_step, 1 if percent else 0,
                  table.on(stream), out.on(stream)))
    table.free()
    for t in temps:
        t.free()
    if device_result and dev_bins is None:  # integer speed beside a DeviceArray direction: the integer bins stay on the host
        return out, de[:-1]
    if device_result:
        bins = DeviceArray.empty(dev_bins.shape, dev_bins.dtype, device)
        _ffi.check(_ffi.lib().ekm_d2d(device, bins.on(stream), dev_bins.on(stream), dev_bins.nbytes, stream))
        return out, bins
    res = out.to_host()
    out.free()
    return res, de[:-1]


# `earthkit.meteo.wind.array.<name>` is how the reference reaches the array-level functions
array = _sys.modules[__name__]
