"""What `ekm_hip.extreme` and `ekm_hip.score` share: the member-axis kernels of csrc/ensemble.hip take member-major
fields [nmember, npts] on the device and small float64 coefficient tables that are computed on the host with NumPy,
exactly as the reference computes them, and kept on the device per (kind, length, device)."""
import math

import numpy as np

from . import _ffi
from .device import DeviceArray, current_device, current_stream
from .vertical import _to_device

_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)
_tables = {}


def as_input(x):
    return x if isinstance(x, DeviceArray) else np.asarray(x)


def arith_dtype(*arrays):
    """f32 only when every array is f32; everything else (f64, mixed, integer, f16) is computed in f64."""
    return _F32 if all(np.dtype(a.dtype) == _F32 for a in arrays) else _F64


def device_of(*arrays):
    return next((a.device for a in arrays if isinstance(a, DeviceArray)), current_device())


def on_device(*arrays):
    return any(isinstance(a, DeviceArray) for a in arrays)


def npoints(shape):
    return int(math.prod(shape))


def upload(x, dtype, device, stream, keep):
    d = _to_device(x, dtype, device)
    d.on(stream)
    keep.append(d)
    return d


def table(kind, n, device, make):
    """The device copy of `make()` (a tuple of float64 vectors), uploaded once per (kind, n, device).  The first use of
    a length uploads, which cannot be recorded: call once outside an `ekm_hip.graph()` block before recording."""
    key = (kind, int(n), int(device))
    if key not in _tables:
        host = tuple(np.ascontiguousarray(t, dtype=np.float64) for t in make())
        _tables[key] = (host, tuple(DeviceArray.from_host(t if t.size else np.zeros(1), device) for t in host))
    return _tables[key]


def finish(out, device_result):
    if device_result:
        return out
    res = out.to_host()
    out.free()
    return res


def tag_of(dtype):
    return "f32" if dtype == _F32 else "f64"


def lib():
    return _ffi.lib()
