"""The host twin's entry points of nanaverage (ekm_host_nanaverage_* of csrc/host_twin.cpp) as a NumPy function -- TEST
INFRASTRUCTURE.  The twin adds in the kernels' own order (csrc/reduce_point.hpp), so the GPU tests compare bits with it."""
import ctypes as C

import numpy as np

import _hosttwin
import _nanaverage_numpy as nn


def _vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def raw(data, outer, m, inner, weights=None, wstrides=(0, 0, 0), path=0):
    """data (flat, f32 or f64), weights (flat, the same dtype, or None) -> [outer * inner]; the return code must be 0."""
    T = data.dtype
    fn = getattr(_hosttwin.lib(), "ekm_host_nanaverage_" + ("f32" if T == nn.F32 else "f64"))
    fn.restype = C.c_int
    out = np.full(outer * inner, 7.0, T)
    rc = fn(_vp(data), C.c_size_t(outer), C.c_size_t(m), C.c_size_t(inner), _vp(weights), *(C.c_size_t(s) for s in wstrides),
            C.c_int(path), _vp(out))
    assert rc == 0, rc
    return out


def nanaverage(data, weights=None, axis=None, keepdims=False, path=0):
    """The public call through the twin: the weights are expanded to the data's shape (strides m * inner, inner, 1)."""
    data = np.asarray(data)
    T = nn.arith_dtype(data) if weights is None else nn.arith_dtype(data, weights)
    outer, m, inner = nn.layout(data.shape, axis)
    d = np.ascontiguousarray(data, T).reshape(-1)
    w = None if weights is None else np.ascontiguousarray(np.broadcast_to(np.asarray(weights).astype(T), data.shape)).reshape(-1)
    out = raw(d, outer, m, inner, w, (m * inner, inner, 1), path)
    return out.reshape(nn.result_shape(data.shape, axis, keepdims))
