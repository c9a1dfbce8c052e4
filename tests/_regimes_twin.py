"""The host twin's entry points of the reduce family (ekm_host_regimes_project_*, ekm_host_regimes_index_*,
ekm_host_pearson_* of csrc/host_twin.cpp) as NumPy functions -- TEST INFRASTRUCTURE.  The twin adds in the kernels' own
order (csrc/reduce_point.hpp), so the GPU tests compare bits with it."""
import ctypes as C

import numpy as np

import _hosttwin
import _regimes_numpy as rn


def _vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def _fn(name, T):
    fn = getattr(_hosttwin.lib(), f"ekm_host_{name}_" + ("f32" if T == rn.F32 else "f64"))
    fn.restype = C.c_int
    return fn


def project_raw(field, coef, npat, coef_stride=0, scale=None):
    """field [N, K], coef (flat), scale [N] or None, all of one dtype -> [npat, N]."""
    T = field.dtype
    nf, k = field.shape
    out = np.full((npat, nf), 7.0, T)
    rc = _fn("regimes_project", T)(_vp(field), C.c_size_t(nf), C.c_size_t(k), _vp(coef), C.c_uint(npat), C.c_size_t(coef_stride),
                                    _vp(scale), _vp(out))
    assert rc == 0, rc
    return out


def project(case):
    """A golden project case through the twin, the host work done as ekm_hip.regimes does it: {label: array}."""
    f, p, wn, mod, nshape = rn._project_terms(case)
    T = rn.project_dtype(case)
    f = np.ascontiguousarray(f, T)
    with np.errstate(all="ignore"):
        c = p.astype(T) * wn.astype(T)  # [P, N or 1, K]
    npat, per_field = c.shape[0], case["plain"]["kind"] == "perfield"
    scale = None if mod is None else np.ascontiguousarray(mod, T)
    if per_field:
        out = np.concatenate([project_raw(f, np.ascontiguousarray(c[i]).reshape(-1), 1, f.shape[1]) for i in range(npat)])
    else:
        out = project_raw(f, np.ascontiguousarray(c).reshape(-1), npat, 0, scale)
    return {label: out[i].reshape(nshape) for i, label in enumerate(case["plain"]["labels"])}


def index_raw(proj, mean, std):
    """proj: an array; mean, std: arrays of its shape and dtype, or numbers."""
    T = proj.dtype
    real = C.c_float if T == rn.F32 else C.c_double
    proj = np.ascontiguousarray(proj)
    out = np.full(proj.shape, 7.0, T)
    arr = [np.ascontiguousarray(np.broadcast_to(v, proj.shape), T) if isinstance(v, np.ndarray) and v.ndim else None for v in (mean, std)]
    val = [real(0.0) if a is not None else real(float(T.type(v))) for a, v in zip(arr, (mean, std))]
    rc = _fn("regimes_index", T)(_vp(proj), _vp(arr[0]), val[0], _vp(arr[1]), val[1], _vp(out), C.c_size_t(proj.size))
    assert rc == 0, rc
    return out


def pearson(x, y, axis=0):
    x, y = np.asarray(x), np.asarray(y)
    T = rn.arith_dtype(x, y)
    x, y = np.ascontiguousarray(x, T), np.ascontiguousarray(y, T)
    outer, m, inner = rn.layout(x.shape, axis)
    axis %= x.ndim
    out = np.full(x.shape[:axis] + x.shape[axis + 1:], 7.0, T)
    rc = _fn("pearson", T)(_vp(x), _vp(y), C.c_size_t(outer), C.c_size_t(m), C.c_size_t(inner), _vp(out))
    assert rc == 0, rc
    return out
