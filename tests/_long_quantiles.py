"""What the long-axis quantile tests share -- TEST INFRASTRUCTURE: access to tests/golden/long_quantiles_golden.npz, the
host twin of the kernel (std::sort on the kernel's keys, then quantile_point) and the judge.  The NumPy restatement is
`_quantiles_numpy.quantiles`, imported unchanged; the judge is `_ensemble_numpy.judge_exact`: dtype, shape, NaN pattern
and every bit."""
import ctypes as C
import functools
import json
import os

import numpy as np

import _hosttwin
import _quantiles_numpy as qn
from _quantiles_numpy import F32, F64, METHODS, Mismatch, judge_exact, quantiles  # noqa: F401

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_quantiles_golden.npz")
CAP = {F32: 16384, F64: 8192}   # one column, padded to a power of two, in 64 KiB of LDS
KINDS = {"f32": (F32, F32), "f64": (F64, F64), "f32_f64": (F32, F64)}  # entry point: data, result


@functools.lru_cache(maxsize=1)
def _load():
    with np.load(PATH) as f:
        meta = json.loads(bytes(f["manifest"]).decode())
        arrays = {k: f[k] for k in f.files if k != "manifest"}
    return meta, arrays


def cases():
    return _load()[0]["cases"]


def cases_of(group):
    """The cases of one "<f32|f64> <method>" group, e.g. "f32 numpy_bulk"."""
    tag, method = group.split()
    return [c for c in cases() if c["note"].startswith(tag + " ") and c["plain"]["method"] == method]


def signature():
    return _load()[0]["signatures"]["iter_quantiles"]


def kwargs_of(case):
    kw = dict(case["plain"])
    kw["arr"] = _load()[1][case["arrays"]["arr"]]
    return kw


def expected_of(case):
    return _load()[1][case["out"]]


def case_id(case):
    return f"{case['id']}-{case['note'].replace(' ', '_')}"


def judge_case(case, got, what=""):
    judge_exact(np.asarray(got), expected_of(case), what or case["note"])


def tables(method, m, qs, T):
    """The position records of the levels `qs` as three float64 vectors, from the restatement's scalar expression."""
    pos = [qn.positions(method, m, q, T) for q in qs]
    return [np.array([float(p[k]) for p in pos]) for k in range(3)]


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def twin(arr, which=100, axis=0, method="sort"):
    """One call through the host twin of the long-axis kernel: the argument handling of ekm_hip.stats restated for
    ekm_host_long_quantiles_* ([outer, m, inner] view, position tables from the restatement)."""
    arr = np.asarray(arr)
    T = qn.arith_dtype(arr)
    out_dtype = T if method == "numpy" else F64
    a = np.ascontiguousarray(arr, T)
    axis %= a.ndim
    m, rest = a.shape[axis], a.shape[:axis] + a.shape[axis + 1:]
    outer, inner = int(np.prod(a.shape[:axis], dtype=np.int64)), int(np.prod(a.shape[axis + 1:], dtype=np.int64))
    lo, hi, w = tables(method, m, qn.levels(which), T)
    nq = len(lo)
    out = np.full((nq,) + rest, 7, out_dtype)
    tag = "f32" if out_dtype == F32 else "f64" if T == F64 else "f32_f64"
    fn = getattr(_hosttwin.lib(), f"ekm_host_long_quantiles_{tag}")
    fn.restype = C.c_int
    rc = fn(_vp(a), C.c_size_t(outer), C.c_uint(m), C.c_size_t(inner), _vp(lo), _vp(hi), _vp(w), C.c_uint(nq),
            C.c_int(0 if method == "sort" else 1), _vp(out))
    assert rc == 0, rc
    return out


def sort_by_key(x):
    """`x` (1-D, f32 or f64) in the order of the kernel's keys, by the twin."""
    x = np.array(x, copy=True)
    fn = getattr(_hosttwin.lib(), "ekm_host_sort_by_key_" + ("f32" if x.dtype == F32 else "f64"))
    fn.restype = None
    fn(_vp(x), C.c_size_t(x.size))
    return x
