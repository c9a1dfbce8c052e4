"""What the long-axis ensemble tests share -- TEST INFRASTRUCTURE: access to tests/golden/long_ensemble_golden.npz, the
host twins of the kernels of csrc/long_ensemble.hip (std::sort on the kernel's keys, then the *_point call of the
read-out) and the judge.  The NumPy restatements are those of `_ensemble_numpy` and `_gumbel_numpy`, imported unchanged;
the judge is `_ensemble_numpy.judge_exact`: dtype, shape, NaN pattern and every bit."""
import ctypes as C
import functools
import json
import os

import numpy as np

import _ensemble_numpy as en
import _gumbel_numpy as gn
import _hosttwin
from _ensemble_numpy import F32, F64, Mismatch, judge_exact  # noqa: F401

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_ensemble_golden.npz")
CAP = {F32: 16384, F64: 8192}   # one column, padded to a power of two, in 64 KiB of LDS
SHORT_CAP = {F32: 256, F64: 128}
TAG = {F32: "f32", F64: "f64"}
FUNCS = ("efi", "sot", "crps_from_ensemble", "fit")
MS = (257, 300, 512, 513, 1980)


@functools.lru_cache(maxsize=1)
def _load():
    with np.load(PATH) as f:
        meta = json.loads(bytes(f["manifest"]).decode())
        arrays = {k: f[k] for k in f.files if k != "manifest"}
    return meta, arrays


def cases(func=None, tag=None):
    return [c for c in _load()[0]["cases"] if (func is None or c["func"] == func) and (tag is None or c["note"].startswith(tag + " "))]


def kwargs_of(case):
    arrays = _load()[1]
    kw = dict(case["plain"])
    kw.update({k: arrays[key] for k, key in case["arrays"].items()})
    return kw


def expected_of(case):
    """The recorded array, or the (mu, sigma) pair of a fit case."""
    arrays, out = _load()[1], case["out"]
    return (arrays[out["mu"]], arrays[out["sigma"]]) if case["func"] == "fit" else arrays[out["out"]]


def recorded_tables():
    """The EFI coefficient tables (101 rows) of the host that recorded the cases: another libm may round an acos otherwise."""
    meta, arrays = _load()
    return tuple(arrays[k] for k in meta["efi_tables"])


def case_id(case):
    return f"{case['id']}-{case['func']}-{case['note'].replace(' ', '_')}"


def judge_case(case, got, what=""):
    """got: an array, or (mu, sigma) / an object with .mu and .sigma for a fit case."""
    what = what or case_id(case)
    want = expected_of(case)
    if case["func"] == "fit":
        mu, sigma = (got.mu, got.sigma) if hasattr(got, "mu") else got
        judge_exact(np.asarray(mu), want[0], what + " mu")
        judge_exact(np.asarray(sigma), want[1], what + " sigma")
    else:
        judge_exact(np.asarray(got), want, what)


# ---- the restatements, under the names of the public functions ----
def restate(func, **kw):
    if func == "fit":
        return gn.fit(kw["sample"], kw.get("axis", 0))
    return en.RESTATEMENT[func](**kw)


def restate_case(case, tables=None):
    """tables: the EFI coefficients to restate an efi case with; the recorded ones by default."""
    extra = dict(tables=tables if tables is not None else recorded_tables()) if case["func"] == "efi" else {}
    return restate(case["func"], **kwargs_of(case), **extra)


# ---- the host twins: the argument handling of ekm_hip.extreme / score / stats restated for ekm_host_long_* ----
def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _fn(name, T):
    fn = getattr(_hosttwin.lib(), f"ekm_host_long_{name}_{TAG[T]}")
    fn.restype = C.c_int
    return fn


def twin_efi(clim, ens, eps=-0.1, tables=None):
    T = en.arith_dtype(clim, ens)
    clim, ens = np.ascontiguousarray(clim, T), np.ascontiguousarray(ens, T)
    (nclim, npts), nens = clim.shape, ens.shape[0]
    tabs = [np.ascontiguousarray(t, F64) for t in (tables if tables is not None else en.efi_tables(nclim))]
    out = np.full(npts, 7.0)
    rc = _fn("efi", T)(_vp(clim), _vp(ens), C.c_uint(nclim), C.c_uint(nens), C.c_size_t(npts), C.c_double(eps), _vp(tabs[0]),
                       _vp(tabs[1]), _vp(tabs[2]), _vp(out))
    assert rc == 0, rc
    return out


def twin_sot(clim, ens, perc, eps=-1e4):
    T = en.arith_dtype(clim, ens)
    pts = clim.shape[1:]
    clim, ens = np.ascontiguousarray(clim, T).reshape(clim.shape[0], -1), np.ascontiguousarray(ens, T).reshape(ens.shape[0], -1)
    qc, tail = np.ascontiguousarray(clim[perc]), np.ascontiguousarray(clim[99 if perc > 50 else 1])
    out = np.full(clim.shape[1], 7, T)
    rc = _fn("sot", T)(_vp(qc), _vp(tail), _vp(ens), C.c_uint(ens.shape[0]), C.c_size_t(clim.shape[1]), C.c_int(perc),
                       C.c_double(eps), _vp(out))
    assert rc == 0, rc
    return out.reshape(pts)


def twin_crps(x, y, nan_policy="propagate", with_missing=False):
    T = en.arith_dtype(x, y)
    pts = np.shape(y)
    x, y = np.ascontiguousarray(x, T).reshape(np.shape(x)[0], -1), np.ascontiguousarray(y, T).reshape(-1)
    n = x.shape[0]
    p = np.arange(n + 1) / float(n)
    p2, q2 = np.ascontiguousarray(p**2), np.ascontiguousarray((1 - p) ** 2)
    out, missing = np.full(y.size, 7.0), np.full(y.size, 9, np.uint8)
    rc = _fn("crps_from_ensemble", T)(_vp(x), _vp(y), C.c_uint(n), C.c_size_t(y.size), _vp(p2), _vp(q2), _vp(out), _vp(missing))
    assert rc == 0, rc
    if nan_policy == "omit":
        return out[missing == 0]
    return (out.reshape(pts), missing.reshape(pts).astype(bool)) if with_missing else out.reshape(pts)


def twin_fit(sample, axis=0):
    sample = np.asarray(sample)
    T = gn.arith_dtype(sample)
    a = np.ascontiguousarray(sample, T)
    axis %= a.ndim
    m, rest = a.shape[axis], a.shape[:axis] + a.shape[axis + 1:]
    outer, inner = int(np.prod(a.shape[:axis], dtype=np.int64)), int(np.prod(a.shape[axis + 1:], dtype=np.int64))
    mu, sigma = np.full(rest, 7.0), np.full(rest, 7.0)
    rc = _fn("gumbel_fit", T)(_vp(a), C.c_size_t(outer), C.c_uint(m), C.c_size_t(inner), _vp(mu), _vp(sigma))
    assert rc == 0, rc
    return mu, sigma


TWIN = {"efi": twin_efi, "sot": twin_sot, "crps_from_ensemble": twin_crps, "fit": twin_fit}


def twin_case(case):
    extra = dict(tables=recorded_tables()) if case["func"] == "efi" else {}
    return TWIN[case["func"]](**kwargs_of(case), **extra)


# ---- data for the tests that need none recorded: tie-heavy, no column mixing the two zeros ----
def field(rng, rows, npts, T, specials=True):
    """[rows, npts]: clamped, rounded to 1/8 (ties; + 0.0: only +0.0); with `specials` and three columns or more a NaN, a +inf and
    a -inf member in three different columns."""
    a = np.round(np.maximum(rng.gamma(1.5, 2.0, (rows, npts)) - 1.0, 0.0) * 8) / 8 + 0.0
    if specials and npts >= 3:
        a[rows // 2, 0], a[rows // 3, npts // 2], a[rows - 1, npts - 1] = np.nan, np.inf, -np.inf
    return a.astype(T)


def climate(rng, npts, T, sort=True):
    c = np.round(np.maximum(rng.gamma(1.5, 2.0, (101, npts)) - 1.0, 0.0) * 8) / 8 + np.linspace(0, 1, 101)[:, None]
    c = np.sort(c, axis=0) if sort else c
    return c.astype(T)


def no_column_mixes_the_zeros(a, axis=0):
    a = np.moveaxis(np.asarray(a), axis, 0).reshape(np.shape(a)[axis], -1)
    neg, pos = (a == 0) & np.signbit(a), (a == 0) & ~np.signbit(a)
    return not (neg.any(axis=0) & pos.any(axis=0)).any()
