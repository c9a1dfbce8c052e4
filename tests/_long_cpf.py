"""What the long_cpf tests share -- TEST INFRASTRUCTURE: access to tests/golden/long_cpf_golden.npz (the arrays of a case
rebuilt from the stored ones as gen_golden_long_cpf.py derived them), the host twins of `long_cpf_tiles` and of `cpf_points`
(ekm_host_long_cpf_* / ekm_host_cpf_*), data for the tests that need none recorded, the tile geometry of a launch and the
judge: `_ensemble_numpy.judge_exact` -- dtype, shape, NaN pattern and every bit.  The NumPy restatement is `_cpf_numpy.cpf`,
imported unchanged."""
import ctypes as C
import functools
import json
import os

import numpy as np

import _cpf_numpy as cn
import _hosttwin
from _cpf_numpy import F32, F64
from _ensemble_numpy import Mismatch, judge_exact  # noqa: F401
from _long_ensemble import no_column_mixes_the_zeros  # noqa: F401

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_cpf_golden.npz")
CAP = {F32: 16384, F64: 8192}         # per axis: one column, padded to a power of two, in 64 KiB of LDS
SMALL = {F32: 4096, F64: 2048}        # the keys of the 16-KiB tile
SHORT_ROWS = {F32: 640, F64: 320}     # what `cpf` holds in 160 KiB: members, plus climate rows when it sorts them
TAG = {F32: "f32", F64: "f64"}
SHAPES = ((101, 700), (700, 51), (513, 257), (1980, 51), (101, 1980), (700, 700))
OPTION_NOTES = ("default", "from_zero", "symmetric", "symmetric from_zero", "epsilon 0.5", "epsilon 0.5 symmetric",
                "sorts off presorted", "sorts off unsorted", "sorts off unsorted symmetric from_zero",
                "sorts off unsorted epsilon 0.5", "sort_clim off", "sort_ens off")
# the 12 option sets as keyword arguments, for the tests that make their own data
OPTION_SETS = (dict(), dict(from_zero=True), dict(symmetric=True), dict(symmetric=True, from_zero=True), dict(epsilon=0.5),
               dict(epsilon=0.5, symmetric=True), dict(sort_clim=False, sort_ens=False),
               dict(sort_clim=False, sort_ens=False, symmetric=True, from_zero=True),
               dict(sort_clim=False, sort_ens=False, epsilon=0.5), dict(sort_clim=False, from_zero=True),
               dict(sort_ens=False, from_zero=True), dict(sort_ens=False, symmetric=True))


@functools.lru_cache(maxsize=1)
def _load():
    with np.load(PATH) as f:
        meta = json.loads(bytes(f["manifest"]).decode())
        arrays = {k: f[k] for k in f.files if k != "manifest"}
    return meta, arrays


def signature():
    return _load()[0]["signature"]


def cases(tag=None):
    return [c for c in _load()[0]["cases"] if tag is None or c["dtype"] == tag]


@functools.lru_cache(maxsize=None)
def _arrays_of(clim_key, ens_key, perm_key, presort, tag):
    arrays, T = _load()[1], F32 if tag == "f32" else F64
    clim, ens = arrays[clim_key], arrays[ens_key]
    clim = (clim[arrays[perm_key]] if perm_key else clim).astype(T)
    ens = (np.sort(ens, axis=0) if presort else ens).astype(T)
    clim.setflags(write=False), ens.setflags(write=False)
    return clim, ens


def kwargs_of(case):
    """The call the reference was given: clim, ens (read-only, shared between the cases that use them) and the options."""
    clim, ens = _arrays_of(case["clim"], case["ens"], case["perm"], case["presort_ens"], case["dtype"])
    return dict(case["plain"], clim=clim, ens=ens)


def expected_of(case):
    return _load()[1][case["out"]]


def case_id(case):
    return f"{case['id']}-{case['note'].replace(' ', '_')}"


def judge_case(case, got, what=""):
    judge_exact(np.asarray(got), expected_of(case), what or case_id(case))


# ---- the host twins: the argument handling of ekm_hip.extreme._cpf restated for ekm_host_long_cpf_* / ekm_host_cpf_* ----
def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _twin(name, clim, ens, sort_clim, sort_ens, epsilon, symmetric, from_zero):
    clim, ens = np.asarray(clim), np.asarray(ens)
    T = cn.arith_dtype(clim, ens)
    clim, ens = np.ascontiguousarray(clim, T), np.ascontiguousarray(ens, T)
    out = np.full(clim.shape[1], 7, np.float32)
    fn = getattr(_hosttwin.lib(), f"{name}_{TAG[T]}")
    fn.restype = C.c_int
    use_eps = epsilon is not None and not symmetric
    rc = fn(_vp(clim), _vp(ens), C.c_uint(clim.shape[0]), C.c_uint(ens.shape[0]), C.c_size_t(clim.shape[1]),
            C.c_int(bool(sort_clim)), C.c_int(bool(sort_ens)), C.c_int(bool(from_zero)), C.c_int(bool(symmetric)),
            C.c_int(use_eps), C.c_double(epsilon if use_eps else 0.0), _vp(out))
    assert rc == 0, rc
    return out


def twin(clim, ens, sort_clim=True, sort_ens=True, epsilon=None, symmetric=False, from_zero=False):
    """long_cpf_tiles on the host: the kernel's keys, std::sort where asked, cpf_value_running."""
    return _twin("ekm_host_long_cpf", clim, ens, sort_clim, sort_ens, epsilon, symmetric, from_zero)


def short_twin(clim, ens, sort_clim=True, sort_ens=True, epsilon=None, symmetric=False, from_zero=False):
    """cpf_points on the host: the insertion sort, cpf_value (the quadratic priming loop)."""
    return _twin("ekm_host_cpf", clim, ens, sort_clim, sort_ens, epsilon, symmetric, from_zero)


# ---- data for the tests that need none recorded ----
def fields(rng, nclim, nens, npts, T, specials=True):
    """(clim unsorted, ens unsorted) on a grid of 1/8 (ties between members and rows), only +0.0; the ensemble narrower
    than the climate and shifted per point, so that crossings of every kind occur; with `specials` and 8 points or more
    a NaN, a +inf and a -inf in columns of their own, in either field."""
    clim = np.round(rng.normal(0, 3, (nclim, npts)) * 8) / 8 + 0.0
    ens = np.round((rng.normal(0, 1.5, (nens, npts)) + rng.normal(0, 3, npts)) * 8) / 8 + 0.0
    if specials and npts >= 8:
        clim[nclim // 2, 1], clim[nclim // 3, 2], clim[nclim - 1, 3] = np.nan, np.inf, -np.inf
        ens[nens // 2, 4], ens[nens // 3, 5], ens[nens - 1, 6] = np.nan, np.inf, -np.inf
        ens[:, 7] = ens[0, 7]
    return clim.astype(T), ens.astype(T)


def columns_per_tile(T, nclim, nens):
    """C of a launch: the columns of the tile that holds fewer (long_cpf_tiles / launch_long_cpf)."""
    def columns(m):
        n = 32
        while n < m:
            n *= 2
        return (SMALL[T] if n <= SMALL[T] else CAP[T]) // n
    return min(columns(nclim), columns(nens))
