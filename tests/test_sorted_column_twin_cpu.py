"""The host twin's sorted-column entry points on what the recorded cases leave out, without a GPU: a sample axis that
does not lead ([outer, m, inner] with outer > 1) for the quantiles and the Gumbel fit, and the flag bytes of
crps_from_ensemble.  The twin runs ensemble_point.hpp -- stage_column and sample_column, and for crps and the fit the
very bodies the kernels call (crps_body, gumbel_fit_body) -- so these lines are checked here, against the NumPy
restatements, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import _ensemble_numpy as en
import _gumbel_numpy as gn
import _hosttwin
import _quantiles_numpy as qn
from test_gumbel_cpu import twin_fit
from test_quantiles_cpu import twin as twin_quantiles

SHAPES = [(2, 5, 3), (3, 4, 1)]


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _sample(shape, dtype):
    a = np.random.default_rng(shape[1]).normal(size=shape).astype(dtype)
    a[-1, 1, 0] = np.nan  # one column with a NaN
    return a


@pytest.mark.parametrize("method", qn.METHODS)
@pytest.mark.parametrize("dtype", [qn.F32, qn.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_quantiles_twin_reads_a_sample_axis_that_does_not_lead(shape, dtype, method):
    a = _sample(shape, dtype)
    got, want = twin_quantiles(a, which=4, axis=1, method=method), qn.quantiles(a, which=4, axis=1, method=method)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.isnan(want[:, -1, 0]).all() and np.isfinite(want).sum() == want.size - want.shape[0]
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("dtype", [gn.F32, gn.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gumbel_fit_twin_reads_a_sample_axis_that_does_not_lead(shape, dtype):
    a = _sample(shape, dtype)
    got, want = twin_fit(a, axis=1), gn.fit(a, axis=1)
    assert np.isnan(want[0][-1, 0]) and np.isfinite(want[0]).sum() == want[0].size - 1
    gn.judge_fit_exact(got, want, f"host twin against the restatement, {shape} axis 1")


@pytest.mark.parametrize("dtype", [en.F32, en.F64], ids=["f32", "f64"])
def test_crps_twin_flags_a_nan_member_and_a_nan_observation(dtype):
    """One point with a NaN member, one with a NaN observation, the rest clean; values against the restatement."""
    rng = np.random.default_rng(3)
    n, npts = 5, 7
    x, y = rng.normal(size=(n, npts)).astype(dtype), rng.normal(size=npts).astype(dtype)
    x[2, 1] = np.nan
    y[4] = np.nan
    p = np.arange(n + 1) / float(n)
    p2, q2 = np.ascontiguousarray(p**2), np.ascontiguousarray((1 - p) ** 2)
    out, flags = np.full(npts, 7.0), np.full(npts, 9, np.uint8)
    fn = getattr(_hosttwin.lib(), f"ekm_host_crps_from_ensemble_{'f32' if dtype == en.F32 else 'f64'}")
    fn.restype = C.c_int
    assert fn(_vp(x), _vp(y), C.c_uint(n), C.c_size_t(npts), _vp(p2), _vp(q2), _vp(out), _vp(flags)) == 0
    want, miss = en.crps(x, y)
    assert flags.tolist() == [0, 1, 0, 0, 1, 0, 0] and miss.tolist() == flags.astype(bool).tolist()
    assert out.tobytes() == np.asarray(want, np.float64).tobytes()
    out2 = np.full(npts, 7.0)  # without the flag array the values are the same
    assert fn(_vp(x), _vp(y), C.c_uint(n), C.c_size_t(npts), _vp(p2), _vp(q2), _vp(out2), None) == 0
    assert out2.tobytes() == out.tobytes()
