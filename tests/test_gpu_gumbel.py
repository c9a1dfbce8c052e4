"""stats.GumbelDistribution, value_to_return_period and return_period_to_value on the GPU: every golden case through the
public API with NumPy, DeviceArray and torch input, the raw entry points in a guarded arena over every layout, position
and layout independence of `fit`, a 65 536-point census at 51 samples against the NumPy restatement (which the CPU suite
pins to the recorded reference), the sample cap, a recorded graph and the argument errors.

fit, ppf and return_period_to_value are compared bit for bit with no point excluded; cdf within 8 * 2^-53 and
value_to_return_period within |ref| (8 * 2^-53 / cdf_ref + 4 * 2^-53) of the recorded reference, and the return period
equals freq / cdf of the same call bit for bit (tests/_gumbel_numpy.py)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _compare
import _gumbel_numpy as gn
from ekm_hip.stats import GumbelDistribution  # noqa: F401  (the class under test: absent before this feature)
from _arena import Arena, DeviceMemory

pytestmark = pytest.mark.gpu
FIT_CASES = gn.fit_cases()
CALLS = gn.call_cases("cdf", "ppf", "value_to_return_period", "return_period_to_value")
CAP = {gn.F32: 256, gn.F64: 128}  # samples whose sorted copy fits the kernels' 64 KiB of LDS per workgroup


def _want_fit(case):
    return gn.recorded_fit(case, "c") or gn.fit(gn.sample_of(case), case["plain"]["axis"])


def _run_call(ek, case, dist, arg):
    if case["func"] in ("cdf", "ppf"):
        return getattr(dist, case["func"])(arg)
    return getattr(ek.stats, case["func"])(dist, arg)


@pytest.mark.parametrize("case", FIT_CASES, ids=gn.case_id)
def test_fit_golden_cases_numpy_and_device_input(ek, case):
    sample, axis = gn.sample_of(case), case["plain"]["axis"]
    before = sample.copy()
    d = ek.stats.GumbelDistribution.fit(sample, axis=axis, freq=2.0)
    assert isinstance(d.mu, np.ndarray) and isinstance(d.sigma, np.ndarray) and d.freq == 2.0
    assert d.shape == _want_fit(case)[0].shape and d.ndim == len(d.shape)
    gn.judge_fit_exact((d.mu, d.sigma), _want_fit(case), "numpy " + case["note"])
    assert before.tobytes() == sample.tobytes()
    if sample.dtype in (gn.F32, gn.F64):
        dev = ek.DeviceArray.from_host(sample)
        dd = ek.stats.GumbelDistribution.fit(dev, axis)
        assert isinstance(dd.mu, ek.DeviceArray) and isinstance(dd.sigma, ek.DeviceArray) and dd.shape == d.shape
        gn.judge_fit_exact((dd.mu.to_host(), dd.sigma.to_host()), _want_fit(case), "device " + case["note"])
        assert np.array_equal(dev.to_host(), before, equal_nan=True)  # never sorted in place


@pytest.mark.parametrize("case", CALLS, ids=gn.case_id)
def test_call_golden_cases_numpy_and_device_input(ek, case):
    kw = gn.call_args(case)
    mu0, sigma0 = kw["mu"].copy(), kw["sigma"].copy()
    dist = ek.stats.GumbelDistribution(kw["mu"], kw["sigma"], freq=kw["freq"])
    if case["raises"]:  # a timedelta freq: the host forms the reference's own expression, which fails as it does there
        with pytest.raises(Exception) as info:
            _run_call(ek, case, dist, kw["arg"])
        assert type(info.value).__name__ == case["raises"][0], info.value
    else:
        got = _run_call(ek, case, dist, kw["arg"])
        if gn.is_timedelta_case(case) and case["func"] == "value_to_return_period":
            # timedelta / cdf: an array of timedelta objects (one timedelta for a scalar distribution), each rounded to
            # the resolution of a timedelta, one microsecond
            got = np.asarray(got)
            assert got.dtype == object and got.shape == gn.expected_of(case).shape
            sec, want = np.array([v.total_seconds() for v in got.reshape(-1)]), gn.expected_of(case).reshape(-1)
            cdf = gn.recorded_cdf_of(case).reshape(-1)
            assert (np.abs(sec - want) <= np.abs(want) * (gn.CDF_BOUND / cdf + 4 * gn.U) + 1e-6).all()
        else:
            assert isinstance(got, np.ndarray)
            gn.judge_call(case, got, "numpy " + gn.case_id(case), _compare.LEDGER)
            if case["func"] == "value_to_return_period":
                freq = 1.0 if kw["freq"] is None else float(kw["freq"])
                with np.errstate(all="ignore"):
                    gn.judge_exact(got, freq / dist.cdf(kw["arg"]), "the return period is freq / cdf of the same call")
    assert mu0.tobytes() == kw["mu"].tobytes() and sigma0.tobytes() == kw["sigma"].tobytes()
    # the same distribution on the device
    ddist = ek.stats.GumbelDistribution(ek.DeviceArray.from_host(np.atleast_1d(kw["mu"])), ek.DeviceArray.from_host(np.atleast_1d(kw["sigma"])),
                                        freq=kw["freq"])
    assert isinstance(ddist.mu, ek.DeviceArray) and ddist.mu.dtype == gn.F64
    if gn.is_timedelta_case(case):
        with pytest.raises(TypeError, match="timedelta"):
            _run_call(ek, case, ddist, kw["arg"])
    elif kw["mu"].ndim:  # (a DeviceArray has at least one axis: the scalar distribution stays a NumPy case)
        got = _run_call(ek, case, ddist, kw["arg"])
        assert isinstance(got, ek.DeviceArray) and got.dtype == gn.F64
        gn.judge_call(case, got.to_host(), "device " + gn.case_id(case), _compare.LEDGER)
        assert np.array_equal(ddist.mu.to_host(), np.broadcast_to(mu0, ddist.shape).astype(gn.F64), equal_nan=True)


def test_torch_device_tensors():
    """torch ROCm tensors in -> torch tensors out, every golden case; in a child process that imports torch first."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_gumbel_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    if r.returncode == 77:
        pytest.skip(r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "torch unavailable")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "GUMBEL_TORCH_OK" in r.stdout


def test_too_many_samples_is_an_error_not_a_wrong_answer(ek):
    for T in (gn.F32, gn.F64):
        for shape, axis in (((CAP[T] + 1, 5), 0), ((5, CAP[T] + 1), -1), ((2, CAP[T] + 1, 3), 1)):
            with pytest.raises(ek.EkmError, match=f"LDS.*{CAP[T]} members"):
                ek.stats.GumbelDistribution.fit(np.zeros(shape, T), axis)
        arr = np.random.default_rng(1).gumbel(20, 5, (70, CAP[T])).astype(T)  # the cap itself, sample axis last
        d = ek.stats.GumbelDistribution.fit(arr, -1)
        gn.judge_fit_exact((d.mu, d.sigma), gn.fit(arr, -1), "cap")


# ---- the raw entry points inside a guarded arena ----
def _arena_fit(tag, outer, m, inner, off, rng):
    from ekm_hip import _ffi

    lib = _ffi.lib()
    T = gn.F32 if tag == "f32" else gn.F64
    arr = np.round(rng.gumbel(20, 5, (outer, m, inner)) * 4) / 4 + 0.0  # ties
    arr[0, m // 2, 0] = np.nan
    arr = arr.astype(T)
    npts = outer * inner
    arena = Arena(DeviceMemory(0, None))
    o = [1, 3, 2] if off else [0] * 3
    try:
        arena.input("sample", arr, o[0])
        arena.output("mu", npts, gn.F64, o[1]), arena.output("sigma", npts, gn.F64, o[2])
        arena.commit()
        _ffi.check(getattr(lib, f"ekm_gumbel_fit_{tag}")(0, None, arena.ptr("sample"), outer, m, inner, arena.ptr("mu"), arena.ptr("sigma")))
        _ffi.check(lib.ekm_stream_sync(0, None))
        arena.check()  # guards and the input untouched, every element of mu and sigma written
        got = arena.result("mu").reshape(outer, inner), arena.result("sigma").reshape(outer, inner)
        gn.judge_fit_exact(got, gn.fit(arr, 1), f"fit {tag} [{outer}, {m}, {inner}] off {off}")
        return got
    finally:
        arena.free()


def _arena_outer(kind, mu, sigma, levels, freq, off):
    from ekm_hip import _ffi

    lib = _ffi.lib()
    npts, nlev = mu.size, levels.size
    arena = Arena(DeviceMemory(0, None))
    o = [1, 3, 2, 1] if off else [0] * 4
    try:
        arena.input("mu", mu, o[0]), arena.input("sigma", sigma, o[1]), arena.input("levels", levels, o[2])
        arena.output("out", nlev * npts, gn.F64, o[3])
        arena.commit()
        args = (0, None, arena.ptr("mu"), arena.ptr("sigma"), npts, arena.ptr("levels"), nlev)
        if kind == "ppf":
            _ffi.check(lib.ekm_gumbel_ppf_f64(*args, arena.ptr("out")))
        else:
            _ffi.check(lib.ekm_gumbel_cdf_f64(*args, freq, 0 if kind == "cdf" else 1, arena.ptr("out")))
        _ffi.check(lib.ekm_stream_sync(0, None))
        arena.check()
        return arena.result("out").reshape(nlev, npts)
    finally:
        arena.free()


LAYOUTS = [(npts, 1) for npts in (1, 63, 64, 65, 130)] + [(outer, inner) for inner in (3, 64, 70) for outer in (1, 3)]


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_fit_entry_points_in_a_guarded_arena(ek, tag):
    """npts in {1, 63, 64, 65, 130} with the sample axis last, inner in {3, 64, 70} x outer in {1, 3}, m in {2, 9, 51};
    buffers 16-B aligned and one to three elements off.  Nothing is written outside mu and sigma, the sample comes back
    unchanged, every output element is written, and the bits are the restatement's."""
    for outer, inner in LAYOUTS:
        for m in (2, 9, 51):
            runs = [_arena_fit(tag, outer, m, inner, off, np.random.default_rng(outer + m)) for off in (False, True)]
            gn.judge_fit_exact(runs[1], runs[0], "aligned against shifted buffers")


def test_cdf_and_ppf_entry_points_in_a_guarded_arena(ek):
    """npts in {1, 3, 63, 64, 65, 70, 130, 192, 210}, the point counts of the layouts above, nx in {1, 5}.

    The levels keep (mu - x) / sigma above -25, so every reference cdf here is above 1e-11.  The return-period bound
    |ref| (8 * 2^-53 / cdf_ref + 4 * 2^-53) is a first-order bound: it is finite, yet for 0 < cdf_ref <= 8 * 2^-53 a cdf
    that lies within the cdf's own bound of 8 * 2^-53 may be 0 and its return period inf.  With a level of 220 this test
    met that on the GPU: at exp((mu - x) / sigma) = 0.99 * 2^-54 a correctly rounded exp(-e) is 1 and the cdf 0 (the
    GPU's result, return period inf), NumPy's exp on the recording host gives 1 - 2^-53 (return period 2.25e16).  The far
    tail, cdf_ref == 0 included, is judged on the recorded cases (levels down to (mu - x) / sigma = -40), which pass."""
    rng = np.random.default_rng(7)
    for npts in sorted({o * i for o, i in LAYOUTS}):
        mu, sigma = 20.0 + rng.normal(0, 3, npts), 5.0 * np.exp(rng.normal(0, 0.2, npts))
        sigma[0] = np.nan
        for levels, probs in ((np.array([31.5]), np.array([0.99])), (np.array([75.0, 60.0, 31.5, 10.0, 0.0]), np.array([0.0, 1e-12, 0.5, 1 - 1e-12, 1.0]))):
            with np.errstate(all="ignore"):
                t = np.log(-np.log(1.0 - probs))
            for off in (False, True):
                what = f"npts {npts} nx {levels.size} off {off}"
                cdf = _arena_outer("cdf", mu, sigma, levels, 1.0, off)
                gn.judge_cdf(cdf, gn.cdf(mu, sigma, levels), "cdf " + what, _compare.LEDGER)
                rp = _arena_outer("rp", mu, sigma, levels, 2.5, off)
                with np.errstate(all="ignore"):
                    gn.judge_exact(rp, 2.5 / cdf, "return period = freq / cdf " + what)
                gn.judge_return_period(rp, gn.value_to_return_period(mu, sigma, 2.5, levels), gn.cdf(mu, sigma, levels), 2.5, "rp " + what, _compare.LEDGER)
                gn.judge_exact(_arena_outer("ppf", mu, sigma, t, 1.0, off), gn.ppf(mu, sigma, probs), "ppf " + what)


def test_entry_point_argument_errors(ek):
    from ekm_hip import _ffi

    lib = _ffi.lib()
    d = ek.DeviceArray.from_host(np.zeros(64, np.float32))
    d64 = ek.DeviceArray.from_host(np.ones(64))
    a, b = ek.DeviceArray.empty((64,), np.float64), ek.DeviceArray.empty((64,), np.float64)
    ARG, ENUM, OK = _ffi.EKM_ERR_ARG, _ffi.EKM_ERR_ENUM, _ffi.EKM_OK
    assert lib.ekm_gumbel_fit_f32(0, None, d.ptr, 8, 1, 1, a.ptr, b.ptr) == ARG            # fewer than two samples
    assert lib.ekm_gumbel_fit_f32(0, None, None, 8, 8, 1, a.ptr, b.ptr) == ARG
    assert lib.ekm_gumbel_fit_f32(0, None, d.ptr, 8, 8, 1, None, b.ptr) == ARG
    assert lib.ekm_gumbel_fit_f32(0, None, d.ptr, 8, 8, 1, a.ptr, b.ptr + 4) == ARG        # misaligned
    assert lib.ekm_gumbel_fit_f32(0, None, d.ptr + 2, 8, 8, 1, a.ptr, b.ptr) == ARG
    assert lib.ekm_gumbel_fit_f64(0, None, d64.ptr, 1, 129, 1, a.ptr, b.ptr) == ARG and b"LDS" in lib.ekm_last_error()
    assert lib.ekm_gumbel_fit_f32(0, None, None, 0, 8, 1, None, None) == OK                # no points
    assert lib.ekm_gumbel_cdf_f64(0, None, d64.ptr, d64.ptr, 8, d64.ptr, 2, 1.0, 2, a.ptr) == ENUM
    assert lib.ekm_gumbel_cdf_f64(0, None, None, d64.ptr, 8, d64.ptr, 2, 1.0, 0, a.ptr) == ARG
    assert lib.ekm_gumbel_cdf_f64(0, None, d64.ptr, d64.ptr, 8, d64.ptr, 2, 1.0, 0, None) == ARG
    assert lib.ekm_gumbel_cdf_f64(0, None, d64.ptr, d64.ptr + 4, 8, d64.ptr, 2, 1.0, 1, a.ptr) == ARG
    assert lib.ekm_gumbel_cdf_f64(0, None, None, None, 0, None, 2, 1.0, 0, None) == OK     # no points
    assert lib.ekm_gumbel_cdf_f64(0, None, None, None, 8, None, 0, 1.0, 0, None) == OK     # no levels
    assert lib.ekm_gumbel_ppf_f64(0, None, d64.ptr, d64.ptr, 8, None, 2, a.ptr) == ARG
    assert lib.ekm_gumbel_ppf_f64(0, None, d64.ptr, d64.ptr, 8, d64.ptr + 4, 2, a.ptr) == ARG
    assert lib.ekm_gumbel_ppf_f64(0, None, None, None, 8, None, 0, None) == OK
    ek.synchronize()


@pytest.mark.parametrize("T", [gn.F32, gn.F64], ids=["f32", "f64"])
def test_a_column_gives_the_same_bits_at_any_position_and_in_any_layout(ek, T):
    rng = np.random.default_rng(11)
    cols = (np.round(rng.gamma(1.5, 2.0, (51, 130)) * 8) / 8).astype(T)
    cols[3, 5], cols[0, 64], cols[50, 129] = np.nan, np.inf, -np.inf
    fit = lambda a, axis: (lambda d: (d.mu, d.sigma))(ek.stats.GumbelDistribution.fit(a, axis))  # noqa: E731
    first = fit(cols, 0)
    gn.judge_fit_exact(first, gn.fit(cols, 0), "axis 0")
    last = np.ascontiguousarray(cols.T)
    gn.judge_fit_exact(fit(last, -1), first, "axis -1")
    mid = np.ascontiguousarray(cols.reshape(51, 2, 65).transpose(1, 0, 2))
    gn.judge_fit_exact(tuple(a.reshape(130) for a in fit(mid, 1)), first, "axis 1")
    for n in (1, 64, 65, 1027):
        pick = rng.integers(0, 130, n)
        gn.judge_fit_exact(fit(cols[:, pick], 0), tuple(a[pick] for a in first), f"picked {n} axis 0")
        gn.judge_fit_exact(fit(last[pick], 1), tuple(a[pick] for a in first), f"picked {n} axis -1")


# ---- census ----
@functools.lru_cache(maxsize=None)
def _census_field(name):
    rng = np.random.default_rng(2026)
    a = np.maximum(rng.gamma(1.5, 2.0, (51, 1 << 16)).astype(np.float32) - np.float32(1.0), 0)  # zero-clamped: ties
    a = (np.round(a * 64) / 64).astype(name)
    a[7, ::1001] = np.nan
    a[9, 5::4099] = np.inf
    a[11, 7::5003] = -np.inf
    return a


@functools.lru_cache(maxsize=None)
def _census_want(name):
    return gn.fit(_census_field(name), 0)


@pytest.mark.parametrize("axis", [0, -1])
@pytest.mark.parametrize("T", [gn.F32, gn.F64], ids=["f32", "f64"])
def test_census_51_samples_on_65536_points(ek, T, axis):
    field, want = _census_field(T.name), _census_want(T.name)
    d = ek.stats.GumbelDistribution.fit(field if axis == 0 else np.ascontiguousarray(field.T), axis)
    equal = gn.equal_bits(d.mu, want[0]) + gn.equal_bits(d.sigma, want[1])
    line = f"gumbel fit census {T.name} axis {axis}: {equal} of {2 * d.mu.size} values equal bits, {int(np.isnan(d.mu).sum())} NaN mu"
    _compare.CENSUS.append(line)
    print(line)
    assert 0 < np.isnan(d.mu).sum() < d.mu.size
    gn.judge_fit_exact((d.mu, d.sigma), want, line)


def test_recorded_graph_replays_the_direct_calls(ek):
    rng = np.random.default_rng(3)
    arr = rng.gumbel(20, 5, (51, 5000))
    d_first, d_last = ek.to_device(arr.astype(np.float32)), ek.to_device(np.ascontiguousarray(arr.T))
    levels, probs, rps = [60.0, 31.5, 10.0], [0.5, 0.99], [10.0, 100.0]

    def run():
        a, b = ek.stats.GumbelDistribution.fit(d_first, 0, freq=2.0), ek.stats.GumbelDistribution.fit(d_last, -1)
        return [a.mu, a.sigma, b.mu, b.sigma, a.cdf(levels), b.ppf(probs), ek.stats.value_to_return_period(a, levels),
                ek.stats.return_period_to_value(a, rps)]

    direct = [o.to_host() for o in run()]  # also uploads the level tables, which a recording cannot
    with ek.graph() as g:
        outs = run()
    g.launch()
    for o, want in zip(outs, direct):
        gn.judge_exact(o.to_host(), want, "graph replay")
    g.close()
    gn.judge_fit_exact(direct[:2], gn.fit(arr.astype(np.float32), 0), "direct f32")
    gn.judge_fit_exact(direct[2:4], gn.fit(arr, 0), "direct f64")
    gn.judge_exact(direct[5], gn.ppf(direct[2], direct[3], probs), "direct ppf")
    gn.judge_exact(direct[7], gn.return_period_to_value(direct[0], direct[1], 2.0, rps), "direct return_period_to_value")
    gn.judge_cdf(direct[4], gn.cdf(direct[0], direct[1], levels), "direct cdf", _compare.LEDGER)
    with np.errstate(all="ignore"):
        gn.judge_exact(direct[6], 2.0 / direct[4], "direct return period = freq / cdf")
