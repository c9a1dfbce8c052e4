"""Ensemble reductions on the GPU (ekm_hip.extreme, ekm_hip.score): every golden case through the public API with NumPy,
DeviceArray and torch input, a 262 144-point census at 101 x 51 against the NumPy restatement, the raw entry points in
a guarded arena, position independence and a recorded graph.  Every comparison is bit for bit with no point excluded,
except the documented mixed-dtype deviation of efi (bound derived in tests/_ensemble_numpy.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _compare
import _ensemble_numpy as en
from ekm_hip import extreme, score  # noqa: F401  (the modules under test: absent before this feature)
from _arena import UNWRITTEN, Arena, DeviceMemory

pytestmark = pytest.mark.gpu
VALUE_CASES = [c for c in en.cases() if not c["raises"]]
CAP = {en.F32: 256, en.F64: 128}  # members whose sorted copy fits the kernels' 64 KiB of LDS per workgroup


def product(ek, func):
    return ek.score.crps_from_ensemble if func == "crps_from_ensemble" else getattr(ek.extreme, func)


def judge(ek, case, got, what):
    """Against the recorded reference; EFI only when this host's coefficient tables are the recorded ones -- with another
    libm the message says so and the restatement with the product's own tables is the reference, still in bits."""
    if case["func"] == "efi" and not en.is_mixed_efi(case):
        kw = en.kwargs_of(case)
        nclim = kw["clim"].shape[0]
        own = ek.extreme.efi_coefficients(nclim)
        if not all(np.array_equal(a, b) for a, b in zip(own, en.recorded_tables(nclim))):
            return en.judge_exact(got, en.efi(**kw, tables=own), what + " [EFI coefficients of this host differ from the "
                                  "recorded ones (another libm): judged against the restatement with the product's tables]")
    en.judge_case(case, got, what, _compare.LEDGER)


@pytest.mark.parametrize("case", VALUE_CASES, ids=en.case_id)
def test_golden_cases_numpy_input(ek, case):
    got = product(ek, case["func"])(**en.kwargs_of(case))
    assert isinstance(got, np.ndarray)
    judge(ek, case, got, "numpy " + case["note"])


def _float_arrays_on_device(ek, kw):
    return {k: (ek.DeviceArray.from_host(v) if isinstance(v, np.ndarray) and v.dtype in (en.F32, en.F64) else v)
            for k, v in kw.items()}


@pytest.mark.parametrize("case", VALUE_CASES, ids=en.case_id)
def test_golden_cases_device_array_input(ek, case):
    got = product(ek, case["func"])(**_float_arrays_on_device(ek, en.kwargs_of(case)))
    assert isinstance(got, ek.DeviceArray)
    judge(ek, case, got.to_host(), "device " + case["note"])


def test_torch_device_tensors():
    """torch ROCm tensors in -> torch tensors out, every golden case; in a child process that imports torch first."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_ensemble_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    if r.returncode == 77:
        pytest.skip(r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "torch unavailable")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ENSEMBLE_TORCH_OK" in r.stdout


def test_raise_policy_on_device_input(ek):
    case = next(c for c in en.cases() if c["raises"] and "nan inf raise" in c["note"])
    with pytest.raises(ValueError, match="Missing values present in input and nan_policy=raise"):
        ek.score.crps_from_ensemble(**_float_arrays_on_device(ek, en.kwargs_of(case)))


def test_too_many_members_is_an_error_not_a_wrong_answer(ek):
    for T in (en.F32, en.F64):
        n = CAP[T] + 1
        with pytest.raises(ek.EkmError, match="LDS"):
            ek.extreme.efi(np.zeros((11, 5), T), np.zeros((n, 5), T))
        with pytest.raises(ek.EkmError, match="LDS"):
            ek.score.crps_from_ensemble(np.zeros((n, 5), T), np.zeros(5, T))
        with pytest.raises(ek.EkmError, match="LDS"):
            ek.extreme.sot(np.zeros((101, 5), T), np.zeros((n, 5), T), 90)


# ---- census ----
def _field(rng, rows, n, T, sort):
    a = np.maximum(rng.gamma(1.5, 2.0, (rows, n)).astype(np.float32) - np.float32(1.0), 0)  # zero-clamped: ties
    a = np.round(a * 64) / 64
    return (np.sort(a, axis=0) if sort else a).astype(T)


@pytest.fixture(scope="module")
def census_fields():
    rng = np.random.default_rng(2026)
    n = 1 << 18
    clim, ens = _field(rng, 101, n, np.float64, True), _field(rng, 51, n, np.float64, False)
    clim = clim + np.linspace(0, 0.5, 101)[:, None]
    y = ens[rng.integers(0, 51, n), np.arange(n)] + np.where(rng.random(n) < 0.5, 0.0, rng.normal(0, 2, n))
    ens[7, ::1001] = np.nan
    return clim, ens, y


@pytest.mark.parametrize("T", [en.F32, en.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("func", ["efi", "efi_eps", "sot", "crps"])
def test_census_101x51_on_262144_points(ek, census_fields, T, func):
    clim, ens, y = (a.astype(T) for a in census_fields)
    if func == "efi":
        got, want = ek.extreme.efi(clim, ens), en.efi(clim, ens, tables=ek.extreme.efi_coefficients(101))
    elif func == "efi_eps":
        got, want = ek.extreme.efi(clim, ens, eps=0.25), en.efi(clim, ens, 0.25, tables=ek.extreme.efi_coefficients(101))
    elif func == "sot":
        got, want = ek.extreme.sot(clim, ens, 90, eps=0.25), en.sot(clim, ens, 90, eps=0.25)
    else:
        got, want = ek.score.crps_from_ensemble(ens, y), en.crps_from_ensemble(ens, y)
    equal = en.equal_bits(got, want)
    line = f"ensemble census {T.name} {func}: {equal} of {got.size} points equal bits, {int(np.isnan(got).sum())} NaN"
    _compare.CENSUS.append(line)
    print(line)
    assert got.dtype == want.dtype and 0 < np.isnan(got).sum() < got.size
    en.judge_exact(got, want, line)


# ---- the raw entry points inside a guarded arena ----
def _arena_run(ek, func, T, npts, nens, nclim, off, rng):
    from ekm_hip import _ffi

    lib, tag = _ffi.lib(), "f32" if T == en.F32 else "f64"
    arena = Arena(DeviceMemory(0, None))
    o = [1, 3, 1, 2, 3] if off else [0] * 5
    ens = _field(rng, nens, npts, T, False)
    try:
        if func == "efi":
            clim = _field(rng, nclim, npts, T, True)
            tabs = [t if t.size else np.zeros(1) for t in en.efi_tables(nclim)]
            arena.input("clim", clim, o[0]), arena.input("ens", ens, o[1])
            for k, t in enumerate(tabs):
                arena.input(f"t{k}", t, o[2])
            arena.output("out", npts, np.float64, o[3])
            arena.commit()
            rc = getattr(lib, f"ekm_efi_{tag}")(0, None, arena.ptr("clim"), arena.ptr("ens"), nclim, nens, npts, 0.25,
                                               arena.ptr("t0"), arena.ptr("t1"), arena.ptr("t2"), arena.ptr("out"))
            want = en.efi(clim, ens, 0.25)
        elif func == "sot":
            qc, tail = _field(rng, 1, npts, T, False)[0], _field(rng, 1, npts, T, False)[0] + T.type(0.5)
            arena.input("qc", qc, o[0]), arena.input("tail", tail, o[2]), arena.input("ens", ens, o[1])
            arena.output("out", npts, T, o[3])
            arena.commit()
            rc = getattr(lib, f"ekm_sot_{tag}")(0, None, arena.ptr("qc"), arena.ptr("tail"), arena.ptr("ens"), nens, npts, 90,
                                               0.25, arena.ptr("out"))
            clim = np.zeros((101, npts), T)
            clim[90], clim[99] = qc, tail
            want = en.sot(clim, ens, 90, eps=0.25)
        else:
            y = (ens[0] + rng.normal(0, 1, npts)).astype(T)
            y[::5] = np.nan
            p = np.arange(nens + 1) / float(nens)
            arena.input("x", ens, o[1]), arena.input("y", y, o[0])
            arena.input("p2", p**2, o[2]), arena.input("q2", (1 - p) ** 2, o[2])
            arena.output("out", npts, np.float64, o[3])
            arena.output("missing", (npts + 3) // 4, np.uint32, 0)
            arena.commit()
            rc = getattr(lib, f"ekm_crps_from_ensemble_{tag}")(0, None, arena.ptr("x"), arena.ptr("y"), nens, npts,
                                                              arena.ptr("p2"), arena.ptr("q2"), arena.ptr("out"), arena.ptr("missing"))
            want, miss = en.crps(ens, y)
        if nens > CAP[T]:
            assert rc == _ffi.EKM_ERR_ARG and b"LDS" in lib.ekm_last_error()
            _ffi.check(lib.ekm_stream_sync(0, None))
            with pytest.raises(AssertionError, match="never written"):  # nothing ran: the outputs still hold the fill
                arena.check()
            return None
        _ffi.check(rc)
        _ffi.check(lib.ekm_stream_sync(0, None))
        arena.check()
        got = arena.result("out")
        en.judge_exact(got, want, f"{func} {tag} npts {npts} nens {nens} nclim {nclim} off {off}")
        if func == "crps":
            flags = arena.result("missing").view(np.uint8)
            assert np.array_equal(flags[:npts], miss.astype(np.uint8))
            assert np.array_equal(flags[npts:], np.array([UNWRITTEN], np.uint32).view(np.uint8)[npts % 4:][:flags.size - npts])
        return got
    finally:
        arena.free()


@pytest.mark.parametrize("T", [en.F32, en.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("func", ["efi", "sot", "crps"])
def test_entry_points_in_a_guarded_arena(ek, func, T):
    """Every npts of the list at 51 members, every member count (the cap and the cap + 1, which must return the error
    code and write nothing) at 257 points, every nclim at 65 points; buffers 16-B aligned and one to three elements
    off: guard words and inputs untouched, every output element written, the restatement's bits."""
    shapes = [(npts, 51, 11) for npts in (1, 63, 64, 65, 255, 257, 1023, 4097)]
    shapes += [(257, nens, 11) for nens in (1, 2, 7, 64, CAP[T], CAP[T] + 1)]
    shapes += [(65, 7, nclim) for nclim in (2, 101)] if func == "efi" else []
    for npts, nens, nclim in shapes:
        a = _arena_run(ek, func, T, npts, nens, nclim, False, np.random.default_rng(npts + nens))
        b = _arena_run(ek, func, T, npts, nens, nclim, True, np.random.default_rng(npts + nens))
        if a is not None:
            en.judge_exact(b, a, "aligned against shifted buffers")


@pytest.mark.parametrize("T", [en.F32, en.F64], ids=["f32", "f64"])
def test_sot_func_in_a_guarded_arena(ek, T):
    from ekm_hip import _ffi

    lib, tag = _ffi.lib(), "f32" if T == en.F32 else "f64"
    for n in (1, 63, 255, 257, 4097):
        for off in (0, 1):
            rng = np.random.default_rng(n)
            q = rng.normal(0, 1, (3, n)).astype(T)
            q[1, ::7] = q[0, ::7]
            arena = Arena(DeviceMemory(0, None))
            try:
                arena.input("a", q[0], off), arena.input("b", q[1], 3 * off), arena.input("c", q[2], 2 * off)
                arena.output("out", n, T, off)
                arena.commit()
                _ffi.check(getattr(lib, f"ekm_sot_func_{tag}")(0, None, arena.ptr("a"), arena.ptr("b"), arena.ptr("c"), n, 1e-3,
                                                              -2.0, 3.0, arena.ptr("out")))
                _ffi.check(lib.ekm_stream_sync(0, None))
                arena.check()
                en.judge_exact(arena.result("out"), en.sot_func(q[0], q[1], q[2], 1e-3, -2.0, 3.0), f"sot_func {tag} {n}")
            finally:
                arena.free()


@pytest.mark.parametrize("T", [en.F32, en.F64], ids=["f32", "f64"])
def test_a_column_gives_the_same_bits_at_any_position(ek, T):
    """13 distinct columns tiled over fields of several lengths: every copy of a column, in whatever lane and workgroup
    it lands and whatever its wave-mates hold, gives the bits of the first copy.  (The launch shape is a constexpr: there
    is no tuning value to vary.)"""
    rng = np.random.default_rng(11)
    clim, ens = _field(rng, 101, 13, T, True), _field(rng, 51, 13, T, False)
    ens[3, 5], clim[40, 9] = np.nan, np.nan
    y = ens[0].copy()
    first = None
    for n in (13, 64, 65, 1027, 70001):
        pick = np.arange(n) % 13 if n < 2000 else rng.integers(0, 13, n)
        got = (ek.extreme.efi(clim[:, pick], ens[:, pick]), ek.extreme.efi(clim[:, pick], ens[:, pick], eps=0.5),
               ek.extreme.sot(clim[:, pick], ens[:, pick], 10, eps=0.5), ek.score.crps_from_ensemble(ens[:, pick], y[pick]))
        if first is None:
            first = [g.copy() for g in got]
        for g, f in zip(got, first):
            en.judge_exact(g, f[pick], f"n = {n}")


@pytest.mark.parametrize("T", [en.F32, en.F64], ids=["f32", "f64"])
def test_recorded_graph_replays_the_direct_call(ek, T):
    rng = np.random.default_rng(3)
    clim, ens = _field(rng, 101, 5000, T, True), _field(rng, 51, 5000, T, False)
    d_clim, d_ens, d_y = ek.to_device(clim), ek.to_device(ens), ek.to_device(ens[1].copy())
    direct = [ek.extreme.efi(d_clim, d_ens).to_host(), ek.extreme.sot(d_clim, d_ens, 90).to_host(),
              ek.score.crps_from_ensemble(d_ens, d_y).to_host()]  # also uploads the coefficient tables, which a recording cannot
    with ek.graph() as g:
        outs = (ek.extreme.efi(d_clim, d_ens), ek.extreme.sot(d_clim, d_ens, 90), ek.score.crps_from_ensemble(d_ens, d_y))
    g.launch()
    for o, want in zip(outs, direct):
        en.judge_exact(o.to_host(), want, "graph replay")
    en.judge_exact(direct[0], en.efi(clim, ens, tables=ek.extreme.efi_coefficients(101)), "direct")
    g.close()
