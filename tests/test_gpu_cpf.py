"""Crossing Point Forecast on the GPU (ekm_hip.extreme.cpf): every golden case through the public API with NumPy,
DeviceArray and torch input, a 65 536-point census at 101 x 51 against the NumPy restatement, the raw entry points in a
guarded arena, position independence and a recorded graph.  Every comparison is bit for bit with no point excluded,
except the documented mixed-dtype deviation (clim f32, ens f64; bound derived in tests/_cpf_numpy.py)."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import _compare
import _cpf_numpy as cn
import _ensemble_numpy as en
from ekm_hip import extreme  # noqa: F401
from _arena import Arena, DeviceMemory

pytestmark = pytest.mark.gpu
CASES = cn.cases()
ROWS_CAP = {cn.F32: 640, cn.F64: 320}  # LDS rows (members, plus climate rows when they are sorted) in 160 KiB


def judge(case, got, what):
    want = cn.expected_of(case)
    if not cn.is_mixed_clim_f32(case):
        return en.judge_exact(got, want, what)
    kw = cn.kwargs_of(case)
    bound = cn.mixed_cpf_bound(kw["clim"], kw["ens"], **cn.options_of(case))
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), what
    err = np.where(np.isnan(want), 0.0, np.abs(got.astype(np.float64) - want.astype(np.float64)))
    _compare.LEDGER.append((what, "cpf mixed-dtype bound", float(np.max(err / np.maximum(bound, 1e-300), initial=0.0)), 1.0, err.size))
    assert (err <= bound).all(), what


# One test walks all recorded cases (a failure names its case): 441 parametrised items would cost the suite more in
# per-item overhead than the launches themselves take.
def test_golden_cases_numpy_input(ek):
    for case in CASES:
        kw = cn.kwargs_of(case)
        before = {k: v.copy() for k, v in kw.items() if isinstance(v, np.ndarray)}
        got = ek.extreme.cpf(**kw)
        assert isinstance(got, np.ndarray), case["id"]
        judge(case, got, "numpy " + cn.case_id(case))
        assert all(np.array_equal(kw[k], v, equal_nan=True) for k, v in before.items()), case["id"]


def test_golden_cases_device_array_input(ek):
    for case in CASES:
        kw = cn.kwargs_of(case)
        dev = {k: (ek.DeviceArray.from_host(v) if isinstance(v, np.ndarray) and v.dtype in (cn.F32, cn.F64) else v) for k, v in kw.items()}
        got = ek.extreme.cpf(**dev)
        assert isinstance(got, ek.DeviceArray), case["id"]
        judge(case, got.to_host(), "device " + cn.case_id(case))
        for k, v in dev.items():  # the kernel sorts in LDS: the device inputs are as uploaded
            if isinstance(v, ek.DeviceArray):
                assert np.array_equal(v.to_host(), kw[k], equal_nan=True), (case["id"], k)
                v.free()
        got.free()


def test_torch_device_tensors():
    """torch ROCm tensors in -> torch tensors out, every golden case; in a child process that imports torch first."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_cpf_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    if r.returncode == 77:
        pytest.skip(r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "torch unavailable")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "CPF_TORCH_OK" in r.stdout


def test_too_many_rows_is_an_error_not_a_wrong_answer(ek):
    for T in (cn.F32, cn.F64):
        cap = ROWS_CAP[T]
        with pytest.raises(ek.EkmError, match="LDS"):
            ek.extreme.cpf(np.zeros((11, 5), T), np.zeros((cap - 10, 5), T))
        with pytest.raises(ek.EkmError, match="LDS"):
            ek.extreme.cpf(np.zeros((11, 5), T), np.zeros((cap + 1, 5), T), sort_clim=False)
        assert ek.extreme.cpf(np.zeros((11, 5), T), np.zeros((cap, 5), T), sort_clim=False).shape == (5,)
    with pytest.raises(ValueError):
        ek.extreme.cpf(np.zeros((101, 2, 2)), np.zeros((51, 2, 2)))


# ---- census ----
N_CENSUS = 1 << 16
CENSUS_OPTIONS = {"default": {}, "from_zero": dict(from_zero=True), "symmetric": dict(symmetric=True), "epsilon": dict(epsilon=0.5)}


@pytest.fixture(scope="module")
def census_fields():
    """A N(0, 3) climate against a forecast of the same spread shifted per point by N(0, 2), on a 1/16 grid so that
    members meet climate rows.  (The lower-tail interpolation happens only with from_zero, where the two lowest members
    lie between climate rows 2 and 3.)  A few columns are sown with a NaN."""
    rng = np.random.default_rng(2026)
    n = N_CENSUS
    clim = np.sort(np.round(rng.normal(0, 3, (101, n)) * 16) / 16 + 0.0, axis=0)
    ens = np.round((rng.normal(0, 3, (51, n)) + rng.normal(0, 2, n)) * 16) / 16 + 0.0
    ens[9, 5::1001] = np.nan
    clim[50, 17::1501] = np.nan
    return clim, ens


@pytest.fixture(scope="module")
def census_reference(census_fields):
    """The restatement's results, computed once per (dtype, option) and shared."""
    cache = {}

    def get(T, option):
        if (T, option) not in cache:
            clim, ens = (a.astype(T) for a in census_fields)
            cache[T, option] = cn.cpf_with_kinds(clim, ens, **CENSUS_OPTIONS[option])
        return cache[T, option]
    return get


@pytest.fixture(scope="module")
def census_device_fields(census_fields):
    """The census fields on the device, uploaded once per dtype and shared by the four options."""
    cache = {}

    def get(ek, T):
        if T not in cache:
            cache[T] = tuple(ek.to_device(a.astype(T)) for a in census_fields)
        return cache[T]
    yield get
    for pair in cache.values():
        for d in pair:
            d.free()


@pytest.mark.parametrize("T", [cn.F32, cn.F64], ids=["f32", "f64"])
def test_census_field_exercises_every_write(census_reference, T):
    """Counted in the restatement alone: each of the three writes decides at least 100 points, at least 30 % of the
    results lie strictly between 0 and 1."""
    counts = {}
    for option in ("default", "from_zero"):
        value, kind, _ = census_reference(T, option)
        counts[option] = {name: int((kind == k).sum()) for name, k in (("lower", cn.LOWER), ("plain", cn.PLAIN), ("upper", cn.UPPER))}
        inside = float(np.mean((value > 0) & (value < 1)))
        print(f"cpf census field {T.name} {option}: {counts[option]}, {100 * inside:.1f} % strictly inside (0, 1)")
        assert inside >= 0.30
    assert counts["from_zero"]["lower"] >= 100
    assert min(counts["default"]["plain"], counts["from_zero"]["plain"]) >= 100
    assert min(counts["default"]["upper"], counts["from_zero"]["upper"]) >= 100


@pytest.mark.parametrize("T", [cn.F32, cn.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("option", list(CENSUS_OPTIONS))
def test_census_101x51_on_65536_points(ek, census_device_fields, census_reference, T, option):
    got = ek.extreme.cpf(*census_device_fields(ek, T), **CENSUS_OPTIONS[option]).to_host()
    want = census_reference(T, option)[0]
    equal = en.equal_bits(got, want)
    line = f"cpf census {T.name} {option}: {equal} of {got.size} points equal bits, {int((got != 0).sum())} non-zero"
    _compare.CENSUS.append(line)
    print(line)
    en.judge_exact(got, want, line)


# ---- the raw entry points inside a guarded arena ----
def _field(rng, rows, n, T, sort):
    a = np.round(rng.normal(0, 3, (rows, n)) * 16) / 16 + 0.0
    return (np.sort(a, axis=0) if sort else a).astype(T)


def _arena_run(ek, T, npts, nens, nclim, off, rng, sort_clim=True, sort_ens=True, from_zero=False, symmetric=False, epsilon=None):
    from ekm_hip import _ffi

    lib, tag = _ffi.lib(), "f32" if T == cn.F32 else "f64"
    arena = Arena(DeviceMemory(0, None))
    o = [1, 3, 2] if off else [0, 0, 0]
    clim = _field(rng, nclim, npts, T, False)
    ens = _field(rng, nens, npts, T, False) + _field(rng, 1, npts, T, False)
    ens[nens // 2, ::97] = np.nan
    try:
        arena.input("clim", clim, o[0]), arena.input("ens", ens, o[1])
        arena.output("out", npts, np.float32, o[2])
        arena.commit()
        rc = getattr(lib, f"ekm_cpf_{tag}")(0, None, arena.ptr("clim"), arena.ptr("ens"), nclim, nens, npts, int(sort_clim),
                                           int(sort_ens), int(from_zero), int(symmetric), int(epsilon is not None),
                                           0.0 if epsilon is None else epsilon, arena.ptr("out"))
        what = f"cpf {tag} npts {npts} nens {nens} nclim {nclim} off {off} flags {sort_clim, sort_ens, from_zero, symmetric, epsilon}"
        if nens + (nclim if sort_clim else 0) > ROWS_CAP[T]:
            assert rc == _ffi.EKM_ERR_ARG and b"LDS" in lib.ekm_last_error(), what
            _ffi.check(lib.ekm_stream_sync(0, None))
            with pytest.raises(AssertionError, match="never written"):  # nothing ran: the outputs still hold the fill
                arena.check()
            return None
        _ffi.check(rc)
        _ffi.check(lib.ekm_stream_sync(0, None))
        arena.check()
        got = arena.result("out")
        en.judge_exact(got, cn.cpf(clim, ens, sort_clim, sort_ens, None if symmetric else epsilon, symmetric, from_zero), what)
        return got
    finally:
        arena.free()


@pytest.mark.parametrize("T", [cn.F32, cn.F64], ids=["f32", "f64"])
def test_entry_points_in_a_guarded_arena(ek, T):
    """Every npts of the list at 11 x 51, every member count (the cap and the cap + 1, which must return the error code
    and write nothing) at 257 points, every nclim at 65 points; buffers 16-B aligned and one to three elements off:
    guard words and inputs untouched, every output element written, the restatement's bits."""
    cap = ROWS_CAP[T] - 11
    shapes = [(npts, 51, 11) for npts in (1, 63, 64, 65, 255, 257, 1023, 4097)]
    shapes += [(257, nens, 11) for nens in (1, 2, 3, 7, 64, cap, cap + 1)]
    shapes += [(65, 7, nclim) for nclim in (3, 101)]
    for npts, nens, nclim in shapes:
        a = _arena_run(ek, T, npts, nens, nclim, False, np.random.default_rng(npts + nens), from_zero=True, symmetric=nens < 100)
        b = _arena_run(ek, T, npts, nens, nclim, True, np.random.default_rng(npts + nens), from_zero=True, symmetric=nens < 100)
        if a is not None:
            en.judge_exact(b, a, "aligned against shifted buffers")


@pytest.mark.parametrize("T", [cn.F32, cn.F64], ids=["f32", "f64"])
def test_every_flag_combination_in_a_guarded_arena(ek, T):
    for k, (sort_clim, sort_ens, from_zero, symmetric, epsilon) in enumerate(
            itertools.product((True, False), (True, False), (False, True), (False, True), (None, 0.5))):
        _arena_run(ek, T, 257, 51, 101, bool(k % 2), np.random.default_rng(5), sort_clim, sort_ens, from_zero, symmetric, epsilon)


@pytest.mark.parametrize("T", [cn.F32, cn.F64], ids=["f32", "f64"])
def test_a_column_gives_the_same_bits_at_any_position(ek, T):
    """13 distinct columns tiled over fields of several lengths: every copy of a column, in whatever lane and workgroup
    it lands and whatever its wave-mates hold, gives the bits of the first copy."""
    rng = np.random.default_rng(11)
    clim, ens = _field(rng, 101, 13, T, True), _field(rng, 51, 13, T, False) + _field(rng, 1, 13, T, False)
    ens[3, 5], clim[40, 9] = np.nan, np.nan
    first = None
    for n in (13, 64, 65, 1027, 70001):
        pick = np.arange(n) % 13 if n < 2000 else rng.integers(0, 13, n)
        got = (ek.extreme.cpf(clim[:, pick], ens[:, pick]), ek.extreme.cpf(clim[:, pick], ens[:, pick], symmetric=True, from_zero=True),
               ek.extreme.cpf(clim[:, pick], ens[:, pick], sort_clim=False, epsilon=0.5))
        if first is None:
            first = [g.copy() for g in got]
            en.judge_exact(first[1], cn.cpf(clim, ens, symmetric=True, from_zero=True), "first copy")
        for g, f in zip(got, first):
            en.judge_exact(g, f[pick], f"n = {n}")


@pytest.mark.parametrize("T", [cn.F32, cn.F64], ids=["f32", "f64"])
def test_recorded_graph_replays_the_direct_call(ek, T):
    rng = np.random.default_rng(3)
    clim, ens = _field(rng, 101, 5000, T, True), _field(rng, 51, 5000, T, False) + _field(rng, 1, 5000, T, False)
    d_clim, d_ens = ek.to_device(clim), ek.to_device(ens)
    direct = [ek.extreme.cpf(d_clim, d_ens).to_host(), ek.extreme.cpf(d_clim, d_ens, symmetric=True, from_zero=True).to_host()]
    with ek.graph() as g:
        outs = (ek.extreme.cpf(d_clim, d_ens), ek.extreme.cpf(d_clim, d_ens, symmetric=True, from_zero=True))
    g.launch()
    for o, want in zip(outs, direct):
        en.judge_exact(o.to_host(), want, "graph replay")
    en.judge_exact(direct[0], cn.cpf(clim, ens), "direct")
    g.close()
