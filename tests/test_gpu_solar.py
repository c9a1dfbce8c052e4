"""Solar functions on the GPU (ekm_hip.solar): every golden case through the public API with NumPy, DeviceArray and
torch input, a 65 536-point census per input dtype and function against the NumPy restatement, the raw entry points in
a guarded arena, position independence, a recorded graph, and the kernel against its host twin.

Every comparison uses the absolute bar B(N) derived in tests/_solar_numpy.py (at most 1e-13; times max(isr) for the
radiation; plus one f32 rounding where the result is f32), the same NaN pattern, no point excluded; the sign of zero is
not compared.  For f32 input the judge is the reference's run on the upcast inputs.

B(N) = (94.3 + N) * 2^-53 for N time nodes: 60.5 u for the reference's own float64 run (47.3 u of it the roundings of
its hour angle at |lon| <= 720), 31.8 u for the kernel (four sines / cosines at 1 ulp = 2 u each, the host-made node
angle, three products and two fma), 2 u for the products of the accumulation and N u for the running sums of both
sides; the derivation, term by term, is the docstring of tests/_solar_numpy.py, where `bar` and `allowed` live because
the CPU tests use them too."""
import ctypes as C
import datetime as dt
import os
import subprocess
import sys

import numpy as np
import pytest

import _compare
import _solar_numpy as sn
from _arena import Arena, DeviceMemory
from test_solar_cpu import records_of, twin_raw

pytestmark = pytest.mark.gpu
CASES = sn.cases()
NAMES = sn.FUNCS


def call(ek, case, lat, lon):
    fn, dates = getattr(ek.solar, NAMES[case["func"]]), sn.dates_of(case)
    return fn(*dates, lat, lon, **case["kwargs"])


# One test walks all recorded cases (a failure names its case), as the CPF tests do.
def test_golden_cases_numpy_input(ek):
    worst = far32 = 0.0
    for case in CASES:
        lat, lon = sn.inputs_of(case)
        before = [np.copy(lat), np.copy(lon)]
        got = call(ek, case, lat, lon)
        assert type(got).__name__ == case["result_type"], (case["id"], type(got))
        worst = max(worst, sn.judge_case(case, got, "numpy " + case["id"], _compare.LEDGER))
        assert np.array_equal(lat, before[0], equal_nan=True) and np.array_equal(lon, before[1], equal_nan=True), case["id"]
        if sn.is_f32(case):
            with np.errstate(all="ignore"):
                far32 = max(far32, float(np.nanmax(np.abs(np.asarray(got, np.float64) - sn.expected_of(case)) / sn.scale_of(case), initial=0.0)))
    line = f"solar goldens, NumPy input: largest use of B(N) {worst:.3f}; distance to the reference's f32 run (not judged): {far32:.3e}"
    _compare.CENSUS.append(line)
    print(line)


def test_golden_cases_device_array_input(ek):
    for case in CASES:
        if case["lat"] is None or sn.array(case["lat"]).dtype.kind != "f":
            continue
        lat, lon = sn.inputs_of(case)
        d_lat, d_lon = ek.DeviceArray.from_host(lat), ek.DeviceArray.from_host(lon)
        got = call(ek, case, d_lat, d_lon)
        assert isinstance(got, ek.DeviceArray), case["id"]
        sn.judge_case(case, got.to_host(), "device " + case["id"], _compare.LEDGER)
        assert np.array_equal(d_lat.to_host(), lat, equal_nan=True) and np.array_equal(d_lon.to_host(), lon, equal_nan=True), case["id"]
        for d in (d_lat, d_lon, got):
            d.free()


def test_torch_device_tensors():
    """torch ROCm tensors in -> torch tensors out, every golden case; in a child process that imports torch first."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_solar_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    if r.returncode == 77:
        pytest.skip(r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "torch unavailable")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "SOLAR_TORCH_OK" in r.stdout


def test_mixed_operands_and_other_broadcasts(ek):
    """A scalar beside a field, f32 latitudes beside f64 longitudes, an integer longitude, and a broadcast pattern the
    kernel does not index (expanded first): against the restatement."""
    rng = np.random.default_rng(8)
    lat, lon = rng.uniform(-90, 90, (3, 4, 5)), rng.uniform(-360, 720, (3, 4, 5))
    day = [dt.datetime(2024, 2, 29, 22, 30), dt.datetime(2024, 3, 1, 1, 30)]
    date = dt.datetime(2023, 7, 15, 9, 37, 21)
    got = ek.solar.cos_solar_zenith_angle(date, lat, 18.0)
    sn.judge(got, sn.call("instant", [date], lat, 18.0), sn.allowed(got, 1), "scalar longitude", _compare.LEDGER)
    got = ek.solar.cos_solar_zenith_angle(date, lat[:, :1, :], lon[:1, :, :1])  # middle-axis patterns: expanded
    assert got.shape == (3, 4, 5) and got.dtype == np.float64
    sn.judge(got, sn.call("instant", [date], lat[:, :1, :], lon[:1, :, :1]), sn.allowed(got, 1), "expanded broadcast", _compare.LEDGER)
    got = ek.solar.cos_solar_zenith_angle_integrated(*day, lat.astype(np.float32), lon)
    assert got.dtype == np.float32 and got.shape == lat.shape
    want = sn.call("integrated", day, lat.astype(np.float32), lon)
    sn.judge(got, want, sn.allowed(want, 9, f32_result=True), "f32 latitudes, f64 longitudes", _compare.LEDGER)
    got = ek.solar.toa_incident_solar_radiation(*day, lat[0, 0], np.array([-170, 0, 18, 400, 7]))
    want = sn.call("toa", day, lat[0, 0], np.array([-170, 0, 18, 400, 7]))
    sn.judge(got, want, sn.allowed(want, 9, 5.06e6), "integer longitudes", _compare.LEDGER)
    got = ek.solar.cos_solar_zenith_angle_integrated(*day, lat, lon[0, 0])  # a vector along the trailing axis
    sn.judge(got, sn.call("integrated", day, lat, np.broadcast_to(lon[0, 0], lat.shape)), sn.allowed(got, 9), "trailing vector", _compare.LEDGER)
    assert ek.solar.cos_solar_zenith_angle(date, np.zeros((0, 3)), np.zeros(3)).shape == (0, 3)


# ---- census ----
N_CENSUS = 1 << 16
CENSUS_CALLS = {"instant": ([dt.datetime(2023, 7, 15, 9, 37, 21)], {}),
                "integrated": ([dt.datetime(2023, 12, 31, 22, 10), dt.datetime(2024, 1, 1, 1, 10)], dict(intervals_per_hour=2)),
                "toa": ([dt.datetime(2024, 2, 29, 22, 30), dt.datetime(2024, 3, 1, 1, 30)], dict(intervals_per_hour=2))}


@pytest.fixture(scope="module")
def census_points():
    rng = np.random.default_rng(2026)
    lat, lon = rng.uniform(-90, 90, N_CENSUS), rng.uniform(-360, 720, N_CENSUS)
    lat[:4], lon[:4] = [90, -90, 0, 45], [720, -360, 0, 180]
    lat[5::9973], lon[7::9973] = np.nan, np.inf
    return lat, lon


@pytest.fixture(scope="module")
def census_reference(census_points):
    """The restatement's values, computed once per (dtype, function) and shared."""
    cache = {}

    def get(T, func):
        if (T, func) not in cache:
            lat, lon = (a.astype(T) for a in census_points)
            dates, kw = CENSUS_CALLS[func]
            cache[T, func] = sn.call(func, dates, lat, lon, **kw)
        return cache[T, func]
    return get


@pytest.mark.parametrize("T", [sn.F32, sn.F64], ids=["f32", "f64"])
@pytest.mark.parametrize("func", list(CENSUS_CALLS))
def test_census_on_65536_points(ek, census_points, census_reference, T, func):
    lat, lon = (a.astype(T) for a in census_points)
    dates, kw = CENSUS_CALLS[func]
    got = getattr(ek.solar, NAMES[func])(*dates, lat, lon, **kw)
    want = census_reference(T, func)
    nn = 1 if func == "instant" else 18
    assert got.dtype == (np.float64 if func == "instant" else T) and got.shape == lat.shape
    scale = float(sn.nodes(*dates, radiation=True, **kw)["isr"].max()) if func == "toa" else 1.0
    used = sn.judge(got, want, sn.allowed(want, nn, scale, f32_result=got.dtype == sn.F32), f"solar census {T.name} {func}", _compare.LEDGER)
    lit = float(np.mean(np.nan_to_num(want) > 0))
    line = f"solar census {T.name} {func}: {got.size} points, {100 * lit:.1f} % sunlit, {int(np.isnan(want).sum())} NaN, used {used:.3f} of its bar"
    _compare.CENSUS.append(line)
    print(line)
    assert 0.2 < lit < 0.9


# ---- the raw entry points inside a guarded arena; kernel against host twin ----
MODES = {"field": 0, "scalar": 1, "major": 2, "minor": 3}


def _arena_run(ek, tag, n, off, lat_mode="field", lon_mode="field", inner=1, nnodes=9):
    from ekm_hip import _ffi

    lib = _ffi.lib()
    T = np.float32 if tag.startswith("f32") else np.float64
    Out = np.float32 if tag == "f32" else np.float64
    rng = np.random.default_rng(n + 7)
    day = [dt.datetime(2023, 12, 31, 22, 10), dt.datetime(2024, 1, 1, 1, 10)]
    rec = ek.solar.kernel_records(records_of("toa", day, dict(integration_order={9: 3, 3: 1, 12: 4}[nnodes])))
    assert rec.shape == (nnodes, 5)

    def operand(mode, lo, hi):
        if mode == "field":
            size, cls = n, (0, 0, 0)
        elif mode == "scalar":
            size, cls = 1, (1, 0, 0)
        elif mode == "major":
            size = -(-n // inner)
            cls = (2, size, inner)
        else:
            size, cls = inner, (3, inner, 0)
        a = rng.uniform(lo, hi, size).astype(T)
        if size > 5:
            a[3] = np.nan
        return a, cls

    lat, lat_cls = operand(lat_mode, -90, 90)
    lon, lon_cls = operand(lon_mode, -360, 720)
    arena = Arena(DeviceMemory(0, None))
    o = [1, 3, 1, 2] if off else [0, 0, 0, 0]
    try:
        arena.input("lat", lat, o[0]), arena.input("lon", lon, o[1]), arena.input("nodes", rec, o[2])
        arena.output("out", n, Out, o[3])
        arena.commit()
        ops = [_ffi.Operand(arena.ptr(k), c[0], 0, c[1], c[2]) for k, c in (("lat", lat_cls), ("lon", lon_cls))]
        _ffi.check(getattr(lib, f"ekm_solar_{tag}")(0, None, C.byref(ops[0]), C.byref(ops[1]), arena.ptr("nodes"), nnodes, arena.ptr("out"), n))
        _ffi.check(lib.ekm_stream_sync(0, None))
        arena.check()
        got = arena.result("out")
    finally:
        arena.free()

    return got, twin_raw(tag, (lat, lat_cls), (lon, lon_cls), rec, n)


@pytest.mark.parametrize("tag", ["f32", "f64", "f32_f64"])
def test_entry_points_in_a_guarded_arena_against_the_host_twin(ek, tag):
    """Point counts around the wave and workgroup sizes, every operand mode, buffers 16-B aligned and one to three
    elements off: guard words and inputs untouched, every output element written; the kernel against its host twin at
    the bar (the count of bit-different points is printed), aligned against shifted buffers bit for bit."""
    shapes = [(n, "field", "field", 1) for n in (1, 63, 64, 65, 255, 256, 257, 1023, 4097)]
    shapes += [(5 * 67, "major", "minor", 67), (257, "scalar", "field", 1), (257, "field", "scalar", 1), (300, "minor", "major", 7),
               (64, "scalar", "scalar", 1)]
    differing = total = 0
    for n, lat_mode, lon_mode, inner in shapes:
        for nnodes in (9, 12) if n == 257 else (9,):
            a, host = _arena_run(ek, tag, n, False, lat_mode, lon_mode, inner, nnodes)
            b, _ = _arena_run(ek, tag, n, True, lat_mode, lon_mode, inner, nnodes)
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"aligned against shifted buffers, n = {n}"
            sn.judge(a, host, sn.allowed(host, nnodes, 5.06e6, f32_result=tag == "f32"), f"kernel against host twin {tag} n {n} {lat_mode}/{lon_mode}",
                     _compare.LEDGER)
            same = (a == host) | (np.isnan(a) & np.isnan(host))
            differing += int((~same).sum())
            total += n
    line = f"solar kernel against host twin {tag}: {differing} of {total} points differ in bits"
    _compare.CENSUS.append(line)
    print(line)


@pytest.mark.parametrize("T", [sn.F32, sn.F64], ids=["f32", "f64"])
def test_a_point_gives_the_same_bits_at_any_position(ek, T):
    """13 distinct points tiled over fields of several lengths and launch shapes: every copy gives the first copy's bits."""
    rng = np.random.default_rng(11)
    lat, lon = rng.uniform(-90, 90, 13).astype(T), rng.uniform(-360, 720, 13).astype(T)
    lat[5], lon[9] = np.nan, np.inf
    day = [dt.datetime(2024, 4, 22), dt.datetime(2024, 4, 23)]
    first = None
    for n in (13, 64, 65, 1027, 70001):
        pick = np.arange(n) % 13 if n < 2000 else rng.integers(0, 13, n)
        got = (ek.solar.cos_solar_zenith_angle(day[0], lat[pick], lon[pick]),
               ek.solar.cos_solar_zenith_angle_integrated(*day, lat[pick], lon[pick]),
               ek.solar.toa_incident_solar_radiation(*day, lat[pick], lon[pick], intervals_per_hour=2, integration_order=4))
        if first is None:
            first = [g.copy() for g in got]
        for g, f in zip(got, first):
            assert np.array_equal(g.view(np.uint8), f[pick].view(np.uint8)), f"n = {n}"
    if T == sn.F64:  # the same points as a (13, 1) x (1, 5) broadcast: indexed operands give the field's bits
        grid = ek.solar.cos_solar_zenith_angle(day[0], lat[:, None], lon[None, :5])
        for j in range(5):
            want = ek.solar.cos_solar_zenith_angle(day[0], lat, np.full(13, lon[j]))
            assert np.array_equal(np.ascontiguousarray(grid[:, j]).view(np.uint8), want.view(np.uint8)), f"column {j}"


@pytest.mark.parametrize("T", [sn.F32, sn.F64], ids=["f32", "f64"])
def test_recorded_graph_replays_the_direct_call(ek, T):
    rng = np.random.default_rng(3)
    lat, lon = rng.uniform(-90, 90, 5000).astype(T), rng.uniform(-360, 720, 5000).astype(T)
    day = [dt.datetime(2024, 4, 22), dt.datetime(2024, 4, 23)]
    d_lat, d_lon = ek.to_device(lat), ek.to_device(lon)
    direct = ek.solar.cos_solar_zenith_angle_integrated(*day, d_lat, d_lon).to_host()  # also caches the node records
    with pytest.raises(ek.EkmError, match="before the block"):
        with ek.graph():
            ek.solar.cos_solar_zenith_angle_integrated(*day, d_lat, d_lon, integration_order=2)
    with ek.graph() as g:
        out = ek.solar.cos_solar_zenith_angle_integrated(*day, d_lat, d_lon)
    g.launch()
    assert np.array_equal(out.to_host().view(np.uint8), direct.view(np.uint8))
    d_lat.copy_from_host(lat[::-1].copy())  # same arrays, new contents
    g.launch()
    assert np.array_equal(out.to_host().view(np.uint8), ek.solar.cos_solar_zenith_angle_integrated(*day, lat[::-1].copy(), lon).view(np.uint8))
    want = sn.call("integrated", day, lat, lon)
    sn.judge(direct, want, sn.allowed(want, 72, f32_result=T == sn.F32), "direct", _compare.LEDGER)
    g.close()
