"""Wind functions on the GPU (ekm_hip.wind): every golden case through the public API with NumPy, DeviceArray and torch
input, a 65 536-point census per dtype and function against the NumPy restatement, the raw entry points in a guarded
arena against the host twin, position independence, a recorded graph of xy_to_polar plus windrose, and the wind rose on
65 537 samples in one cell, uniform over the cells and through the over-cap path, twice with identical bytes.

The bars are derived in tests/_wind_numpy.py: speed 2 eps relative, direction 4 eps 360 on the circular distance (a
0 / 360 wrap only at the branch point), polar_to_xy and coriolis (3 + 1.5 |a|) eps |m|; a float32
result (float arithmetic) is judged against the reference's float64 run on the upcast inputs with the float kernels' own
derived terms on top (1, 3.5, 2 + 0.5 |a| and 2.5 eps32); wind rose bit for bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _compare
import _wind_numpy as wn
from _arena import Arena, DeviceMemory
from test_wind_cpu import KIND, mode_of, rose_inputs, twin, twin_rose

pytestmark = pytest.mark.gpu
N_CENSUS = wn.N_CENSUS


def as_tuple(x):
    return x if isinstance(x, tuple) else (x,)


def test_golden_cases_numpy_input(ek):
    worst = {}
    for case in wn.cases():
        ins = wn.inputs_of(case)
        before = [np.array(x, copy=True) for x in ins]
        got = as_tuple(getattr(ek.wind, case["func"])(*ins, **case["kwargs"]))
        assert [type(g).__name__ for g in got] == case["result_type"], (case["id"], [type(g) for g in got])
        used = wn.judge_case(case, got, "numpy " + case["id"], _compare.LEDGER)
        worst[case["func"]] = max(worst.get(case["func"], 0.0), used)
        assert all(np.array_equal(np.asarray(x), b, equal_nan=True) for x, b in zip(ins, before)), case["id"]
    line = "wind goldens, NumPy input, largest use of each bar: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items()))
    _compare.CENSUS.append(line)
    print(line)


def test_golden_cases_device_array_input(ek):
    for case in wn.cases():
        if case["tag"] not in ("f32", "f64"):
            continue
        ins = wn.inputs_of(case)
        dev = [ek.DeviceArray.from_host(a) for a in ins]
        got = as_tuple(getattr(ek.wind, case["func"])(*dev, **case["kwargs"]))
        assert all(isinstance(g, ek.DeviceArray) for g in got), case["id"]
        wn.judge_case(case, tuple(g.to_host() for g in got), "device " + case["id"], _compare.LEDGER)
        assert all(np.array_equal(d.to_host(), a, equal_nan=True) for d, a in zip(dev, ins)), case["id"]
        for d in dev + list(got):
            d.free()


def test_golden_wind_roses(ek):
    for case in wn.cases("windrose"):
        sp, di, bins = rose_inputs(case)
        want = wn.expected_of(dict(case, nout=2))
        before = [np.array(sp, copy=True), np.array(di, copy=True)]
        wn.judge_rose(ek.wind.windrose(sp, di, sectors=case["sectors"], speed_bins=bins, percent=case["percent"]), want, "numpy " + case["id"])
        assert np.array_equal(sp, before[0], equal_nan=True) and np.array_equal(di, before[1], equal_nan=True)
        if not case["scalar"] and all(np.asarray(a).dtype in (wn.F32, wn.F64) and np.asarray(a).size for a in (sp, di)):
            d_sp, d_di = ek.DeviceArray.from_host(sp), ek.DeviceArray.from_host(di)
            got = ek.wind.windrose(d_sp, d_di, sectors=case["sectors"], speed_bins=bins, percent=case["percent"])
            assert all(isinstance(g, ek.DeviceArray) for g in got), case["id"]
            wn.judge_rose(tuple(g.to_host() for g in got), want, "device " + case["id"])
            for d in (d_sp, d_di) + got:
                d.free()


def test_torch_device_tensors():
    """torch ROCm tensors in -> torch tensors out, every golden case; in a child process that imports torch first."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_wind_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    if r.returncode == 77:
        pytest.skip(r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "torch unavailable")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "WIND_TORCH_OK" in r.stdout


# ---- census ----
CENSUS_CALLS = [("speed", {}), ("direction", {}), ("direction", dict(convention="polar")), ("direction", dict(convention="polar", to_positive=False)),
                ("xy_to_polar", {}), ("polar_to_xy", {}), ("polar_to_xy", dict(convention="polar")), ("coriolis", {})]


@pytest.mark.parametrize("T", [wn.F32, wn.F64], ids=["f32", "f64"])
def test_census_against_the_restatement(ek, T):
    u, v, m, d = wn.census_inputs(T)
    for func, kw in CENSUS_CALLS:
        ins = [d] if func == "coriolis" else [m, d] if func == "polar_to_xy" else [u, v]
        got = as_tuple(getattr(ek.wind, func)(*ins, **kw))
        with np.errstate(all="ignore"):
            want = as_tuple(wn.FUNCS[func](*[x.astype(wn.F64) for x in ins], **kw))  # the float64 run on the upcast inputs
        assert all(g.dtype == T for g in got)
        used = wn.judge_call(func, kw, ins, got, want, f"wind census {T.name} {func} {kw}", _compare.LEDGER)
        line = f"wind census {T.name} {func} {kw or ''}: {N_CENSUS} points, largest use of the bar {used:.3f}"
        _compare.CENSUS.append(line)
        print(line)


# ---- the raw entry points inside a guarded arena; kernel against host twin ----
def _arena_elementwise(tag, func, kw, n, off, modes=("field", "field"), inner=1):
    from ekm_hip import _ffi

    lib, T = _ffi.lib(), np.float32 if tag == "f32" else np.float64
    rng = np.random.default_rng(n + 3)
    nin = 1 if func == "coriolis" else 2

    def operand(mode):
        size, cls = {"field": (n, (0, 0, 0)), "scalar": (1, (1, 0, 0)), "major": (-(-n // inner), (2, -(-n // inner), inner)),
                     "minor": (inner, (3, inner, 0))}[mode]
        a = rng.normal(0, 30, size).astype(T)
        if size > 5:
            a[3], a[4] = np.nan, 0.0
        return a, cls

    ops = [operand(m) for m in modes[:nin]]
    arena = Arena(DeviceMemory(0, None))
    o = [1, 3, 1, 2] if off else [0, 0, 0, 0]
    try:
        for k, (a, _) in enumerate(ops):
            arena.input(f"in{k}", a, o[k])
        want0, want1 = func in ("speed", "xy_to_polar", "polar_to_xy", "coriolis"), func in ("direction", "xy_to_polar", "polar_to_xy")
        if want0:  # an output that is not wanted gets a null pointer, and no buffer
            arena.output("out0", n, T, o[2])
        if want1:
            arena.output("out1", n, T, o[3])
        arena.commit()
        cops = [_ffi.Operand(arena.ptr(f"in{k}"), c[0], 0, c[1], c[2]) for k, (_, c) in enumerate(ops)]
        if func == "coriolis":
            rc = getattr(lib, f"ekm_wind_coriolis_{tag}")(0, None, C.byref(cops[0]), arena.ptr("out0"), n)
        else:
            entry = "xy" if func == "polar_to_xy" else "polar"
            rc = getattr(lib, f"ekm_wind_{entry}_{tag}")(0, None, C.byref(cops[0]), C.byref(cops[1]), mode_of(func, kw),
                                                        arena.ptr("out0") if want0 else None, arena.ptr("out1") if want1 else None, n)
        _ffi.check(rc)
        _ffi.check(lib.ekm_stream_sync(0, None))
        arena.check()
        got = tuple(arena.result(k) for k, w in (("out0", want0), ("out1", want1)) if w)
    finally:
        arena.free()
    shaped = [a if c[0] == 0 else a[0] if c[0] == 1 else np.repeat(a, inner)[:n] if c[0] == 2 else np.resize(a, n) for a, c in ops]
    return got, twin(func, shaped, kw)


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_entry_points_in_a_guarded_arena_against_the_host_twin(ek, tag):
    """Lengths 1, around the vector tile and 65 537, every operand mode, buffers aligned and one to three elements off:
    guard words and inputs untouched, every wanted output element written and no other; kernel and host twin bit for bit (NaN for NaN)."""
    tile = wn.TILE[tag]
    runs = [(f, kw, n, ("field", "field"), 1) for n in (1, 3, tile - 1, tile, tile + 1, 65537)
            for f, kw in (("xy_to_polar", {}), ("polar_to_xy", {}), ("coriolis", {}))]
    runs += [("speed", {}, 257, ("field", "field"), 1), ("direction", dict(convention="polar"), 257, ("field", "field"), 1),
             ("direction", dict(convention="polar", to_positive=False), 5 * 67, ("major", "minor"), 67),
             ("xy_to_polar", {}, 257, ("scalar", "field"), 1), ("polar_to_xy", dict(convention="polar"), 300, ("minor", "major"), 7)]
    for func, kw, n, modes, inner in runs:
        a, host = _arena_elementwise(tag, func, kw, n, False, modes, inner)
        b, _ = _arena_elementwise(tag, func, kw, n, True, modes, inner)
        for x, y, h in zip(a, b, host):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"aligned against shifted buffers, {func} n = {n}"
            h = h.astype(x.dtype).ravel()
            same = ((x == h) & (np.signbit(x) == np.signbit(h))) | (np.isnan(x) & np.isnan(h))  # (a NaN's sign and payload are not compared)
            assert same.all(), f"kernel against host twin, {func} n = {n} {modes}: {np.flatnonzero(~same)[:4]}, {x[~same][:4]}, {h[~same][:4]}"


def test_misaligned_and_null_pointers_are_refused(ek):
    from ekm_hip import _ffi

    lib = _ffi.lib()
    d = ek.DeviceArray.empty((64,), np.float64)
    p = d.on(None)
    good, odd, null = _ffi.Operand(p, 0, 0, 0, 0), _ffi.Operand(p + 4, 0, 0, 0, 0), _ffi.Operand(None, 0, 0, 0, 0)
    for a, b, o0, o1 in ((odd, good, p, p), (good, null, p, p), (good, good, p + 4, p), (good, good, None, None)):
        assert lib.ekm_wind_polar_f64(0, None, C.byref(a), C.byref(b), 0, o0, o1, 8) == _ffi.EKM_ERR_ARG
    assert lib.ekm_wind_xy_f64(0, None, C.byref(good), C.byref(good), 0, p, None, 8) == _ffi.EKM_ERR_ARG
    assert lib.ekm_wind_polar_f64(0, None, C.byref(good), C.byref(good), 3, p, p, 8) == _ffi.EKM_ERR_ENUM
    assert lib.ekm_wind_coriolis_f64(0, None, C.byref(null), p, 8) == _ffi.EKM_ERR_ARG
    assert lib.ekm_windrose_f64(0, None, p + 4, p, 8, p, 2, 3, 0.0, 0, p, p) == _ffi.EKM_ERR_ARG
    assert lib.ekm_windrose_f64(0, None, p, p, 8, None, 2, 3, 0.0, 0, p, p) == _ffi.EKM_ERR_ARG
    assert lib.ekm_windrose_f64(0, None, p, p, 8, p, 1, 3, 0.0, 0, p, p) == _ffi.EKM_ERR_ARG
    d.free()


@pytest.mark.parametrize("T", [wn.F32, wn.F64], ids=["f32", "f64"])
def test_a_point_gives_the_same_bits_at_any_position(ek, T):
    rng = np.random.default_rng(11)
    u, v = rng.normal(0, 9, 13).astype(T), rng.normal(0, 9, 13).astype(T)
    u[5], v[9], u[2] = np.nan, np.inf, 0.0
    first = None
    for n in (13, 64, 65, 1027, 70001):
        pick = np.arange(n) % 13 if n < 2000 else rng.integers(0, 13, n)
        got = ek.wind.xy_to_polar(u[pick], v[pick]) + ek.wind.polar_to_xy(u[pick], v[pick]) + (ek.wind.coriolis(v[pick]),)
        if first is None:
            first = [g.copy() for g in got]
        for g, f in zip(got, first):
            assert np.array_equal(g.view(np.uint8), f[pick].view(np.uint8)), f"n = {n}"
    grid = ek.wind.direction(u[:, None], v[None, :5])  # indexed operands give the field's bits
    for j in range(5):
        assert np.array_equal(np.ascontiguousarray(grid[:, j]).view(np.uint8), ek.wind.direction(u, np.full(13, v[j], T)).view(np.uint8))


def test_recorded_graph_replays_xy_to_polar_and_windrose(ek):
    rng = np.random.default_rng(3)
    u, v = rng.normal(0, 9, 5000), rng.normal(0, 9, 5000)
    bins = [0.0, 2.0, 5.0, 10.0, 50.0]
    d_u, d_v = ek.to_device(u), ek.to_device(v)
    sp, di = ek.wind.xy_to_polar(d_u, d_v)
    direct = ek.wind.windrose(sp, di, sectors=16, speed_bins=bins)[0].to_host()  # also caches the edges
    with pytest.raises(ek.EkmError, match="before the block"):
        with ek.graph():
            ek.wind.windrose(sp, di, sectors=12, speed_bins=bins)
    with ek.graph() as g:
        g_sp, g_di = ek.wind.xy_to_polar(d_u, d_v)
        rose, rose_bins = ek.wind.windrose(g_sp, g_di, sectors=16, speed_bins=bins)
    g.launch()
    assert np.array_equal(rose.to_host().view(np.uint8), direct.view(np.uint8))
    d_u.copy_from_host(u[::-1].copy())  # same arrays, new contents
    g.launch()
    want = wn.windrose(*wn.xy_to_polar(u[::-1], v), sectors=16, speed_bins=bins)
    host_sp, host_di = ek.wind.xy_to_polar(u[::-1].copy(), v)
    wn.judge_rose((rose.to_host(), rose_bins.to_host()), ek.wind.windrose(host_sp, host_di, sectors=16, speed_bins=bins), "replay")
    assert abs(rose.to_host() - want[0]).max() < 0.1  # (the restatement's own directions may fall one sector off at an edge)
    g.close()


# ---- the wind rose at size ----
@pytest.mark.parametrize("shape", ["one_cell", "uniform", "over_cap"])
@pytest.mark.parametrize("T", [wn.F32, wn.F64], ids=["f32", "f64"])
def test_wind_rose_on_65537_samples(ek, T, shape):
    rng = np.random.default_rng(17)
    n = 65537
    sectors, bins = (1000, list(np.linspace(0.0, 40.0, 41))) if shape == "over_cap" else (16, [0.0, 2.0, 4.0, 8.0, 16.0, 40.0])
    if shape == "one_cell":
        sp, di = np.full(n, 5.0, T), np.full(n, 200.0, T)
    else:
        sp, di = rng.uniform(-1, 41, n).astype(T), rng.uniform(0, 360, n).astype(T)
        di[:40], sp[40:80] = np.nan, np.nan
    for percent in (False, True):
        want = wn.windrose(sp, di, sectors=sectors, speed_bins=bins, percent=percent)
        got = ek.wind.windrose(sp, di, sectors=sectors, speed_bins=bins, percent=percent)
        wn.judge_rose(got, want, f"{shape} {T.name} percent={percent}")
        again = ek.wind.windrose(sp, di, sectors=sectors, speed_bins=bins, percent=percent)
        assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()
        wn.judge_rose(twin_rose(sp, di, sectors, bins, percent), want, f"host twin {shape}")
    plain = ek.wind.windrose(sp, di, sectors=sectors, speed_bins=bins, percent=False)
    if shape == "one_cell":
        assert plain[0].sum() == n and np.count_nonzero(plain[0]) == 1
