"""regimes.project, regimes.regime_index and score.pearson_correlation on the GPU: every golden case through the public
API with NumPy, DeviceArray and torch input, the raw entry points in a guarded arena against the host twin (equal bits:
the twin adds in the kernels' order), position independence, repeatability, a recorded graph and a census.

project is judged within (K + 4) eps sum |f p w| of the exact sum, pearson along a non-contiguous axis bit for bit with
the recorded reference and along the contiguous axis within (2 m + 16) eps, regime_index bit for bit
(tests/_regimes_numpy.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _compare
import _regimes_numpy as rn
import _regimes_twin as twin
from ekm_hip import regimes  # noqa: F401  (the module under test: absent before this feature)
from _arena import Arena, DeviceMemory

pytestmark = pytest.mark.gpu
PROJECT = [c for c in rn.cases("project") if not c["raises"]]
INDEX = rn.cases("regime_index")
PEARSON = [c for c in rn.cases("pearson_correlation") if not c["raises"]]


def _host(d):
    return {k: v.to_host() for k, v in d.items()}


@pytest.mark.parametrize("case", PROJECT, ids=rn.case_id)
def test_project_golden_cases_numpy_and_device_input(ek, case):
    a = rn.arrays_of(case)
    patterns, extra = rn.build_patterns(case, ek.regimes)
    field = a["field"].copy()
    got = ek.regimes.project(field, patterns, a["weights"], **extra)
    nshape = rn.recorded(case)[case["plain"]["labels"][0]].shape
    assert all(isinstance(np.asarray(v), np.ndarray) and np.shape(v) == nshape for v in got.values())
    rn.judge_project(case, got, "numpy " + case["note"], _compare.LEDGER)
    rn.judge_index(got, twin.project(case), "numpy against the host twin " + case["note"])
    assert field.tobytes() == a["field"].tobytes()
    if field.ndim > 2:  # (a DeviceArray result has at least one axis)
        dev = ek.DeviceArray.from_host(field)
        dgot = ek.regimes.project(dev, patterns, a["weights"], **extra)
        assert all(isinstance(v, ek.DeviceArray) and v.shape == nshape and v.dtype == rn.project_dtype(case) for v in dgot.values())
        rn.judge_index(_host(dgot), got, "device against numpy input " + case["note"])
        assert np.array_equal(dev.to_host(), a["field"], equal_nan=True)


@pytest.mark.parametrize("case", INDEX, ids=rn.case_id)
def test_regime_index_golden_cases_numpy_and_device_input(ek, case):
    proj, mean, std = rn.index_args(case)
    before = {k: v.copy() for k, v in proj.items()}
    got = ek.regimes.regime_index(proj, mean, std)
    rn.judge_index(got, rn.recorded(case), "numpy " + case["note"])
    assert all(before[k].tobytes() == proj[k].tobytes() for k in proj)
    dev = {k: ek.DeviceArray.from_host(v) for k, v in proj.items()}
    dmean = {k: ek.DeviceArray.from_host(v) if isinstance(v, np.ndarray) else v for k, v in mean.items()}
    dgot = ek.regimes.regime_index(dev, dmean, std)
    assert all(isinstance(v, ek.DeviceArray) for v in dgot.values())
    rn.judge_index(_host(dgot), rn.recorded(case), "device " + case["note"])
    assert all(np.array_equal(dev[k].to_host(), proj[k]) for k in proj)


@pytest.mark.parametrize("case", PEARSON, ids=rn.case_id)
def test_pearson_golden_cases_numpy_and_device_input(ek, case):
    a, axis, want = rn.arrays_of(case), case["plain"]["axis"], rn.recorded(case)
    x, y = a["x"].copy(), a["y"].copy()
    got = ek.score.pearson_correlation(x, y, axis=axis)
    assert isinstance(got, np.ndarray)
    rn.judge_pearson(x, y, axis, got, want, "numpy " + case["note"], _compare.LEDGER)
    rn.judge_exact(got, twin.pearson(x, y, axis), "numpy against the host twin " + case["note"])
    assert x.tobytes() == a["x"].tobytes() and y.tobytes() == a["y"].tobytes()
    if x.dtype in (rn.F32, rn.F64):
        dx, dy = ek.DeviceArray.from_host(x), ek.DeviceArray.from_host(y)
        dgot = ek.score.pearson_correlation(dx, dy, axis)
        assert isinstance(dgot, ek.DeviceArray) and dgot.shape == want.shape and dgot.dtype == want.dtype
        rn.judge_exact(dgot.to_host(), got, "device against numpy input " + case["note"])
        assert np.array_equal(dx.to_host(), x, equal_nan=True) and np.array_equal(dy.to_host(), y, equal_nan=True)


def test_torch_device_tensors():
    """torch ROCm tensors in -> torch tensors out; in a child process that imports torch first."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_regimes_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    if r.returncode == 77:
        pytest.skip(r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "torch unavailable")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "REGIMES_TORCH_OK" in r.stdout


# ---- the raw entry points inside a guarded arena, against the host twin ----
def _arena_project(ek, T, nf, k, npat, off, per_field=False, scaled=False, seed=0):
    from ekm_hip import _ffi

    rng = np.random.default_rng(seed + 7 * k + nf)
    field = rng.normal(0, 50, (nf, k)).astype(T)
    coef = rng.normal(0, 1, ((nf if per_field else 1) * npat * k)).astype(T)
    scale = rng.normal(1, 0.3, nf).astype(T) if scaled else None
    arena = Arena(DeviceMemory(0, None))
    o = [1, 3, 2, 1] if off else [0] * 4
    try:
        arena.input("field", field, o[0]), arena.input("coef", coef, o[1])
        if scaled:
            arena.input("scale", scale, o[2])
        arena.output("out", npat * nf, T, o[3])
        arena.commit()
        fn = getattr(_ffi.lib(), "ekm_regimes_project_" + ("f32" if T == rn.F32 else "f64"))
        _ffi.check(fn(0, None, arena.ptr("field"), nf, k, arena.ptr("coef"), npat, npat * k if per_field else 0,
                      arena.ptr("scale") if scaled else None, arena.ptr("out")))
        _ffi.check(_ffi.lib().ekm_stream_sync(0, None))
        arena.check()  # guards and inputs untouched, every output element written
        got = arena.result("out").reshape(npat, nf)
    finally:
        arena.free()
    rn.judge_exact(got, twin.project_raw(field, coef, npat, npat * k if per_field else 0, scale), f"project {T} nf {nf} k {k} P {npat} off {off}")
    return got


@pytest.mark.parametrize("T", [rn.F32, rn.F64], ids=["f32", "f64"])
def test_project_entry_points_in_a_guarded_arena_equal_the_host_twin(ek, T):
    """K in {1, 3, 63, 64, 65, 255, 256, 257, 1023, 1025} x N in {1, 2, 300}; 9 patterns (two launches) with a scale
    where N is small, 3 where N is 300; buffers 16-B aligned and one to three elements off; a per-field coefficient run."""
    for k in (1, 3, 63, 64, 65, 255, 256, 257, 1023, 1025):
        for nf in (1, 2, 300):
            runs = [_arena_project(ek, T, nf, k, 3 if nf == 300 else 9, off, scaled=nf != 300) for off in (False, True)]
            rn.judge_exact(runs[1], runs[0], "aligned against shifted buffers")
    for k in (3, 257):
        _arena_project(ek, T, 5, k, 2, True, per_field=True)


def _arena_pearson(ek, T, outer, m, inner, off):
    from ekm_hip import _ffi

    rng = np.random.default_rng(m * 131 + inner)
    x = (280 + rng.normal(0, 5, (outer, m, inner))).astype(T)
    y = (0.5 * (x - 280) + rng.normal(0, 1, x.shape)).astype(T)
    if m > 1:
        x[0, 1, 0] = np.nan
    arena = Arena(DeviceMemory(0, None))
    o = [1, 3, 2] if off else [0] * 3
    try:
        arena.input("x", x, o[0]), arena.input("y", y, o[1])
        arena.output("out", outer * inner, T, o[2])
        arena.commit()
        fn = getattr(_ffi.lib(), "ekm_pearson_" + ("f32" if T == rn.F32 else "f64"))
        _ffi.check(fn(0, None, arena.ptr("x"), arena.ptr("y"), outer, m, inner, arena.ptr("out")))
        _ffi.check(_ffi.lib().ekm_stream_sync(0, None))
        arena.check()
        got = arena.result("out").reshape(outer, inner)
    finally:
        arena.free()
    rn.judge_exact(got, twin.pearson(x, y, 1), f"pearson {T} [{outer}, {m}, {inner}] off {off}")
    return got


@pytest.mark.parametrize("T", [rn.F32, rn.F64], ids=["f32", "f64"])
def test_pearson_entry_points_in_a_guarded_arena_equal_the_host_twin(ek, T):
    """(m, inner) over {1, 2, 51, 257} x {1, 2, 63, 65}, outer 3 (with inner 1: 195 rows, more than one workgroup)."""
    for m in (1, 2, 51, 257):
        for inner in (1, 2, 63, 65):
            outer = 195 if inner == 1 else 3
            runs = [_arena_pearson(ek, T, outer, m, inner, off) for off in (False, True)]
            rn.judge_exact(runs[1], runs[0], "aligned against shifted buffers")


@pytest.mark.parametrize("T", [rn.F32, rn.F64], ids=["f32", "f64"])
def test_index_entry_points_in_a_guarded_arena_equal_the_host_twin(ek, T):
    from ekm_hip import _ffi

    rng = np.random.default_rng(2)
    for n in (1, 255, 256, 257, 1000):
        proj, mean, std = (rng.normal(0, 5, n).astype(T) for _ in range(3))
        std[0] = 0
        for use_arrays in (True, False):
            arena = Arena(DeviceMemory(0, None))
            try:
                arena.input("proj", proj, 1), arena.input("mean", mean, 3), arena.input("std", std, 2)
                arena.output("out", n, T, 1)
                arena.commit()
                fn = getattr(_ffi.lib(), "ekm_regimes_index_" + ("f32" if T == rn.F32 else "f64"))
                args = (arena.ptr("mean"), 0.0, arena.ptr("std"), 0.0) if use_arrays else (None, 1.5, None, 0.3)
                _ffi.check(fn(0, None, arena.ptr("proj"), *args, arena.ptr("out"), n))
                _ffi.check(_ffi.lib().ekm_stream_sync(0, None))
                arena.check()
                want = twin.index_raw(proj, mean, std) if use_arrays else twin.index_raw(proj, 1.5, 0.3)
                rn.judge_exact(arena.result("out"), want, f"index n {n} arrays {use_arrays}")
            finally:
                arena.free()


def test_entry_point_argument_errors(ek):
    from ekm_hip import _ffi

    lib = _ffi.lib()
    d = ek.DeviceArray.from_host(np.zeros(64, np.float32))
    ARG, OK = _ffi.EKM_ERR_ARG, _ffi.EKM_OK
    assert lib.ekm_regimes_project_f32(0, None, None, 4, 8, d.ptr, 2, 0, None, d.ptr) == ARG
    assert lib.ekm_regimes_project_f32(0, None, d.ptr, 4, 0, d.ptr, 2, 0, None, d.ptr) == ARG      # no grid points
    assert lib.ekm_regimes_project_f32(0, None, d.ptr, 4, 8, d.ptr, 2, 8, None, d.ptr) == ARG      # stride below npat * k
    assert lib.ekm_regimes_project_f32(0, None, d.ptr + 2, 4, 8, d.ptr, 2, 0, None, d.ptr) == ARG  # misaligned
    assert lib.ekm_regimes_project_f32(0, None, None, 0, 8, None, 2, 0, None, None) == OK          # no fields
    assert lib.ekm_regimes_index_f32(0, None, d.ptr, None, 0.0, None, 1.0, None, 8) == ARG
    assert lib.ekm_regimes_index_f32(0, None, None, None, 0.0, None, 1.0, None, 0) == OK
    assert lib.ekm_pearson_f32(0, None, d.ptr, d.ptr, 2, 0, 4, d.ptr) == ARG and b"empty" in lib.ekm_last_error()
    assert lib.ekm_pearson_f32(0, None, d.ptr, None, 2, 4, 4, d.ptr) == ARG
    assert lib.ekm_pearson_f32(0, None, None, None, 0, 4, 4, None) == OK
    ek.synchronize()


@pytest.mark.parametrize("T", [rn.F32, rn.F64], ids=["f32", "f64"])
def test_a_field_gives_the_same_bits_at_any_position_and_twice(ek, T):
    rng = np.random.default_rng(11)
    k = 91 * 121  # odd: every second row starts off a 16-byte boundary
    pats = ek.regimes.ConstantPatterns([f"R{i}" for i in range(7)], rn.grid_of((91, 121)), rng.normal(0, 1, (7, 91, 121)).astype(T))
    w = np.cos(np.deg2rad(np.linspace(30, 80, 91)))[:, None].astype(T) * np.ones(121, T)
    row = rng.normal(0, 60, (91, 121)).astype(T)
    alone = ek.regimes.project(row, pats, w)
    batch = rng.normal(0, 60, (6, 91, 121)).astype(T)
    for at in (0, 1, 2, 5):
        batch[at] = row
    dev = ek.DeviceArray.from_host(batch)
    first, second = _host(ek.regimes.project(dev, pats, w)), _host(ek.regimes.project(dev, pats, w))
    for label in alone:
        assert first[label].tobytes() == second[label].tobytes(), "the same call twice"
        for at in (0, 1, 2, 5):
            rn.judge_exact(first[label][at], np.asarray(alone[label]), f"{label} at row {at}")
    # one element further into an allocation: the rows start 4 or 8 bytes off
    shifted = ek.DeviceArray.from_host(np.concatenate([np.zeros(1, T), batch.reshape(-1)])).flat_slice(1, 1 + batch.size).reshape(batch.shape)
    rn.judge_index(_host(ek.regimes.project(shifted, pats, w)), first, "shifted by one element")
    x = (280 + rng.normal(0, 5, (300, k // 121))).astype(T)
    y = rng.normal(0, 1, x.shape).astype(T)
    for axis in (0, 1):
        a, b = ek.score.pearson_correlation(x, y, axis), ek.score.pearson_correlation(x, y, axis)
        assert a.tobytes() == b.tobytes()
    rn.judge_exact(ek.score.pearson_correlation(np.ascontiguousarray(x.T), np.ascontiguousarray(y.T), 1),
                   twin.pearson(np.ascontiguousarray(x.T), np.ascontiguousarray(y.T), 1), "rows against the twin")


def test_recorded_graph_replays_project_and_regime_index(ek):
    rng = np.random.default_rng(3)
    labels = ["NAO+", "NAO-", "BL", "AR"]
    pats = ek.regimes.ConstantPatterns(labels, rn.grid_of((25, 41)), rng.normal(0, 1, (4, 25, 41)).astype(np.float32))
    w = np.ones((25, 41), np.float32)
    mean, std = {k: float(i) for i, k in enumerate(labels)}, {k: 20.0 + i for i, k in enumerate(labels)}
    fields = [rng.normal(0, 60, (51, 4, 25, 41)).astype(np.float32) for _ in range(2)]
    dev = ek.DeviceArray.from_host(fields[0])

    def run():
        return ek.regimes.regime_index(ek.regimes.project(dev, pats, w), mean, std)

    direct = _host(run())  # also uploads the coefficient matrix, which a recording cannot
    with ek.graph() as g:
        outs = run()
    g.launch()
    rn.judge_index(_host(outs), direct, "graph replay")
    dev.copy_from_host(fields[1])
    g.launch()
    want = ek.regimes.regime_index(ek.regimes.project(fields[1], pats, w), mean, std)
    rn.judge_index(_host(outs), want, "graph replay on changed fields")
    assert not np.array_equal(want["BL"], direct["BL"])
    g.close()


def test_census_4096_fields_and_65536_points(ek):
    rng = np.random.default_rng(2026)
    k, nf, npat = 1001, 4096, 4
    for T in (rn.F32, rn.F64):
        field = (80 * np.sin(np.linspace(0, 3, k)) + rng.normal(0, 60, (nf, 1, k))).astype(T)
        stack = rng.normal(0, 1, (npat, 1, k)).astype(T)
        w = (0.5 + rng.uniform(0, 1, (1, k))).astype(T)
        labels = [f"R{i}" for i in range(npat)]
        case = dict(note="census", plain=dict(kind="constant", labels=labels, pshape=[1, k]), arrays={})
        arrays = dict(field=field, patterns=stack, weights=w)
        got = ek.regimes.project(field, ek.regimes.ConstantPatterns(labels, rn.grid_of((1, k)), stack), w)
        used = _census_judge_project(case, arrays, got)
        line = f"regimes project census {np.dtype(T).name}: {nf} fields x K {k} x P {npat}: largest share of the bar used {used:.4f}"
        _compare.CENSUS.append(line)
        print(line)
        x = (280 + rng.normal(0, 5, (51, 1 << 16))).astype(T)
        y = (0.3 * (x - 280) + rng.normal(0, 1, x.shape)).astype(T)
        x[7, ::1001] = np.nan
        got = ek.score.pearson_correlation(x, y, 0)
        want = rn.pearson(x, y, 0)
        rn.judge_exact(got, want, "pearson census axis 0")
        xt, yt = np.ascontiguousarray(x.T), np.ascontiguousarray(y.T)
        used = rn.judge_pearson(xt, yt, 1, ek.score.pearson_correlation(xt, yt, 1), want, "pearson census rows", _compare.LEDGER)
        line = (f"pearson census {np.dtype(T).name}: 65536 points x m 51: axis 0 {rn.equal_bits(got, want)} of {got.size} equal bits; "
                f"contiguous axis: largest share of the bar used {used:.4f}")
        _compare.CENSUS.append(line)
        print(line)


def _census_judge_project(case, arrays, got):
    """judge_project on arrays that are not in the golden file."""
    saved = rn.arrays_of
    rn.arrays_of = lambda c: arrays
    try:
        return rn.judge_project(case, got, "project census", _compare.LEDGER)
    finally:
        rn.arrays_of = saved
