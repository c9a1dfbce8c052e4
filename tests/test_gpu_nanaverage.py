"""stats.nanaverage on the GPU: every golden case through the public API with NumPy, DeviceArray and torch input, the
three kernels at the shapes where they can go wrong (forced through `path` of the raw entry points), special columns,
the raw entry points in a guarded arena against the host twin (equal bits: the twin adds in the kernels' order), the
launch checks, a recorded graph and a census.

Parity (tests/_nanaverage_numpy.py): bit for bit with the recorded reference where the averaged axis is not the
contiguous one; along the contiguous axis equal bits with the host twin and within (n + 4 + n kappa) eps sum |d w| /
|sum w| of the exact mean."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _compare
import _nanaverage_numpy as nn
import _nanaverage_twin as twin
from ekm_hip.stats import nanaverage  # noqa: F401  (the function under test: absent before this feature)
from _arena import Arena, DeviceMemory

pytestmark = pytest.mark.gpu
VALID = [c for c in nn.cases() if not c["raises"] and not c["product_raises"]]
CHUNK = nn.SPLIT_CHUNK


@pytest.mark.parametrize("case", VALID, ids=nn.case_id)
def test_golden_cases_numpy_and_device_input(ek, case):
    d, w, kw = nn.call_of(case)
    axis, keepdims, want = kw.get("axis"), kw.get("keepdims", False), nn.recorded(case)
    outer, m, inner = nn.layout(d.shape, axis)
    data = d.copy()
    got = ek.stats.nanaverage(data, w, **kw)
    assert isinstance(got, (np.ndarray, np.generic)) and np.shape(got) == want.shape
    assert data.tobytes() == d.tobytes()
    if outer * inner == 0:
        assert np.asarray(got).dtype == want.dtype
        return
    nn.judge(d, w, axis, got, want, "numpy " + case["note"], _compare.LEDGER, keepdims)
    nn.judge_exact(np.asarray(got), twin.nanaverage(d, w, axis, keepdims), "numpy against the host twin " + case["note"])
    if d.dtype in (nn.F32, nn.F64) and d.ndim:
        dev = ek.DeviceArray.from_host(d)
        dw = ek.DeviceArray.from_host(w) if w is not None and w.dtype == d.dtype and w.ndim else w
        dgot = ek.stats.nanaverage(dev, dw, **kw)
        assert isinstance(dgot, ek.DeviceArray) and dgot.shape == want.shape and dgot.dtype == want.dtype
        nn.judge_exact(dgot.to_host(), np.asarray(got), "device against numpy input " + case["note"])
        assert np.array_equal(dev.to_host(), d, equal_nan=True), "the device input came back changed"
        if isinstance(dw, ek.DeviceArray):
            assert np.array_equal(dw.to_host(), w, equal_nan=True)


def test_torch_device_tensors():
    """torch ROCm tensors in -> torch tensors out; in a child process that imports torch first."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_nanaverage_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    if r.returncode == 77:
        pytest.skip(r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "torch unavailable")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "NANAVERAGE_TORCH_OK" in r.stdout


# ---- the raw entry points inside a guarded arena, against the host twin ----
def _sample(T, outer, m, inner, seed=0):
    rng = np.random.default_rng(seed + 131 * m + inner)
    x = (280 + rng.normal(0, 5, (outer, m, inner))).astype(T)
    x[rng.uniform(size=x.shape) < 0.1] = np.nan
    return x, rng


def _arena_call(T, x, path, weights=None, wstrides=(0, 0, 0), off=False, dirty_work=True):
    """One call of ekm_nanaverage_* on x [outer, m, inner] in a guarded arena; returns the result [outer * inner]."""
    from ekm_hip import _ffi

    lib = _ffi.lib()
    outer, m, inner = x.shape
    tag = "f32" if T == nn.F32 else "f64"
    need = int(lib.ekm_nanaverage_work_bytes(T.itemsize, outer, m, inner, int(weights is not None), path))
    arena = Arena(DeviceMemory(0, None))
    o = [1, 3, 2, 1] if off else [0] * 4
    try:
        arena.input("data", x, o[0])
        if weights is not None:
            arena.input("weights", weights, o[1])
        if need:  # garbage on entry: the kernels must not read what they have not written
            arena.inout("work", np.full(need // T.itemsize, np.nan if dirty_work else 0.0, T), o[2])
        arena.output("out", outer * inner, T, o[3])
        arena.commit()
        fn = getattr(lib, "ekm_nanaverage_" + tag)
        args = (0, None, arena.ptr("data"), outer, m, inner, arena.ptr("weights") if weights is not None else None, *wstrides, path,
                arena.ptr("work") if need else None, need, arena.ptr("out"))
        _ffi.check(fn(*args))
        _ffi.check(lib.ekm_stream_sync(0, None))
        arena.check()  # guards and inputs untouched, every output element written
        first = arena.result("out")
        _ffi.check(fn(*args))
        _ffi.check(lib.ekm_stream_sync(0, None))
        arena.check()
        assert arena.result("out").tobytes() == first.tobytes(), "two launches give different bytes"
    finally:
        arena.free()
    want = twin.raw(x.reshape(-1), outer, m, inner, None if weights is None else np.ascontiguousarray(weights).reshape(-1), wstrides, path)
    nn.judge_exact(first, want, f"nanaverage {T} {x.shape} path {path} weights {wstrides if weights is not None else None} off {off}")
    return first


def _both(T, x, path, rng, what):
    """Unweighted and weighted (a vector along the axis, shared through strides of 0), aligned and at odd offsets; the
    results are judged against NumPy's."""
    outer, m, inner = x.shape
    w = (0.5 + rng.uniform(0, 1, m)).astype(T)
    for weights, ws in ((None, (0, 0, 0)), (w, (0, 1, 0))):
        runs = [_arena_call(T, x, path, weights, ws, off) for off in (False, True)]
        nn.judge_exact(runs[1], runs[0], "aligned against shifted buffers")
        want = nn.numpy_formula(x, None if weights is None else w[:, None], axis=1).reshape(-1)
        nn.judge(x, None if weights is None else w[:, None], 1, runs[0].reshape(outer, inner), want.reshape(outer, inner),
                 f"{what} {x.shape} path {path} weighted {weights is not None}", _compare.LEDGER, bit_for_bit=inner > 1)


@pytest.mark.parametrize("T", [nn.F32, nn.F64], ids=["f32", "f64"])
def test_path_1_shapes_in_a_guarded_arena(ek, T):
    """inner over the workgroup edges with outer 1 and 3; m over 1, 2, 3, 51, 257 (the batch of 8 and its tail); every
    tenth sample NaN, so neighbours in the wave end their valid runs at different samples."""
    for k, inner in enumerate((2, 63, 64, 65, 255, 256, 257)):
        for outer in (1, 3):
            m = (1, 2, 3, 51, 257)[(k + outer) % 5]
            x, rng = _sample(T, outer, m, inner)
            _both(T, x, nn.POINTS, rng, "path 1")
    for m in (1, 2, 3, 51, 257):
        x, rng = _sample(T, 3, m, 65)
        _both(T, x, nn.POINTS, rng, "path 1")


@pytest.mark.parametrize("T", [nn.F32, nn.F64], ids=["f32", "f64"])
def test_path_2_shapes_in_a_guarded_arena(ek, T):
    """m over the wave and chunk edges; rows 1, 3, 4, 5 (the workgroup holds 4); a row of odd m starts off a 16-byte boundary."""
    for k, m in enumerate((1, 63, 64, 65, 129, 4097)):
        for rows in ((1, 4), (3, 5))[k % 2] + ((5,) if m == 4097 else ()):
            x, rng = _sample(T, rows, m, 1)
            _both(T, x, nn.ROWS, rng, "path 2")
            _both(T, x, nn.POINTS, rng, "path 1 on rows")


@pytest.mark.parametrize("T", [nn.F32, nn.F64], ids=["f32", "f64"])
def test_path_3_shapes_in_a_guarded_arena(ek, T):
    for m in (CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5):
        for rows in (1, 3):
            x, rng = _sample(T, rows, m, 1)
            _both(T, x, nn.SPLIT, rng, "path 3")
    x, rng = _sample(T, 2, 2 * CHUNK + 3, 1)
    assert _ffi_work_bytes(T, 2, 2 * CHUNK + 3, 1, 0) > 0, "the rule picks path 3 here"
    _both(T, x, 0, rng, "path 0 taking path 3")
    nn.judge_exact(_arena_call(T, x, 0), _arena_call(T, x, nn.SPLIT, dirty_work=False), "path 0 against path 3")
    # a row gives the same bits at another row index and address
    y = np.stack([x[1], x[0], x[1]])
    got = _arena_call(T, y, nn.SPLIT, off=True)
    alone = _arena_call(T, x, nn.SPLIT)
    nn.judge_exact(got, alone[[1, 0, 1]], "rows moved")


def _ffi_work_bytes(T, outer, m, inner, path):
    from ekm_hip import _ffi

    return int(_ffi.lib().ekm_nanaverage_work_bytes(T.itemsize, outer, m, inner, 0, path))


@pytest.mark.parametrize("T", [nn.F32, nn.F64], ids=["f32", "f64"])
def test_special_columns_on_every_path(ek, T):
    """A NaN in the first and in the last element of a lane's run, an all-NaN row, a row of -0.0; weights with stride 0 in
    each of the three groups."""
    rng = np.random.default_rng(9)
    V = 16 // T.itemsize
    for path, m in ((nn.POINTS, 51), (nn.ROWS, 64 * V * 2 + 3), (nn.SPLIT, CHUNK + 256 * V + 1)):
        inner = 5 if path == nn.POINTS else 1
        x = (280 + rng.normal(0, 5, (6, m, inner))).astype(T)
        x[0, 0], x[0, V - 1], x[0, V] = np.nan, np.nan, np.nan   # the first and last element of lane 0's first chunk, and lane 1's first
        x[1, -1], x[1, m - V - 1] = np.nan, np.nan               # the last element of the row (the ragged tail) and of a full chunk
        x[2] = np.nan                                            # an all-NaN row: NaN, or 0.0 with weights
        x[3] = T.type(-0.0)                                      # -0.0 + ... from +0: +0.0
        x[4, ::2] = np.nan
        plain = _arena_call(T, x, path).reshape(6, inner)
        assert np.isnan(plain[2]).all() and (plain[3] == 0).all() and not np.signbit(plain[3]).any()
        nn.judge(x, None, 1, plain, nn.numpy_formula(x, axis=1), f"special columns path {path}", _compare.LEDGER, bit_for_bit=inner > 1)
        full = (0.5 + rng.uniform(0, 1, x.shape)).astype(T)
        per_m = np.ascontiguousarray(full[0, :, 0])
        per_o = np.ascontiguousarray(full[:, 0, 0])
        per_i = np.ascontiguousarray(full[0, 0, :])
        for what, w, ws, bw in (("full", full, (m * inner, inner, 1), full),
                                ("stride 0 in outer and inner", per_m, (0, 1, 0), per_m[None, :, None]),
                                ("stride 0 in m and inner", per_o, (1, 0, 0), per_o[:, None, None]),
                                ("stride 0 in outer and m", per_i, (0, 0, 1), per_i[None, None, :]),
                                ("stride 0 in all three", per_m[:1], (0, 0, 0), per_m[0])):
            got = _arena_call(T, x, path, w, ws, off=True).reshape(6, inner)
            assert (got[2] == 0).all() and not np.signbit(got[2]).any(), "a weighted all-NaN row gives +0.0"
            bw = np.broadcast_to(bw, x.shape)
            nn.judge(x, bw, 1, got, nn.numpy_formula(x, bw, axis=1), f"special columns path {path} weights {what}", _compare.LEDGER,
                     bit_for_bit=inner > 1)


def test_launch_checks(ek):
    from ekm_hip import _ffi

    lib = _ffi.lib()
    ARG, ENUM, OK = _ffi.EKM_ERR_ARG, _ffi.EKM_ERR_ENUM, _ffi.EKM_OK
    d = ek.DeviceArray.from_host(np.ones(4 * CHUNK, np.float32))
    out = ek.DeviceArray.from_host(np.full(64, 7.0, np.float32))
    work = ek.DeviceArray.from_host(np.full(64, 7.0, np.float32))
    f = lib.ekm_nanaverage_f32

    def err(rc, code, *words):
        msg = lib.ekm_last_error().decode()
        assert rc == code and msg.startswith("nanaverage") and all(w in msg for w in words), (rc, msg)

    err(f(0, None, None, 2, 3, 4, None, 0, 0, 0, 0, None, 0, out.ptr), ARG, "null")
    err(f(0, None, d.ptr, 2, 3, 4, None, 0, 0, 0, 0, None, 0, None), ARG, "null")
    err(f(0, None, d.ptr + 2, 2, 3, 4, None, 0, 0, 0, 0, None, 0, out.ptr), ARG, "aligned")
    err(f(0, None, d.ptr, 2, 3, 4, None, 0, 0, 0, 0, None, 0, out.ptr + 1), ARG, "aligned")
    err(f(0, None, d.ptr, 2, 3, 4, d.ptr + 2, 0, 1, 0, 0, None, 0, out.ptr), ARG, "aligned")
    err(f(0, None, d.ptr, 2, 3, 4, None, 0, 0, 0, 2, None, 0, out.ptr), ARG, "inner")
    err(f(0, None, d.ptr, 2, 3, 4, None, 0, 0, 0, 3, work.ptr, 256, out.ptr), ARG, "inner")
    err(f(0, None, d.ptr, 2, 3, 4, None, 0, 0, 0, 4, None, 0, out.ptr), ENUM, "path=4")
    err(f(0, None, d.ptr, 2, 3, 4, None, 0, 0, 0, -1, None, 0, out.ptr), ENUM, "path=-1")
    err(f(0, None, d.ptr, 1 << 40, 1 << 40, 1, None, 0, 0, 0, 0, None, 0, out.ptr), ARG, "too many")
    need = int(lib.ekm_nanaverage_work_bytes(4, 2, 2 * CHUNK, 1, 0, 0))
    assert need == 2 * 2 * 2 * 4
    err(f(0, None, d.ptr, 2, 2 * CHUNK, 1, None, 0, 0, 0, 0, work.ptr, need - 1, out.ptr), ARG, f"needs {need} bytes")
    err(f(0, None, d.ptr, 2, 2 * CHUNK, 1, None, 0, 0, 0, 0, None, need, out.ptr), ARG, f"needs {need} bytes")
    err(f(0, None, d.ptr, 2, 2 * CHUNK, 1, None, 0, 0, 0, 3, work.ptr + 2, need, out.ptr), ARG, "aligned")
    assert f(0, None, None, 0, 3, 4, None, 0, 0, 0, 0, None, 0, None) == OK  # no points
    ek.synchronize()
    assert (out.to_host() == 7.0).all() and (work.to_host() == 7.0).all(), "an error launched something"
    assert f(0, None, d.ptr, 2, 2 * CHUNK, 1, None, 0, 0, 0, 0, work.ptr, need, out.ptr) == OK
    ek.synchronize()
    assert (out.to_host()[:2] == 1.0).all() and (out.to_host()[2:] == 7.0).all()


def test_recorded_graph_replays_the_call(ek):
    rng = np.random.default_rng(3)
    fields = [(280 + rng.normal(0, 5, (4, 2 * CHUNK + 7))).astype(np.float32) for _ in range(2)]
    for f in fields:
        f[rng.uniform(size=f.shape) < 0.1] = np.nan
    w = ek.DeviceArray.from_host((0.5 + rng.uniform(0, 1, 2 * CHUNK + 7)).astype(np.float32))
    dev = ek.DeviceArray.from_host(fields[0])
    cube = ek.DeviceArray.from_host(fields[0][:, :51 * 64].reshape(4, 51, 64))

    def run():
        return ek.stats.nanaverage(dev, w, axis=1), ek.stats.nanaverage(dev), ek.stats.nanaverage(cube, axis=1)

    direct = [r.to_host() for r in run()]
    with ek.graph() as g:
        outs = run()
    g.launch()
    for o, want in zip(outs, direct):
        nn.judge_exact(o.to_host(), want, "graph replay")
    dev.copy_from_host(fields[1])
    g.launch()
    want = [ek.stats.nanaverage(fields[1], w.to_host(), axis=1), ek.stats.nanaverage(fields[1])]
    nn.judge_exact(outs[0].to_host(), want[0], "graph replay on changed data")
    nn.judge_exact(outs[1].to_host(), np.asarray(want[1]), "graph replay on changed data, axis None")
    assert not np.array_equal(want[0], direct[0])
    g.close()


def test_census_65536_points_51_samples(ek):
    rng = np.random.default_rng(2026)
    for T in (nn.F32, nn.F64):
        x = (280 + rng.normal(0, 5, (51, 1 << 16))).astype(T)
        x[rng.uniform(size=x.shape) < 0.1] = np.nan
        w = (0.5 + rng.uniform(0, 1, (51, 1))).astype(T)
        for weights in (None, w):
            got = ek.stats.nanaverage(x, weights, axis=0)
            want = nn.numpy_formula(x, weights, axis=0)
            nn.judge_exact(got, want, "nanaverage census axis 0")
            line = (f"nanaverage census {T.name} {'weighted' if weights is not None else 'unweighted'}: 65536 points x m 51, 10 % NaN, "
                    f"axis 0: {nn.equal_bits(got, want)} of {got.size} equal bits")
            _compare.CENSUS.append(line)
            print(line)
