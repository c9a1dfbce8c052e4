"""stats.iter_quantiles / stats.quantiles on the GPU: every golden case through the public API with NumPy, DeviceArray
and torch input, the raw entry points in a guarded arena over every layout, position and layout independence, a 65 536-point census at 51 samples against the NumPy restatement (which the CPU suite pins to the
recorded reference), the sample cap and a recorded graph.  Every comparison is bit for bit with no point excluded."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _compare
import _quantiles_numpy as qn
from ekm_hip import stats  # noqa: F401  (the module under test: absent before this feature)
from _arena import Arena, DeviceMemory

pytestmark = pytest.mark.gpu
VALUE_CASES = qn.value_cases()
CAP = {qn.F32: 256, qn.F64: 128}  # samples whose sorted copy fits the kernels' 64 KiB of LDS per workgroup
KINDS = {"f32": (qn.F32, qn.F32), "f64": (qn.F64, qn.F64), "f32_f64": (qn.F32, qn.F64)}  # entry point: data, result


@pytest.mark.parametrize("case", VALUE_CASES, ids=qn.case_id)
def test_golden_cases_numpy_input(ek, case):
    kw = qn.kwargs_of(case)
    before = kw["arr"].copy()
    got = ek.stats.quantiles(**kw)
    assert isinstance(got, np.ndarray)
    qn.judge_case(case, got, "numpy " + case["note"])
    rows = list(ek.stats.iter_quantiles(**kw))
    assert len(rows) == case["rows"] and all(isinstance(r, np.ndarray) for r in rows)
    if rows:
        qn.judge_case(case, np.stack(rows), "numpy rows " + case["note"])
    assert before.tobytes() == kw["arr"].tobytes()  # never sorted in place


@pytest.mark.parametrize("case", VALUE_CASES, ids=qn.case_id)
def test_golden_cases_device_array_input(ek, case):
    kw = qn.kwargs_of(case)
    if kw["arr"].dtype in (qn.F32, qn.F64):
        kw["arr"] = ek.DeviceArray.from_host(kw["arr"])
    rows = list(ek.stats.iter_quantiles(**kw))
    assert len(rows) == case["rows"]
    if isinstance(kw["arr"], ek.DeviceArray) and rows:
        shape, axis = tuple(kw["arr"].shape), kw.get("axis", 0) % len(kw["arr"].shape)
        rest = shape[:axis] + shape[axis + 1:]
        assert all(isinstance(r, ek.DeviceArray) and r.shape == rest for r in rows)
        assert len({id(r._alloc) for r in rows}) == 1  # the rows share one allocation
        qn.judge_case(case, np.stack([r.to_host() for r in rows]), "device " + case["note"])
        assert np.array_equal(kw["arr"].to_host(), qn.kwargs_of(case)["arr"], equal_nan=True)
    elif rows:
        qn.judge_case(case, np.stack(rows), "numpy (integer) " + case["note"])
    got = ek.stats.quantiles(**kw)
    if isinstance(kw["arr"], ek.DeviceArray):
        assert isinstance(got, ek.DeviceArray) and got.shape[0] == case["rows"]


def test_torch_device_tensors():
    """torch ROCm tensors in -> torch tensors out, every golden case; in a child process that imports torch first."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_quantiles_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    if r.returncode == 77:
        pytest.skip(r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "torch unavailable")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "QUANTILES_TORCH_OK" in r.stdout


def test_too_many_samples_is_an_error_not_a_wrong_answer(ek):
    for T in (qn.F32, qn.F64):
        for shape, axis in (((CAP[T] + 1, 5), 0), ((5, CAP[T] + 1), -1), ((2, CAP[T] + 1, 3), 1)):
            for method in qn.METHODS:
                with pytest.raises(ek.EkmError, match=f"LDS.*{CAP[T]} members"):
                    ek.stats.quantiles(np.zeros(shape, T), 4, axis, method)
        arr = np.random.default_rng(1).normal(0, 1, (70, CAP[T])).astype(T)  # the cap itself, sample axis last
        qn.judge_exact(ek.stats.quantiles(arr, 4, -1, "numpy"), qn.quantiles(arr, 4, -1, "numpy"), "cap")


# ---- the raw entry points inside a guarded arena ----
def _tables(method, m, qs, T):
    pos = [qn.positions(method, m, q, T) for q in qs]
    return [np.array([float(p[k]) for p in pos]) for k in range(3)]


def _arena_run(tag, outer, m, inner, qs, method, off, rng):
    from ekm_hip import _ffi

    lib = _ffi.lib()
    T, Out = KINDS[tag]
    arr = np.round(rng.normal(0, 2, (outer, m, inner)) * 4) / 4 + 0.0  # ties; + 0.0: no -0.0 beside +0.0 in a column
    arr[0, m // 2, 0] = np.nan
    arr = arr.astype(T)
    lo, hi, w = _tables(method, m, qs, T)
    npts, nq = outer * inner, len(qs)
    arena = Arena(DeviceMemory(0, None))
    o = [1, 3, 2, 1, 3] if off else [0] * 5
    try:
        arena.input("arr", arr, o[0]), arena.input("lo", lo, o[1]), arena.input("hi", hi, o[2]), arena.input("w", w, o[3])
        arena.output("out", nq * npts, Out, o[4])
        arena.commit()
        _ffi.check(getattr(lib, f"ekm_quantiles_{tag}")(0, None, arena.ptr("arr"), outer, m, inner, arena.ptr("lo"), arena.ptr("hi"),
                                                       arena.ptr("w"), nq, 0 if method == "sort" else 1, arena.ptr("out")))
        _ffi.check(lib.ekm_stream_sync(0, None))
        arena.check()  # guards and inputs untouched, every element of out written
        got = arena.result("out").reshape(nq, outer, inner)
        qn.judge_exact(got, qn.quantiles(arr, list(qs), 1, method),
                       f"{tag} {method} [{outer}, {m}, {inner}] nq {nq} off {off}")
        return got
    finally:
        arena.free()


@pytest.mark.parametrize("tag", sorted(KINDS))
def test_entry_points_in_a_guarded_arena(ek, tag):
    """npts in {1, 63, 64, 65, 130} with the sample axis last, inner in {3, 64, 70} x outer in {1, 3},
    nq in {1, 5}, m in {1, 9, 51}; buffers 16-B aligned and one to three elements off.  Nothing is written outside
    `out`, the inputs come back unchanged, every element of `out` is written, and the bits are the restatement's."""
    layouts = [(npts, 1) for npts in (1, 63, 64, 65, 130)] + [(outer, inner) for inner in (3, 64, 70) for outer in (1, 3)]
    methods = ("numpy",) if tag == "f32" else ("sort", "numpy_bulk")
    for outer, inner in layouts:
        for m in (1, 9, 51):
            for qs in ((0.33,), (0.9, 0.0, 0.5, 1.0, 0.25)):
                method = methods[(m + len(qs)) % len(methods)]
                runs = [_arena_run(tag, outer, m, inner, qs, method, off, np.random.default_rng(outer + m)) for off in (False, True)]
                qn.judge_exact(runs[1], runs[0], "aligned against shifted buffers")


def test_entry_point_argument_errors(ek):
    from ekm_hip import _ffi

    lib = _ffi.lib()
    d = ek.DeviceArray.from_host(np.zeros(64, np.float32))
    t = ek.DeviceArray.from_host(np.zeros(4))
    out = ek.DeviceArray.empty((64,), np.float32)
    assert lib.ekm_quantiles_f32(0, None, d.ptr, 8, 8, 1, t.ptr, t.ptr, t.ptr, 1, 0, out.ptr) == _ffi.EKM_ERR_ARG  # sort needs f64 out
    assert lib.ekm_quantiles_f32(0, None, d.ptr, 8, 8, 1, t.ptr, t.ptr, t.ptr, 1, 2, out.ptr) == _ffi.EKM_ERR_ENUM
    assert lib.ekm_quantiles_f32(0, None, d.ptr, 8, 8, 1, None, t.ptr, t.ptr, 1, 1, out.ptr) == _ffi.EKM_ERR_ARG
    assert lib.ekm_quantiles_f32(0, None, d.ptr, 8, 8, 1, t.ptr, t.ptr, t.ptr, 1, 1, None) == _ffi.EKM_ERR_ARG
    assert lib.ekm_quantiles_f32(0, None, d.ptr, 0, 8, 1, t.ptr, t.ptr, t.ptr, 1, 1, None) == _ffi.EKM_OK   # no points
    assert lib.ekm_quantiles_f32(0, None, d.ptr, 8, 8, 1, t.ptr, t.ptr, t.ptr, 0, 1, None) == _ffi.EKM_OK   # no levels
    assert lib.ekm_quantiles_f32(0, None, d.ptr, 8, 0, 1, t.ptr, t.ptr, t.ptr, 1, 1, out.ptr) == _ffi.EKM_ERR_ARG
    ek.synchronize()


@pytest.mark.parametrize("T", [qn.F32, qn.F64], ids=["f32", "f64"])
def test_a_column_gives_the_same_bits_at_any_position_and_in_any_layout(ek, T):
    """The same 130 columns laid out with the sample axis first, last and in the middle, and picked into fields of other
    lengths: a column's bits depend on nothing but its samples.  (One load path: the staged one for the sample-axis-last
    layout was measured slower and removed, profiles/HISTORY.md.)"""
    rng = np.random.default_rng(11)
    cols = (np.round(rng.gamma(1.5, 2.0, (51, 130)) * 8) / 8).astype(T)
    cols[3, 5], cols[0, 64], cols[50, 129] = np.nan, np.inf, -np.inf
    for method in qn.METHODS:
        first = ek.stats.quantiles(cols, 100, 0, method)
        qn.judge_exact(first, qn.quantiles(cols, 100, 0, method), f"axis 0 {method}")
        last = np.ascontiguousarray(cols.T)
        qn.judge_exact(ek.stats.quantiles(last, 100, -1, method), first, f"axis -1 {method}")
        mid = np.ascontiguousarray(cols.reshape(51, 2, 65).transpose(1, 0, 2))
        qn.judge_exact(ek.stats.quantiles(mid, 100, 1, method).reshape(101, 130), first, f"axis 1 {method}")
        for n in (1, 64, 65, 1027):
            pick = rng.integers(0, 130, n)
            qn.judge_exact(ek.stats.quantiles(cols[:, pick], 100, 0, method), first[:, pick], f"picked {n} axis 0 {method}")
            qn.judge_exact(ek.stats.quantiles(last[pick], 100, 1, method), first[:, pick], f"picked {n} axis -1 {method}")


# ---- census ----
@functools.lru_cache(maxsize=None)
def _census_field(name):
    rng = np.random.default_rng(2026)
    a = np.maximum(rng.gamma(1.5, 2.0, (51, 1 << 16)).astype(np.float32) - np.float32(1.0), 0)  # zero-clamped: ties
    a = (np.round(a * 64) / 64).astype(name)
    a[7, ::1001] = np.nan
    a[9, 5::4099] = np.inf
    return a


@functools.lru_cache(maxsize=None)
def _census_want(name, method):
    return qn.quantiles(_census_field(name), 100, 0, method)


@pytest.mark.parametrize("axis", [0, -1])
@pytest.mark.parametrize("method", ["sort", "numpy"])
@pytest.mark.parametrize("T", [qn.F32, qn.F64], ids=["f32", "f64"])
def test_census_51_samples_on_65536_points(ek, T, method, axis):
    field, want = _census_field(T.name), _census_want(T.name, method)
    got = ek.stats.quantiles(field if axis == 0 else np.ascontiguousarray(field.T), 100, axis, method)
    equal = qn.equal_bits(got, want)
    line = f"quantiles census {T.name} {method} axis {axis}: {equal} of {got.size} values equal bits, {int(np.isnan(got).sum())} NaN"
    _compare.CENSUS.append(line)
    print(line)
    assert got.dtype == want.dtype and 0 < np.isnan(got).sum() < got.size
    qn.judge_exact(got, want, line)


@pytest.mark.parametrize("T", [qn.F32, qn.F64], ids=["f32", "f64"])
def test_recorded_graph_replays_the_direct_call(ek, T):
    rng = np.random.default_rng(3)
    arr = rng.normal(0, 1, (51, 5000)).astype(T)
    d_first, d_last = ek.to_device(arr), ek.to_device(np.ascontiguousarray(arr.T))
    levels = [0.1, 0.25, 0.5, 0.75, 0.9]
    calls = [(d_first, 100, 0, "sort"), (d_first, levels, 0, "numpy"), (d_last, levels, -1, "numpy_bulk")]
    direct = [ek.stats.quantiles(*c).to_host() for c in calls]  # also uploads the position tables, which a recording cannot
    with ek.graph() as g:
        outs = [ek.stats.quantiles(*c) for c in calls]
    g.launch()
    for o, want, c in zip(outs, direct, calls):
        qn.judge_exact(o.to_host(), want, "graph replay")
        qn.judge_exact(want, qn.quantiles(arr, c[1], 0, c[3]), "direct")
    g.close()
    with ek.graph() as g2:
        with pytest.raises(ek.EkmError, match=r"inside an ekm_hip.graph\(\) block"):
            ek.stats.quantiles(d_first, [0.123], 0, "sort")  # a level set that has no table yet cannot be recorded
    g2.close()
