"""stats.long_quantiles / stats.iter_long_quantiles on the GPU: the golden cases (257 to 1980 samples) through the public
API with NumPy, DeviceArray and torch input; the raw entry points in a guarded arena over point counts that straddle every
tile width, both load paths and shifted buffers; short axes against stats.quantiles; the cap; position and layout
independence; a census at 1980 samples on 4096 points against the NumPy restatement (which the CPU suite pins to the
recorded reference); a recorded graph; and a column mixing the two zeros against the host twin.  Every comparison is
bit for bit with no point excluded."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _compare
import _long_quantiles as lq
from _arena import Arena, DeviceMemory
from ekm_hip import stats  # noqa: F401

pytestmark = pytest.mark.gpu
CASES = lq.cases()
stats.long_quantiles  # the functions under test: absent before this feature


GROUPS = [f"{tag} {method}" for tag in ("f32", "f64") for method in lq.METHODS]  # 39 recorded cases each


def _golden_case(ek, case):
    kw = lq.kwargs_of(case)
    before = kw["arr"].copy()
    got = ek.stats.long_quantiles(**kw)
    assert isinstance(got, np.ndarray)
    lq.judge_case(case, got, "numpy " + lq.case_id(case))
    assert before.tobytes() == kw["arr"].tobytes()  # never sorted in place
    kw["arr"] = ek.DeviceArray.from_host(kw["arr"])
    rows = list(ek.stats.iter_long_quantiles(**kw))
    shape, axis = tuple(before.shape), kw.get("axis", 0) % before.ndim
    assert len(rows) == case["rows"] and all(isinstance(r, ek.DeviceArray) and r.shape == shape[:axis] + shape[axis + 1:] for r in rows)
    assert len({id(r._alloc) for r in rows}) == 1  # the rows are views of one allocation
    lq.judge_case(case, np.stack([r.to_host() for r in rows]), "device rows " + lq.case_id(case))
    assert before.tobytes() == kw["arr"].to_host().tobytes()
    if case["note"].endswith("which 1"):
        got = ek.stats.long_quantiles(**kw)
        assert isinstance(got, ek.DeviceArray) and got.shape[0] == 2
        rows = list(ek.stats.iter_long_quantiles(**lq.kwargs_of(case)))
        assert len(rows) == 2 and all(isinstance(r, np.ndarray) for r in rows)
        lq.judge_case(case, np.stack(rows), "numpy rows " + lq.case_id(case))


@pytest.mark.parametrize("group", GROUPS)
def test_golden_cases_numpy_and_device_array_input(ek, group):
    cases = lq.cases_of(group)
    assert len(cases) == 39
    for case in cases:
        _golden_case(ek, case)


def test_torch_device_tensors():
    """torch ROCm tensors in -> torch tensors out, every golden case; in a child process that imports torch first."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_long_quantiles_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    if r.returncode == 77:
        pytest.skip(r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "torch unavailable")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "LONG_QUANTILES_TORCH_OK" in r.stdout


# ---- the raw entry points inside a guarded arena ----
def _arena_run(tag, arr, tabs, nq, method, off):
    from ekm_hip import _ffi

    lib = _ffi.lib()
    outer, m, inner = arr.shape
    arena = Arena(DeviceMemory(0, None))
    o = [1, 3, 2, 1, 3] if off else [0] * 5
    try:
        arena.input("arr", arr, o[0]), arena.input("lo", tabs[0], o[1]), arena.input("hi", tabs[1], o[2]), arena.input("w", tabs[2], o[3])
        arena.output("out", nq * outer * inner, lq.KINDS[tag][1], o[4])
        arena.commit()
        _ffi.check(getattr(lib, f"ekm_long_quantiles_{tag}")(0, None, arena.ptr("arr"), outer, m, inner, arena.ptr("lo"), arena.ptr("hi"),
                                                            arena.ptr("w"), nq, 0 if method == "sort" else 1, arena.ptr("out")))
        _ffi.check(lib.ekm_stream_sync(0, None))
        arena.check()  # guards and inputs untouched, every element of out written
        return arena.result("out").reshape(nq, outer, inner)
    finally:
        arena.free()


LAYOUTS = [(npts, 1) for npts in (1, 2, 3, 7, 8, 9, 17, 33, 65)] + [(outer, inner) for inner in (3, 70) for outer in (1, 3)]


@pytest.mark.parametrize("m", [1, 2, 257, 300, 512, 513, 1980])
@pytest.mark.parametrize("tag", sorted(lq.KINDS))
def test_entry_points_in_a_guarded_arena(ek, tag, m):
    """npts in {1, 2, 3, 7, 8, 9, 17, 33, 65} with the sample axis last (the contiguous-run load; the tiles hold 1 to 128
    columns, so a short last workgroup is always among them), inner in {3, 70} x outer in {1, 3} (the strided load);
    nq in {1, 5}; buffers 16-B aligned and one to three elements off.  Nothing is written outside `out`, the inputs come
    back unchanged, every element of `out` is written, the bits are the restatement's, and shifting the buffers changes
    none of them."""
    T = lq.KINDS[tag][0]
    methods = ("numpy",) if tag == "f32" else ("sort", "numpy_bulk")
    for n, (outer, inner) in enumerate(LAYOUTS):
        rng = np.random.default_rng(1000 * m + n)
        arr = np.round(rng.normal(0, 2, (outer, m, inner)) * 4) / 4 + 0.0  # ties; + 0.0: no -0.0 beside +0.0 in a column
        arr[0, m // 2, 0] = np.nan
        if outer * inner > 2:
            arr[-1, 0, -1], arr[-1, m - 1, -1] = np.inf, -np.inf
        arr = arr.astype(T)
        for qs in ((0.33,), (0.9, 0.0, 0.5, 1.0, 0.25)):
            method = methods[(n + len(qs)) % len(methods)]
            tabs = lq.tables(method, m, qs, T)
            want = lq.quantiles(arr, list(qs), 1, method)
            runs = [_arena_run(tag, arr, tabs, len(qs), method, off) for off in (False, True)]
            lq.judge_exact(runs[0], want, f"{tag} {method} [{outer}, {m}, {inner}] nq {len(qs)} aligned")
            lq.judge_exact(runs[1], runs[0], f"{tag} {method} [{outer}, {m}, {inner}] nq {len(qs)} shifted against aligned")


def test_entry_point_argument_errors(ek):
    from ekm_hip import _ffi

    lib = _ffi.lib()
    d = ek.DeviceArray.from_host(np.zeros(64, np.float32))
    t = ek.DeviceArray.from_host(np.zeros(4))
    out = ek.DeviceArray.empty((64,), np.float32)
    fn = lib.ekm_long_quantiles_f32
    assert fn(0, None, d.ptr, 8, 8, 1, t.ptr, t.ptr, t.ptr, 1, 0, out.ptr) == _ffi.EKM_ERR_ARG  # sort needs f64 out
    assert fn(0, None, d.ptr, 8, 8, 1, t.ptr, t.ptr, t.ptr, 1, 2, out.ptr) == _ffi.EKM_ERR_ENUM
    assert fn(0, None, d.ptr, 8, 8, 1, None, t.ptr, t.ptr, 1, 1, out.ptr) == _ffi.EKM_ERR_ARG      # null table
    assert fn(0, None, d.ptr, 8, 8, 1, t.ptr, t.ptr, t.ptr, 1, 1, None) == _ffi.EKM_ERR_ARG
    assert fn(0, None, d.ptr, 1 << 40, 8, 1 << 40, t.ptr, t.ptr, t.ptr, 1, 1, out.ptr) == _ffi.EKM_ERR_ARG  # too many points
    assert fn(0, None, d.ptr, 0, 8, 1, t.ptr, t.ptr, t.ptr, 1, 1, None) == _ffi.EKM_OK   # no points
    assert fn(0, None, d.ptr, 8, 8, 1, t.ptr, t.ptr, t.ptr, 0, 1, None) == _ffi.EKM_OK   # no levels
    assert fn(0, None, d.ptr, 8, 0, 1, t.ptr, t.ptr, t.ptr, 1, 1, out.ptr) == _ffi.EKM_ERR_ARG      # m == 0
    for tag, (T, Out) in lq.KINDS.items():  # one past the cap: refused before anything is read
        rc = getattr(lib, f"ekm_long_quantiles_{tag}")(0, None, d.ptr, 1, lq.CAP[T] + 1, 1, t.ptr, t.ptr, t.ptr, 1, 1, out.ptr)
        assert rc == _ffi.EKM_ERR_ARG and f"cap of {lq.CAP[T]}" in lib.ekm_last_error().decode()
    ek.synchronize()


@pytest.mark.parametrize("T,m", [(lq.F32, 1), (lq.F32, 9), (lq.F32, 51), (lq.F32, 256), (lq.F64, 128)],
                         ids=["f32-1", "f32-9", "f32-51", "f32-256", "f64-128"])
def test_short_axes_give_the_bits_of_quantiles(ek, T, m):
    rng = np.random.default_rng(m)
    arr = (np.round(rng.gamma(1.5, 2.0, (m, 3, 67)) * 8) / 8).astype(T)
    arr[m // 2, 1, 5], arr[0, 2, 66] = np.nan, np.inf
    for method in lq.METHODS:
        for axis, a in ((0, arr), (-1, np.ascontiguousarray(np.moveaxis(arr, 0, -1))), (1, np.ascontiguousarray(np.moveaxis(arr, 0, 1)))):
            lq.judge_exact(ek.stats.long_quantiles(a, 100, axis, method), ek.stats.quantiles(a, 100, axis, method), f"m {m} {method} axis {axis}")


@pytest.mark.parametrize("T", [lq.F32, lq.F64], ids=["f32", "f64"])
def test_the_cap_itself_and_one_past_it(ek, T):
    cap = lq.CAP[T]
    arr = np.random.default_rng(2).normal(0, 1, (cap, 3)).astype(T)
    arr[7, 1] = np.nan
    for method, axis, a in (("sort", 0, arr), ("numpy", -1, np.ascontiguousarray(arr.T))):
        lq.judge_exact(ek.stats.long_quantiles(a, 100, axis, method), lq.quantiles(a, 100, axis, method), f"cap {method} axis {axis}")
    for shape, axis in (((cap + 1, 2), 0), ((2, cap + 1), -1), ((2, cap + 1, 3), 1)):
        for method in lq.METHODS:
            with pytest.raises(ek.EkmError, match=f"past the cap of {cap}"):
                ek.stats.long_quantiles(np.zeros(shape, T), 4, axis, method)


@pytest.mark.parametrize("T", [lq.F32, lq.F64], ids=["f32", "f64"])
def test_a_column_gives_the_same_bits_at_any_position_and_in_any_layout(ek, T):
    """The same 40 columns of 300 samples with the sample axis first, last and in the middle, and picked into fields of 1,
    9 and 130 points: a column's bits depend on nothing but its samples."""
    rng = np.random.default_rng(11)
    cols = (np.round(rng.gamma(1.5, 2.0, (300, 40)) * 8) / 8).astype(T)
    cols[3, 5], cols[0, 17], cols[299, 39] = np.nan, np.inf, -np.inf
    for method in lq.METHODS:
        first = ek.stats.long_quantiles(cols, 100, 0, method)
        lq.judge_exact(first, lq.quantiles(cols, 100, 0, method), f"axis 0 {method}")
        last = np.ascontiguousarray(cols.T)
        lq.judge_exact(ek.stats.long_quantiles(last, 100, -1, method), first, f"axis -1 {method}")
        mid = np.ascontiguousarray(cols.reshape(300, 4, 10).transpose(1, 0, 2))
        lq.judge_exact(ek.stats.long_quantiles(mid, 100, 1, method).reshape(101, 40), first, f"axis 1 {method}")
        for n in (1, 9, 130):
            pick = rng.integers(0, 40, n)
            lq.judge_exact(ek.stats.long_quantiles(cols[:, pick], 100, 0, method), first[:, pick], f"picked {n} axis 0 {method}")
            lq.judge_exact(ek.stats.long_quantiles(last[pick], 100, 1, method), first[:, pick], f"picked {n} axis -1 {method}")


# ---- census ----
@functools.lru_cache(maxsize=None)
def _census_field(name):
    rng = np.random.default_rng(2026)
    a = np.maximum(rng.gamma(1.5, 2.0, (1980, 4096)).astype(np.float32) - np.float32(1.0), 0)  # zero-clamped: ties
    a = (np.round(a * 64) / 64).astype(name)
    a[7, ::101] = np.nan
    a[9, 5::409] = np.inf
    return a


@functools.lru_cache(maxsize=None)
def _census_want(name, method):
    return lq.quantiles(_census_field(name), 100, 0, method)


@pytest.mark.parametrize("axis", [0, -1])
@pytest.mark.parametrize("method", ["sort", "numpy"])
@pytest.mark.parametrize("T", [lq.F32, lq.F64], ids=["f32", "f64"])
def test_census_1980_samples_on_4096_points(ek, T, method, axis):
    field, want = _census_field(T.name), _census_want(T.name, method)
    got = ek.stats.long_quantiles(field if axis == 0 else np.ascontiguousarray(field.T), 100, axis, method)
    equal = lq.qn.equal_bits(got, want)
    line = f"long_quantiles census {T.name} {method} axis {axis}: {equal} of {got.size} values equal bits, {int(np.isnan(got).sum())} NaN"
    _compare.CENSUS.append(line)
    print(line)
    assert got.dtype == want.dtype and 0 < np.isnan(got).sum() < got.size
    lq.judge_exact(got, want, line)


@pytest.mark.parametrize("T", [lq.F32, lq.F64], ids=["f32", "f64"])
def test_recorded_graph_replays_the_direct_call(ek, T):
    rng = np.random.default_rng(3)
    arr = rng.normal(0, 1, (700, 500)).astype(T)
    d_first, d_last = ek.to_device(arr), ek.to_device(np.ascontiguousarray(arr.T))
    levels = [0.1, 0.25, 0.5, 0.75, 0.9]
    calls = [(d_first, 100, 0, "sort"), (d_first, levels, 0, "numpy"), (d_last, levels, -1, "numpy_bulk")]
    direct = [ek.stats.long_quantiles(*c).to_host() for c in calls]  # also uploads the position tables, which a recording cannot
    with ek.graph() as g:
        outs = [ek.stats.long_quantiles(*c) for c in calls]
    g.launch()
    for o, want, c in zip(outs, direct, calls):
        lq.judge_exact(o.to_host(), want, "graph replay")
        lq.judge_exact(want, lq.quantiles(arr, c[1], 0, c[3]), "direct")
    g.close()
    with ek.graph() as g2:
        with pytest.raises(ek.EkmError, match=r"inside an ekm_hip.graph\(\) block"):
            ek.stats.long_quantiles(d_first, [0.123], 0, "sort")  # a level set that has no table yet cannot be recorded
    g2.close()


@pytest.mark.parametrize("T", [lq.F32, lq.F64], ids=["f32", "f64"])
def test_a_column_mixing_the_two_zeros_is_the_host_twins(ek, T):
    """NumPy leaves the order of -0.0 and +0.0 open; the keys do not (-0.0 first), and the twin sorts the same keys."""
    rng = np.random.default_rng(8)
    arr = np.round(rng.normal(0, 1, (300, 9)) * 2) / 2  # a third of the values are zeros
    arr[rng.random(arr.shape) < 0.5] *= -1.0             # ... of either sign
    arr = arr.astype(T)
    assert ((arr == 0) & np.signbit(arr)).any(axis=0).all() and ((arr == 0) & ~np.signbit(arr)).any(axis=0).all()
    for method in lq.METHODS:
        for axis, a in ((0, arr), (-1, np.ascontiguousarray(arr.T))):
            lq.judge_exact(ek.stats.long_quantiles(a, 100, axis, method), lq.twin(a, 100, axis, method), f"zeros {method} axis {axis}")
