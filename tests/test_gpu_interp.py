"""Vertical interpolation on the GPU: every golden case through the public API (NumPy, DeviceArray and torch input), a census
of a 137-level, 1 M-column, 37-target problem against the NumPy restatement, the new entry points inside a guarded
arena, and launch-shape independence."""
import ctypes as C

import numpy as np
import pytest

import _interp_golden as gold
import _interp_numpy as inp
from _arena import Arena, DeviceMemory

pytestmark = pytest.mark.gpu
ALL = gold.cases()
HEIGHT = gold.cases("interpolate_hybrid_to_height_levels")
STD_P = 100.0 * np.array([1000, 975, 950, 925, 900, 875, 850, 825, 800, 775, 750, 700, 650, 600, 550, 500, 450, 400, 350, 300,
                          250, 225, 200, 175, 150, 125, 100, 70, 50, 30, 20, 10, 7, 5, 3, 2, 1], dtype=np.float64)


def ledger():
    from _compare import LEDGER

    return LEDGER


def judge(case, got, what):
    """monotonic / hybrid->pressure: linear and nearest bit for bit against the recorded reference, log under the bound
    derived in tests/_interp_golden.py (no point excluded), used / allowed logged to the ledger.
    hybrid->height: see test_hybrid_to_height_*."""
    gold.judge_case(case, got, what, ledger())


@pytest.mark.parametrize("case", [c for c in ALL if c not in HEIGHT], ids=gold.case_id)
def test_golden_cases_numpy_input(ek, case):
    got = getattr(ek.vertical, case["func"])(**gold.kwargs_of(case))
    assert isinstance(got, np.ndarray) and str(got.dtype) == case["out_dtype"]
    judge(case, got, "numpy " + case["note"])


def _on_device(ek, kw):
    out = {}
    for k, v in kw.items():
        if isinstance(v, np.ndarray) and k not in ("A", "B") and v.dtype in (np.float32, np.float64):
            out[k] = ek.DeviceArray.from_host(v)
        else:
            out[k] = v
    return out


@pytest.mark.parametrize("case", [c for c in ALL if c not in HEIGHT and not c["plain"].get("vertical_axis")], ids=gold.case_id)
def test_golden_cases_device_array_input(ek, case):
    """DeviceArray in -> DeviceArray out, level-major, in the arithmetic dtype (cast to data's dtype here, as the NumPy
    path does)."""
    got = getattr(ek.vertical, case["func"])(**_on_device(ek, gold.kwargs_of(case)))
    assert isinstance(got, ek.DeviceArray)
    want = gold.expected_of(case)
    host = got.to_host()
    assert host.shape == want.shape
    judge(case, host.astype(want.dtype), "device " + case["note"])


def test_device_array_needs_vertical_axis_0(ek):
    case = next(c for c in ALL if c["plain"].get("vertical_axis") == 1)
    with pytest.raises(ValueError):
        getattr(ek.vertical, case["func"])(**_on_device(ek, gold.kwargs_of(case)))


def test_integer_data_is_computed_and_returned_in_f64(ek):
    case = next(c for c in ALL if c["note"] == "f64 linear field coord, vector target")
    kw = gold.kwargs_of(case)
    ints = np.rint(kw["data"]).astype(np.int64)
    got = ek.vertical.interpolate_monotonic(**{**kw, "data": ints})
    assert got.dtype == np.float64
    assert inp.same_bits(got, ek.vertical.interpolate_monotonic(**{**kw, "data": ints.astype(np.float64)}))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("ascending", [False, True], ids=["descending", "ascending"])
def test_level_vector_coordinate_over_several_tiles(ek, dtype, ascending):
    """A 1-D coordinate shared by every column of a field of a few tiles plus a ragged tail: targets on a level, between
    levels and beyond both ends, bit for bit against the restatement."""
    nlev, n = 23, 3 * TILE * V[np.dtype(dtype)] + V[np.dtype(dtype)] + 1
    rng = np.random.default_rng(5)
    coord = np.linspace(100000.0, 500.0, nlev).astype(dtype)
    coord = coord[::-1].copy() if ascending else coord
    data = rng.uniform(200.0, 300.0, (nlev, n)).astype(dtype)
    target = np.array([110000.0, coord[0], coord[7], 64321.0, 31000.5, coord[-1], 100.0], dtype)
    for mode in ("linear", "nearest"):
        got = ek.vertical.interpolate_monotonic(data, coord, target, interpolation=mode)
        assert inp.same_bits(got, inp.monotonic(data, coord, target, mode)), mode


# ---- hybrid -> height ----
def _judge_against_own_height_field(ek, case, kw, got):
    """`got` against the NumPy restatement applied to the height field the GPU itself produced (its parity is
    tests/test_gpu_vertical.py's): linear and nearest bit for bit; log under the bound derived in tests/_interp_golden.py
    -- both sides take three logarithms of the same coordinates, which is the case that bound is derived for."""
    h = ek.vertical.height_on_hybrid_levels(kw["t"], kw["q"], kw["zs"], kw["A"], kw["B"], kw["sp"], h_type=kw["h_type"],
                                            h_reference=kw["h_reference"])
    mono = dict(data=kw["data"], coord=h, target_coord=kw["target_h"], aux_min_level_data=kw.get("aux_bottom_data"),
                aux_min_level_coord=kw.get("aux_bottom_h"), aux_max_level_data=kw.get("aux_top_data"),
                aux_max_level_coord=kw.get("aux_top_h"))
    want = inp.monotonic(interpolation=kw["interpolation"], **mono)
    if kw["interpolation"] == "log":
        T = inp.arith_dtype(*[v for v in mono.values() if v is not None])
        bound = gold.log_bound(*gold.bracket_terms(dict(case, func="interpolate_monotonic"), T, mono), T)
        gold.judge_log(got, want, bound.reshape(want.shape), case["note"], ledger())
    else:
        gold.judge_exact(got, want, case["note"])


@pytest.mark.parametrize("case", HEIGHT, ids=gold.case_id)
def test_hybrid_to_height_against_the_restatement_on_the_gpus_own_height_field(ek, case):
    kw = gold.kwargs_of(case)
    _judge_against_own_height_field(ek, case, kw, ek.vertical.interpolate_hybrid_to_height_levels(**kw))


@pytest.mark.parametrize("case", HEIGHT, ids=gold.case_id)
def test_hybrid_to_height_device_array_input(ek, case):
    """DeviceArray in -> DeviceArray out: the height field never leaves device memory and feeds the generic kernel as a
    DeviceArray coordinate, whose ordering is read back from two elements of its first column."""
    kw = gold.kwargs_of(case)
    got = ek.vertical.interpolate_hybrid_to_height_levels(**_on_device(ek, kw))
    assert isinstance(got, ek.DeviceArray)
    want = gold.expected_of(case)
    host = got.to_host()
    assert host.shape == want.shape
    _judge_against_own_height_field(ek, case, kw, host.astype(want.dtype))


def test_torch_device_tensors_through_the_four_functions():
    """torch ROCm tensors into the four functions (every golden case with the level axis first): torch tensors out,
    linear and nearest bit for bit against the recorded reference.  Runs in a child process that imports torch before
    the library is loaded, as tests/test_gpu_streaming.py does for the thermo functions."""
    import os
    import subprocess
    import sys

    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_interp_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    if r.returncode == 77:
        pytest.skip(r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "torch unavailable")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "INTERP_TORCH_OK" in r.stdout


@pytest.mark.parametrize("case", [c for c in HEIGHT if c["plain"]["interpolation"] == "linear"], ids=gold.case_id)
def test_hybrid_to_height_end_to_end_against_the_reference(ek, case):
    """f64, no point excluded (the generator asserts that no target lies within 1e-3 relative of a column's end height).
    The height field agrees with the reference's to 1e-6 relative (the existing bar of tests/test_gpu_vertical.py); a
    relative error e of the coordinates moves the weight (tc - hb) / (ht - hb) by at most e (|tc| + 2|h|max) / |ht - hb|
    <= 3 e |h|max / |dh| with |tc| <= |h|max inside a bracket, and the blend by that times |dt - db|:
    |got - want| <= 3e-6 |h|max / |dh_layer| |dd|  + 8 u max|d| for the rounding of the blend itself."""
    kw = gold.kwargs_of(case)
    got = ek.vertical.interpolate_hybrid_to_height_levels(**kw)
    want = gold.expected_of(case)
    assert got.dtype == want.dtype and np.array_equal(np.isnan(got), np.isnan(want))
    h = ek.vertical.height_on_hybrid_levels(kw["t"], kw["q"], kw["zs"], kw["A"], kw["B"], kw["sp"], h_type=kw["h_type"],
                                            h_reference=kw["h_reference"])
    aux = [kw.get(n) for n in ("aux_bottom_data", "aux_bottom_h", "aux_top_data", "aux_top_h")]
    # bracket terms from the restatement on the GPU's height field
    mono = dict(data=kw["data"], coord=h, target_coord=kw["target_h"], aux_min_level_data=aux[0], aux_min_level_coord=aux[1],
                aux_max_level_data=aux[2], aux_max_level_coord=aux[3])
    tc, c_b, c_t, d_b, d_t = gold.bracket_terms(dict(case, func="interpolate_monotonic"), np.float64, mono)
    hmax = np.maximum(np.abs(c_b), np.abs(c_t))
    bound = 3e-6 * hmax / np.abs(c_t - c_b) * np.abs(d_t - d_b) + 8 * 2.0 ** -53 * np.maximum(np.abs(d_t), np.abs(d_b))
    fin = np.isfinite(want)
    err = np.abs(got - want)[fin]
    worst = float(np.max(err / bound[fin])) if err.size else 0.0
    ledger().append((case["note"], "interp hybrid->height end to end: worst used/allowed in 1e-6", int(round(worst * 1e6)), 1e6, int(fin.sum())))
    assert worst <= 1.0, worst


# ---- census ----
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mode", ["linear", "nearest"])
def test_census_137_levels_1m_columns_37_pressure_levels(ek, dtype, mode):
    """sp from 520 to 1040 hPa: the low targets are below ground in part of the columns.  Bit for bit against the
    restatement; the equal-bits count and the NaN count are printed."""
    from _compare import CENSUS

    n = 1 << 20
    rng = np.random.default_rng(7)
    A, B = ek.vertical.hybrid_level_parameters(137)
    A, B = A.astype(dtype), B.astype(dtype)
    sp = rng.uniform(52000.0, 104000.0, n).astype(dtype)
    data = (250.0 + 40.0 * rng.standard_normal((137, n), dtype=np.float32)).astype(dtype)
    tp = STD_P.astype(dtype)
    got = ek.vertical.interpolate_hybrid_to_pressure_levels(data, tp, A, B, sp, interpolation=mode)
    want = inp.hybrid_to_pressure(data, tp, A, B, sp, interpolation=mode)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    equal = int(np.sum((got == want) | (nan_g & nan_w)))
    line = f"interp census {np.dtype(dtype).name} {mode}: {equal} of {got.size} points equal bits, {int(nan_g.sum())} NaN (restatement {int(nan_w.sum())})"
    CENSUS.append(line)
    print(line)
    assert got.dtype == dtype and np.array_equal(nan_g, nan_w) and equal == got.size
    if mode == "linear":
        assert 0 < nan_g.sum() < got.size  # below ground in part of the columns


# ---- the entry points inside a guarded arena ----
V = {np.dtype(np.float32): 4, np.dtype(np.float64): 2}
TILE = 256


def _arena_problem(dtype, npts, nlev, ntarget, rng):
    x = np.linspace(0.0, 1.0, nlev + 1)
    A, B = 30000.0 * x * (1.0 - x), x ** 2  # half-level pressures increase downwards for every sp >= 520 hPa
    A, B = A.astype(dtype), B.astype(dtype)
    sp = rng.uniform(52000.0, 104000.0, npts).astype(dtype)
    data = rng.uniform(200.0, 300.0, (nlev, npts)).astype(dtype)
    target = np.linspace(110000.0, 100.0, ntarget).astype(dtype)
    return A, B, sp, data, target


def _run_arena(ek, dtype, npts, fused, offsets, mode=0, target_field=False):
    from ekm_hip import _ffi

    lib = _ffi.lib()
    dtype = np.dtype(dtype)
    nlev, ntarget = 23, 5
    rng = np.random.default_rng(npts * 2 + int(fused))
    A, B, sp, data, target = _arena_problem(dtype, npts, nlev, ntarget, rng)
    coord = inp.hybrid_pressure(A, B, sp, nlev, dtype)
    if target_field:
        target = (target[:, None] * rng.uniform(0.9, 1.1, (ntarget, npts))).astype(dtype)
    aux_d, aux_c = rng.uniform(280.0, 300.0, npts).astype(dtype), (sp * dtype.type(1.001)).astype(dtype)
    arena = Arena(DeviceMemory(0, None))
    o = iter(offsets)
    arena.input("data", data, next(o))
    arena.input("coord", coord, next(o)) if not fused else None
    arena.input("A", A), arena.input("B", B), arena.input("sp", sp, next(o))
    arena.input("target", target, next(o))
    arena.input("aux_d", aux_d, next(o)), arena.input("aux_c", aux_c, next(o)), arena.input("top_d", np.array([210.0], dtype)), arena.input("top_c", np.array([50.0], dtype))
    arena.output("out", ntarget * npts, dtype, next(o))
    arena.commit()
    tag = "f32" if dtype == np.float32 else "f64"
    tail = [arena.ptr("target"), int(target_field), ntarget, npts, nlev, 0, mode, arena.ptr("top_d"), arena.ptr("top_c"),
            arena.ptr("aux_d"), arena.ptr("aux_c"), 0b1100, arena.ptr("out")]
    try:
        if fused:
            _ffi.check(getattr(lib, f"ekm_interpolate_hybrid_to_pressure_{tag}")(
                0, None, arena.ptr("data"), arena.ptr("A"), arena.ptr("B"), arena.ptr("sp"), *tail))
        else:
            _ffi.check(getattr(lib, f"ekm_interpolate_monotonic_{tag}")(0, None, arena.ptr("data"), arena.ptr("coord"), 1, *tail))
        _ffi.check(lib.ekm_stream_sync(0, None))
        arena.check()
        return arena.result("out").reshape(ntarget, npts), (data, coord, target, aux_d, aux_c)
    finally:
        arena.free()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("fused", [False, True], ids=["generic", "fused"])
def test_entry_points_in_a_guarded_arena(ek, dtype, fused):
    """Sizes 1, V-1, V+1, one tile +- 1, a few tiles plus a ragged tail; aligned and misaligned starts: guard words and
    inputs untouched, every output element written, bits equal to the aligned run and to the restatement."""
    v = V[np.dtype(dtype)]
    per_tile = TILE * v
    for npts in (1, v - 1, v + 1, per_tile - 1, per_tile, per_tile + 1, 3 * per_tile + v + 1, 4 * per_tile):
        for mode in (0, 2):
            aligned, (data, coord, target, aux_d, aux_c) = _run_arena(ek, dtype, npts, fused, [0] * 8, mode)
            shifted, _ = _run_arena(ek, dtype, npts, fused, [1, 3, 1, 2, 3, 1, 1, 3], mode)
            assert inp.same_bits(aligned, shifted), (npts, mode)
            want, _ = inp.columns(data, coord, target, ("linear", "log", "nearest")[mode], (np.array([210.0], dtype), np.array([50.0], dtype)),
                                  (aux_d, aux_c), dtype=dtype, descending=False)
            assert inp.same_bits(aligned, want), (npts, mode)
        field, (data, coord, target, aux_d, aux_c) = _run_arena(ek, dtype, npts, fused, [1, 0, 3, 1, 0, 2, 1, 1], 0, target_field=True)
        want, _ = inp.columns(data, coord, target, "linear", (np.array([210.0], dtype), np.array([50.0], dtype)), (aux_d, aux_c),
                              dtype=dtype, descending=False)
        assert inp.same_bits(field, want), npts


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_column_gives_the_same_bits_at_any_position(ek, dtype):
    """Launch-shape independence: 13 distinct columns tiled over arrays of several lengths; every copy of a column, at
    whatever lane, tile or band it lands and whatever its neighbours bracket, gives the bits of the first copy."""
    rng = np.random.default_rng(11)
    A, B = ek.vertical.hybrid_level_parameters(137)
    A, B = A.astype(dtype), B.astype(dtype)
    base_sp = rng.uniform(52000.0, 104000.0, 13).astype(dtype)
    base_d = rng.uniform(200.0, 300.0, (137, 13)).astype(dtype)
    tp = STD_P.astype(dtype)
    first = None
    for n in (13, 1024, 1027, 5 * 1024 + 3, 300001):
        pick = np.arange(n) % 13 if n < 2000 else rng.integers(0, 13, n)
        for mode in ("linear", "log", "nearest"):
            got = ek.vertical.interpolate_hybrid_to_pressure_levels(base_d[:, pick], tp, A, B, base_sp[pick], interpolation=mode)
            p = ek.vertical.pressure_on_hybrid_levels(A, B, base_sp[pick])
            two = ek.vertical.interpolate_monotonic(base_d[:, pick], p, tp, interpolation=mode)
            if first is None or mode not in first:
                first = dict(first or {}, **{mode: got[:, :13].copy()})
                assert n == 13
            assert inp.same_bits(got, first[mode][:, pick]), (n, mode)
            if mode != "log":  # the generic kernel on the stored pressure: same bits wherever that pressure has the reference's bits
                same_p = np.all(p == inp.hybrid_pressure(A, B, base_sp[pick], 137, dtype), axis=0)
                assert inp.same_bits(two[:, same_p], got[:, same_p]), (n, mode)
