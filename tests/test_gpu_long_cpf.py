"""extreme.long_cpf on the GPU: the recorded cases (columns the short `cpf` refuses) through the public API with NumPy,
DeviceArray and torch input; the tile geometry (each pairing of the small and the full tile, ragged last tiles, the
contiguous-run load of a single point, the cap) against the host twin, which the CPU suite pins to the recorded reference
and to the restatement; short shapes against `cpf`; one past either cap; the raw entry points in a guarded arena.  Every
comparison is bit for bit with no point excluded; no input column mixes the two zeros."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _long_cpf as lc
from _arena import Arena, DeviceMemory
from ekm_hip import extreme

pytestmark = pytest.mark.gpu
extreme.long_cpf  # absent before this feature

TYPES = pytest.mark.parametrize("T", [lc.F32, lc.F64], ids=["f32", "f64"])


def _host(res):
    return np.asarray(res.to_host() if hasattr(res, "to_host") else res)


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_golden_cases_numpy_and_device_array_input(ek, tag):
    cases = lc.cases(tag)
    assert len(cases) == 72
    for case in cases:
        kw = lc.kwargs_of(case)
        clim, ens = kw["clim"].copy(), kw["ens"].copy()
        options = {k: v for k, v in kw.items() if k not in ("clim", "ens")}
        got = ek.extreme.long_cpf(clim, ens, **options)
        assert isinstance(got, np.ndarray)
        lc.judge_case(case, got, "numpy " + lc.case_id(case))
        d_clim, d_ens = ek.DeviceArray.from_host(clim), ek.DeviceArray.from_host(ens)
        got = ek.extreme.long_cpf(d_clim, d_ens, **options)
        assert isinstance(got, ek.DeviceArray)  # DeviceArray in -> DeviceArray out
        lc.judge_case(case, got.to_host(), "device " + lc.case_id(case))
        for mine, dev, given in ((clim, d_clim, kw["clim"]), (ens, d_ens, kw["ens"])):  # never sorted in place
            assert mine.tobytes() == given.tobytes() == dev.to_host().tobytes()


def test_torch_device_tensors():
    """torch ROCm tensors in -> torch tensors out; in a child process that imports torch first."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_long_cpf_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    if r.returncode == 77:
        pytest.skip(r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "torch unavailable")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "LONG_CPF_TORCH_OK" in r.stdout


# (nclim, nens) for f32 and, the large axis halved, for f64; the columns per workgroup C each must give
GEOMETRY = [(lc.F32, 40, 300, 8), (lc.F32, 101, 5000, 2), (lc.F32, 5000, 51, 2), (lc.F32, 4097, 4097, 2), (lc.F32, 16384, 16384, 1),
            (lc.F64, 40, 150, 8), (lc.F64, 101, 2500, 2), (lc.F64, 2500, 51, 2), (lc.F64, 2049, 2049, 2), (lc.F64, 8192, 8192, 1)]
GEOMETRY_OPTIONS = (dict(), dict(symmetric=True, from_zero=True), dict(sort_clim=False, sort_ens=False, from_zero=True),
                    dict(sort_ens=False, epsilon=0.5), dict(sort_clim=False, symmetric=True))


@pytest.mark.parametrize("T,nclim,nens,C", GEOMETRY, ids=[f"{lc.TAG[g[0]]}-{g[1]}x{g[2]}" for g in GEOMETRY])
def test_tile_geometry_against_the_host_twin(ek, T, nclim, nens, C):
    """small + small (f32: 64 climate columns against 8 ensemble columns), small + full, full + small, full + full (2
    columns) and the cap on both axes (1 column).  npts = 1 is the contiguous-run load, the others the strided load with
    a ragged last tile (C - 1, C + 1, 3 C + 1) or a full one (C)."""
    assert lc.columns_per_tile(T, nclim, nens) == C
    rng = np.random.default_rng(nclim * 7 + nens)
    for k, npts in enumerate(sorted({n for n in (1, C - 1, C, C + 1, 3 * C + 1) if n > 0})):
        clim, ens = lc.fields(rng, nclim, nens, npts, T)
        assert lc.no_column_mixes_the_zeros(clim) and lc.no_column_mixes_the_zeros(ens)
        for options in (GEOMETRY_OPTIONS[k % 5], GEOMETRY_OPTIONS[(k + 2) % 5]):
            got = ek.extreme.long_cpf(clim, ens, **options)
            lc.judge_exact(got, lc.twin(clim, ens, **options), f"{nclim}x{nens} npts {npts} {options}")


@pytest.mark.parametrize("nclim,nens", [(101, 51), (3, 1), (2, 5)])
@TYPES
def test_short_shapes_give_the_bits_of_cpf(ek, T, nclim, nens):
    """Where both functions apply, the long result is the short result, every bit, under the 12 option sets; fewer than
    three climate rows give zeros (ones under `symmetric`)."""
    rng = np.random.default_rng(nclim + nens)
    clim, ens = lc.fields(rng, nclim, nens, 257, T)
    d_clim, d_ens = ek.DeviceArray.from_host(clim), ek.DeviceArray.from_host(ens)
    for options in lc.OPTION_SETS:
        got = ek.extreme.long_cpf(d_clim, d_ens, **options).to_host()
        lc.judge_exact(got, ek.extreme.cpf(d_clim, d_ens, **options).to_host(), f"{nclim}x{nens} {options}")
        lc.judge_exact(got, lc.twin(clim, ens, **options), f"twin {nclim}x{nens} {options}")
        if nclim < 3:  # no interior row: the scan writes nothing, and `symmetric` turns that 0 into 1 - 0 (cpf.py:150-153)
            assert got.tobytes() == np.full(257, 1 if options.get("symmetric") else 0, np.float32).tobytes()


@TYPES
def test_one_past_either_cap_is_an_error_that_names_the_axis_and_writes_nothing(ek, T):
    """The argument check refuses the call before any launch."""
    from ekm_hip import _ffi

    cap, tag, lib = lc.CAP[T], lc.TAG[T], _ffi.lib()
    rows, over = np.zeros((101, 3), T), np.zeros((cap + 1, 3), T)
    with pytest.raises(ek.EkmError, match=f"long_cpf: {cap + 1} members are past the cap of {cap}"):
        ek.extreme.long_cpf(rows, over)
    with pytest.raises(ek.EkmError, match=f"long_cpf: {cap + 1} climate rows are past the cap of {cap}"):
        ek.extreme.long_cpf(over, rows, sort_clim=False)
    d_rows, d_over = ek.DeviceArray.from_host(rows), ek.DeviceArray.from_host(over)
    out = ek.DeviceArray.from_host(np.full(3, 7, np.float32))
    fn = getattr(lib, f"ekm_long_cpf_{tag}")
    assert fn(0, None, d_rows.ptr, d_over.ptr, 101, cap + 1, 3, 1, 1, 0, 0, 0, 0.0, out.ptr) == _ffi.EKM_ERR_ARG
    assert f"{cap + 1} members are past the cap of {cap}" in lib.ekm_last_error().decode()
    assert fn(0, None, d_over.ptr, d_rows.ptr, cap + 1, 101, 3, 1, 1, 0, 0, 0, 0.0, out.ptr) == _ffi.EKM_ERR_ARG
    assert f"{cap + 1} climate rows are past the cap of {cap}" in lib.ekm_last_error().decode()
    assert fn(0, None, d_rows.ptr, d_rows.ptr, 0, 101, 3, 1, 1, 0, 0, 0, 0.0, out.ptr) == _ffi.EKM_ERR_ARG
    assert fn(0, None, d_rows.ptr, d_rows.ptr, 101, 0, 3, 1, 1, 0, 0, 0, 0.0, out.ptr) == _ffi.EKM_ERR_ARG
    assert fn(0, None, d_rows.ptr, d_rows.ptr, 101, 101, 3, 1, 1, 0, 0, 0, 0.0, None) == _ffi.EKM_ERR_ARG          # no output
    assert fn(0, None, d_rows.ptr + 1, d_rows.ptr, 101, 100, 3, 1, 1, 0, 0, 0, 0.0, out.ptr) == _ffi.EKM_ERR_ARG   # misaligned
    assert fn(0, None, d_rows.ptr, d_rows.ptr, 101, 101, 0, 1, 1, 0, 0, 0, 0.0, None) == _ffi.EKM_OK               # no points
    ek.synchronize()
    assert (out.to_host() == 7).all()


def _arena_run(ek, T, nclim, nens, npts, options, off):
    """One launch with every buffer inside a guarded arena, 16-B aligned (off = 0) or one to three elements off: guards
    and inputs untouched, every output element written (the arena's own checks), the host twin's bits."""
    from ekm_hip import _ffi

    clim, ens = lc.fields(np.random.default_rng(nclim + 3 * nens + npts), nclim, nens, npts, T)
    o = [1, 3, 2] if off else [0, 0, 0]
    arena = Arena(DeviceMemory(0, None))
    try:
        arena.input("clim", clim, o[0]), arena.input("ens", ens, o[1])
        arena.output("out", npts, np.float32, o[2])
        arena.commit()
        use_eps = options.get("epsilon") is not None and not options.get("symmetric", False)
        rc = getattr(_ffi.lib(), f"ekm_long_cpf_{lc.TAG[T]}")(
            0, None, arena.ptr("clim"), arena.ptr("ens"), nclim, nens, npts, int(options.get("sort_clim", True)),
            int(options.get("sort_ens", True)), int(options.get("from_zero", False)), int(options.get("symmetric", False)),
            int(use_eps), float(options["epsilon"]) if use_eps else 0.0, arena.ptr("out"))
        _ffi.check(rc)
        _ffi.check(_ffi.lib().ekm_stream_sync(0, None))
        arena.check()
        got = arena.result("out")
        lc.judge_exact(got, lc.twin(clim, ens, **options), f"arena {nclim}x{nens} npts {npts} {options} off {off}")
        return got
    finally:
        arena.free()


@TYPES
def test_entry_points_in_a_guarded_arena(ek, T):
    """Each pairing of tiles at point counts on both sides of a tile and at a single point (the contiguous run, whose
    ragged head and tail a shifted buffer moves); shifting the buffers changes no bit."""
    big = 5000 if T == lc.F32 else 2500
    for k, (nclim, nens, npts) in enumerate(((101, 51, 65), (700, 300, 9), (101, big, 3), (big, 51, 5), (big, big, 1), (1980, 51, 1))):
        options = GEOMETRY_OPTIONS[k % 5]
        a = _arena_run(ek, T, nclim, nens, npts, options, False)
        b = _arena_run(ek, T, nclim, nens, npts, options, True)
        lc.judge_exact(b, a, f"{nclim}x{nens}: shifted against aligned buffers")
