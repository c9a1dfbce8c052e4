"""extreme.long_efi, extreme.long_sot, score.long_crps_from_ensemble and stats.GumbelDistribution.long_fit on the GPU: the
golden cases (257 to 1980 members) through the public API with NumPy, DeviceArray and torch input; short axes against the
short functions; the tile geometry (short last tiles, the switch between the two tile sizes, the cap and one past it)
against the NumPy restatements, which the CPU suite pins to the recorded reference; the fit with its sample axis first, in
the middle and last; the raw entry points in a guarded arena with shifted buffers; a non-default stream and a recorded
graph.  Every comparison is bit for bit with no point excluded; no input column mixes the two zeros."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _long_ensemble as le
from _arena import UNWRITTEN, Arena, DeviceMemory
from ekm_hip import extreme, score, stats

pytestmark = pytest.mark.gpu
extreme.long_efi, extreme.long_sot, score.long_crps_from_ensemble, stats.GumbelDistribution.long_fit  # absent before this feature

TYPES = pytest.mark.parametrize("T", [le.F32, le.F64], ids=["f32", "f64"])


def _long(ek, func):
    return {"efi": ek.extreme.long_efi, "sot": ek.extreme.long_sot, "crps_from_ensemble": ek.score.long_crps_from_ensemble,
            "fit": ek.stats.GumbelDistribution.long_fit}[func]


def _short(ek, func):
    return {"efi": ek.extreme.efi, "sot": ek.extreme.sot, "crps_from_ensemble": ek.score.crps_from_ensemble,
            "fit": ek.stats.GumbelDistribution.fit}[func]


def _host(res):
    """A result as NumPy: an array, or the (mu, sigma) of a distribution."""
    if isinstance(res, stats.GumbelDistribution):
        return tuple(np.asarray(v.to_host() if hasattr(v, "to_host") else v) for v in (res.mu, res.sigma))
    return np.asarray(res.to_host() if hasattr(res, "to_host") else res)


def _judge(got, want, what):
    got, want = _host(got), _host(want)
    if isinstance(want, tuple):
        le.judge_exact(got[0], want[0], what + " mu")
        le.judge_exact(got[1], want[1], what + " sigma")
    else:
        le.judge_exact(got, want, what)


def _want_of(ek, case):
    """What a golden case must give here: the recorded result, or -- where this host's libm rounds an EFI coefficient
    otherwise than the recording host's -- the restatement with the product's own tables, still in bits."""
    if case["func"] == "efi":
        own = ek.extreme.efi_coefficients(101)
        if not all(np.array_equal(a, b) for a, b in zip(own, le.recorded_tables())):
            return le.restate_case(case, tables=own)
    return le.expected_of(case)


@pytest.mark.parametrize("func,tag", [(f, t) for f in le.FUNCS for t in ("f32", "f64")])
def test_golden_cases_numpy_and_device_array_input(ek, func, tag):
    cases = le.cases(func, tag)
    assert len(cases) == (20 if func in ("efi", "sot") else 5)
    for case in cases:
        kw, want = le.kwargs_of(case), _want_of(ek, case)
        before = {k: v.copy() for k, v in kw.items() if isinstance(v, np.ndarray)}
        got = _long(ek, func)(**kw)
        assert all(isinstance(v, np.ndarray) for v in (_host(got) if func == "fit" else (got,)))
        if func == "fit":
            assert isinstance(got.mu, np.ndarray) and isinstance(got.sigma, np.ndarray)
        _judge(got, want, "numpy " + le.case_id(case))
        dev = {k: (ek.DeviceArray.from_host(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
        got = _long(ek, func)(**dev)
        assert isinstance(got.mu if func == "fit" else got, ek.DeviceArray)
        _judge(got, want, "device " + le.case_id(case))
        for k, v in before.items():  # never sorted in place
            assert v.tobytes() == kw[k].tobytes() and v.tobytes() == dev[k].to_host().tobytes()
    if func == "fit":  # the same class: its functions work on the result unchanged
        dist = ek.stats.GumbelDistribution.long_fit(le.kwargs_of(cases[0])["sample"][:, :9], freq=2.0)
        same = ek.stats.GumbelDistribution(dist.mu, dist.sigma, freq=2.0)
        assert type(dist) is ek.stats.GumbelDistribution and dist.shape == (9,)
        for call in (lambda d: d.cdf([290.0, 300.0]), lambda d: d.ppf([0.5, 0.99]), lambda d: ek.stats.value_to_return_period(d, 300.0),
                     lambda d: ek.stats.return_period_to_value(d, [10.0, 100.0])):
            le.judge_exact(call(dist), call(same), "functions of the fitted distribution")


def test_torch_device_tensors():
    """torch ROCm tensors in -> torch tensors out, every golden case; in a child process that imports torch first."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_long_ensemble_torch_child.py")
    r = subprocess.run([sys.executable, child], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    if r.returncode == 77:
        pytest.skip(r.stdout.strip().splitlines()[-1] if r.stdout.strip() else "torch unavailable")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "LONG_ENSEMBLE_TORCH_OK" in r.stdout


# ---- one call of every function on one ensemble ----
def _calls(ek, pick, clim, ens, y, nclim_efi=101):
    """{name: result} of the long (`pick` = _long) or the short (`pick` = _short) functions on one ensemble [nens, npts]."""
    c_efi = clim if nclim_efi == 101 else np.ascontiguousarray(clim[::100 // (nclim_efi - 1)])
    res = {"efi -0.1": pick(ek, "efi")(c_efi, ens), "efi 0.5": pick(ek, "efi")(c_efi, ens, eps=0.5),
           "sot 10 0.75": pick(ek, "sot")(clim, ens, 10, eps=0.75), "sot 90": pick(ek, "sot")(clim, ens, 90),
           "crps": pick(ek, "crps_from_ensemble")(ens, y)}
    if ens.shape[0] >= 2:
        res["fit"] = pick(ek, "fit")(ens)
    return res


def _restated(ek, clim, ens, y, nclim_efi=101):
    c_efi = clim if nclim_efi == 101 else np.ascontiguousarray(clim[::100 // (nclim_efi - 1)])
    tables = ek.extreme.efi_coefficients(c_efi.shape[0])
    res = {"efi -0.1": le.restate("efi", clim=c_efi, ens=ens, tables=tables),
           "efi 0.5": le.restate("efi", clim=c_efi, ens=ens, eps=0.5, tables=tables),
           "sot 10 0.75": le.restate("sot", clim=clim, ens=ens, perc=10, eps=0.75), "sot 90": le.restate("sot", clim=clim, ens=ens, perc=90),
           "crps": le.restate("crps_from_ensemble", x=ens, y=y)}
    if ens.shape[0] >= 2:
        res["fit"] = le.restate("fit", sample=ens)
    return res


def _data(seed, nens, npts, T):
    rng = np.random.default_rng(seed)
    ens, clim = le.field(rng, nens, npts, T), le.climate(rng, npts, T, sort=bool(seed % 2))
    y = (ens[0] + T.type(0.5)).astype(T)
    if npts > 1:
        y[-1] = np.nan
    assert le.no_column_mixes_the_zeros(ens) and le.no_column_mixes_the_zeros(clim)
    return clim, ens, y


@pytest.mark.parametrize("npts", [1, 63, 65, 257, 4097])
@TYPES
def test_short_axes_give_the_bits_of_the_short_functions(ek, T, npts):
    """Where both functions apply, the long result is the short result, every bit."""
    for nens in (1, 2, 31, 32, 33, 51, 64, 65, 128) + ((256,) if T == le.F32 else ()):
        clim, ens, y = _data(1000 * nens + npts, nens, npts, T)
        long_res, short_res = _calls(ek, _long, clim, ens, y), _calls(ek, _short, clim, ens, y)
        assert set(long_res) == set(short_res) and len(long_res) == (6 if nens >= 2 else 5)
        for name in long_res:
            _judge(long_res[name], short_res[name], f"{name} nens {nens} npts {npts}")


GEOMETRY = [(le.F32, 51, npts) for npts in (63, 64, 65)] + [(le.F32, 1980, npts) for npts in (7, 8, 9)]  # a short last tile
GEOMETRY += [(le.F32, 4096, 3), (le.F32, 4097, 3), (le.F64, 2048, 3), (le.F64, 2049, 3)]                     # the tile switch
GEOMETRY += [(le.F32, le.CAP[le.F32], 3), (le.F64, le.CAP[le.F64], 3)]                                       # the cap itself


@pytest.mark.parametrize("T,nens,npts", GEOMETRY, ids=[f"{le.TAG[T]}-{nens}-{npts}" for T, nens, npts in GEOMETRY])
def test_tile_geometry_against_the_restatement(ek, T, nens, npts):
    """f32: 64 columns per small tile at 51 members, 8 per full tile at 1980; 4096 / 4097 (f64 2048 / 2049) members are
    the last small tile and the first full one; at the cap a tile is one column.  (efi against 11 climate rows.)"""
    clim, ens, y = _data(nens + npts, nens, npts, T)
    got, want = _calls(ek, _long, clim, ens, y, 11), _restated(ek, clim, ens, y, 11)
    assert set(got) == set(want) and len(got) == 6
    for name in got:
        _judge(got[name], want[name], f"{name} nens {nens} npts {npts}")


@TYPES
def test_one_past_the_cap_is_an_error_that_names_it_and_writes_nothing(ek, T):
    from ekm_hip import _ffi

    cap, tag, lib = le.CAP[T], le.TAG[T], _ffi.lib()
    clim, ens = np.zeros((101, 3), T), np.zeros((cap + 1, 3), T)
    for call in (lambda: ek.extreme.long_efi(clim, ens), lambda: ek.extreme.long_sot(clim, ens, 90),
                 lambda: ek.score.long_crps_from_ensemble(ens, ens[0]), lambda: ek.stats.GumbelDistribution.long_fit(ens),
                 lambda: ek.stats.GumbelDistribution.long_fit(np.zeros((2, cap + 1, 3), T), axis=1),
                 lambda: ek.stats.GumbelDistribution.long_fit(np.zeros((3, cap + 1), T), axis=-1)):
        with pytest.raises(ek.EkmError, match=f"past the cap of {cap}"):
            call()
    # the raw entry points: the outputs keep what they held
    d_c, d_e, d_t = ek.DeviceArray.from_host(clim), ek.DeviceArray.from_host(ens), ek.DeviceArray.from_host(np.zeros(cap + 2))
    fill = np.full(3, 7.0)
    o64, o64b, oT = ek.DeviceArray.from_host(fill), ek.DeviceArray.from_host(fill), ek.DeviceArray.from_host(fill.astype(T))
    flags = ek.DeviceArray.from_host(np.full(4, 7, np.int32))
    rcs = [getattr(lib, f"ekm_long_efi_{tag}")(0, None, d_c.ptr, d_e.ptr, 101, cap + 1, 3, -0.1, d_t.ptr, d_t.ptr, d_t.ptr, o64.ptr),
           getattr(lib, f"ekm_long_sot_{tag}")(0, None, d_c.ptr, d_c.ptr, d_e.ptr, cap + 1, 3, 90, -1e4, oT.ptr),
           getattr(lib, f"ekm_long_crps_from_ensemble_{tag}")(0, None, d_e.ptr, d_c.ptr, cap + 1, 3, d_t.ptr, d_t.ptr, o64.ptr, flags.ptr),
           getattr(lib, f"ekm_long_gumbel_fit_{tag}")(0, None, d_e.ptr, 1, cap + 1, 3, o64.ptr, o64b.ptr)]
    for rc in rcs:
        assert rc == _ffi.EKM_ERR_ARG
    assert f"past the cap of {cap}" in lib.ekm_last_error().decode()
    ek.synchronize()
    assert (o64.to_host() == 7).all() and (o64b.to_host() == 7).all() and (oT.to_host() == 7).all() and (flags.to_host() == 7).all()
    assert getattr(lib, f"ekm_long_gumbel_fit_{tag}")(0, None, d_e.ptr, 3, 1, 1, o64.ptr, o64b.ptr) == _ffi.EKM_ERR_ARG  # one sample
    assert getattr(lib, f"ekm_long_efi_{tag}")(0, None, d_c.ptr, d_e.ptr, 101, 0, 3, -0.1, d_t.ptr, d_t.ptr, d_t.ptr, o64.ptr) == _ffi.EKM_ERR_ARG
    assert getattr(lib, f"ekm_long_efi_{tag}")(0, None, d_c.ptr, d_e.ptr, 101, 300, 0, -0.1, d_t.ptr, d_t.ptr, d_t.ptr, None) == _ffi.EKM_OK  # no points


@TYPES
def test_fit_with_the_sample_axis_first_in_the_middle_and_last(ek, T):
    """The [outer, m, inner] addressing: inner > 1 is the strided tile load, inner == 1 the contiguous run."""
    rng = np.random.default_rng(21)
    for m, npts in ((300, 40), (51, 130), (1980, 10)):
        cols = le.field(rng, m, npts, T)
        want = le.restate("fit", sample=cols)
        _judge(ek.stats.GumbelDistribution.long_fit(cols), want, f"axis 0 m {m}")
        last = np.ascontiguousarray(cols.T)
        _judge(ek.stats.GumbelDistribution.long_fit(last, axis=-1), want, f"axis -1 m {m}")
        mid = np.ascontiguousarray(cols.reshape(m, 2, npts // 2).transpose(1, 0, 2))
        got = ek.stats.GumbelDistribution.long_fit(ek.to_device(mid), axis=1)
        assert got.shape == (2, npts // 2)
        _judge((got.mu.to_host().reshape(-1), got.sigma.to_host().reshape(-1)), want, f"axis 1 m {m}")


# ---- the raw entry points inside a guarded arena ----
def _arena_run(ek, func, T, nens, npts, off):
    """One launch with every buffer inside a guarded arena, 16-B aligned (off = 0) or one to three elements off.  Returns
    the outputs after the arena's own checks: guards and inputs untouched, every output element written."""
    from ekm_hip import _ffi

    lib, tag = _ffi.lib(), le.TAG[T]
    clim, ens, y = _data(7 * nens + npts, nens, npts, T)
    o = [1, 3, 2, 1, 3] if off else [0] * 5
    arena = Arena(DeviceMemory(0, None))
    try:
        arena.input("ens", ens, o[0])
        if func == "efi":
            c11 = np.ascontiguousarray(clim[::10])
            tables = ek.extreme.efi_coefficients(11)
            arena.input("clim", c11, o[1])
            for name, tab in zip(("acosdiff", "proddiff", "acoef"), tables):
                arena.input(name, tab, o[2])
            arena.output("out", npts, np.float64, o[3])
            arena.commit()
            rc = getattr(lib, f"ekm_long_efi_{tag}")(0, None, arena.ptr("clim"), arena.ptr("ens"), 11, nens, npts, 0.5, arena.ptr("acosdiff"),
                                                   arena.ptr("proddiff"), arena.ptr("acoef"), arena.ptr("out"))
            want = {"out": le.restate("efi", clim=c11, ens=ens, eps=0.5, tables=tables)}
        elif func == "sot":
            arena.input("qc", clim[10], o[1]), arena.input("tail", clim[1], o[2])
            arena.output("out", npts, T, o[3])
            arena.commit()
            rc = getattr(lib, f"ekm_long_sot_{tag}")(0, None, arena.ptr("qc"), arena.ptr("tail"), arena.ptr("ens"), nens, npts, 10, 0.75,
                                                   arena.ptr("out"))
            want = {"out": le.restate("sot", clim=clim, ens=ens, perc=10, eps=0.75)}
        elif func == "crps":
            p = np.arange(nens + 1) / float(nens)
            arena.input("y", y, o[1]), arena.input("p2", p**2, o[2]), arena.input("q2", (1 - p) ** 2, o[4])
            arena.output("out", npts, np.float64, o[3])
            arena.output("missing", (npts + 3) // 4 + 1, np.uint32, 0)
            arena.commit()
            rc = getattr(lib, f"ekm_long_crps_from_ensemble_{tag}")(0, None, arena.ptr("ens"), arena.ptr("y"), nens, npts, arena.ptr("p2"),
                                                                  arena.ptr("q2"), arena.ptr("out"), arena.ptr("missing") + o[1])
            total, miss = le.en.crps(ens, y)
            want = {"out": total, "flags": miss.astype(np.uint8)}
        else:
            arena.output("mu", npts, np.float64, o[3]), arena.output("sigma", npts, np.float64, o[4])
            arena.commit()
            rc = getattr(lib, f"ekm_long_gumbel_fit_{tag}")(0, None, arena.ptr("ens"), 1, nens, npts, arena.ptr("mu"), arena.ptr("sigma"))
            mu, sigma = le.restate("fit", sample=ens)
            want = {"mu": mu, "sigma": sigma}
        _ffi.check(rc)
        _ffi.check(lib.ekm_stream_sync(0, None))
        if func == "crps":  # the byte flags: exactly npts bytes written, from the byte the call was given
            arena.image = arena.mem.download(arena.base, arena.size)
            raw = arena.result("missing").view(np.uint8)
            fill = np.resize(np.array([UNWRITTEN], np.uint32).view(np.uint8), raw.size)
            assert np.array_equal(raw[:o[1]], fill[:o[1]]) and np.array_equal(raw[o[1] + npts:], fill[o[1] + npts:])
            got_flags = raw[o[1]:o[1] + npts].copy()
            arena.bufs["missing"].kind = "inout"  # judged here: its unwritten tail is as it must be
        arena.check()
        got = {k: arena.result(k) for k in want if k != "flags"}
        if func == "crps":
            got["flags"] = got_flags
        for k in want:
            le.judge_exact(got[k], want[k], f"{func} {tag} {k} nens {nens} npts {npts} off {off}")
        return got
    finally:
        arena.free()


@pytest.mark.parametrize("func", ["efi", "sot", "crps", "fit"])
@TYPES
def test_entry_points_in_a_guarded_arena(ek, T, func):
    """51 members (small tile, 64 / 32 columns), 300 (small tile), 1980 (full tile, 8 / 4 columns) at point counts on both sides
    of a tile; buffers 16-B aligned and one to three elements off: guard words and inputs untouched, every output element
    written and no other (mu and sigma; the `missing` bytes of crps), the restatement's bits, and shifting the buffers
    changes none of them."""
    for nens, npts in ((51, 65), (300, 33), (1980, 9), (1980, 1)):
        a = _arena_run(ek, func, T, nens, npts, False)
        b = _arena_run(ek, func, T, nens, npts, True)
        for k in a:
            le.judge_exact(b[k], a[k], f"{func} {k}: shifted against aligned buffers")


@TYPES
def test_a_call_on_a_non_default_stream(ek, T):
    clim, ens, y = _data(5, 300, 130, T)
    want = _restated(ek, clim, ens, y)
    s = ek.stream_create()
    try:
        ek.set_stream(s)
        got = _calls(ek, _long, ek.to_device(clim), ek.to_device(ens), ek.to_device(y))
        host = {k: _host(v) for k, v in got.items()}
    finally:
        ek.set_stream(None)
        ek.synchronize()
        ek.stream_destroy(s)
    for name in want:
        _judge(host[name], want[name], f"stream {name}")


@TYPES
def test_recorded_graph_replays_the_direct_call(ek, T):
    clim, ens, y = _data(3, 700, 500, T)
    d_clim, d_ens, d_y = ek.to_device(clim), ek.to_device(ens), ek.to_device(y)
    direct = {k: _host(v) for k, v in _calls(ek, _long, d_clim, d_ens, d_y).items()}  # also uploads the tables, which a recording cannot
    with ek.graph() as g:
        outs = _calls(ek, _long, d_clim, d_ens, d_y)
    g.launch()
    want = _restated(ek, clim, ens, y)
    for name in want:
        _judge(outs[name], direct[name], f"graph replay {name}")
        _judge(direct[name], want[name], f"direct {name}")
    g.close()
    # member and row counts that have no table yet cannot be recorded
    d_odd, d_clim37 = ek.to_device(np.ascontiguousarray(ens[:677])), ek.to_device(np.ascontiguousarray(clim[:37]))
    with ek.graph() as g2:
        with pytest.raises(ek.EkmError, match=r"inside an ekm_hip.graph\(\) block"):
            ek.score.long_crps_from_ensemble(d_odd, d_y)
        with pytest.raises(ek.EkmError, match=r"inside an ekm_hip.graph\(\) block"):
            ek.extreme.long_efi(d_clim37, d_ens)
    g2.close()
