"""The hybrid-level kernels (csrc/hybrid.hip) against an extended-precision reference, each element under a bound derived
from the roundings the kernel performs (tests/_hybrid_exact.py; the judges are proven on the CPU in
tests/test_hybrid_judges_cpu.py).  tests/test_gpu_vertical.py stays the parity check against the recorded reference
vectors at the reference's tolerances; this file is the rounding-level one, fp32 and fp64, no element excluded.

Column counts: 1, V - 1, V + 1, 1027, 4 * 256 * V + V + 1 (V = 4 in fp32, 2 in fp64: all ragged) and 4 * 256 * V (the
vector variants).  Level tables: hx.tables -- the 137 IFS levels, their lowest 24 / 5 / 2 / 1, layer ratios up to 10 with and
without a zero-pressure top, and the table whose layers sit within 4 ulp of the fp32 kernel's series-to-libm switch
(|s| = 0.25).  Both pressure kernels (hybrid_rows = 1 / 0), level subsets, both alpha_top, all six chain modes, the scan
in one launch and in chunks of 3 and 5 levels, and the scan on given alpha / delta judged on the GPU's own alpha and delta.
The worst used / allowed per output, dtype and kernel variant is printed when the module is done
(profiles/hybrid_bounds.md) and goes to the census."""
import contextlib

import numpy as np
import pytest

import _compare
import _hybrid_exact as hx

pytestmark = pytest.mark.gpu

OUT = ("full", "half", "delta", "alpha")
TYPES = {"f32": (np.float32, 4), "f64": (np.float64, 2)}
RESULTS = {}  # (output, tag, variant) -> [worst share, elements]


def _note(output, tag, variant, share, n):
    r = RESULTS.setdefault((output, tag, variant), [0.0, 0])
    r[0], r[1] = max(r[0], share), r[1] + n


@pytest.fixture(scope="module", autouse=True)
def record():
    yield
    if not RESULTS:
        return
    print("\n| output | dtype | kernel variant | worst used / allowed | elements |\n|---|---|---|---|---|")
    for (output, tag, variant), (share, n) in sorted(RESULTS.items()):
        print(f"| {output} | {tag} | {variant} | {share:.3f} | {n} |")
    for tag in TYPES:
        for output in OUT + hx.MODES + ("from_alpha_delta",):
            rows = [v for k, v in RESULTS.items() if k[0] == output and k[1] == tag]
            if rows:
                line = (f"hybrid bounds {output} {tag}: worst used/allowed {max(r[0] for r in rows):.3f} "
                        f"over {sum(r[1] for r in rows)} elements")
                _compare.CENSUS.append(line)
                print(line)


@contextlib.contextmanager
def _tuning(name, value, default):
    from ekm_hip import _ffi

    lib = _ffi.lib()
    _ffi.check(lib.ekm_set_tuning_param(name, value))
    try:
        yield
    finally:
        _ffi.check(lib.ekm_set_tuning_param(name, default))


def _grid(V):
    return sorted({1, V - 1, V + 1, 1027, 4 * 256 * V + V + 1, 4 * 256 * V})


def _tables(ek, T):
    return hx.tables(*ek.vertical.hybrid_level_parameters(137), T)


def _subset(A, B, levels):
    """The contiguous half-level range a `levels=` request is computed on, and the rows it hands back."""
    levels = np.asarray(levels)
    lmin, lmax = int(levels.min()), int(levels.max())
    return A[lmin - 1:lmax + 1], B[lmin - 1:lmax + 1], levels - lmin


_EXACT = {}


def _exact_pressure(key, A, B, sp, alpha_top, T):
    if key not in _EXACT:
        P = hx.pressure(A, B, sp, alpha_top)
        _EXACT[key] = (P, hx.pressure_bounds(P, T, "kernel"))
    return _EXACT[key]


def _pressure_cases(tabs, V):
    for npts in _grid(V):
        yield "ifs137", npts, "ifs", None
    for name in ("low24", "low5", "low2", "low1", "thick", "thick_zero_top", "switch"):
        for npts in (V + 1, 1027):
            yield name, npts, "ifs", None
    for name in ("ifs137", "thick_zero_top", "thick"):  # the top-layer rule on (A[0] = B[0] = 0) and off, alpha_top = 1
        yield name, 1027, "arpege", None
    for levels in ([100, 101, 137], [3, 50, 51, 120], [1, 2, 137], [137, 7, 64]):
        yield "ifs137", 1027, "ifs", levels
        yield "ifs137", 4 * 256 * V, "ifs", levels


@pytest.mark.parametrize("tag", sorted(TYPES))
def test_pressure_on_hybrid_levels_within_rounding_bounds(ek, tag):
    T, V = TYPES[tag]
    tabs = _tables(ek, T)
    switch_s = None
    for rows, variant in ((1, "hybrid_rows"), (0, "hybrid_levels")):
        with _tuning(b"hybrid_rows", rows, 1):
            for case, (name, npts, alpha_top, levels) in enumerate(_pressure_cases(tabs, V)):
                A, B = tabs[name]
                sp = hx.draw(np.random.default_rng(100 + case), T, npts, 1)[0]
                res = ek.vertical.pressure_on_hybrid_levels(A, B, ek.to_device(sp), levels=levels, alpha_top=alpha_top, output=OUT)
                a_, b_, sel = (A, B, None) if levels is None else _subset(A, B, levels)
                P, E = _exact_pressure((tag, case), a_, b_, sp, alpha_top, T)
                assert P["top"] == (name in ("ifs137", "thick_zero_top") and (levels is None or 1 in levels))
                for k, r in zip(OUT, res):
                    idx = slice(None) if sel is None else (sel + 1 if k == "half" else sel)
                    what = f"{variant} {tag} {name} npts={npts} {alpha_top} levels={levels} {k}"
                    v = variant + (" vec" if npts % V == 0 else " ragged")
                    got = r.to_host()
                    hx.judge(got, P[k][idx], E[k][idx], what, _compare.LEDGER, T)
                    # for the record, the top layer under its rule (delta = log(p_1 / 0.1), alpha = alpha_top) apart from the rest
                    ruled = np.zeros(got.shape[0], bool)
                    if P["top"] and k in ("delta", "alpha"):
                        ruled[:] = (np.arange(got.shape[0]) == 0) if sel is None else (sel == 0)
                    for rows_, v_ in ((~ruled, v), (ruled, v + ", top-layer rule")):
                        if rows_.any():
                            _note(k, tag, v_, hx.judge(got[rows_], P[k][idx][rows_], E[k][idx][rows_], what, [], T), got[rows_].size)
                if name == "switch" and npts == 1027:
                    switch_s = np.abs(E["s"])
    # the table at the switch did put layers on both sides of it, and within the band where either path may run
    u = float(hx.unit(T))
    assert (switch_s < 0.25).sum() > 100 and (switch_s >= 0.25).sum() > 100 and np.abs(switch_s - 0.25).max() < 16 * u


def _chain_calls(ek, d_t, d_q, d_zs, A, B, d_sp, alpha_top):
    v = ek.vertical
    out = {"thickness": v.relative_geopotential_thickness_on_hybrid_levels(d_t, d_q, A, B, d_sp, alpha_top=alpha_top),
           "geopotential": v.geopotential_on_hybrid_levels(d_t, d_q, d_zs, A, B, d_sp, alpha_top=alpha_top)}
    for ht in ("geometric", "geopotential"):
        for hr in ("sea", "ground"):
            out[f"h_{ht}_{hr}"] = v.height_on_hybrid_levels(d_t, d_q, d_zs, A, B, d_sp, alpha_top=alpha_top, h_type=ht, h_reference=hr)
    return {k: r.to_host() for k, r in out.items()}


def _chain_cases(V):
    for npts in _grid(V):
        yield "ifs137", 137, npts, "ifs"
    for npts in (V + 1, 1027, 4 * 256 * V + V + 1, 4 * 256 * V):
        yield "low24", 24, npts, "ifs"
    for name, n in (("low5", 5), ("low2", 2), ("low1", 1), ("thick", 5), ("thick_zero_top", 6), ("switch", 9),
                    ("ifs137", 47)):  # 47: fewer levels of data than the table has, the bottom-most ones
        yield name, n, 1027, "ifs"
    for name, n in (("ifs137", 137), ("thick_zero_top", 6), ("thick", 5)):
        yield name, n, 1027, "arpege"


@pytest.mark.parametrize("tag", sorted(TYPES))
def test_geopotential_chain_within_rounding_bounds(ek, tag):
    """All six modes of the fused scan, and the scan on given alpha / delta: fed the GPU's own alpha and delta (so that only
    the scan is judged), and against the fused call's exact value under the fused bound."""
    T, V = TYPES[tag]
    tabs = _tables(ek, T)
    F = ek.vertical.relative_geopotential_thickness_on_hybrid_levels_from_alpha_delta
    for case, (name, n, npts, alpha_top) in enumerate(_chain_cases(V)):
        A, B = tabs[name]
        sp, t, q, zs = hx.draw(np.random.default_rng(200 + case), T, npts, n)
        d_sp, d_t, d_q, d_zs = (ek.to_device(x) for x in (sp, t, q, zs))
        ex, eb = hx.chain(A, B, sp, zs, t, q, T, alpha_top)
        lane = "vec" if npts % V == 0 else "ragged"
        runs = [("one launch", 1 << 20)] + ([("chunks of 3", 3), ("chunks of 5", 5)] if name == "low24" else [])
        whole = None
        for label, chunk in runs:
            with _tuning(b"geo_chunk_levels", chunk, 1 << 20):
                got = _chain_calls(ek, d_t, d_q, d_zs, A, B, d_sp, alpha_top)
            for k in hx.MODES:
                what = f"geopotential_columns {tag} {name} n={n} npts={npts} {alpha_top} {label} {k}"
                _note(k, tag, f"fused {lane}, {label}", hx.judge(got[k], ex[k], eb[k], what, _compare.LEDGER, T), ex[k].size)
                if whole is not None:
                    hx.judge_identical(got[k], whole[k], what + " against one launch")
            whole = whole or got
        # alpha and delta of the table's bottom-most n layers, as the fused scan forms them
        a_, b_ = A[A.size - 1 - n:], B[B.size - 1 - n:]
        al, de = ek.vertical.pressure_on_hybrid_levels(a_, b_, d_sp, alpha_top=alpha_top, output=("alpha", "delta"))
        for label, chunk in runs:
            with _tuning(b"geo_chunk_levels", chunk, 1 << 20):
                z = F(d_t, d_q, al, de).to_host()
            X = hx.scan(t, q, al.to_host(), de.to_host())
            what = f"from_alpha_delta {tag} {name} n={n} npts={npts} {label}"
            _note("from_alpha_delta", tag, f"given alpha/delta {lane}, {label}",
                  hx.judge(z, X["dphi"], hx.scan_bounds(X, T), what, _compare.LEDGER, T), z.size)
            # the same result as an answer to the fused question: the thickness of (A, B, sp), under the fused bound
            _note("thickness", tag, f"pressure kernel + given alpha/delta {lane}, {label}",
                  hx.judge(z, ex["thickness"], eb["thickness"], what + " as the fused thickness", _compare.LEDGER, T), z.size)
