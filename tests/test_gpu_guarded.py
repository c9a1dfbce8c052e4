"""Every entry point of the C ABI run inside a guarded arena (tests/_arena.py): what the parity suite cannot see.

The parity tests ask whether the `n` values a kernel returned are close to the oracle's.  Here each call is made with
256 KiB of guard words round every buffer, the outputs pre-filled with a NaN no computation yields, and buffer starts
16-B aligned or 1 / V-1 elements off, and must
  1. leave every guard word and every input bit as it was and write every output element (arena.check());
  2. return the very bits of the same call on separately allocated, 16-B-aligned buffers;
  3. at one size per (op, operand mode) -- a few tiles plus a ragged tail -- meet the oracle under the bars of
     tests/_compare.py as tests/test_gpu_parity.py applies them.
Table-driven from ekm_hip/_optable.py::OPS: every op x every value of every int parameter (x both eps values) x both
dtypes, at the sizes where the launch skeleton of csrc/map_kernel.hpp turns (V = elements per 16-B chunk, NT =
workgroup size): 1, V-1, V, V+1, 2V+1, NT*V-1, NT*V, NT*V+1, 2*NT*V+V-1 and 3*NT*V+V+1 -- every op takes all of them (the
whole file costs about a fifth of the parity suite's time: nothing needed thinning); the last operand as a full
field, a scalar, a level-major vector with rows of NT*V-1, NT*V+1 and 255 (map_bcast) points with whole levels and a
partial last one, a level-minor vector of 7 and of V values, and -- where it is a pressure -- the hybrid definition with leading flat levels, with none and
with flat levels only, aligned and ragged column counts.  The column kernels of csrc/hybrid.hip follow through their
own entry points.  Inputs are benign (_guarded.typical_operands, _guarded.physical_fields): NaN and infinities
have tests of their own.
"""
import ctypes as C

import numpy as np
import pytest

import _guarded as G
from _arena import Arena, DeviceMemory
from ekm_hip._optable import OPS

pytestmark = pytest.mark.gpu
np.seterr(all="ignore")
VISITED = set()     # (name, ints, eps, tag)
COUNTS = {}         # family -> cases


def _tables():
    import ekm_hip.vertical as V

    A, B = V.hybrid_level_parameters(137)
    # leading flat levels + hybrid ones (5 + 6: the level walk's last group is partial; p 50-110 hPa), hybrid only, flat only
    return {"flat+hybrid": (A[48:60], B[48:60]), "hybrid": (A[60:], B[60:]), "flat": (A[:40], B[:40])}


def _cases(name, ints, tag):
    """(mode label, n, builder(rng) -> operand list, compare with the oracle?)"""
    keys = OPS[name][0]
    dt, v = G.TAGS[tag], G.VEC[tag]
    nts = G.threads(name, ints, tag)
    few = G.few_tiles(nts, v)
    out = []

    def typical(mode, n):
        return lambda rng: G.with_mode(G.typical_operands(keys, n, dt, rng), mode, n, rng)

    for n in G.sizes(nts, v):
        out.append(("field", n, typical("field", n), n == few))
    if len(keys) < 2:
        return out
    for n in G.sizes(nts, v):
        out.append(("scalar", n, typical("scalar", n), n == few))
    tile = max(nts) * v
    for inner in (tile - 1, tile + 1, 255):
        n = 2 * inner + inner // 2 + 1  # a partial last level
        out.append((f"major{inner}", n, typical(("major", inner), n), inner == tile + 1))
        out.append((f"major{inner}", 3 * inner, typical(("major", inner), 3 * inner), False))
    for length in (7, v):
        out.append((f"minor{length}", few, typical(("minor", length), few), length == 7))
    if keys[-1] == "p":
        for label, (A, B) in _tables().items():
            for npts in (tile, tile + v + 1):
                def build(rng, A=A, B=B, npts=npts):
                    hop = G.hybrid_operand(A, B, rng.uniform(5.2e4, 1.04e5, npts).astype(dt))
                    return [G.Op(a) for a in G.physical_fields(keys[:-1], hop.full(hop.len * npts), rng)] + [hop]
                out.append((f"hybrid:{label}", (len(A) - 1) * npts, build, label == "flat+hybrid" and npts != tile))
    return out


@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("name", sorted(OPS))
def test_map_entry_point_in_the_arena(ek, name, tag):
    from ekm_hip import _ffi

    lib = _ffi.lib()
    ncase = 0
    for ints, eps in G.variants(name):
        for k, (mode, n, build, with_oracle) in enumerate(_cases(name, ints, tag)):
            what = f"{name}{ints}{'' if eps is None else f' eps={eps:g}'} {tag} {mode} n={n}"
            ops = build(np.random.default_rng(1000 * k + n % 997))
            try:
                got = G.run_guarded(lib, name, tag, ops, ints, eps, n, shift=k)
            except AssertionError as exc:
                raise AssertionError(f"{what}: {exc}") from None
            want = G.run_plain(ek, lib, name, tag, ops, ints, eps, n)
            for j, (g_, w_) in enumerate(zip(got, want)):
                assert G.same_bits(g_, w_), f"{what}: output {j} in the arena differs from the aligned run, {G.first_difference(g_, w_)}"
            if with_oracle:
                G.assert_oracle_parity(name, tag, [o.full(n) for o in ops], ints, eps, got, what)
            ncase += 1
        VISITED.add((name, ints, eps, tag))
    COUNTS[f"map kernels {tag}"] = COUNTS.get(f"map kernels {tag}", 0) + ncase


# ---- the column kernels of csrc/hybrid.hip through their own entry points -------------------------------------------------------
def _raw_twice(ek, what, bufs, call, shift=0):
    """`bufs`: name -> ("in" | "inout", array) or ("out", count, dtype).  `call(ptr)` makes the ABI call with ptr(name) ->
    device pointer.  Once in the arena (checked), once on separate aligned allocations; the outputs must agree in every bit."""
    arena = Arena(DeviceMemory())
    for k, (nm, b) in enumerate(bufs.items()):
        if b[0] == "out":
            arena.output(nm, b[1], b[2], (0, 1)[(shift + k) % 2])
        else:
            getattr(arena, {"in": "input", "inout": "inout"}[b[0]])(nm, b[1], (0, 1)[(shift + k) % 2])
    arena.commit()
    try:
        call(arena.ptr)
        try:
            arena.check()
        except AssertionError as exc:
            raise AssertionError(f"{what}: {exc}") from None
        got = {nm: arena.result(nm) for nm, b in bufs.items() if b[0] != "in"}
    finally:
        arena.free()
    from ekm_hip.vertical import _dev_bytes

    plain = {nm: _dev_bytes(b[1] if b[0] != "out" else np.zeros(b[1], b[2]), 0) for nm, b in bufs.items()}
    call(lambda nm: plain[nm].ptr)
    ek.synchronize()
    from ekm_hip import _ffi

    for nm, g_ in got.items():
        w_ = np.empty_like(g_)
        _ffi.check(_ffi.lib().ekm_d2h(0, w_.ctypes.data, plain[nm].ptr, w_.nbytes, None))
        ek.synchronize()
        assert G.same_bits(g_, w_), f"{what}: '{nm}' in the arena differs from the aligned run, {G.first_difference(g_, w_)}"
    for a in plain.values():
        a.free()
    return got


def _column_inputs(dt, nlev_from, npts, seed):
    import ekm_hip.vertical as V

    A, B = V.hybrid_level_parameters(137)
    A, B = A[nlev_from:].astype(dt), B[nlev_from:].astype(dt)
    rng = np.random.default_rng(seed)
    sp = rng.uniform(5.2e4, 1.04e5, npts).astype(dt)
    nfull = A.size - 1
    t = rng.uniform(200.0, 300.0, (nfull, npts)).astype(dt)
    q = rng.uniform(0.0, 0.02, (nfull, npts)).astype(dt)
    zs = rng.uniform(0.0, 3e4, npts).astype(dt)
    return A, B, sp, zs, t, q, nfull


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_pressure_on_hybrid_levels_in_the_arena(ek, tag):
    """Every output combination, the identity and a selection of rows (row_full / row_half with skipped levels), both
    kernels (hybrid_rows 1: one workgroup per (level, tile); 0: one lane per column), ragged and aligned column counts."""
    import itertools

    from ekm_hip import _ffi
    lib, dt, real = _ffi.lib(), G.TAGS[tag], (C.c_float if tag == "f32" else C.c_double)
    fn = getattr(lib, f"ekm_pressure_on_hybrid_levels_{tag}")
    names = ("full", "half", "delta", "alpha")
    ncase = 0
    try:
        for rows in (1, 0):
            _ffi.check(lib.ekm_set_tuning_param(b"hybrid_rows", rows))
            for npts, nlev_from in ((1, 130), (G.VEC[tag] + 1, 130), (1024, 120), (1031, 0)):
                A, B, sp, _, _, _, nfull = _column_inputs(dt, nlev_from, npts, 7)
                top = int(bool(np.any(A[0] + B[0] * sp <= 0.1)))  # the reference's any(p_half[0] <= 0.1)
                combos = [c for r in range(1, 5) for c in itertools.combinations(names, r)]
                for k, combo in enumerate(combos if npts != 1031 else [names, ("half",), ("full", "alpha")]):
                    for select in (False, True):
                        row_full = row_half = None
                        nrf, nrh = nfull, nfull + 1
                        if select:  # every third layer, in reverse order; the half levels 0, 2 and the last
                            pick = np.arange(nfull)[::3][::-1]
                            row_full = np.full(nfull, -1, np.int32)
                            row_full[pick] = np.arange(pick.size)
                            hpick = np.unique([0, min(2, nfull), nfull])
                            row_half = np.full(nfull + 1, -1, np.int32)
                            row_half[hpick] = np.arange(hpick.size)
                            nrf, nrh = pick.size, hpick.size
                        bufs = {"A": ("in", A), "B": ("in", B), "sp": ("in", sp)}
                        if select:
                            bufs.update(row_full=("in", row_full), row_half=("in", row_half))
                        for nm in combo:
                            bufs[nm] = ("out", (nrh if nm == "half" else nrf) * npts, dt)

                        def call(ptr):
                            opt = lambda nm: ptr(nm) if nm in bufs else None  # noqa: E731
                            _ffi.check(fn(0, None, ptr("A"), ptr("B"), ptr("sp"), npts, nfull, opt("row_full"), opt("row_half"),
                                          top, real(float(np.log(2))), opt("full"), opt("half"), opt("delta"), opt("alpha")))
                        what = f"pressure_on_hybrid_levels {tag} hybrid_rows={rows} npts={npts} nfull={nfull} {'+'.join(combo)} select={select}"
                        got = _raw_twice(ek, what, bufs, call, shift=k)
                        ncase += 1
    finally:
        _ffi.check(lib.ekm_set_tuning_param(b"hybrid_rows", 1))
    COUNTS[f"pressure_on_hybrid_levels {tag}"] = ncase


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_geopotential_scan_in_the_arena(ek, tag):
    """Modes 0-5, the scan cut into launches of 5, 3 and 1 levels (the running sum crosses a chunk boundary in the output row
    above it: that row must hold its own result again at the end, and nothing may land outside the output) -- all equal to
    the single launch in every bit; and the same scan from given alpha and delta."""
    from ekm_hip import _ffi

    lib, dt, real = _ffi.lib(), G.TAGS[tag], (C.c_float if tag == "f32" else C.c_double)
    fn = getattr(lib, f"ekm_geopotential_on_hybrid_levels_{tag}")
    ncase = 0
    try:
        for npts in (1, G.VEC[tag] + 1, 1024, 1031):
            A, B, sp, zs, t, q, nfull = _column_inputs(dt, 137 - 24, npts, 3)
            top = int(bool(np.any(A[0] + B[0] * sp <= 0.1)))
            for mode in range(6):
                first = None
                for k, chunk in enumerate((1 << 20, 5, 3, 1)):
                    _ffi.check(lib.ekm_set_tuning_param(b"geo_chunk_levels", chunk))
                    bufs = {"A": ("in", A), "B": ("in", B), "sp": ("in", sp), "zs": ("in", zs), "t": ("in", t), "q": ("in", q),
                            "out": ("out", nfull * npts, dt)}

                    def call(ptr):
                        _ffi.check(fn(0, None, ptr("A"), ptr("B"), ptr("sp"), ptr("zs"), ptr("t"), ptr("q"), npts, nfull, top,
                                      real(float(np.log(2))), mode, ptr("out")))
                    what = f"geopotential_on_hybrid_levels {tag} mode={mode} npts={npts} geo_chunk_levels={chunk}"
                    got = _raw_twice(ek, what, bufs, call, shift=k + mode)["out"]
                    ncase += 1
                    if first is None:
                        first = got
                    assert G.same_bits(got, first), f"{what}: differs from the single launch, {G.first_difference(got, first)}"
    finally:
        _ffi.check(lib.ekm_set_tuning_param(b"geo_chunk_levels", 1 << 20))
    fn = getattr(lib, f"ekm_geopotential_thickness_from_alpha_delta_{tag}")
    for k, npts in enumerate((1, G.VEC[tag] + 1, 1024, 1031)):
        _, _, _, _, t, q, nfull = _column_inputs(dt, 137 - 24, npts, 4)
        rng = np.random.default_rng(9)
        alpha, delta = rng.uniform(0.01, 0.7, t.shape).astype(dt), rng.uniform(0.01, 0.3, t.shape).astype(dt)
        bufs = {"t": ("in", t), "q": ("in", q), "alpha": ("in", alpha), "delta": ("in", delta), "out": ("out", nfull * npts, dt)}

        def call(ptr):
            _ffi.check(fn(0, None, ptr("t"), ptr("q"), ptr("alpha"), ptr("delta"), npts, nfull, ptr("out")))
        _raw_twice(ek, f"geopotential_thickness_from_alpha_delta {tag} npts={npts}", bufs, call, shift=k)
        ncase += 1
    COUNTS[f"geopotential scans {tag}"] = ncase


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_any_le_in_the_arena(ek, tag):
    """The flag word: ORed into, nothing beside it touched, set exactly when some a0 + b0*sp <= thresh."""
    from ekm_hip import _ffi

    lib, dt, real = _ffi.lib(), G.TAGS[tag], (C.c_float if tag == "f32" else C.c_double)
    fn = getattr(lib, f"ekm_any_le_{tag}")
    ncase = 0
    for k, n in enumerate((1, G.VEC[tag] + 1, 1023, 1024, 1025, 70001)):
        sp = np.random.default_rng(n).uniform(5e4, 1.05e5, n).astype(dt)
        for hit in (False, True):
            x = sp.copy()
            if hit:
                x[n - 1] = 0.05
            bufs = {"sp": ("in", x), "flag": ("inout", np.zeros(1, np.int32))}

            def call(ptr):
                _ffi.check(fn(0, None, ptr("sp"), n, real(0.0), real(1.0), real(0.1), ptr("flag")))
            got = _raw_twice(ek, f"any_le {tag} n={n} hit={hit}", bufs, call, shift=k)
            assert bool(got["flag"][0]) == hit, (tag, n, hit, got["flag"])
            ncase += 1
    COUNTS[f"any_le {tag}"] = ncase


def test_every_case_of_the_case_table_was_visited(ek):
    """Runs last in this file: every OPS entry x every int-parameter value x dtype, hence the 94 function x variant cases
    of tests/golden/_case_table.py in both dtypes, and the column entry points."""
    for tag in ("f32", "f64"):
        seen = {(n, i, e) for n, i, e, t in VISITED if t == tag}
        assert {n for n, _, _ in seen} == set(OPS), sorted(set(OPS) - {n for n, _, _ in seen})
        for name in OPS:
            assert {(i, e) for n, i, e in seen if n == name} == set(G.variants(name)), name
        assert G.case_table_covered(seen) == []
    from _fuzz import _case_table

    print(f"\nguarded runs: {len(VISITED)} (entry point, variant, dtype) combinations of {len(OPS)} entry points; the case table's "
          f"{len(_case_table())} function x variant cases covered in both dtypes")
    for fam, c in sorted(COUNTS.items()):
        print(f"  {fam}: {c} guarded cases")
    assert all(COUNTS.get(f"{k} {t}", 0) > 0 for k in ("map kernels", "pressure_on_hybrid_levels", "geopotential scans", "any_le") for t in ("f32", "f64"))
