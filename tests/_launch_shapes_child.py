"""Child process of tests/test_gpu_launch_shapes.py: the launch-shape knobs of csrc/map_kernel.hpp::launch_map, each run
in a guarded arena (tests/_arena.py) and compared bit for bit with the default-shape result for the same data.

A process of its own because ekm_set_tuning latches `g_tuning_user_set` for the life of the process (nothing clears it):
inside pytest it would switch the size heuristics off for every test that runs afterwards.  Order of work:
  1. BEFORE any ekm_set_tuning call: the default shape, at sizes straddling the heuristic (ntile = 4095, 4096, 4097 tiles
     plus a ragged tail, full fields) and at the moderate sizes of the sweeps, for every family x operand mode;
  2. the knobs: tiles_per_block x unroll, table_tiles, hybrid_band_kb, lev_per_wg; each result must equal step 1's;
  3. a few large cases, generated on the device and compared GPU against GPU: fields long enough that the table ops take
     2...16 tiles by the ntile / (4 CUs) rule, and a hybrid call whose default bands exceed one.
Why every bit must agree: in map_fields, map_bcast and map_levels a wave always holds 64 consecutive 16-B chunks starting
at a multiple of 64 chunks (of the array, resp. of the row), whatever tiles, unroll, band or grid are, so neither a
point's arithmetic nor its wave-mates change with the launch shape.  The one comparison with a fallback is lev_per_wg = 1
(map_levels<..., PM_HYBRID, false> recomputes the lower half-level pressure) against lev_per_wg > 1 (the WALK body
carries it): two template bodies of the same expressions.  If they differ in bits the line says so and both must meet
the oracle under the bars of tests/_compare.py.

One JSON line per case on stdout; the first failure ends the process with status 1.
"""
import ctypes as C
import hashlib
import json
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "earthkit-meteo_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

import _guarded as G  # noqa: E402
from ekm_hip._optable import OPS  # noqa: E402

np.seterr(all="ignore")
IFS, B35, B39, BISECT, NEWTON = 0, 1, 2, 0, 1
WB = "wet_bulb_temperature_from_specific_humidity"
FAMILIES = [("one-in", "saturation_vapour_pressure", (0,)), ("two-in", "potential_temperature", ()),
            ("three-in three-out", "pipeline_svp_td_rh", ()), ("three-in six-out", "pipeline_full", ()),
            ("newton", WB, (IFS, NEWTON)), ("tree ifs", WB, (IFS, BISECT)), ("tree bolton35", WB, (B35, BISECT)),
            ("tree bolton39", WB, (B39, BISECT))]
TILES, UNROLL = (1, 2, 3, 5, 16, 64), (1, 2)
TABLE_TILES = (1, 2, 7, 16, 64)
LEV_PER_WG = (1, 2, 3, 4, 7, 200)
BAND_KB = (4, 12, 64, 8192)
MODES = ("field", "major", "scalar", "hybrid")


def emit(**kw):
    print(json.dumps(kw), flush=True)


def tables():
    import ekm_hip.vertical as V

    A, B = V.hybrid_level_parameters(137)
    return {1: (A[136:], B[136:]), 5: (A[51:57], B[51:57]), 11: (A[48:60], B[48:60]), 137: (A, B)}


def nt_of(name, ints, tag):
    nts = G.threads(name, ints, tag)
    return nts[0] if len(nts) == 1 else (1024 if tag == "f32" and ints[0] == IFS else 512)


def build(name, ints, tag, mode, n_or_cols, nlev=11, seed=1):
    """(operands, n) of one case; hybrid: `n_or_cols` columns x `nlev` levels of the IFS table."""
    keys, dt, rng = OPS[name][0], G.TAGS[tag], np.random.default_rng(seed)
    if mode == "hybrid":
        A, B = tables()[nlev]
        hop = G.hybrid_operand(A, B, rng.uniform(5.2e4, 1.04e5, n_or_cols).astype(dt))
        n = hop.len * n_or_cols
        return [G.Op(a) for a in G.physical_fields(keys[:-1], hop.full(n), rng)] + [hop], n
    n = n_or_cols
    m = {"field": "field", "scalar": "scalar", "major": ("major", n // 3 + 1)}[mode]  # three levels, the last one partial
    return G.with_mode(G.typical_operands(keys, n, dt, rng), m, n, rng), n


def digest(outs):
    return [hashlib.blake2b(o.tobytes(), digest_size=16).hexdigest() for o in outs]


def main():
    from ekm_hip import _ffi

    lib = _ffi.lib()
    import ekm_hip as ek

    def guarded(name, ints, tag, ops, n, shift=0):
        return G.run_guarded(lib, name, tag, ops, ints, None, n, shift)

    def param(key, value):
        _ffi.check(lib.ekm_set_tuning_param(key.encode(), value))

    def modes_of(name):
        return MODES if len(OPS[name][0]) > 1 else ("field",)

    built = {}

    def moderate(name, ints, tag, mode):
        key = (name, ints, tag, mode)
        if key not in built:
            built[key] = _moderate(name, ints, tag, mode)
        return built[key]

    def _moderate(name, ints, tag, mode):
        """37 tiles and a ragged tail per row: 64 tiles per workgroup exceed it, 3, 5 and 16 do not divide it; 38 workgroups
        along a hybrid row make 5 bands of 8 (the last of 6), 3 of 16 (the last of 6), or one."""
        tile = nt_of(name, ints, tag) * G.VEC[tag]
        cols = 37 * tile + G.VEC[tag] + 1
        return build(name, ints, tag, mode, cols if mode in ("field", "scalar", "hybrid") else 3 * cols - cols // 2)

    # ---- 1. default shapes, before any ekm_set_tuning call ---------------------------------------------------------------------
    tpb, unr = C.c_int(), C.c_int()
    _ffi.check(lib.ekm_get_tuning(C.byref(tpb), C.byref(unr)))
    assert (tpb.value, unr.value) == (1, 1), (tpb.value, unr.value)
    big, base = {}, {}
    for fam, name, ints in FAMILIES:
        for tag in G.TAGS:
            tile = nt_of(name, ints, tag) * G.VEC[tag]
            for ntile in (4095, 4096, 4097):
                ops, n = build(name, ints, tag, "field", ntile * tile + G.VEC[tag] + 1, seed=ntile)
                big[fam, tag, ntile] = digest(guarded(name, ints, tag, ops, n))
                emit(family=fam, tag=tag, mode="field", knob="default", value=f"ntile={ntile}", n=n, ok=True)
            for mode in modes_of(name):
                ops, n = moderate(name, ints, tag, mode)
                base[fam, tag, mode] = guarded(name, ints, tag, ops, n)
                emit(family=fam, tag=tag, mode=mode, knob="default", value="moderate", n=n, ok=True)

    def same(fam, tag, mode, knob, value, got, want, n):
        for j, (g_, w_) in enumerate(zip(got, want)):
            if not G.same_bits(g_, w_):
                emit(family=fam, tag=tag, mode=mode, knob=knob, value=value, n=n, ok=False,
                     error=f"output {j} differs from the default shape's, {G.first_difference(g_, w_)}")
                sys.exit(1)
        emit(family=fam, tag=tag, mode=mode, knob=knob, value=value, n=n, ok=True)

    try:
        # ---- 2a. tiles_per_block x unroll (from here on the size heuristics stand back) -------------------------------------------
        for t in TILES:
            for u in UNROLL:
                _ffi.check(lib.ekm_set_tuning(t, u))
                for fam, name, ints in FAMILIES:
                    for tag in G.TAGS:
                        for k, mode in enumerate(modes_of(name)):
                            ops, n = moderate(name, ints, tag, mode)
                            same(fam, tag, mode, "tiles_per_block,unroll", f"{t},{u}", guarded(name, ints, tag, ops, n, shift=t + u + k),
                                 base[fam, tag, mode], n)
                        if (t, u) in ((1, 1), (2, 2)):  # the sizes round the heuristic's threshold: one tile per workgroup, and pairs in flight
                            tile = nt_of(name, ints, tag) * G.VEC[tag]
                            for ntile in (4095, 4096, 4097):
                                ops, n = build(name, ints, tag, "field", ntile * tile + G.VEC[tag] + 1, seed=ntile)
                                d = digest(guarded(name, ints, tag, ops, n, shift=1))
                                ok = d == big[fam, tag, ntile]
                                emit(family=fam, tag=tag, mode="field", knob="tiles_per_block,unroll", value=f"{t},{u} ntile={ntile}", n=n, ok=ok,
                                     **({} if ok else {"error": f"digests {d} differ from the default shape's {big[fam, tag, ntile]}"}))
                                if not ok:
                                    sys.exit(1)
        _ffi.check(lib.ekm_set_tuning(1, 1))
        # ---- 2b. table_tiles --------------------------------------------------------------------------------------------------------
        for v in TABLE_TILES:
            param("table_tiles", v)
            for fam, name, ints in FAMILIES:
                for tag in G.TAGS:
                    for k, mode in enumerate(modes_of(name)):
                        ops, n = moderate(name, ints, tag, mode)
                        same(fam, tag, mode, "table_tiles", v, guarded(name, ints, tag, ops, n, shift=v + k), base[fam, tag, mode], n)
        param("table_tiles", 0)
        # ---- 2c. hybrid_band_kb: 38 workgroups along a row in bands of 8, 8, 16 and all -------------------------------------------------
        for v in BAND_KB:
            param("hybrid_band_kb", v)
            for fam, name, ints in FAMILIES:
                if "hybrid" in modes_of(name):
                    for tag in G.TAGS:
                        ops, n = moderate(name, ints, tag, "hybrid")
                        same(fam, tag, "hybrid", "hybrid_band_kb", v, guarded(name, ints, tag, ops, n, shift=v), base[fam, tag, "hybrid"], n)
        param("hybrid_band_kb", 8192)
        # ---- 2d. lev_per_wg on tables of 1, 5 and 137 levels: theta walks, the three-output pipeline must not care ----------------------
        for fam, name, ints in FAMILIES[1:3]:
            for tag in G.TAGS:
                cols = 256 * G.VEC[tag] + G.VEC[tag] + 1
                for nlev in (1, 5, 137):
                    ops, n = build(name, ints, tag, "hybrid", cols, nlev)
                    param("lev_per_wg", 0)
                    dflt = guarded(name, ints, tag, ops, n)
                    for v in LEV_PER_WG:
                        param("lev_per_wg", v)
                        got = guarded(name, ints, tag, ops, n, shift=v)
                        knob, value = "lev_per_wg", f"{v} levels={nlev}"
                        if v == 1 and not all(G.same_bits(a, b) for a, b in zip(got, dflt)):
                            # the recomputing body against the walking one: the documented fallback, both within the oracle's bar
                            full = [o.full(n) for o in ops]
                            for res in (got, dflt):
                                G.assert_oracle_parity(name, tag, full, ints, None, res, f"{name} {tag} lev_per_wg")
                            emit(family=fam, tag=tag, mode="hybrid", knob=knob, value=value, n=n, ok=True,
                                 note="lev_per_wg=1 differs in bits from the level walk; both meet the oracle's bar: " + G.first_difference(got[0], dflt[0]))
                        else:
                            same(fam, tag, "hybrid", knob, value, got, dflt, n)
        param("lev_per_wg", 0)
        # ---- 3. large cases, GPU against GPU ------------------------------------------------------------------------------------------------
        large(ek, lib, _ffi, emit, param)
    finally:
        for key, v in (("table_tiles", 0), ("hybrid_band_kb", 8192), ("lev_per_wg", 0)):
            param(key, v)
        _ffi.check(lib.ekm_set_tuning(1, 1))
    emit(done=True)


def large(ek, lib, _ffi, emit, param):
    """Fields of tens of millions of points filled on the device (ekm_synth_fill_f32); each result downloaded once."""
    cus = lib.ekm_device_cus(0)
    for fam, name, ints in FAMILIES[5:]:
        tag, dt = "f32", np.float32
        tile = nt_of(name, ints, tag) * 4
        n = (16 * 4 * cus + 3) * tile + 5  # ntile / (4 CUs) = 16: the default takes 16 tiles per workgroup, table_tiles = 2, 7 that many
        t, q, p = (ek.DeviceArray.empty((n,), dt) for _ in range(3))
        _ffi.check(lib.ekm_synth_fill_f32(0, None, t.ptr, q.ptr, p.ptr, 0, n, n // 8 + 1, 8, 11))
        ref = None
        for v in (0,) + TABLE_TILES:
            param("table_tiles", v)
            out = ek.DeviceArray.empty((n,), dt)
            _ffi.check(lib.ekm_fill_u32(0, out.ptr, 0x7FF8A17E, n, None))
            G._call(lib, name, tag, [_ffi.Operand(x.ptr, 0, 0, 0, 0) for x in (t, q, p)], ints, None, [out.ptr], n)
            host = out.to_host()
            out.free()
            unwritten = int((host.view(np.uint32) == 0x7FF8A17E).sum())
            ok = unwritten == 0 and (ref is None or G.same_bits(host, ref))
            emit(family=fam, tag=tag, mode="field", knob="table_tiles (large)", value=v, n=n, ok=ok,
                 **({} if ok else {"error": f"{unwritten} elements unwritten" if unwritten else G.first_difference(host, ref)}))
            if not ok:
                sys.exit(1)
            ref = host if ref is None else ref
        param("table_tiles", 0)
        for x in (t, q, p):
            x.free()
    # hybrid: 8 MiB of surface pressure per band = 2 Mi columns; 2 bands and a ragged third
    name, tag, dt = "potential_temperature", "f32", np.float32
    A, B = tables()[5]
    cols = 2 * (2 << 20) + 1029
    n = 5 * cols
    sp = np.random.default_rng(3).uniform(5.2e4, 1.04e5, cols).astype(dt)
    hop = G.hybrid_operand(A, B, sp)
    d_sp, d_a, d_b = ek.to_device(sp), ek.to_device(hop.A), ek.to_device(hop.B)
    t, q = ek.DeviceArray.empty((n,), dt), ek.DeviceArray.empty((n,), dt)
    _ffi.check(lib.ekm_synth_fill_f32(0, None, t.ptr, q.ptr, None, 0, n, cols, 5, 12))
    ref = None
    for v in (8192, 64, 1 << 20):
        param("hybrid_band_kb", v)
        out = ek.DeviceArray.empty((n,), dt)
        _ffi.check(lib.ekm_fill_u32(0, out.ptr, 0x7FF8A17E, n, None))
        G._call(lib, name, tag, [_ffi.Operand(t.ptr, 0, 0, 0, 0), _ffi.Operand(d_sp.ptr, G.HYBRID_FULL, hop.nflat, hop.len, cols, d_a.ptr, d_b.ptr)],
                (), None, [out.ptr], n)
        host = out.to_host()
        out.free()
        unwritten = int((host.view(np.uint32) == 0x7FF8A17E).sum())
        ok = unwritten == 0 and (ref is None or G.same_bits(host, ref))
        emit(family="two-in", tag=tag, mode="hybrid", knob="hybrid_band_kb (large)", value=v, n=n, ok=ok,
             **({} if ok else {"error": f"{unwritten} elements unwritten" if unwritten else G.first_difference(host, ref)}))
        if not ok:
            sys.exit(1)
        ref = host if ref is None else ref
    param("hybrid_band_kb", 8192)


if __name__ == "__main__":
    try:
        main()
    except SystemExit:
        raise
    except BaseException:
        traceback.print_exc()
        print(json.dumps({"ok": False, "error": traceback.format_exc()[-1500:]}), flush=True)
        sys.exit(1)
