"""Guarded launches through the raw C ABI -- shared by tests/test_gpu_guarded.py (every entry point at the ragged sizes
and operand modes of csrc/map_kernel.hpp) and tests/_launch_shapes_child.py (the launch-shape knobs).

One call = `[dev, stream] + operands + ints (+ eps) + output pointers + [n]` (ekm_hip/_engine.py::_submit).  It is made
twice on the same data: inside a guarded arena (tests/_arena.py), with buffer starts 16-B aligned or 1 / V-1 elements
off, and on separately allocated 16-B-aligned DeviceArrays -- the path the parity suite ties to the oracle.  The arena
run must leave guards and inputs intact and every output element written, and return the plain run's very bits."""
import ctypes as C

import numpy as np

from _arena import Arena, DeviceMemory
from ekm_hip._ffi import EPT_METHOD, FIELD, HYBRID_FULL, LCL_METHOD, LEVEL_MAJOR, LEVEL_MINOR, PHASE, SCALAR, T_METHOD
from ekm_hip._optable import OPS

TAGS = {"f32": np.float32, "f64": np.float64}
VEC = {"f32": 4, "f64": 2}          # elements per 16-B chunk (map_kernel.hpp::VecOf)
EPS_VALUES = (1e-4, 5.0e4)          # the default and the value of tests/golden/_case_table.py


def _typical():
    """tests/_fuzz.py::TYPICAL (the one benign value per operand the special-operand tests use) with the four operands it
    lacks: those of the entry points outside the case table.  Extended here, not there: _fuzz.py stays as the suites that
    share it have it."""
    from _fuzz import TYPICAL as base

    return dict(base, es_slope=70.0, t_def=290.0, p_def=1e5, omega=-0.5)


def typical_operands(keys, n, dtype, rng, jitter=5e-3):
    """`n` benign in-domain points per key: the typical value, each point moved by up to +-`jitter` of itself (t stays above
    td, the parcel unsaturated, every pressure above every vapour pressure).  No NaN, no infinity."""
    typ = _typical()
    return [(typ[k] * (1.0 + jitter * rng.uniform(-1.0, 1.0, n))).astype(dtype) for k in keys]


def _inv(d):
    return {v: k for k, v in d.items()}


def _enum(name, key):
    if key == "phase":
        return PHASE
    if key == "method":
        return LCL_METHOD if name.startswith("lcl") else EPT_METHOD
    if key == "ept_method":
        return EPT_METHOD
    assert key == "t_method", key
    return T_METHOD if "potential" in name else {k: v for k, v in T_METHOD.items() if k != "direct"}


def variants(name):
    """Every (ints, eps) of entry point `name`: the product of all values of its int parameters (x both eps values)."""
    import itertools

    ins, outs, int_names, has_eps = OPS[name]
    out = []
    for ints in itertools.product(*[sorted(_enum(name, k).values()) for k in int_names]):
        for eps in (EPS_VALUES if has_eps else (None,)):
            out.append((tuple(ints), eps))
    return out


def reference_kwargs(name, ints, eps):
    kw = {k: _inv(_enum(name, k))[v] for k, v in zip(OPS[name][2], ints)}
    if eps is not None:
        kw["eps"] = eps
    return kw


def case_table_covered(visited):
    """The (function, variant) cases of tests/golden/_case_table.py that `visited` -- a set of (name, ints, eps) -- lacks."""
    from _fuzz import _case_table

    missing = []
    for func, _, kw in _case_table():
        kw = dict(kw)
        eps = kw.pop("eps", 1e-4) if OPS[func][3] else None
        defaults = {"phase": "mixed", "method": "davies" if func.startswith("lcl") else "ifs", "ept_method": "ifs",
                    "t_method": "direct" if "potential" in func else "bisect"}
        ints = tuple(_enum(func, k)[kw.get(k, defaults[k])] for k in OPS[func][2])
        if (func, ints, eps) not in visited:
            missing.append((func, ints, eps))
    return missing


def threads(name, ints, tag):
    """Workgroup sizes the op may run with (ops.hpp::OpThreads): 256; a bisection's tree walk 512, its fp32 IFS form 1024
    (both are returned for a tree walk: the sizes derived from either are then all visited)."""
    names = OPS[name][2]
    if "t_method" in names and ints[names.index("t_method")] == T_METHOD["bisect"]:
        return (512, 1024)
    return (256,)


def sizes(nts, v):
    """Derived from the code: one element, the chunk boundary, the tile boundary, two tiles and a chunk's ragged end, and
    a few tiles plus a ragged tail (returned last: the size that is also compared with the oracle)."""
    s = set()
    for nt in nts:
        tile = nt * v
        s |= {1, v - 1, v, v + 1, 2 * v + 1, tile - 1, tile, tile + 1, 2 * tile + v - 1}
    s.discard(0)
    few = few_tiles(nts, v)
    return sorted(s - {few}) + [few]


def few_tiles(nts, v):
    return 3 * max(nts) * v + v + 1


# ---- operands -------------------------------------------------------------------------------------------------------------
class Op:
    """One operand as the ABI takes it; `data` is the host array behind the pointer; hybrid: the A and B tables too."""

    def __init__(self, data, mode=FIELD, length=0, inner=0, nflat=0, A=None, B=None):
        self.data, self.mode, self.len, self.inner, self.nflat, self.A, self.B = np.ascontiguousarray(data), mode, length, inner, nflat, A, B

    def full(self, n):
        """The operand materialised per point (what the oracle is given)."""
        d = self.data.reshape(-1)
        if self.mode == FIELD:
            return d
        if self.mode == SCALAR:
            return np.full(n, d[0], d.dtype)
        if self.mode == LEVEL_MAJOR:
            return np.repeat(d, self.inner)[:n]
        if self.mode == LEVEL_MINOR:
            return np.resize(d, n)
        from oracle import vertical_oracle as vo

        return np.ascontiguousarray(vo.pressure_on_hybrid_levels(self.A, self.B, d)).reshape(-1)[:n]


def with_mode(fields, mode, n, rng):
    """`fields`: one full array of n points per input.  Returns the operand list with the LAST one turned into `mode`:
    "field", "scalar", ("major", inner), ("minor", length) -- the level values are the last field's first points."""
    ops = [Op(a) for a in fields]
    last = fields[-1]
    if mode == "scalar":
        ops[-1] = Op(last[:1], SCALAR)
    elif mode != "field" and mode[0] == "major":
        inner = mode[1]
        nlev = -(-n // inner)
        ops[-1] = Op(np.resize(last, nlev), LEVEL_MAJOR, nlev, inner)
    elif mode != "field":
        ops[-1] = Op(np.resize(last, mode[1]), LEVEL_MINOR, mode[1], 0)
    return ops


def hybrid_operand(A, B, sp):
    dt = sp.dtype
    nz = np.flatnonzero(np.asarray(B) != 0.0)
    nflat = int(max(0, (nz[0] if nz.size else len(B)) - 1))   # as ekm_hip.vertical.HybridPressure counts them
    return Op(sp, HYBRID_FULL, len(A) - 1, sp.size, nflat, np.asarray(A, dt), np.asarray(B, dt))


def physical_fields(keys, p, rng):
    """Operands that fit a given pressure field (hybrid levels: 1 Pa to 1040 hPa): the standard atmosphere's temperature
    with a few K of scatter, humidity of 1-100 % but <= 0.04 kg/kg, and everything derived from them by the oracle --
    the recipe of tests/test_gpu_vertical.py::test_hybrid_pressure_operand."""
    from oracle import synthetic
    from oracle import thermo_oracle as o

    dt = p.dtype.type
    p64 = p.astype(np.float64)
    t = synthetic.standard_temperature(p64) + rng.normal(0, 4, p.shape)
    with np.errstate(all="ignore"):
        q = o.specific_humidity_from_relative_humidity(t, rng.uniform(1, 100, p.shape), p64)
        q = np.where(np.isfinite(q), np.clip(q, 1e-7, 0.04), 3e-6)
        omega = rng.uniform(-2.0, 2.0, p.shape)
        derived = dict(t=lambda: t, q=lambda: q, p=lambda: p64, omega=lambda: omega, w=lambda: q / (1 - q),
                       e=lambda: o.vapour_pressure_from_specific_humidity(q, p64), r=lambda: o.relative_humidity_from_specific_humidity(t, q, p64),
                       td=lambda: np.minimum(o.dewpoint_from_specific_humidity(q, p64), t - 0.1), th=lambda: o.potential_temperature(t, p64),
                       ept=lambda: o.ept_from_specific_humidity(t, q, p64))
        d = {k: derived[k]() for k in set(keys)}
    return [d[k].astype(dt) for k in keys]


# ---- the two runs -----------------------------------------------------------------------------------------------------------
def _call(lib, name, tag, operands, ints, eps, out_ptrs, n, dev=0, stream=None):
    from ekm_hip import _ffi

    cargs = [dev, stream] + [C.byref(o) for o in operands] + [int(v) for v in ints]
    if eps is not None:
        cargs.append(float(eps))
    _ffi.check(getattr(lib, f"ekm_{name}_{tag}")(*(cargs + list(out_ptrs) + [n])))


def run_guarded(lib, name, tag, ops, ints, eps, n, shift=0):
    """The call inside a guarded arena.  Buffer j starts (0, 1, V-1)[(shift + j) % 3] elements behind a 16-B boundary.
    Returns the outputs after arena.check()."""
    from ekm_hip import _ffi

    dt, v = TAGS[tag], VEC[tag]
    offs = (0, 1, v - 1)
    arena = Arena(DeviceMemory())
    k = shift
    for j, o in enumerate(ops):
        arena.input(f"in{j}:{OPS[name][0][j]}", o.data.astype(dt, copy=False), offs[k % 3])
        k += 1
        if o.mode == HYBRID_FULL:
            arena.input(f"in{j}:A", o.A, offs[k % 3])
            arena.input(f"in{j}:B", o.B, offs[(k + 1) % 3])
            k += 2
    for j, oname in enumerate(OPS[name][1]):
        arena.output(f"out{j}:{oname}", n, dt, offs[k % 3])
        k += 1
    arena.commit()
    try:
        operands = [_ffi.Operand(arena.ptr(f"in{j}:{OPS[name][0][j]}"), o.mode, o.nflat, o.len, o.inner,
                                 arena.ptr(f"in{j}:A") if o.mode == HYBRID_FULL else None,
                                 arena.ptr(f"in{j}:B") if o.mode == HYBRID_FULL else None) for j, o in enumerate(ops)]
        _call(lib, name, tag, operands, ints, eps, [arena.ptr(f"out{j}:{oname}") for j, oname in enumerate(OPS[name][1])], n)
        arena.check()
        return [arena.result(f"out{j}:{oname}") for j, oname in enumerate(OPS[name][1])]
    finally:
        arena.free()


def run_plain(ek, lib, name, tag, ops, ints, eps, n):
    """The same call on separately allocated, 16-B-aligned DeviceArrays."""
    from ekm_hip import _ffi

    dt = TAGS[tag]
    keep, operands = [], []
    for o in ops:
        d = ek.to_device(o.data.astype(dt, copy=False))
        keep.append(d)
        a = b = None
        if o.mode == HYBRID_FULL:
            a, b = ek.to_device(o.A), ek.to_device(o.B)
            keep += [a, b]
        operands.append(_ffi.Operand(d.ptr, o.mode, o.nflat, o.len, o.inner, a.ptr if a else None, b.ptr if b else None))
    outs = [ek.DeviceArray.empty((n,), dt) for _ in OPS[name][1]]
    assert all(x.ptr % 16 == 0 for x in keep + outs)
    _call(lib, name, tag, operands, ints, eps, [x.ptr for x in outs], n)
    host = [x.to_host() for x in outs]
    for x in keep + outs:
        x.free()
    return host


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(f"u{a.dtype.itemsize}"), b.view(f"u{b.dtype.itemsize}"))


def first_difference(a, b):
    i = int(np.flatnonzero(a.view(f"u{a.dtype.itemsize}") != b.view(f"u{b.dtype.itemsize}"))[0])
    return f"element {i}: {a[i]!r} against {b[i]!r}"


# ---- parity with the oracle, under the bars of tests/_compare.py as tests/test_gpu_parity.py applies them ---------------------------
def oracle_outputs(name, full, ints, eps):
    from oracle import thermo_oracle as orc
    from oracle import wind_oracle

    kw = reference_kwargs(name, ints, eps)
    ins = [a.copy() for a in full]
    with np.errstate(all="ignore"):
        if name.endswith("_from_es"):
            out = getattr(orc, name[:-len("_from_es")])(None, ins[0], es=ins[1], es_slope=ins[2], **kw)
        elif name == "w_from_omega":
            out = wind_oracle.w_from_omega(*ins)
        else:
            out = getattr(orc, name)(*ins, **kw)
    return out if isinstance(out, tuple) else (out,)


def assert_oracle_parity(name, tag, full, ints, eps, got, what):
    """As tests/test_gpu_parity.py::test_every_function_on_synthetic_columns judges a call (nothing relaxed beyond it)."""
    from _compare import assert_parity, bisect_sign_noise, bisect_unstable, newton_regime_boundary
    from oracle import thermo_oracle as orc

    kw = reference_kwargs(name, ints, eps)
    tm = kw.get("t_method")
    newton = tm == "newton" or name == "pipeline_full"
    want = oracle_outputs(name, full, ints, eps)
    want64 = oracle_outputs(name, [a.astype(np.float64) for a in full], ints, eps) if tag == "f32" and (tm in ("bisect", "newton") or newton) else None
    assert len(got) == len(want)
    for k, (g_, w_) in enumerate(zip(got, want)):
        unstable = ref64 = noise_t = None
        if tm == "bisect":
            unstable, noise_t = bisect_sign_noise(orc, name, full, {a: b for a, b in kw.items()}, 3e-6 if tag == "f32" else 1e-14, return_points=True)
            if want64 is not None:
                unstable |= bisect_unstable(w_, want64[k])
                ref64 = want64[k]
        elif newton and (tm == "newton" or k == 5):
            unstable = newton_regime_boundary(name, full, {a: b for a, b in kw.items()}, 1e-5 if tag == "f32" else 1e-13)
            if want64 is not None:
                ref64 = want64[k]
        assert_parity(g_, np.asarray(w_).reshape(-1), tag, f"{what}[out{k}]", bisect=tm == "bisect", unstable=unstable, ref64=ref64, noise_t=noise_t)
