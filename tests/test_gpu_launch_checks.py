"""The argument checks of every C entry point outside the map kernels (ensemble, reduce, solar, wind, interp, hybrid
units), as a table: the valid call, every pointer null, every pointer one byte off, no points, a bad enum, one member too
many.  Each case is held to the exact return code; an error also leaves a message that starts with the function's name
and outputs that still hold their fill.  Every error is returned before anything is launched.

Sizes: 65 points (a wave and one lane), 3 members / samples over 5 climate rows, [outer, m, inner] = [2, 3, 3], 2 targets
over 4 levels, 2 time nodes, 3 + 4 rose edges, 2 patterns of 5 points.  Every buffer is 1024 elements, so a pointer one
byte on stays inside its allocation where an entry point accepts it (the hybrid unit takes unaligned fields on its
element-wise path; the float64 tables of efi, crps and the quantiles are only checked for null)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, HIP, ARG, ENUM = 0, -1, -2, -3
NPTS, NENS, NCLIM = 65, 3, 5
FILL = 7.0
ELEMS = 1024


def IN(key):
    return ("in", key)


def OUT(key, dtype="T"):
    return ("out", key, dtype)


def OP(key):
    return ("op", key)


def N(value):
    return ("n", value)


def entry(name, args, tags=("f32", "f64"), null_ok=(), odd_ok=(), enum=None, cap=None, extra=(), prefix=None):
    return [dict(name=name, tag=t, args=args, null_ok=set(null_ok), odd_ok=set(odd_ok), enum=enum, cap=cap, extra=extra,
                 prefix=prefix or name) for t in tags]


ENS_CAP = {"f32": 257, "f64": 129, "f32_f64": 257}  # 64 KiB of LDS per workgroup / (64 lanes * element) + 1
CPF_CAP = {"f32": 641, "f64": 321}                  # 160 KiB
HYB = ("A", "B", "sp", "zs", "t", "q", "alpha", "delta", "full", "half", "out", "flag")  # the hybrid unit checks null only
AUX = [("amin_d", IN("one")), ("amin_c", IN("one")), ("amax_d", IN("one")), ("amax_c", IN("one"))]

TABLE = sum([
    # ---- ensemble.hip
    entry("efi", [("clim", IN("one")), ("ens", IN("one")), ("nclim", NCLIM), ("nens", NENS), ("npts", N(NPTS)), ("eps", -1.0),
                  ("acosdiff", IN("one64")), ("proddiff", IN("one64")), ("acoef", IN("one64")), ("out", OUT("out", "f8"))],
          odd_ok=("acosdiff", "proddiff", "acoef"), cap=("nens", ENS_CAP),
          extra=[("one climate row needs no tables", dict(nclim=1, acosdiff=None, proddiff=None, acoef=None), OK)]),
    entry("sot", [("qc", IN("one")), ("qc_tail", IN("ramp")), ("ens", IN("one")), ("nens", NENS), ("npts", N(NPTS)), ("perc", 90),
                  ("eps", -1.0), ("out", OUT("out"))], cap=("nens", ENS_CAP)),
    entry("sot_func", [("qc_tail", IN("ramp")), ("qc", IN("one")), ("qf", IN("one")), ("n", N(NPTS)), ("eps", -1.0), ("lo", -10.0),
                       ("hi", 10.0), ("out", OUT("out"))]),
    entry("cpf", [("clim", IN("one")), ("ens", IN("one")), ("nclim", NCLIM), ("nens", NENS), ("npts", N(NPTS)), ("sort_clim", 1),
                  ("sort_ens", 1), ("from_zero", 0), ("symmetric", 0), ("use_epsilon", 0), ("epsilon", 0.0), ("out", OUT("out", "f4"))],
          cap=("nens", CPF_CAP)),
    entry("crps_from_ensemble", [("x", IN("one")), ("y", IN("one")), ("nens", NENS), ("npts", N(NPTS)), ("p2", IN("one64")),
                                 ("q2", IN("one64")), ("out", OUT("out", "f8")), ("missing", OUT("missing", "f4"))],
          null_ok=("missing",), odd_ok=("p2", "q2", "missing"), cap=("nens", ENS_CAP)),
    entry("quantiles", [("arr", IN("one")), ("outer", N(2)), ("m", 3), ("inner", 3), ("lo", IN("zero64")), ("hi", IN("zero64")),
                        ("w", IN("zero64")), ("nq", 2), ("mode", 1), ("out", OUT("out"))],
          odd_ok=("lo", "hi", "w"), enum=("mode", 2), cap=("m", ENS_CAP)),
    entry("quantiles", [("arr", IN("one")), ("outer", N(2)), ("m", 3), ("inner", 3), ("lo", IN("zero64")), ("hi", IN("zero64")),
                        ("w", IN("zero64")), ("nq", 2), ("mode", 0), ("out", OUT("out", "f8"))], tags=("f32_f64",),
          odd_ok=("lo", "hi", "w"), enum=("mode", 2), cap=("m", ENS_CAP)),
    entry("gumbel_fit", [("sample", IN("ramp")), ("outer", N(2)), ("m", 3), ("inner", 3), ("mu", OUT("mu", "f8")),
                         ("sigma", OUT("sigma", "f8"))], cap=("m", ENS_CAP)),
    entry("gumbel_cdf", [("mu", IN("one64")), ("sigma", IN("one64")), ("npts", N(NPTS)), ("x", IN("one64")), ("nx", 2), ("freq", 1.0),
                         ("mode", 0), ("out", OUT("out", "f8"))], tags=("f64",), enum=("mode", 2)),
    entry("gumbel_ppf", [("mu", IN("one64")), ("sigma", IN("one64")), ("npts", N(NPTS)), ("t", IN("one64")), ("nt", 2),
                         ("out", OUT("out", "f8"))], tags=("f64",)),
    # ---- reduce.hip
    entry("regimes_project", [("field", IN("one")), ("nfields", N(3)), ("k", 5), ("coef", IN("one")), ("npat", 2), ("coef_stride", 0),
                              ("scale", IN("one")), ("out", OUT("out"))], null_ok=("scale",)),
    entry("regimes_index", [("proj", IN("one")), ("mean", IN("one")), ("mean_value", 0.0), ("std", IN("one")), ("std_value", 1.0),
                            ("out", OUT("out")), ("n", N(NPTS))], null_ok=("mean", "std")),
    entry("pearson", [("x", IN("ramp")), ("y", IN("ramp")), ("outer", N(2)), ("m", 3), ("inner", 3), ("out", OUT("out"))],
          extra=[("an empty sample axis", dict(m=0), ARG)]),
    entry("pearson", [("x", IN("ramp")), ("y", IN("ramp")), ("outer", N(6)), ("m", 3), ("inner", 1), ("out", OUT("out"))]),
    # ---- solar.hip
    entry("solar", [("lat", OP("one")), ("lon", OP("one")), ("nodes", IN("one64")), ("nnodes", 2), ("out", OUT("out")), ("n", N(NPTS))]),
    entry("solar", [("lat", OP("one")), ("lon", OP("one")), ("nodes", IN("one64")), ("nnodes", 2), ("out", OUT("out", "f8")),
                    ("n", N(NPTS))], tags=("f32_f64",)),
    # ---- wind.hip
    entry("wind_polar", [("u", OP("one")), ("v", OP("one")), ("mode", 0), ("speed", OUT("speed")), ("direction", OUT("direction")),
                         ("n", N(NPTS))], null_ok=("speed", "direction"), enum=("mode", 3)),
    entry("wind_xy", [("magnitude", OP("one")), ("direction", OP("one")), ("mode", 0), ("x", OUT("x")), ("y", OUT("y")), ("n", N(NPTS))],
          enum=("mode", 2)),
    entry("wind_coriolis", [("lat", OP("one")), ("out", OUT("out")), ("n", N(NPTS))]),
    entry("windrose", [("speed", IN("one")), ("direction", IN("one")), ("n", N(NPTS)), ("edges", IN("edges")), ("ns", 3), ("nd", 4),
                       ("inv_step", 1.0 / 120.0), ("percent", 0), ("table", OUT("table", "f8")), ("out", OUT("out", "f8"))]),
    # ---- interp.hip
    entry("interpolate_monotonic", [("data", IN("one")), ("coord", IN("ramp")), ("coord_is_field", 0), ("target", IN("ramp")),
                                    ("target_is_field", 0), ("ntarget", 2), ("npts", N(NPTS)), ("nlev", 4), ("descending", 0), ("mode", 0)]
          + AUX + [("aux_field_mask", 0), ("out", OUT("out"))], null_ok=("amin_d", "amin_c", "amax_d", "amax_c"), enum=("mode", 3)),
    entry("interpolate_hybrid_to_pressure", [("data", IN("one")), ("A", IN("ramp")), ("B", IN("zero")), ("sp", IN("one")),
                                             ("target", IN("ramp")), ("target_is_field", 0), ("ntarget", 2), ("npts", N(NPTS)), ("nfull", 4),
                                             ("descending", 0), ("mode", 0)] + AUX + [("aux_field_mask", 0), ("out", OUT("out"))],
          null_ok=("amin_d", "amin_c", "amax_d", "amax_c"), odd_ok=("A", "B"), enum=("mode", 3)),
    entry("height_from_geopotential", [("z", IN("one")), ("zs", IN("one")), ("npts", N(NPTS)), ("nlev", 4), ("mode", 4), ("out", OUT("out"))],
          enum=("mode", 6), extra=[("above sea level zs is not read", dict(mode=2, zs=None), OK)]),
    # ---- hybrid.hip
    entry("pressure_on_hybrid_levels", [("A", IN("ramp")), ("B", IN("one")), ("sp", IN("one")), ("npts", N(NPTS)), ("nfull", 4), ("row_full", None),
                                        ("row_half", None), ("top_is_zero", 0), ("alpha_top", 0.5), ("full", OUT("full")), ("half", OUT("half")),
                                        ("delta", OUT("delta")), ("alpha", OUT("alpha"))], null_ok=("full", "half", "delta", "alpha"),
          odd_ok=HYB + ("delta",)),
    entry("geopotential_on_hybrid_levels", [("A", IN("ramp")), ("B", IN("one")), ("sp", IN("one")), ("zs", IN("one")), ("t", IN("one")),
                                            ("q", IN("zero")), ("npts", N(NPTS)), ("nfull", 4), ("top_is_zero", 0), ("alpha_top", 0.5), ("mode", 1),
                                            ("out", OUT("out"))], odd_ok=HYB, enum=("mode", 6),
          extra=[("the thickness does not read zs", dict(mode=0, zs=None), OK)]),
    entry("geopotential_thickness_from_alpha_delta", [("t", IN("one")), ("q", IN("zero")), ("alpha", IN("one")), ("delta", IN("one")),
                                                      ("npts", N(NPTS)), ("nfull", 4), ("out", OUT("out"))], odd_ok=HYB),
    # (no lane finds a value at or below the threshold, so the flag is never touched)
    entry("any_le", [("sp", IN("one")), ("n", N(NPTS)), ("a0", 0.0), ("b0", 1.0), ("thresh", -1.0), ("flag", OUT("flag", "f4"))], odd_ok=HYB),
], [])


@pytest.fixture(scope="module")
def inputs(ek):
    made = {}
    for tag, T in (("f32", np.float32), ("f64", np.float64)):
        made[tag] = {"one": ek.to_device(np.ones(ELEMS, T)), "zero": ek.to_device(np.zeros(ELEMS, T)),
                     "ramp": ek.to_device(np.arange(ELEMS, dtype=T))}
    edges = np.zeros(ELEMS)
    edges[:7] = [0.0, 2.0, 4.0, 0.0, 120.0, 240.0, 360.0]
    shared = {"one64": ek.to_device(np.ones(ELEMS)), "zero64": ek.to_device(np.zeros(ELEMS)), "edges": ek.to_device(edges)}
    for tag in made:
        made[tag].update(shared)
    made["f32_f64"] = made["f32"]
    yield made
    for arr in list(made["f32"].values()) + [made["f64"][k] for k in ("one", "zero", "ramp")]:
        arr.free()


def _cases(e):
    """(what, overrides, expected code): overrides maps an argument's name to a value, ('null',) or ('odd',)."""
    ptrs = [n for n, s in e["args"] if isinstance(s, tuple) and s[0] in ("in", "out", "op")]
    size = next(n for n, s in e["args"] if isinstance(s, tuple) and s[0] == "n")
    cases = [(f"{n} null", {n: ("null",)}, OK if n in e["null_ok"] else ARG) for n in ptrs]
    cases += [(f"{n} one byte on", {n: ("odd",)}, OK if n in e["odd_ok"] else ARG) for n in ptrs]
    if e["enum"]:
        cases.append((f"{e['enum'][0]} out of range", {e["enum"][0]: e["enum"][1]}, ENUM))
    if e["cap"]:
        cases.append((f"{e['cap'][0]} one past the cap", {e["cap"][0]: e["cap"][1][e["tag"]]}, ARG))
    cases += list(e["extra"])
    cases.sort(key=lambda c: c[2] == OK)  # errors first: they must find and leave the outputs' fill
    return cases + [("valid", {}, OK), ("no points", {size: 0}, OK)]


@pytest.mark.parametrize("e", TABLE, ids=lambda e: f"{e['name']}_{e['tag']}")
def test_entry_point(ek, inputs, e):
    from ekm_hip import _ffi

    lib = _ffi.lib()
    fn = getattr(lib, f"ekm_{e['name']}_{e['tag']}")
    T = np.float64 if e["tag"] == "f64" else np.float32
    dtypes = {"T": T, "f4": np.float32, "f8": np.float64}
    outs = {s[1]: ek.to_device(np.full(ELEMS, FILL, dtypes[s[2]])) for _, s in e["args"] if isinstance(s, tuple) and s[0] == "out"}
    keep = []

    def value(name, spec, how):
        if not isinstance(spec, tuple):
            return spec
        if spec[0] == "n":
            return spec[1]
        base = (outs[spec[1]] if spec[0] == "out" else inputs[e["tag"]][spec[1]]).on(None)
        ptr = None if how == "null" else base + 1 if how == "odd" else base
        if spec[0] != "op":
            return ptr
        keep.append(_ffi.Operand(ptr, _ffi.FIELD, 0, 0, 0))
        return C.byref(keep[-1])

    try:
        for what, over, want in _cases(e):
            args = []
            for name, spec in e["args"]:
                o = over.get(name, ())
                args.append(value(name, spec, o[0]) if isinstance(o, tuple) and o else o if name in over else value(name, spec, ""))
            rc = fn(0, None, *args)
            print(f"{e['name']}_{e['tag']} {what}: {rc}" + (f" {lib.ekm_last_error()!r}" if rc else ""))
            assert rc == want, (what, rc, lib.ekm_last_error())
            if want != OK:
                msg = lib.ekm_last_error()
                assert msg and msg.decode().startswith(e["prefix"]), (what, msg)
                for key, arr in outs.items():
                    assert (arr.to_host() == FILL).all(), f"{what}: {key} was written"
        ek.synchronize()
    finally:
        for arr in outs.values():
            arr.free()
