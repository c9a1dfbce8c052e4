#!/usr/bin/env python3
"""Golden vectors for `wind` (speed, direction, xy_to_polar, polar_to_xy, coriolis, windrose), recorded from the
REFERENCE (build container only; stand-in for the un-vendored earthkit-utils in tests/golden/_standin).  Writes
tests/golden/wind_polar_golden.npz, data only:
  * `index`: JSON -- the cases (function, input set, dtype tag, keyword arguments, result types, dtypes and shapes),
    the error cases with type and message, the reference's own known answers and its constants;
  * (all arrays live in one blob per dtype; `index["arrays"]` says where: dtype, offset, shape)
  * `in.<set>.a / .b`: the inputs of a set as float64 (integer sets as int64); a case's inputs are these cast as its
    tag says (tests/_wind_numpy.py::cast_inputs), so float32 inputs are not stored twice;
  * `out.<case>.<k>`: the reference's k-th result; for every f32 case also on the inputs upcast to float64 (`.up`).
While recording, the reference's f32 run is judged against its own f64 run on the upcast inputs with the direction
judge of tests/_wind_numpy.py: a 0 / 360 wrap outside the neighbourhood of the branch point stops the recording."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("EKM_REFERENCE", "/root/reference")
sys.path[:0] = [os.path.join(HERE, "_standin"), os.path.join(REF, "src"), os.path.dirname(HERE)]

from earthkit.meteo import constants  # noqa: E402
from earthkit.meteo.wind.array import wind as ref  # noqa: E402

import _wind_numpy as wn  # noqa: E402

np.seterr(all="ignore")
E64, E32 = np.finfo(np.float64).eps, np.finfo(np.float32).eps
DIRECTION_KW = [dict(convention="meteo"), dict(convention="polar"), dict(convention="polar", to_positive=False)]
CONVENTION_KW = [dict(convention="meteo"), dict(convention="polar")]


def pairs(values):
    a, b = np.meshgrid(np.array(values, np.float64), np.array(values, np.float64))
    return a.ravel(), b.ravel()


def main():
    store, cases, errors = {}, [], []
    rng = np.random.default_rng(20261019)

    def add_set(name, a, b=None):
        store[f"in.{name}.a"] = np.asarray(a)
        if b is not None:
            store[f"in.{name}.b"] = np.asarray(b)

    # ---- input sets ----
    longest = max(wn.TILE.values()) + 1
    field_u, field_v = rng.normal(0, 12, longest), rng.normal(0, 12, longest)
    for n in [63, 64, 257] + [t + k for t in sorted(set(wn.TILE.values())) for k in (-1, 0, 1)]:
        add_set(f"uv{n}", field_u[:n], field_v[:n])  # prefixes of one field: the packer stores them once
    for n in (1, 65):
        add_set(f"uv{n}", rng.normal(0, 12, n), rng.normal(0, 12, n))
    for n in (1, 63, 64, 65, 257):
        add_set(f"md{n}", rng.uniform(0, 60, n), rng.uniform(-90, 450, n))
        add_set(f"lat{n}", rng.uniform(-90, 90, n))
    special = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-30, -1e-30, 1e30, -1e30, 5e-324, -5e-324, 1e-310, 1e-40, 1e-45, 1.0, -1.0]
    add_set("uvspecial", *pairs(special))
    # the neighbourhood of the meteo branch point (v < 0, |u| = k eps |v|), both signs of u, eps of both dtypes; the axes
    ks = np.array([0.25, 0.5, 1.0, 2.0, 4.0])
    bu, bv = [], []
    for v in (-1.0, -3.7, -2.0 ** -20, -1234.5):
        for eps in (E64, E32):
            for s in (1.0, -1.0):
                bu += list(s * ks * eps * abs(v))
                bv += [v] * len(ks)
    bu += [1.0, -1.0, 0.0, 0.0, 7.5, -7.5, 0.0, 0.0]
    bv += [0.0, 0.0, 1.0, -1.0, 0.0, -0.0, 7.5, -7.5]
    add_set("uvbranch", bu, bv)
    add_set("uvhuge", [3e200, 1e-320, 3e38, 3e38, 1e308, 1e-160, 2e-23], [4e200, 1e-320, 1e38, 3e38, 1e308, 1e-160, 1e-23])
    known_u = [0, 1, 1, 1, 0, -1, -1, -1, 0, np.nan, 1, np.nan]
    known_v = [1, 1, 0, -1, -1, -1, 0, 1, 0, 1, np.nan, np.nan]
    add_set("uvknown", known_u, known_v)
    add_set("uvint", np.array([0, 1, 1, 1, 0, -1, -1, -1, 0, 3, -40], np.int64), np.array([1, 1, 0, -1, -1, -1, 0, 1, 0, 4, 9], np.int64))
    add_set("uvscalar", [1.0], [1.0])
    add_set("uvscalar_nan", [1.0], [np.nan])
    add_set("uvgrid", rng.normal(0, 9, (5, 1)), rng.normal(0, 9, (1, 67)))
    mags = [0.0, 1.0, -2.5, np.inf, -np.inf, np.nan, 1e30, 5e-324]
    dirs = [0.0, 90.0, 180.0, 270.0, 360.0, 45.0, -90.0, 720.0, 1e6, np.inf, -np.inf, np.nan, 123.456, 1e-30]
    m, d = np.meshgrid(np.array(mags), np.array(dirs))
    add_set("mdspecial", m.ravel(), d.ravel())
    add_set("mdknown", [1.0, 1.4142135624, 1.0, 1.4142135624, 1.0, 1.4142135624, 1.0, 1.4142135624, 0.0, np.nan, 1, np.nan],
            [180.0, 225, 270, 315, 0, 45, 90, 135, 270, 1, np.nan, np.nan])
    add_set("mdint", np.array([0, 1, 5, 12], np.int64), np.array([0, 90, 225, 359], np.int64))
    add_set("mdscalar", [10.0], [225.0])
    add_set("latspecial", dirs + [-20.0, 50.0, 89.999999, -0.0])
    add_set("latint", np.array([-20, 0, 50, 90, -90], np.int64))
    add_set("latscalar", [50.0])

    def record(func, setname, tag, kwargs, nin):
        base = [store[f"in.{setname}.{n}"] for n in "ab"[:nin]]
        cid = f"{func}.{setname}.{tag}" + "".join(f".{k[:3]}{v}" for k, v in sorted(kwargs.items()))
        fn = getattr(ref, func)
        ins = wn.cast_inputs(base, tag)
        kept = [np.array(x, copy=True) for x in ins]
        out = fn(*ins, **kwargs)
        assert all(np.array_equal(np.asarray(x), k, equal_nan=True) for x, k in zip(ins, kept)), "the reference modified an input"
        outs = out if isinstance(out, tuple) else (out,)
        cases.append(dict(id=cid, func=func, set=setname, tag=tag, kwargs=kwargs, nin=nin, nout=len(outs),
                          result_type=[type(o).__name__ for o in outs], dtype=[str(np.asarray(o).dtype) for o in outs],
                          shape=[list(np.shape(o)) for o in outs]))
        for k, o in enumerate(outs):
            store[f"out.{cid}.{k}"] = np.asarray(o)
        if tag == "f32":
            up = fn(*[x.astype(np.float64) for x in ins], **kwargs)
            up = up if isinstance(up, tuple) else (up,)
            for k, o in enumerate(up):
                store[f"out.{cid}.{k}.up"] = np.asarray(o)
            if func in ("direction", "xy_to_polar"):
                wrap_check(cid, ins[0], ins[1], outs[-1], up[-1], kwargs)

    def wrap_check(what, u, v, got32, want64, kwargs):
        """The reference's f32 run against its f64 run on the upcast inputs: a 0 / 360 wrap only where v < 0 and
        |u| <= 4 eps32 |v|.  The polar convention has its own branch point, v -> -0 beside u > 0 (there atan2f underflows
        to -0, which is not < 0): the mirrored neighbourhood is used for it.  Off the wrap the two runs are within
        2 eps32 360: atan2f 1 ulp of pi (0.5), the float subtraction (0.5), 1.5 pi rounded to float (0.32), the product
        rounded to float (0.5): 1.82."""
        g, w = np.asarray(got32, np.float64), np.asarray(want64, np.float64)
        plain = np.where(np.isnan(w) | (g == w), 0.0, np.abs(g - w))
        at_branch = (v < 0) & (np.abs(u) <= 4 * E32 * np.abs(v))
        if kwargs.get("convention") == "polar":
            at_branch = (v < 0) & (u > 0) & (np.abs(v) <= 4 * E32 * np.abs(u))
        err = np.where(at_branch, np.minimum(plain, np.abs(360.0 - plain)), plain)
        assert (err <= 2 * E32 * 360).all(), (what, float(err.max()), int(np.argmax(err)))

    # the census inputs of tests/test_gpu_wind.py through the same check
    cu, cv, _, _ = wn.census_inputs(np.float32, get=lambda key: store[key])
    for kw in DIRECTION_KW:
        wrap_check(f"census {kw}", cu, cv, ref.direction(cu, cv, **kw), ref.direction(cu.astype(np.float64), cv.astype(np.float64), **kw), kw)

    # ---- elementwise cases ----
    for tag in ("f64", "f32"):
        for s in ("uv1", "uv65", "uvspecial", "uvbranch", "uvhuge", "uvknown"):
            record("speed", s, tag, {}, 2)
            for kw in DIRECTION_KW:
                record("direction", s, tag, kw, 2)
            for kw in CONVENTION_KW:
                record("xy_to_polar", s, tag, kw, 2)
        for s in ["uv63", "uv64", "uv257", "uvgrid"] + [f"uv{wn.TILE[tag] + k}" for k in (-1, 0, 1)]:
            record("xy_to_polar", s, tag, {}, 2)
            if s != "uvgrid":  # speed and direction are kernels of their own (one output each): their body and tail too
                record("speed", s, tag, {}, 2)
                for kw in DIRECTION_KW:
                    record("direction", s, tag, kw, 2)
        for s in ("md1", "md65", "mdspecial", "mdknown"):
            for kw in CONVENTION_KW:
                record("polar_to_xy", s, tag, kw, 2)
        for s in ("md63", "md64", "md257"):
            record("polar_to_xy", s, tag, {}, 2)
        for s in [f"lat{n}" for n in (1, 63, 64, 65, 257)] + ["latspecial"]:
            record("coriolis", s, tag, {}, 1)
    for tag, uv, md, lat in (("int", "uvint", "mdint", "latint"), ("mixed", "uv65", "md65", None), ("scalar", "uvscalar", "mdscalar", "latscalar")):
        record("speed", uv, tag, {}, 2)
        for kw in DIRECTION_KW:
            record("direction", uv, tag, kw, 2)
        for kw in CONVENTION_KW:
            record("xy_to_polar", uv, tag, kw, 2)
            record("polar_to_xy", md, tag, kw, 2)
        if lat:
            record("coriolis", lat, tag, {}, 1)
    for kw in DIRECTION_KW[:2]:
        record("direction", "uvscalar_nan", "scalar", kw, 2)

    # ---- wind rose ----
    def rose_samples(dtype, sectors, bins, n=120):
        """Random samples, then one on every edge of both axes (each against a mid value of the other axis), then
        out-of-range and NaN values."""
        se, de = wn.rose_edges(np.dtype(dtype), sectors, bins)
        se, de = se.astype(np.float64), de.astype(np.float64)
        sp = rng.uniform(se[0] - 0.1 * (se[-1] - se[0]), se[-1] + 0.1 * (se[-1] - se[0]), n)
        di = rng.uniform(0, 360, n)
        mid_s, mid_d = 0.5 * (se[0] + se[-1]), 123.4
        sp = np.concatenate([sp, se, np.full(len(de), mid_s), [se[-1], se[0], mid_s, np.nan, mid_s, np.nan, se[-1] + 1, se[0] - 1, mid_s, mid_s]])
        di = np.concatenate([di, np.full(len(se), mid_d), de, [de[-1], de[0], np.nan, mid_d, 0.0, np.nan, mid_d, mid_d, de[-1] + 1, de[0] - 1]])
        return sp, di

    def record_rose(name, sp, di, sectors, bins, percent, note=""):
        out = ref.windrose(sp, di, sectors=sectors, speed_bins=bins, percent=percent)
        cid = f"windrose.{name}.s{sectors}.b{len(bins)}.{'pct' if percent else 'cnt'}"
        key = f"rose.{name}.s{sectors}.b{len(bins)}"  # (the samples are shared by the percent / count pair)
        store[f"{key}.speed"], store[f"{key}.direction"], store[f"{key}.bins"] = np.asarray(sp), np.asarray(di), np.asarray(bins)
        store[f"out.{cid}.0"], store[f"out.{cid}.1"] = np.asarray(out[0]), np.asarray(out[1])
        cases.append(dict(id=cid, func="windrose", samples=key, sectors=sectors, percent=percent, note=note, scalar=np.ndim(sp) == 0,
                          bins_is_list=isinstance(bins, list), dtype=[str(out[0].dtype), str(out[1].dtype)],
                          shape=[list(out[0].shape), list(out[1].shape)]))

    bin_sets = {"two": [0.0, 5.0], "uniform": list(np.linspace(0.0, 40.0, 41)), "ragged": [0.0, 0.5, 2.0, 3.5, 7.0, 12.0, 30.0]}
    for sectors in (1, 4, 7, 16, 360, 1000):
        for bname, bins in bin_sets.items():
            if sectors == 1000 and bname == "ragged":
                continue
            sp, di = rose_samples(np.float64, sectors, bins)
            for percent in (False, True):
                record_rose(f"f64.{bname}", sp, di, sectors, bins, percent)
    for sectors in (7, 16, 360):
        sp, di = rose_samples(np.float32, sectors, bin_sets["ragged"])
        sp32, di32 = sp.astype(np.float32), di.astype(np.float32)
        record_rose("f32.ragged", sp32, di32, sectors, bin_sets["ragged"], True)
        record_rose("f32f64.ragged", sp32, di, sectors, bin_sets["ragged"], False, "float32 speed, float64 direction")
        record_rose("f64f32.ragged", sp, di32, sectors, bin_sets["ragged"], False, "float64 speed, float32 direction")
        spi = rng.integers(-2, 34, 200)
        dii = rng.integers(0, 361, 200)
        record_rose("int.ragged", spi, dii, sectors, [0.5, 2.9, 3.0, 7.7, 12.0, 30.0], False, "integer samples: truncated integer edges")
        record_rose("intf64.ragged", spi, dii.astype(np.float64) + 0.25, sectors, [0, 2, 3, 7, 12, 30], True, "integer speed, float64 direction")
    record_rose("f64.empty", np.array([50.0, -3.0, np.nan]), np.array([10.0, 20.0, 30.0]), 16, [0.0, 5.0, 10.0], True, "nothing counted: all NaN")
    record_rose("f64.empty", np.array([50.0, -3.0, np.nan]), np.array([10.0, 20.0, 30.0]), 16, [0.0, 5.0, 10.0], False, "nothing counted")
    record_rose("f64.nosamples", np.zeros(0), np.zeros(0), 4, [0.0, 5.0], False, "no samples")
    record_rose("f64.flatbins", np.array([1.0, 2.0, 2.0, 3.0]), np.array([5.0, 95.0, 185.0, 275.0]), 4, [0.0, 2.0, 2.0, 4.0], False, "a repeated edge")
    known_sp = [3.5, 1, 1.1, 2.1, 0.1, 0.0, 2.4, 1.9, 1.7, 3.9, 3.1, 2.1, np.nan, np.nan]
    known_di = [1.0, 29, 31, 93.0, 121, 171, 189, 245, 240.11, 311, 359.1, np.nan, 11, np.nan]
    for percent in (False, True):
        record_rose("known", np.array(known_sp), np.array(known_di), 6, [0, 1, 2, 3, 4], percent, "the reference's own test")
    record_rose("known.scalar", 3.4, 90.01, 6, [0, 5], False, "Python scalars")
    record_rose("known.scalar", 3.4, 90.01, 1, [0, 5], False, "Python scalars, one sector")

    def record_error(name, call, **args):
        try:
            call()
        except Exception as exc:  # noqa: BLE001
            errors.append(dict(id=name, type=type(exc).__name__, bases=[b.__name__ for b in type(exc).__mro__], message=str(exc), **args))
        else:
            raise AssertionError(f"{name}: the reference did not raise")

    one = (np.array([3.4]), np.array([90.01]))
    record_error("rose.sectors0", lambda: ref.windrose(*one, sectors=0, speed_bins=[0, 1]), sectors=0, bins=[0, 1])
    record_error("rose.onebin", lambda: ref.windrose(*one, sectors=6, speed_bins=[0]), sectors=6, bins=[0])
    record_error("rose.nobins", lambda: ref.windrose(*one, sectors=6, speed_bins=None), sectors=6, bins=None)
    record_error("rose.decreasing", lambda: ref.windrose(*one, sectors=6, speed_bins=[0, 2, 1]), sectors=6, bins=[0, 2, 1])
    record_error("rose.2d", lambda: ref.windrose(np.ones((2, 3)), np.ones((2, 3)), sectors=6, speed_bins=[0, 2]), sectors=6, bins=[0, 2], message_compared=False)
    record_error("direction.convention", lambda: ref.direction(1.0, 1.0, convention="north"))
    record_error("polar_to_xy.convention", lambda: ref.polar_to_xy(1.0, 1.0, convention="north"))

    known = dict(u=known_u, v=known_v, speed=[1.0, 1.4142135624, 1.0, 1.4142135624, 1.0, 1.4142135624, 1.0, 1.4142135624, 0.0, np.nan, np.nan, np.nan],
                 meteo=[180.0, 225, 270, 315, 0, 45, 90, 135, 270, np.nan, np.nan, np.nan],
                 polar=[90, 45, 0, 315, 270, 225, 180, 135.0, 0, np.nan, np.nan, np.nan],
                 polar_signed=[90, 45, 0, -45, -90, -135, 180, 135, 0, np.nan, np.nan, np.nan],
                 coriolis=[[-20, 0, 50], [-0.0000498810, 0.0, 0.0001117217]],
                 specials=[[0.0, -1.0, 0.0], [-0.0, -1.0, 0.0], [0.0, 0.0, 270.0], [-0.0, -0.0, 90.0], [-np.inf, -np.inf, 45.0], [np.inf, 1.0, 270.0]])
    for u, v, want in known["specials"]:  # (the issue's list of IEEE corner values, checked here against the reference)
        got = float(ref.direction(np.array([u]), np.array([v]))[0])
        assert abs(got - want) < 1e-12, (u, v, got, want)
    consts = dict(omega=float(constants.omega).hex(), degree=float(constants.degree).hex(), radian=float(constants.radian).hex())
    # every array goes into one blob per dtype (hundreds of small members would cost more in zip headers than in data)
    blobs, where = {}, {}
    # (largest first, and an array whose bytes are a prefix of one already stored -- the tile-edge lengths, the speed of
    # speed() and of xy_to_polar() -- points into that one)
    for key, a in sorted(store.items(), key=lambda kv: -np.asarray(kv[1]).size):
        a = np.asarray(a)
        parts = blobs.setdefault(a.dtype.str, [])
        flat, offset, hit = np.ascontiguousarray(a).ravel(), 0, None
        for p in parts:
            if hit is None and 0 < flat.size <= p.size and p[:flat.size].tobytes() == flat.tobytes():
                hit = offset
            offset += p.size
        where[key] = [a.dtype.str, int(offset if hit is None else hit), list(a.shape)]
        if hit is None:
            parts.append(flat)
    index = dict(cases=cases, errors=errors, known=known, constants=consts, arrays=where, numpy=np.__version__)
    packed = {"blob" + dt: np.concatenate(parts) for dt, parts in blobs.items()}
    packed["index"] = np.frombuffer(json.dumps(index).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "wind_polar_golden.npz")
    np.savez_compressed(path, **packed)
    print("wrote", len(store), "arrays,", len(cases), "cases,", len(errors), "errors,", os.path.getsize(path), "bytes;",
          "solar_golden.npz is", os.path.getsize(os.path.join(HERE, "solar_golden.npz")))


if __name__ == "__main__":
    main()
