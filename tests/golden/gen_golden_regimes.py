#!/usr/bin/env python3
"""Golden vectors for regimes.project, regimes.regime_index and score.pearson_correlation, recorded from the REFERENCE
(build container only; stand-ins for the un-vendored packages in tests/golden/_standin, as in gen_golden_gumbel.py).  The
reference's regimes/array/index.py, regimes/patterns.py and score/array/deterministic.py are loaded by file path, so
nothing else of the package is imported.

Writes tests/golden/regimes_golden.npz: data only; arrays are stored once and shared between cases; a JSON manifest with
the NumPy version that computed them and the recorded signature strings; the file regenerates byte for byte.

project cases: pattern shapes (1,1), (7,9), (1,64), (5,13), (16,16), (1,257), (25,41) and one (91,121); field batches (),
(1,), (5,), (2,3,4) (the last only up to 65 grid points, every case at most 5200 field values: the file stays small);
1, 3, 8 and 9 patterns (1 or 3 on the (25,41) grid); f32/f32/f32, f32 fields with f64 patterns, all f64; uniform and cos-latitude weights;
ConstantPatterns, ModulatedPatterns with one modulator value per field (and a 0-d one), a subclass whose patterns have
the field's full shape; a field with a NaN and one with an infinity; the error cases.
pearson cases: f32 and f64; sample counts 1, 2, 3, 9, 51, 257; inner 1, 2, 63, 64, 65, 1000 and outer 1, 3 by way of
axes 0, 1, 2 and -1 of 2-D and 3-D arrays; temperature-like (280 +- 5) and anomaly-like (0 +- 1) data; x and y built
from two fixed vectors with prescribed r in {1, -1, 0, 0.42, -0.13}; a constant column, a NaN member, integer input.
regime_index cases: scalar and array mean and std, std of 0, f32 and f64, an f32 projection with f64 arrays.
"""
import importlib.util
import inspect
import io
import json
import os
import sys
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("EKM_REFERENCE", "/root/reference")
sys.path[:0] = [os.path.join(HERE, "_standin"), os.path.join(REF, "src")]

warnings.simplefilter("ignore")
np.seterr(all="ignore")

F32, F64 = np.float32, np.float64


def load_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_METEO = os.path.join(REF, "src", "earthkit", "meteo")
ref_index = load_path("_ref_regimes_index", os.path.join(_METEO, "regimes", "array", "index.py"))
ref_patterns = load_path("_ref_regimes_patterns", os.path.join(_METEO, "regimes", "patterns.py"))
ref_score = load_path("_ref_score_deterministic", os.path.join(_METEO, "score", "array", "deterministic.py"))


def bare_signature(fn):
    sig = inspect.signature(fn)
    params = [p.replace(annotation=inspect.Parameter.empty) for p in sig.parameters.values()]
    return str(sig.replace(parameters=params, return_annotation=inspect.Signature.empty))


def write_npz(path, store):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, arr in store.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def grid_of(shape):
    return {"area": [shape[0] - 1, 0, 0, shape[1] - 1], "grid": [1, 1]}


class FieldShapedPatterns(ref_patterns.Patterns):
    """Patterns that depend on the field: every evaluated pattern has the field's full shape."""

    def __init__(self, labels, grid, evaluated):
        super().__init__(labels, grid, np)
        self._evaluated = evaluated

    def patterns(self):
        return dict(zip(self._labels, self._evaluated))


class Recorder:
    def __init__(self):
        self.store, self.manifest, self.seen = {}, [], {}

    def put(self, v):
        v = np.asarray(v)
        key = (v.dtype.str, v.shape, v.tobytes())
        if key not in self.seen:
            self.seen[key] = f"a{len(self.seen):04d}"
            self.store[self.seen[key]] = v
        return self.seen[key]

    def entry(self, func, note, arrays, plain):
        e = dict(id=f"c{len(self.manifest):04d}", func=func, note=note, arrays={k: self.put(v) for k, v in arrays.items()},
                 plain=plain, out=None, raises=None)
        self.manifest.append(e)
        return e

    def add_project(self, note, kind, field, stack, weights, labels, pshape, modulator=None):
        """kind: constant (stack: [P, *pshape]), modulated (stack: the base patterns; modulator: one value per field),
        perfield (stack: [P, *field.shape])."""
        arrays = dict(field=field, patterns=stack)
        if weights is not None:
            arrays["weights"] = weights
        if modulator is not None:
            arrays["modulator"] = modulator
        e = self.entry("project", note, arrays, dict(kind=kind, labels=list(labels), pshape=list(pshape)))
        before = field.copy()
        try:
            grid, extra = grid_of(pshape), {}
            if kind == "constant":
                pats = ref_patterns.ConstantPatterns(labels, grid, stack)
            elif kind == "modulated":
                pats, extra = ref_patterns.ModulatedPatterns(labels, grid, stack, lambda step: step), dict(step=modulator)
            else:
                pats = FieldShapedPatterns(labels, grid, stack)
            out = ref_index.project(field, pats, weights, **extra)
            assert list(out) == list(labels)
            e["out"] = {label: self.put(np.asarray(v)) for label, v in out.items()}
        except Exception as exc:  # the error convention is part of the record
            e["raises"] = [type(exc).__name__, str(exc)]
        assert before.tobytes() == field.tobytes(), "the reference modified its input"

    def add_index(self, note, proj, mean, std):
        arrays, plain = {}, dict(labels=list(proj), mean={}, std={})
        for label in proj:
            arrays["proj_" + label] = proj[label]
            for name, d in (("mean", mean), ("std", std)):
                if isinstance(d[label], np.ndarray):
                    arrays[f"{name}_{label}"] = d[label]
                else:
                    plain[name][label] = d[label]
        e = self.entry("regime_index", note, arrays, plain)
        out = ref_index.regime_index(proj, mean, std)
        e["out"] = {label: self.put(np.asarray(v)) for label, v in out.items()}

    def add_pearson(self, note, x, y, axis, r=None):
        e = self.entry("pearson_correlation", note, dict(x=x, y=y), dict(axis=axis, r=r))
        bx, by = x.copy(), y.copy()
        try:
            e["out"] = self.put(np.asarray(ref_score.pearson_correlation(x, y, axis=axis)))
        except Exception as exc:
            e["raises"] = [type(exc).__name__, str(exc)]
        assert bx.tobytes() == x.tobytes() and by.tobytes() == y.tobytes(), "the reference modified its input"


KSHAPES = [(1, 1), (7, 9), (1, 64), (5, 13), (16, 16), (1, 257), (25, 41)]
NSHAPES = [(), (1,), (5,), (2, 3, 4)]
PS = [1, 3, 8, 9]
COMBOS = [("f32", F32, F32, F32), ("f32 fields f64 patterns", F32, F64, F32), ("f64", F64, F64, F64)]


def weights_of(pshape, which, dt):
    if which == "uniform":
        return np.ones(pshape, dt)
    lat = np.linspace(30.0, 80.0, pshape[0])
    return (np.cos(np.deg2rad(lat))[:, None] * np.ones(pshape[1])).astype(dt)


def fields_of(rng, nshape, pshape, dt):
    """Geopotential-height anomalies: a smooth part shared by the batch plus noise, in metres."""
    k = int(np.prod(pshape))
    base = 80.0 * np.sin(np.linspace(0.0, 3.0, k)).reshape(pshape)
    return (base + rng.normal(0.0, 60.0, tuple(nshape) + tuple(pshape))).astype(dt)


def labels_of(p):
    return [f"R{i}" for i in range(p)]


def project_cases(rec, rng):
    n = 0
    for i, pshape in enumerate(KSHAPES):
        for j, nshape in enumerate(NSHAPES):
            k, nf = int(np.prod(pshape)), int(np.prod(nshape))
            if nf * k > 5200 or (len(nshape) == 3 and k > 65):
                continue
            p = PS[(i + j) % 4] if k <= 300 else PS[(i + j) % 2]  # (25,41): 1 or 3 patterns
            name, fdt, pdt, wdt = COMBOS[(i + 2 * j) % 3]
            wkind = ("uniform", "coslat")[n % 2]
            n += 1
            rec.add_project(f"constant {pshape} fields {nshape} P {p} {name} {wkind}", "constant", fields_of(rng, nshape, pshape, fdt),
                            rng.normal(0.0, 1.0, (p,) + pshape).astype(pdt), weights_of(pshape, wkind, wdt), labels_of(p), pshape)
    big = (91, 121)
    rec.add_project(f"constant {big} fields (1,) P 1 f32 coslat", "constant", fields_of(rng, (1,), big, F32),
                    rng.normal(0.0, 1.0, (1,) + big).astype(F32), weights_of(big, "coslat", F32), labels_of(1), big)
    # ModulatedPatterns: one modulator value per field
    for pshape, nshape, p, fdt, mdt, wkind in (((5, 13), (5,), 3, F32, F32, "coslat"), ((7, 9), (2, 3, 4), 9, F32, F64, "uniform"),
                                               ((16, 16), (1,), 8, F64, F64, "coslat"), ((5, 13), (), 3, F64, F64, "uniform")):
        mod = (1.0 + 0.3 * rng.normal(0.0, 1.0, nshape)).astype(mdt)
        rec.add_project(f"modulated {pshape} fields {nshape} P {p} {np.dtype(fdt).name} modulator {np.dtype(mdt).name} {wkind}", "modulated",
                        fields_of(rng, nshape, pshape, fdt), rng.normal(0.0, 1.0, (p,) + pshape).astype(fdt),
                        weights_of(pshape, wkind, fdt), labels_of(p), pshape, modulator=mod)
    # patterns of the field's full shape
    for pshape, nshape, p, dt in (((5, 13), (5,), 3, F32), ((7, 9), (2, 3, 4), 1, F64), ((1, 257), (2,), 2, F64)):
        rec.add_project(f"perfield {pshape} fields {nshape} P {p} {np.dtype(dt).name}", "perfield", fields_of(rng, nshape, pshape, dt),
                        rng.normal(0.0, 1.0, (p,) + nshape + pshape).astype(dt), weights_of(pshape, "coslat", dt), labels_of(p), pshape)
    # special values
    for what, value in (("NaN", np.nan), ("inf", np.inf)):
        for dt in (F32, F64):
            f = fields_of(rng, (5,), (5, 13), dt)
            f[2, 1, 7] = value
            rec.add_project(f"a field with {what} {np.dtype(dt).name}", "constant", f, rng.normal(0.0, 1.0, (3, 5, 13)).astype(dt),
                            weights_of((5, 13), "coslat", dt), labels_of(3), (5, 13))
    # the error cases, in the reference's order of checks
    f, pat, w = fields_of(rng, (5,), (5, 13), F64), rng.normal(0.0, 1.0, (3, 5, 13)), weights_of((5, 13), "uniform", F64)
    rec.add_project("error field shape", "constant", f[:, :, :12].copy(), pat, w, labels_of(3), (5, 13))
    rec.add_project("error field has too few axes", "constant", f[0, 0].copy(), pat, w, labels_of(3), (5, 13))
    rec.add_project("error weights None", "constant", f, pat, None, labels_of(3), (5, 13))
    rec.add_project("error weights shape", "constant", f, pat, w[:, :12].copy(), labels_of(3), (5, 13))
    rec.add_project("error field shape before weights shape", "constant", f[:, :4].copy(), pat, w[:, :12].copy(), labels_of(3), (5, 13))


def index_cases(rec, rng):
    for dt in (F32, F64):
        tag = np.dtype(dt).name
        proj = {"NAO+": rng.normal(5.0, 20.0, (5,)).astype(dt), "BL": rng.normal(-3.0, 20.0, (2, 3)).astype(dt)}
        rec.add_index(f"{tag} scalar mean and std", proj, {"NAO+": 4.5, "BL": -2}, {"NAO+": 18.25, "BL": 0.1})
        mean = {k: rng.normal(0.0, 3.0, v.shape).astype(dt) for k, v in proj.items()}
        std = {k: (15.0 + rng.uniform(0.0, 10.0, v.shape)).astype(dt) for k, v in proj.items()}
        rec.add_index(f"{tag} array mean and std", proj, mean, std)
        std0 = {k: v.copy() for k, v in std.items()}
        std0["NAO+"][1], std0["BL"][1, 2] = 0.0, 0.0
        mean0 = {k: v.copy() for k, v in mean.items()}
        mean0["NAO+"][1] = proj["NAO+"][1]  # 0 / 0
        rec.add_index(f"{tag} std of 0", proj, mean0, std0)
        rec.add_index(f"{tag} scalar mean array std", proj, {"NAO+": 0.1, "BL": 0.0}, std)
        rec.add_index(f"{tag} scalar std of 0", proj, mean, {"NAO+": 0.0, "BL": 3})
    proj = {"AR": rng.normal(5.0, 20.0, (7,)).astype(F32)}
    rec.add_index("f32 projection f64 arrays", proj, {"AR": rng.normal(0.0, 3.0, 7)}, {"AR": 15.0 + rng.uniform(0.0, 10.0, 7)})
    rec.add_index("f32 projection f64 mean scalar std", proj, {"AR": rng.normal(0.0, 3.0, 7)}, {"AR": 2.5})


def sample_of(rng, shape, kind, dt):
    if kind == "temperature":
        return (280.0 + rng.normal(0.0, 5.0, shape)).astype(dt)
    return rng.normal(0.0, 1.0, shape).astype(dt)


def pearson_cases(rec, rng):
    n = 0

    def add(shape, axis, dt):
        nonlocal n
        kind = ("temperature", "anomaly")[n % 2]
        n += 1
        x = sample_of(rng, shape, kind, dt)
        y = (0.6 * (x - x.mean()) + sample_of(rng, shape, kind, F64)).astype(dt)
        rec.add_pearson(f"{np.dtype(dt).name} {shape} axis {axis} {kind}", x, y, axis)

    for dt in (F32, F64):
        first = [(1, 2), (1, 65), (2, 2), (2, 64), (3, 63), (3, 65), (9, 65), (9, 2), (51, 2), (257, 2)]
        if dt is F32:
            first += [(3, 1000), (51, 63)]
        for shape in first:
            add(shape, 0, dt)
        for m in (1, 2, 3, 9, 51, 257):
            add((3, m), -1 if m % 2 else 1, dt)
        add((9, 1), 0, dt)
        for m, inner in ((2, 2), (9, 63), (51, 2), (3, 64)):
            add((3, m, inner), 1, dt)
        add((3, 4, 9), 2, dt)
        add((2, 2, 257), -1, dt)
        add((9, 5, 13), 0, dt)
        add((9, 5, 13), -3, dt)
        # x and y from two fixed vectors with a prescribed correlation, one per column
        u = np.array([1.0, -2.0, 0.5, 3.0, -1.5, 0.25, -0.75, 2.5, -3.0])
        v = np.array([2.0, 1.0, -1.0, 0.5, 3.0, -2.5, -0.5, -1.5, -1.0])
        u, v = u - u.mean(), v - v.mean()
        v = v - u * (u @ v) / (u @ u)
        u, v = u / np.linalg.norm(u), v / np.linalg.norm(v)
        rs = [1.0, -1.0, 0.0, 0.42, -0.13]
        x = np.stack([280.0 + 5.0 * u for _ in rs], axis=1)
        y = np.stack([3.0 + 2.0 * (r * u + np.sqrt(1.0 - r * r) * v) for r in rs], axis=1)
        rec.add_pearson(f"{np.dtype(dt).name} prescribed r axis 0", x.astype(dt), y.astype(dt), 0, r=rs)
        rec.add_pearson(f"{np.dtype(dt).name} prescribed r axis -1", np.ascontiguousarray(x.T).astype(dt),
                        np.ascontiguousarray(y.T).astype(dt), -1, r=rs)
        # special columns
        x, y = sample_of(rng, (9, 6), "temperature", dt), sample_of(rng, (9, 6), "anomaly", dt)
        x[:, 1] = dt(281.5)          # a constant column: 0 / 0
        y[:, 2] = dt(0.0)
        x[4, 3] = np.nan             # a NaN member
        y[0, 4] = np.inf
        rec.add_pearson(f"{np.dtype(dt).name} special columns axis 0", x, y, 0)
        rec.add_pearson(f"{np.dtype(dt).name} special columns axis -1", np.ascontiguousarray(x.T), np.ascontiguousarray(y.T), -1)
    xi = np.round(sample_of(rng, (9, 6), "temperature", F64)).astype(np.int64)
    yi = np.round(10 * sample_of(rng, (9, 6), "anomaly", F64)).astype(np.int32)
    rec.add_pearson("integer input axis 0", xi, yi, 0)
    rec.add_pearson("error shapes differ", np.zeros((9, 6)), np.zeros((9, 5)), 0)
    rec.add_pearson("error axis out of range", np.zeros((9, 6)), np.zeros((9, 6)), 2)


def main():
    rec = Recorder()
    rng = np.random.default_rng(20261019)
    project_cases(rec, rng)
    index_cases(rec, rng)
    pearson_cases(rec, rng)
    sigs = {"project": bare_signature(ref_index.project), "regime_index": bare_signature(ref_index.regime_index),
            "pearson_correlation": bare_signature(ref_score.pearson_correlation),
            "Patterns": bare_signature(ref_patterns.Patterns.__init__),
            "ConstantPatterns": bare_signature(ref_patterns.ConstantPatterns.__init__),
            "ModulatedPatterns": bare_signature(ref_patterns.ModulatedPatterns.__init__)}
    meta = dict(cases=rec.manifest, numpy=np.__version__, signatures=sigs)
    rec.store["manifest"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "regimes_golden.npz")
    write_npz(path, rec.store)
    print(len(rec.manifest), "cases,", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
