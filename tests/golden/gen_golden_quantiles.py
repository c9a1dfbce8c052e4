#!/usr/bin/env python3
"""Golden vectors for stats.iter_quantiles, recorded from the REFERENCE (build container only; stand-ins for the
un-vendored packages in tests/golden/_standin, as in gen_golden_ensemble.py).  `earthkit.meteo.stats` is loaded by file
path (stats/array/quantiles.py), so nothing else of the package is imported.

Writes tests/golden/quantiles_golden.npz: for every case the arguments of one call and the rows the reference yielded,
stacked (or the name and text of the exception it raised), a JSON manifest with the NumPy version that computed them and
the recorded signature string.  Data only; arrays are stored once and shared between cases; the file regenerates byte
for byte.

Cases (24 points each unless an axis case): f32 and f64, the three methods, m in {1, 2, 7, 8, 9, 51, 128} plus 256 for
f32, `which` in {0, 1, 4, 100, [0.1, 0.5, 1.0], [0.9, 0.0, 0.33], []}, tie-heavy and smooth data; special columns
(all-equal, a NaN member, +inf on top, -inf at the bottom, both, two +inf on top so that a level with x == 0 meets one);
axes 0, 1, 2 and -1 of a (4, 7, 5) array; integer input; the error cases.  No column mixes -0.0 and +0.0 (NumPy's sort
does not define their order).  Integer input is recorded for "sort" and "numpy_bulk" only: with "numpy" the reference
casts every level to the integer dtype (0 or 1), which the product does not imitate.
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

NPTS = 24
F32, F64 = np.float32, np.float64
METHODS = ("sort", "numpy_bulk", "numpy")
WHICH = (0, 1, 4, 100, [0.1, 0.5, 1.0], [0.9, 0.0, 0.33], [])


def load_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = load_path("_ref_stats_quantiles", os.path.join(REF, "src", "earthkit", "meteo", "stats", "array", "quantiles.py"))


def bare_signature(fn):
    sig = inspect.signature(fn)
    params = [p.replace(annotation=inspect.Parameter.empty) for p in sig.parameters.values()]
    return str(sig.replace(parameters=params, return_annotation=inspect.Signature.empty))


class Recorder:
    def __init__(self):
        self.store, self.manifest, self.seen = {}, [], {}

    def put(self, v):
        key = (v.dtype.str, v.shape, v.tobytes())
        if key not in self.seen:
            self.seen[key] = f"a{len(self.seen):04d}"
            self.store[self.seen[key]] = v
        return self.seen[key]

    def add(self, note, arr, deviation=None, **plain):
        entry = dict(id=f"c{len(self.manifest):04d}", func="iter_quantiles", note=note, arrays=dict(arr=self.put(arr)),
                     plain=plain, out=None, rows=None, raises=None)
        before = arr.copy()
        try:
            rows = [np.asarray(r) for r in ref.iter_quantiles(arr, **plain)]
            entry["rows"] = len(rows)
            if rows:
                entry["out"] = self.put(np.stack(rows))
        except Exception as exc:  # the error convention is part of the record
            entry["raises"] = [type(exc).__name__, str(exc)]
        assert before.tobytes() == arr.tobytes(), "the reference modified its input"
        if deviation:
            entry["deviation"] = deviation
        self.manifest.append(entry)


def write_npz(path, store):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, arr in store.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def precip(rng, rows, npts, dt):
    """gen_golden_ensemble.precip: gamma-distributed, clamped at zero (many ties), rounded to 1/8."""
    a = np.maximum(rng.gamma(1.5, 2.0, (rows, npts)) - 1.5, 0.0)
    return (np.round(a * 8) / 8).astype(dt)


def smooth(rng, rows, npts, dt):
    return (280.0 + 12.0 * rng.normal(0, 1, (rows, npts))).astype(dt)


def special(rng, m, dt):
    a = smooth(rng, m, NPTS, dt)
    a[:, 0:2] = dt(3.25)                       # all-equal columns
    a[m // 2, 2:4] = np.nan                    # a NaN member
    a[m // 3, 4] = np.inf                      # +inf on top
    a[m // 3, 5] = -np.inf                     # -inf at the bottom
    a[0, 6], a[m - 1, 6] = np.inf, -np.inf     # both
    a[1, 7], a[m - 2, 7] = np.inf, np.inf      # two on top: a level with x == 0 has one as its upper neighbour
    a[0, 8], a[m - 1, 8] = -np.inf, -np.inf
    a[:, 9] = np.inf                           # all-equal and infinite
    return a


def value_cases(rec, rng):
    for dt, tag in ((F64, "f64"), (F32, "f32")):
        for m in (1, 2, 7, 8, 9, 51, 128) + ((256,) if dt is F32 else ()):
            for kind, make in (("ties", precip), ("smooth", smooth)):
                arr = make(rng, m, NPTS, dt)
                for method in METHODS:
                    for which in WHICH:
                        rec.add(f"{tag} m {m} {kind} {method} which {which}", arr, which=which, method=method)
        for m in (9, 51):
            arr = special(rng, m, dt)
            for method in METHODS:
                for which in WHICH[:-1]:
                    rec.add(f"{tag} m {m} special {method} which {which}", arr, which=which, method=method)
        cube = smooth(rng, 4, 35, dt).reshape(4, 7, 5)
        cube[1, 2, 3] = np.nan
        for axis in (0, 1, 2, -1):
            for method in METHODS:
                for which in (4, [0.9, 0.0, 0.33]):
                    rec.add(f"{tag} cube axis {axis} {method} which {which}", cube, which=which, axis=axis, method=method)
        rec.add(f"{tag} defaults", precip(rng, 7, NPTS, dt))
    ints = np.round(smooth(rng, 7, NPTS, F64)).astype(np.int64)
    for method in ("sort", "numpy_bulk"):
        for which in (4, [0.9, 0.0, 0.33]):
            rec.add(f"integer input {method} which {which}", ints, which=which, method=method)


def error_cases(rec, rng):
    arr = smooth(rng, 7, NPTS, F64)
    rec.add("unknown method", arr, method="bogus")
    rec.add("unknown method, levels out of range too", arr, which=[2.0], method="median")
    sort_dev = "the product raises ValueError('Quantiles must be in the range [0, 1]') in every method"
    for levels, what in (([0.5, 1.5], "above 1"), ([-0.25, 0.5], "below 0"), ([0.5, float("nan")], "nan")):
        for method in METHODS:
            rec.add(f"level {what} {method}", arr, which=levels, method=method,
                    deviation=sort_dev if method == "sort" else None)


def main():
    rec = Recorder()
    rng = np.random.default_rng(20261018)
    value_cases(rec, rng)
    error_cases(rec, rng)
    meta = dict(cases=rec.manifest, numpy=np.__version__, signatures={"iter_quantiles": bare_signature(ref.iter_quantiles)})
    rec.store["manifest"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "quantiles_golden.npz")
    write_npz(path, rec.store)
    print(len(rec.manifest), "cases,", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
