#!/usr/bin/env python3
"""Golden vectors for stats.nanaverage, recorded from the REFERENCE (build container only; stand-ins for the un-vendored
packages in tests/golden/_standin, as in gen_golden_regimes.py).  The reference's stats/array/numpy_extended.py is loaded
by file path, so nothing else of the package is imported.

Writes tests/golden/nanaverage_golden.npz: data only; arrays are stored once and shared between cases; a JSON manifest
with the NumPy version that computed them and the recorded signature string; the file regenerates byte for byte.

Cases: f32 and f64, integer data, f32 data with f64 weights; axes 0, 1, 2 and -1 of 2-D and 3-D arrays, axis=None, the
tuples (0, 1), (-2, -1) and (0, 2), a tuple with weights, keepdims; no weights, a scalar, a vector along the axis, a full
array, [m, 1] against [outer, m, inner], cos-latitude; a NaN weight, weights summing to 0, weights of mixed sign; 10 % NaN
at random, one all-NaN column, an all-NaN array, a column of -0.0; +-inf; sample counts 1, 2, 3, 9, 51, 257 (and 0); the
error cases with the reference's exception type, and the product's own where it deviates (`product_raises`).
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


ref = load_path("_ref_numpy_extended", os.path.join(REF, "src", "earthkit", "meteo", "stats", "array", "numpy_extended.py"))


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

    def add(self, note, data, weights=None, product_raises=None, **kwargs):
        """kwargs: what the call passes besides data and weights.  A tuple axis is stored as a list (`axis_is_tuple`)."""
        arrays = dict(data=data)
        if weights is not None:
            arrays["weights"] = np.asarray(weights)
        plain = {k: (list(v) if isinstance(v, tuple) else v) for k, v in kwargs.items()}
        e = dict(id=f"c{len(self.manifest):04d}", func="nanaverage", note=note, arrays={k: self.put(v) for k, v in arrays.items()},
                 plain=dict(kwargs=plain, axis_is_tuple=isinstance(kwargs.get("axis"), tuple)), out=None, raises=None,
                 product_raises=product_raises)
        self.manifest.append(e)
        before = data.copy()
        try:
            e["out"] = self.put(np.asarray(ref.nanaverage(data, weights, **{k: (np.dtype(v) if k == "dtype" else v) for k, v in kwargs.items()})))
        except Exception as exc:  # the error convention is part of the record
            e["raises"] = [type(exc).__name__, str(exc)]
            if product_raises is None:
                e["product_raises"] = type(exc).__name__
        assert before.tobytes() == data.tobytes(), "the reference modified its input"


def temperature(rng, shape, dt, nan=0.1):
    x = (280.0 + rng.normal(0.0, 5.0, shape)).astype(dt)
    if nan:
        x[rng.uniform(size=shape) < nan] = np.nan
    return x


def coslat(n, dt):
    return np.cos(np.deg2rad(np.linspace(-80.0, 80.0, n))).astype(dt)


def cases(rec, rng):
    for dt in (F32, F64):
        tag = np.dtype(dt).name
        # sample counts on both layouts: [m, 5] along axis 0 (lane per point), [5, m] along the contiguous axis
        for m in (1, 2, 3, 9, 51, 257):
            x = temperature(rng, (m, 5), dt)
            xt = np.ascontiguousarray(x.T)
            w = (0.5 + rng.uniform(0.0, 1.0, m)).astype(dt)
            rec.add(f"{tag} ({m}, 5) axis 0", x, axis=0)
            rec.add(f"{tag} (5, {m}) axis -1", xt, axis=-1)
            rec.add(f"{tag} ({m}, 5) axis 0 weights [m, 1]", x, w[:, None], axis=0)
            rec.add(f"{tag} (5, {m}) axis 1 weights vector", xt, w, axis=1)
        # a 3-D array: every axis, None, tuples, keepdims, every kind of weights
        x = temperature(rng, (3, 9, 7), dt)
        full = (0.5 + rng.uniform(0.0, 1.0, x.shape)).astype(dt)
        for axis in (0, 1, 2, -1, None):
            rec.add(f"{tag} (3, 9, 7) axis {axis}", x, axis=axis)
            rec.add(f"{tag} (3, 9, 7) axis {axis} full weights", x, full, axis=axis)
            rec.add(f"{tag} (3, 9, 7) axis {axis} scalar weight", x, 2.5, axis=axis)
        rec.add(f"{tag} (3, 9, 7) no keywords", x)
        rec.add(f"{tag} (3, 9, 7) axis 1 keepdims", x, axis=1, keepdims=True)
        rec.add(f"{tag} (3, 9, 7) axis None keepdims weights", x, full, axis=None, keepdims=True)
        rec.add(f"{tag} (3, 9, 7) axis 2 keepdims weights vector", x, coslat(7, dt), axis=2, keepdims=True)
        rec.add(f"{tag} (3, 9, 7) axis (0, 1)", x, axis=(0, 1))
        rec.add(f"{tag} (3, 9, 7) axis (-2, -1)", x, axis=(-2, -1))
        rec.add(f"{tag} (3, 9, 7) axis (-2, -1) keepdims", x, axis=(-2, -1), keepdims=True)
        rec.add(f"{tag} (3, 9, 7) axis (0, 2) not adjacent", x, axis=(0, 2), product_raises="ValueError")
        rec.add(f"{tag} (3, 9, 7) axis 1 cos-latitude [m, 1]", x, coslat(9, dt)[:, None], axis=1)
        rec.add(f"{tag} (3, 9, 7) axis 0 weights [3, 1, 1]", x, np.array([1.0, 2.0, 3.0], dt)[:, None, None], axis=0)
        rec.add(f"{tag} (3, 9, 7) axis 1 weights [3, 1, 7] broadcast along the axis", x, (0.5 + rng.uniform(0, 1, (3, 1, 7))).astype(dt), axis=1)
        rec.add(f"{tag} (3, 9, 7) axis None weights [9, 1] does not collapse", x, coslat(9, dt)[:, None], axis=None)
        # NaN weights, zero weights, weights of mixed sign
        y = temperature(rng, (9, 6), dt)
        yt = np.ascontiguousarray(y.T)
        w = (0.5 + rng.uniform(0.0, 1.0, 9)).astype(dt)
        wn = w.copy()
        wn[3] = np.nan
        rec.add(f"{tag} (9, 6) axis 0 a NaN weight", y, wn[:, None], axis=0)
        rec.add(f"{tag} (6, 9) axis 1 a NaN weight", yt, wn, axis=1)
        mixed = np.array([1.0, -0.5, 2.0, 0.25, -1.0, 1.5, 0.75, -0.25, 1.0], dt)
        rec.add(f"{tag} (9, 6) axis 0 weights of mixed sign", y, mixed[:, None], axis=0)
        rec.add(f"{tag} (6, 9) axis 1 weights of mixed sign", yt, mixed, axis=1)
        clean = temperature(rng, (8, 6), dt, nan=0)
        rec.add(f"{tag} (8, 6) axis 0 weights summing to 0", clean, np.array([1, -1, 2, -2, 0.5, -0.5, 4, -4], dt)[:, None], axis=0)
        rec.add(f"{tag} (9, 6) axis 0 weights all zero", y, np.zeros((9, 1), dt), axis=0)
        rec.add(f"{tag} (6, 9) axis 1 weights all zero", yt, np.zeros(9, dt), axis=1)
        # missing data and special values
        z = temperature(rng, (9, 6), dt)
        z[:, 1] = np.nan            # an all-NaN column
        z[:, 2] = dt(-0.0)          # a column of -0.0
        z[4, 3] = np.inf
        z[2, 4], z[6, 4] = np.inf, -np.inf
        z[0, 5] = -np.inf
        zt = np.ascontiguousarray(z.T)
        rec.add(f"{tag} special columns axis 0", z, axis=0)
        rec.add(f"{tag} special columns axis -1", zt, axis=-1)
        rec.add(f"{tag} special columns axis 0 weights", z, w[:, None], axis=0)
        rec.add(f"{tag} special columns axis -1 weights", zt, w, axis=-1)
        allnan = np.full((4, 5), np.nan, dt)
        rec.add(f"{tag} an all-NaN array axis None", allnan)
        rec.add(f"{tag} an all-NaN array axis None weights", allnan, 1.0)
        rec.add(f"{tag} an all-NaN array axis 0", allnan, axis=0)
        rec.add(f"{tag} an all-NaN array axis 0 weights", allnan, np.ones((4, 1), dt), axis=0)
        # degenerate shapes
        rec.add(f"{tag} m 0 axis 0", np.zeros((0, 5), dt), axis=0)
        rec.add(f"{tag} m 0 axis 0 weights", np.zeros((0, 5), dt), np.zeros((0, 1), dt), axis=0)
        rec.add(f"{tag} m 0 axis 1", np.zeros((5, 0), dt), axis=1)
        rec.add(f"{tag} m 0 axis 1 weights", np.zeros((5, 0), dt), 2.0, axis=1)
        rec.add(f"{tag} an empty result", np.zeros((4, 0), dt), axis=0)
        rec.add(f"{tag} an empty result weights", np.zeros((4, 0), dt), np.ones((4, 1), dt), axis=0)
        rec.add(f"{tag} 0-d data", np.asarray(dt(281.5)))
        rec.add(f"{tag} 1-d data", temperature(rng, (51,), dt), axis=0)
    # integer data; f32 data with f64 weights
    xi = np.round(temperature(rng, (9, 6), F64, nan=0)).astype(np.int64)
    rec.add("integer data axis 0", xi, axis=0)
    rec.add("integer data axis -1", xi, axis=-1)
    rec.add("integer data axis 0 float64 weights", xi, 0.5 + rng.uniform(0.0, 1.0, (9, 1)), axis=0)
    rec.add("integer data axis 1 integer weights", xi.astype(np.int32), np.arange(1, 7), axis=1, product_raises=False)  # the product computes it
    x32 = temperature(rng, (9, 6), F32)
    rec.add("float32 data float64 weights axis 0", x32, 0.5 + rng.uniform(0.0, 1.0, (9, 1)), axis=0)
    rec.add("float32 data float64 weights axis -1", x32, 0.5 + rng.uniform(0.0, 1.0, 6), axis=-1)
    rec.add("float32 data float64 scalar weight axis 0", x32, 2.0, axis=0)
    # the error cases
    e = temperature(rng, (3, 4, 5), F64)
    rec.add("error a tuple of axes with weights", e, np.ones((3, 4, 5)), axis=(0, 1))
    rec.add("error axis out of range", e, axis=3)
    rec.add("error axis out of range weights", e, np.ones(5), axis=-4)
    rec.add("error axis out of range in a tuple", e, axis=(1, 3))
    rec.add("error weights enlarge the shape", e, np.ones((2, 3, 4, 5)), axis=0, product_raises="ValueError")
    rec.add("error weights do not broadcast", e, np.ones(4), axis=0)
    rec.add("error the keyword dtype", e, axis=0, dtype="float32", product_raises="TypeError")
    rec.add("error the keyword initial", e, np.ones(5), axis=0, initial=1.0, product_raises="TypeError")
    rec.add("error a repeated axis in a tuple", e, axis=(1, 1))


def main():
    rec = Recorder()
    rng = np.random.default_rng(20261020)
    cases(rec, rng)
    meta = dict(cases=rec.manifest, numpy=np.__version__, signatures={"nanaverage": bare_signature(ref.nanaverage)})
    rec.store["manifest"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "nanaverage_golden.npz")
    write_npz(path, rec.store)
    print(len(rec.manifest), "cases,", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
