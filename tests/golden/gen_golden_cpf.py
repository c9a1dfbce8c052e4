#!/usr/bin/env python3
"""Golden vectors for the Crossing Point Forecast (extreme.cpf), recorded from the REFERENCE (build container only;
stand-ins for the un-vendored packages in tests/golden/_standin, as in gen_golden_ensemble.py).

Writes tests/golden/cpf_golden.npz: for every case the arguments of one call and the float32 array the reference
returned, a JSON manifest, the recorded signature string and the data and known answers of the reference's own tests
(tests/extreme/_cpf.py), stored as data.  Arrays are stored once and shared between cases; the file regenerates byte
for byte.
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

from earthkit.meteo.extreme import array as ref_extreme  # noqa: E402

warnings.simplefilter("ignore")
np.seterr(all="ignore")

NPTS = 24
F32, F64 = np.float32, np.float64
SHAPES = ((101, 51), (101, 50), (11, 7), (3, 1), (3, 2), (5, 3), (101, 3), (11, 128))


def load_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


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

    def add(self, note, known=None, **kwargs):
        entry = dict(id=f"c{len(self.manifest):04d}", note=note, arrays={}, plain={}, out=None)
        call = {}
        for k, v in kwargs.items():
            if isinstance(v, (bool, int, float)):
                entry["plain"][k] = v
                call[k] = v
            else:
                v = np.asarray(v)
                entry["arrays"][k] = self.put(v)
                call[k] = v.copy()
        out = np.asarray(ref_extreme.cpf(**call))
        assert out.dtype == F32 and out.shape == (kwargs["clim"].shape[1],)
        for k, key in entry["arrays"].items():  # the reference leaves its inputs alone
            assert np.array_equal(call[k], self.store[key], equal_nan=True)
        entry["out"] = self.put(out)
        if known is not None:
            entry["known"] = self.put(np.asarray(known, F32))
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


def gamma_fields(rng, nclim, nens, dt):
    """Zero-clamped gamma (many ties), rounded to 1/8 so that members meet climate rows exactly; the forecast is scaled
    per point so that some columns lie below and some above their climate."""
    clim = np.round(np.maximum(rng.gamma(1.5, 2.0, (nclim, NPTS)) - 1.5, 0.0) * 8) / 8
    ens = np.round(np.maximum(rng.gamma(1.5, 2.0, (nens, NPTS)) * rng.uniform(0.3, 2.5, NPTS) - 1.5, 0.0) * 8) / 8
    return np.sort(clim, axis=0).astype(dt), ens.astype(dt)


def normal_fields(rng, nclim, nens, dt):
    """Normal climate, rounded to 1/16; the forecast is narrower and shifted per point (adding 0.0 turns -0.0 into 0.0)."""
    clim = np.round(rng.normal(0, 3, (nclim, NPTS)) * 16) / 16 + 0.0
    ens = np.round((rng.normal(0, 1.5, (nens, NPTS)) + rng.normal(0, 3, NPTS)) * 16) / 16 + 0.0
    return np.sort(clim, axis=0).astype(dt), ens.astype(dt)


def shuffled(rng, a):
    return np.stack([rng.permutation(a[:, j]) for j in range(a.shape[1])], axis=1)


def option_cases(rec, rng, head, clim, ens):
    """clim arrives sorted, ens unsorted."""
    rec.add(f"{head} default", clim=clim, ens=ens)
    rec.add(f"{head} from_zero", clim=clim, ens=ens, from_zero=True)
    rec.add(f"{head} symmetric", clim=clim, ens=ens, symmetric=True)
    rec.add(f"{head} symmetric from_zero", clim=clim, ens=ens, symmetric=True, from_zero=True)
    rec.add(f"{head} epsilon 0.5", clim=clim, ens=ens, epsilon=0.5)
    rec.add(f"{head} epsilon 0.5 symmetric", clim=clim, ens=ens, epsilon=0.5, symmetric=True)  # epsilon is ignored
    mixed_up = shuffled(rng, clim)
    rec.add(f"{head} sorts off presorted", clim=clim, ens=np.sort(ens, axis=0), sort_clim=False, sort_ens=False)
    rec.add(f"{head} sorts off unsorted", clim=mixed_up, ens=ens, sort_clim=False, sort_ens=False)
    rec.add(f"{head} sorts off unsorted symmetric from_zero", clim=mixed_up, ens=ens, sort_clim=False,
            sort_ens=False, symmetric=True, from_zero=True)
    rec.add(f"{head} sorts off unsorted epsilon 0.5", clim=mixed_up, ens=ens, sort_clim=False, sort_ens=False, epsilon=0.5)
    rec.add(f"{head} sort_clim off", clim=clim, ens=ens, sort_clim=False, from_zero=True)
    rec.add(f"{head} sort_ens off", clim=mixed_up, ens=ens, sort_ens=False, from_zero=True)


def shape_cases(rec, rng):
    for dt, tag in ((F64, "f64"), (F32, "f32")):
        for nclim, nens in SHAPES:
            for kind, make in (("gamma", gamma_fields), ("normal", normal_fields)):
                clim, ens = make(rng, nclim, nens, dt)
                option_cases(rec, rng, f"{tag} {nclim}x{nens} {kind}", clim, ens)


def special_cases(rec, rng):
    for dt, tag in ((F64, "f64"), (F32, "f32")):
        for nclim, nens in ((101, 51), (11, 7)):
            clim, ens = normal_fields(rng, nclim, nens, dt)
            sp_c, sp_e = clim.copy(), ens.copy()
            sp_c[:, 0:2], sp_e[:, 0:2] = dt(3.25), dt(3.25)      # all-equal columns, climate = ensemble
            sp_c[:, 2] = dt(0)                                     # all-equal climate of zeros
            sp_e[:, 3] = np.linspace(sp_c[0, 3], sp_c[-1, 3], nens).astype(dt)
            sp_c[:, 20], sp_e[:, 20] = np.arange(nclim, dtype=dt), np.arange(nens, dtype=dt) * dt((nclim - 1) / nens)
            sp_c[:, 4:8] += dt(1000)                               # climate entirely above the ensemble
            sp_c[:, 8:12] -= dt(1000)                              # entirely below
            sp_c[nclim // 2, 12:14] = np.nan                       # NaN in one climate row
            sp_e[nens // 2, 14:16] = np.nan                        # NaN in one member
            sp_e[0, 16], sp_e[nens - 1, 17] = np.inf, -np.inf      # infinite members
            sp_c[0, 18], sp_c[-1, 18], sp_c[-1, 19] = -np.inf, np.inf, np.inf
            sp_e[1, 21], sp_e[2, 21], sp_c[0, 21] = np.inf, -np.inf, -np.inf
            head = f"{tag} {nclim}x{nens} equal above below nan inf"
            for kw in ({}, dict(from_zero=True), dict(symmetric=True), dict(symmetric=True, from_zero=True), dict(epsilon=0.5),
                       dict(sort_clim=False, sort_ens=False, from_zero=True),
                       dict(sort_clim=False, sort_ens=False, symmetric=True)):
                rec.add(f"{head} {' '.join(f'{k}={v}' for k, v in kw.items()) or 'default'}", clim=sp_c, ens=sp_e, **kw)
            # a NaN in every column, at a row of its own
            n_c, n_e = clim.copy(), ens.copy()
            n_c[rng.integers(0, nclim, NPTS // 2), np.arange(NPTS // 2)] = np.nan
            n_e[rng.integers(0, nens, NPTS // 2), np.arange(NPTS // 2, NPTS)] = np.nan
            for kw in ({}, dict(from_zero=True), dict(symmetric=True, from_zero=True)):
                rec.add(f"{tag} {nclim}x{nens} nan everywhere {' '.join(kw) or 'default'}", clim=n_c, ens=n_e, **kw)


def reference_data_cases(rec):
    d = load_path("_ref_cpf_data", os.path.join(REF, "tests", "extreme", "_cpf.py"))
    table = (("data", d.cpf_clim, d.cpf_ens, dict(sort_clim=True), d.cpf_val),
             ("data2 epsilon", d.cpf_clim2, d.cpf_ens2, dict(sort_clim=True, epsilon=0.5), d.cpf_val2),
             ("data3 symmetric", d.cpf_clim3, d.cpf_ens3, dict(sort_clim=True, symmetric=True), d.cpf_val3),
             ("data from_zero", d.cpf_clim, d.cpf_ens, dict(sort_clim=True, from_zero=True), d.cpf_val_fromzero))
    for dt, tag in ((F32, "f32"), (F64, "f64")):
        for name, clim, ens, kw, val in table:
            rec.add(f"{tag} reference {name}", known=val, clim=np.asarray(clim, dt), ens=np.asarray(ens, dt), **kw)


def mixed_cases(rec, rng):
    clim, ens = normal_fields(rng, 101, 51, F64)
    # off the 1/16 grid, so that the rounding of a climate-row difference to f32 shows
    clim = np.sort(clim + rng.uniform(0, 0.01, clim.shape), axis=0)
    ens = ens + rng.uniform(0, 0.01, ens.shape)
    for kw in ({}, dict(from_zero=True), dict(symmetric=True, from_zero=True), dict(epsilon=0.5)):
        name = " ".join(kw) or "default"
        rec.add(f"mixed clim f32 ens f64 {name}", clim=clim.astype(F32), ens=ens, **kw)
        rec.add(f"mixed clim f64 ens f32 {name}", clim=clim, ens=ens.astype(F32), **kw)
    rec.add("integer ens", clim=clim, ens=np.round(ens).astype(np.int64), from_zero=True)


def main():
    rec = Recorder()
    rng = np.random.default_rng(20261018)
    reference_data_cases(rec)
    shape_cases(rec, rng)
    special_cases(rec, rng)
    mixed_cases(rec, rng)
    meta = dict(cases=rec.manifest, signature=bare_signature(ref_extreme.cpf))
    rec.store["manifest"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "cpf_golden.npz")
    write_npz(path, rec.store)
    print(len(rec.manifest), "cases,", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
