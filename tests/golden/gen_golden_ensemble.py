#!/usr/bin/env python3
"""Golden vectors for the ensemble reductions (efi, sot, sot_func, crps_from_ensemble), recorded from the REFERENCE
(build container only; stand-ins for the un-vendored packages in tests/golden/_standin, as in gen_golden_interp.py).
`earthkit.meteo.score` imports xarray, which is not installed, so score/array/ensemble.py is loaded by file path.

Writes tests/golden/ensemble_golden.npz: for every case the arguments of one call and the array the reference returned
(or the name of the exception it raised), a JSON manifest, the recorded signature strings, the reference's own known
answers (tests/extreme/test_extreme.py) and the EFI coefficient tables as this host's libm computes them.  Data only;
arrays are stored once and shared between cases; the file regenerates byte for byte.
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


def load_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref_score = load_path("_ref_score_ensemble", os.path.join(REF, "src", "earthkit", "meteo", "score", "array", "ensemble.py"))
FUNCS = {"efi": ref_extreme.efi, "sot": ref_extreme.sot, "sot_func": ref_extreme.sot_func,
         "crps_from_ensemble": ref_score.crps_from_ensemble}


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

    def add(self, func, note, known=None, **kwargs):
        entry = dict(id=f"c{len(self.manifest):04d}", func=func, note=note, arrays={}, plain={}, out=None, raises=None)
        call = {}
        for k, v in kwargs.items():
            if isinstance(v, (str, int, float)):
                entry["plain"][k] = v
                call[k] = v
            else:
                v = np.asarray(v)
                entry["arrays"][k] = self.put(v)
                call[k] = v.copy()
        try:
            out = np.asarray(FUNCS[func](**call))
            entry["out"] = self.put(out)
        except Exception as exc:  # the error convention is part of the record
            entry["raises"] = [type(exc).__name__, str(exc)]
        if known is not None:
            entry["known"] = known
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


def precip(rng, rows, npts, dt, sort):
    """Gamma-distributed, clamped at zero (many ties), rounded to 1/8 so that members meet climate rows exactly."""
    a = np.maximum(rng.gamma(1.5, 2.0, (rows, npts)) - 1.5, 0.0)
    a = np.round(a * 8) / 8
    return (np.sort(a, axis=0) if sort else a).astype(dt)


def efi_cases(rec, rng):
    for dt, tag in ((F64, "f64"), (F32, "f32")):
        for nclim, nens in ((101, 51), (101, 50), (11, 7), (2, 1), (101, 128)):
            clim, ens = precip(rng, nclim, NPTS, dt, True), precip(rng, nens, NPTS, dt, False)
            for eps in (-0.1, 0.0, 1e-4, 1.0):
                rec.add("efi", f"{tag} {nclim}x{nens} eps {eps}", clim=clim, ens=ens, eps=eps)
        for nclim, nens in ((101, 51), (11, 7)):
            clim, ens = precip(rng, nclim, NPTS, dt, True), precip(rng, nens, NPTS, dt, False)
            unsorted = np.stack([rng.permutation(clim[:, j]) for j in range(NPTS)], axis=1)
            sp_c, sp_e = clim.copy(), ens.copy()
            sp_c[:, 0:2], sp_e[:, 0:2] = dt(3.25), dt(3.25)      # all-equal columns, climate = ensemble
            sp_c[:, 2:4] = dt(0)                                   # all-equal climate of zeros
            sp_c[:, 4:8] += dt(1000)                               # climate entirely above the ensemble
            sp_c[:, 8:12] -= dt(1000)                              # entirely below
            sp_c[nclim // 2, 12:14] = np.nan                       # NaN in one climate row
            sp_e[nens // 2, 14:16] = np.nan                        # NaN in one member
            sp_e[0, 16], sp_e[nens - 1, 17] = np.inf, -np.inf      # infinite members
            sp_c[0, 18], sp_c[-1, 18], sp_c[-1, 19] = -np.inf, np.inf, np.inf
            for eps in (-0.1, 1e-4):
                rec.add("efi", f"{tag} {nclim}x{nens} unsorted clim eps {eps}", clim=unsorted, ens=ens, eps=eps)
                rec.add("efi", f"{tag} {nclim}x{nens} equal above below nan inf eps {eps}", clim=sp_c, ens=sp_e, eps=eps)
    # mixed dtypes (computed in f64 by the product): only "clim f32, ens f64" differs from the reference, within a bound
    clim, ens = precip(rng, 101, NPTS, F64, True), precip(rng, 51, NPTS, F64, False) + rng.uniform(0, 0.01, (51, NPTS))
    for eps in (-0.1, 0.0):
        rec.add("efi", f"mixed clim f32 ens f64 eps {eps}", clim=clim.astype(F32), ens=ens, eps=eps)
        rec.add("efi", f"mixed clim f64 ens f32 eps {eps}", clim=clim, ens=ens.astype(F32), eps=eps)
    rec.add("efi", "integer ens", clim=clim, ens=np.round(ens).astype(np.int64))


def reference_data_cases(rec):
    d = load_path("_ref_extreme_data", os.path.join(REF, "tests", "extreme", "_data.py"))
    for dt, tag in ((F64, "f64"), (F32, "f32")):
        c, e = np.asarray(d.clim, dt), np.asarray(d.ens, dt)
        rec.add("efi", f"{tag} reference data", known=-0.1838425040642013, clim=c, ens=e)
        rec.add("efi", f"{tag} reference data eps 1e-4", known=-0.18384250406420133, clim=c, ens=e, eps=1e-4)
        rec.add("efi", f"{tag} reference data eps", known=0.46039347745967046, clim=np.asarray(d.clim_eps, dt),
                ens=np.asarray(d.ens_eps, dt), eps=1e-4)
        rec.add("efi", f"{tag} reference data eps2", known=0.6330071575726789, clim=np.asarray(d.clim_eps2, dt),
                ens=np.asarray(d.ens_eps2, dt), eps=1e-4)
        rec.add("efi", f"{tag} reference data sorted ens", known=-0.18384250406420133, clim=c, ens=np.sort(e, axis=0))
        rec.add("efi", f"{tag} all nan", clim=np.full((101, 1), np.nan, dt), ens=np.full((51, 1), np.nan, dt))
        rec.add("sot", f"{tag} reference data 90", known=-2.14617638, clim=c, ens=e, perc=90)
        rec.add("sot", f"{tag} reference data 10", known=-1.3086723, clim=c, ens=e, perc=10)
        rec.add("sot", f"{tag} reference data eps2 eps 1e4", clim=np.asarray(d.clim_eps2, dt), ens=np.asarray(d.ens_eps2, dt),
                perc=90, eps=1e4)
        table = [([1.0, 1.0, 1.0, 1.0], [1.1, 1.0, 1.0, 1.00001], [1.5, 1.2, 1.0, 0.9], dict(eps=1e-4)),
                 ([1.0, 1.0], [1.1, 1.1], [15, -15.0], {}), ([0.05], [0.1], [0.2], {}), ([0.05], [0.1], [0.2], dict(eps=0.15)),
                 ([0.05], [0.1], [np.nan], {}), ([0.05], [np.nan], [0.1], {}), ([np.nan], [0.1], [0.2], {})]
        for i, (qt, qc, qf, kw) in enumerate(table):
            rec.add("sot_func", f"{tag} reference table {i}", qc_tail=np.asarray(qt, dt), qc=np.asarray(qc, dt),
                    qf=np.asarray(qf, dt), **kw)


def sot_cases(rec, rng):
    for dt, tag in ((F64, "f64"), (F32, "f32")):
        clim = precip(rng, 101, NPTS, dt, True) + np.linspace(0, 1, 101, dtype=dt)[:, None]
        clim[:, 0] = dt(2.5)                                      # zero denominator
        for nens in (51, 50, 7, 1):
            ens = precip(rng, nens, NPTS, dt, False) + rng.uniform(0, 0.5, (nens, NPTS)).astype(dt)
            ens[:, 1], ens[:, 2] = ens[:, 1] + dt(1e4), ens[:, 2] - dt(1e4)  # both clamps
            ens[nens // 2, 3] = np.nan
            ens[0, 4], ens[nens - 1, 5] = np.inf, -np.inf
            for perc in (2, 10, 33, 49, 51, 90, 98):
                for eps in (-1e4, 0.75):
                    rec.add("sot", f"{tag} nens {nens} perc {perc} eps {eps}", clim=clim, ens=ens, perc=perc, eps=eps)
        ens = precip(rng, 51, NPTS, dt, False)
        rec.add("sot", f"{tag} default eps 3-D", clim=clim.reshape(101, 4, 6), ens=ens.reshape(51, 4, 6), perc=90)
        q = rng.normal(0, 1, (3, 40)).astype(dt)
        q[1, :6] = q[0, :6]                                       # zero denominator
        q[1, 6:12] = q[0, 6:12] + dt(5e-5)                        # below eps
        q[2, 12:18] *= dt(1e3)
        for kw in ({}, dict(eps=1e-4), dict(eps=1e-4, lower_bound=-2, upper_bound=3), dict(lower_bound=-0.5, upper_bound=0.25)):
            rec.add("sot_func", f"{tag} random {sorted(kw)}", qc_tail=q[0], qc=q[1], qf=q[2], **kw)
    c64, e64 = precip(rng, 101, NPTS, F64, True) + np.linspace(0, 1, 101)[:, None], precip(rng, 51, NPTS, F64, False)
    rec.add("sot", "mixed clim f64 ens f32", clim=c64, ens=e64.astype(F32), perc=10)
    # error conventions
    rec.add("sot", "perc 50", clim=c64, ens=e64, perc=50)
    rec.add("sot", "perc 1", clim=c64, ens=e64, perc=1)
    rec.add("sot", "perc float", clim=c64, ens=e64, perc=90.0)
    rec.add("sot", "clim 100 rows", clim=c64[:100], ens=e64, perc=90)


def crps_cases(rec, rng):
    for dt, tag in ((F64, "f64"), (F32, "f32")):
        for nens in (1, 7, 51):
            x = np.round(rng.normal(0, 2, (nens, NPTS)) * 16) / 16
            s = np.sort(x, axis=0)
            y = rng.normal(0, 2, NPTS)
            y[0:3] = s[0, 0:3] - 1.5                                # below the ensemble
            y[3:6] = s[-1, 3:6] + 0.75                              # above
            y[6:9] = s[nens // 2, 6:9]                              # on a member
            y[9], y[10] = s[0, 9], s[-1, 10]                        # on the lowest / highest member
            x[:, 11] = 1.25                                         # all members equal
            x, y = x.astype(dt), y.astype(dt)
            for policy in ("propagate", "raise", "omit"):
                rec.add("crps_from_ensemble", f"{tag} nens {nens} clean {policy}", x=x, y=y, nan_policy=policy)
            xm, ym = x.copy(), y.copy()
            xm[nens // 2, 12], ym[13] = np.nan, np.nan
            xm[0, 14], xm[nens - 1, 15], ym[16] = np.inf, -np.inf, np.inf
            for policy in ("propagate", "raise", "omit"):
                rec.add("crps_from_ensemble", f"{tag} nens {nens} nan inf {policy}", x=xm, y=ym, nan_policy=policy)
        x = rng.normal(0, 1, (9, 4, 6)).astype(dt)
        rec.add("crps_from_ensemble", f"{tag} 2-D points", x=x, y=rng.normal(0, 1, (4, 6)).astype(dt))
    x = rng.normal(0, 1, (9, NPTS))
    rec.add("crps_from_ensemble", "bad policy", x=x, y=x[0], nan_policy="drop")


def main():
    rec = Recorder()
    rng = np.random.default_rng(20261018)
    reference_data_cases(rec)
    efi_cases(rec, rng)
    sot_cases(rec, rng)
    crps_cases(rec, rng)
    tables = {}
    for nclim in (2, 11, 101):
        p = np.linspace(0.0, 1.0, nclim)
        acosdiff, proddiff = np.diff(np.acos(np.sqrt(p))), np.diff(np.sqrt(p * (1.0 - p)))
        tables[str(nclim)] = [rec.put(t) for t in (acosdiff, proddiff, (1.0 - 2.0 * p[:-1]) * acosdiff + proddiff)]
    meta = dict(cases=rec.manifest, efi_tables=tables, signatures={f: bare_signature(fn) for f, fn in FUNCS.items()})
    rec.store["manifest"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "ensemble_golden.npz")
    write_npz(path, rec.store)
    print(len(rec.manifest), "cases,", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
