#!/usr/bin/env python3
"""Golden vectors for the vertical interpolation functions, recorded from the REFERENCE (build container only; stand-ins
for the un-vendored packages in tests/golden/_standin, as in gen_golden_vertical.py).

Writes tests/golden/interp_golden.npz: for every case the arguments of one call of `interpolate_monotonic`,
`interpolate_hybrid_to_pressure_levels`, `interpolate_hybrid_to_height_levels` or
`interpolate_pressure_to_height_levels` and the array the reference returned,
plus a JSON manifest (case ids, the non-array arguments) and the recorded signature strings.  Data only.

The reference's own case tables (tests/vertical/_monotonic_cases.py, _pl_data.py, _hybrid_height_data.py) are replayed
as data; the new cases cover all three modes x f32/f64 with 1-D and same-shape coordinates, scalar / vector / field
targets, both level orders, targets on a level and one nextafter either side, beyond both ends, inside the isclose
band at half its width and outside at twice its width, every aux layout, NaN / inf in data, coord and sp,
vertical_axis 1 and 2, a level subset and mixed dtypes.  Every array of a case has the dtype the case names, so the
arithmetic dtype of the product (f32 only when everything is f32) is the dtype the reference computed in.
"""
import importlib.util
import inspect
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("EKM_REFERENCE", "/root/reference")
sys.path[:0] = [os.path.join(HERE, "_standin"), os.path.join(REF, "src")]

from earthkit.meteo.vertical import array as ref  # noqa: E402

warnings.simplefilter("ignore")
np.seterr(all="ignore")

MODES = ("linear", "log", "nearest")
FUNCS = ("interpolate_monotonic", "interpolate_hybrid_to_pressure_levels", "interpolate_hybrid_to_height_levels",
         "interpolate_pressure_to_height_levels")


def load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, "tests", "vertical", name + ".py"))
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
        """Arrays are stored once: most cases share their inputs."""
        key = (v.dtype.str, v.shape, v.tobytes())
        if key not in self.seen:
            self.seen[key] = f"a{len(self.seen):04d}"
            self.store[self.seen[key]] = v
        return self.seen[key]

    def add(self, func, note, expected=None, **kwargs):
        cid = f"c{len(self.manifest):04d}"
        entry = dict(id=cid, func=func, note=note, arrays={}, plain={})
        call = {}
        for k, v in kwargs.items():
            if v is None or isinstance(v, (str, int)):
                entry["plain"][k] = v
                call[k] = v
            else:
                v = np.asarray(v)
                entry["arrays"][k] = self.put(v)
                call[k] = v
        out = np.asarray(getattr(ref, func)(**call) if expected is None else expected(call))
        entry["out"] = self.put(out)
        entry["out_dtype"], entry["out_shape"] = str(out.dtype), list(out.shape)
        self.manifest.append(entry)
        return out


def column_targets(c, dt):
    """Per-column targets [nt, ncol] for a DESCENDING coordinate field c [nlev, ncol]: on a level and one nextafter either
    side, beyond both ends, inside (half width) and outside (twice the width) the isclose band of both end levels."""
    big = np.asarray(np.inf, dt)
    rows = [c[2], np.nextafter(c[2], big), np.nextafter(c[2], -big), c[0], c[-1], np.nextafter(c[0], big),
            np.nextafter(c[-1], -big), c[0] * dt(1.1), c[-1] * dt(0.9), c[0] * dt(1 + 0.5e-5), c[0] * dt(1 + 2e-5),
            c[-1] * dt(1 - 0.5e-5), c[-1] * dt(1 - 2e-5), (c[1] + c[2]) * dt(0.5), c[3] * dt(0.75) + c[4] * dt(0.25),
            (c[-2] + c[-1]) * dt(0.5)]
    return np.stack(rows).astype(dt)


def new_monotonic_cases(rec, rng):
    nlev, ncol = 9, 7
    base = np.array([101000.0, 92500.0, 85000.0, 70000.0, 50000.0, 30000.0, 10000.0, 3000.0, 500.0])
    for dt in (np.float64, np.float32):
        tag = "f64" if dt is np.float64 else "f32"
        c = (base[:, None] * (1.0 + 0.03 * rng.uniform(-1, 1, (nlev, ncol)))).astype(dt)
        c = -np.sort(-c, axis=0)
        d = (250.0 + 40.0 * rng.uniform(-1, 1, (nlev, ncol))).astype(dt)
        tf = column_targets(c, dt)
        tv = np.concatenate([tf[:, 0], base.astype(dt)[2:5] * dt(0.97)]).astype(dt)
        c1 = c[:, 0].copy()
        d_bad = d.copy()
        d_bad[0, 1], d_bad[3, 2], d_bad[-1, 3], d_bad[4, 4] = np.nan, np.inf, -np.inf, np.nan
        c_bad = c.copy()
        c_bad[:, 1] = np.nan       # a column without a coordinate
        c_bad[0, 2] = np.inf       # still descending
        t_bad = tf.copy()
        t_bad[5, 3], t_bad[6, 4], t_bad[7, 5] = np.nan, np.inf, -np.inf
        # aux layers: beyond the end level in some columns, not beyond it in others
        amax_c = (c[0] * np.array([1.2, 1.05, 0.99, 1.0, 1.3, 1.101, 0.5])).astype(dt)
        amin_c = (c[-1] * np.array([0.5, 0.95, 1.01, 1.0, 0.2, 0.899, 2.0])).astype(dt)
        amax_d = (300.0 + rng.uniform(-5, 5, ncol)).astype(dt)
        amin_d = (200.0 + rng.uniform(-5, 5, ncol)).astype(dt)
        for mode in MODES:
            k = dict(interpolation=mode)
            rec.add("interpolate_monotonic", f"{tag} {mode} field coord, field target, descending", data=d, coord=c, target_coord=tf, **k)
            rec.add("interpolate_monotonic", f"{tag} {mode} field coord, field target, ascending", data=d[::-1].copy(),
                    coord=c[::-1].copy(), target_coord=tf, **k)
            rec.add("interpolate_monotonic", f"{tag} {mode} field coord, vector target", data=d, coord=c, target_coord=tv, **k)
            rec.add("interpolate_monotonic", f"{tag} {mode} field coord, scalar target", data=d, coord=c,
                    target_coord=np.asarray(tv[13]), **k)
            rec.add("interpolate_monotonic", f"{tag} {mode} 1-D coord, vector target", data=d, coord=c1, target_coord=tv, **k)
            rec.add("interpolate_monotonic", f"{tag} {mode} 1-D coord ascending, scalar target", data=d[::-1].copy(),
                    coord=c1[::-1].copy(), target_coord=np.asarray(tv[14]), **k)
            rec.add("interpolate_monotonic", f"{tag} {mode} 1-D data and coord", data=d[:, 0].copy(), coord=c1, target_coord=tv, **k)
            rec.add("interpolate_monotonic", f"{tag} {mode} NaN / inf in data", data=d_bad, coord=c, target_coord=tf, **k)
            rec.add("interpolate_monotonic", f"{tag} {mode} NaN / inf in coord and target", data=d, coord=c_bad, target_coord=t_bad, **k)
            rec.add("interpolate_monotonic", f"{tag} {mode} aux max alone (field)", data=d, coord=c, target_coord=tf,
                    aux_max_level_data=amax_d, aux_max_level_coord=amax_c, **k)
            rec.add("interpolate_monotonic", f"{tag} {mode} aux min alone (field), ascending", data=d[::-1].copy(),
                    coord=c[::-1].copy(), target_coord=tf, aux_min_level_data=amin_d, aux_min_level_coord=amin_c, **k)
            rec.add("interpolate_monotonic", f"{tag} {mode} both aux (field data, scalar coord)", data=d, coord=c, target_coord=tv,
                    aux_min_level_data=amin_d, aux_min_level_coord=np.asarray(c[-1].min() * dt(0.8), dt),
                    aux_max_level_data=amax_d, aux_max_level_coord=np.asarray(c[0].max() * dt(1.06), dt), **k)
            rec.add("interpolate_monotonic", f"{tag} {mode} both aux (scalars), NaN data", data=d_bad, coord=c, target_coord=tf,
                    aux_min_level_data=np.asarray(210.0, dt), aux_min_level_coord=np.asarray(c[-1].mean(), dt),
                    aux_max_level_data=np.asarray(290.0, dt), aux_max_level_coord=np.asarray(c[0].mean(), dt), **k)
            rec.add("interpolate_monotonic", f"{tag} {mode} aux data without coord is ignored", data=d, coord=c, target_coord=tv,
                    aux_max_level_data=amax_d, **k)
            rec.add("interpolate_monotonic", f"{tag} {mode} 1-D data and coord with both aux", data=d[:, 0].copy(), coord=c1,
                    target_coord=tv, aux_min_level_data=np.asarray(210.0, dt), aux_min_level_coord=np.asarray(c1[-1] * dt(0.5), dt),
                    aux_max_level_data=np.asarray(290.0, dt), aux_max_level_coord=np.asarray(c1[0] * dt(1.2), dt), **k)
            # vertical_axis 1 and 2: [a, level, b] and [a, b, level]
            c3 = np.stack([c[:, :6].reshape(nlev, 2, 3), c[:, 1:7].reshape(nlev, 2, 3)])[0]
            d3 = d[:, :6].reshape(nlev, 2, 3)
            t3 = tf[:, :6].reshape(-1, 2, 3)
            for ax in (1, 2):
                rec.add("interpolate_monotonic", f"{tag} {mode} vertical_axis={ax}, field target",
                        data=np.moveaxis(d3, 0, ax).copy(), coord=np.moveaxis(c3, 0, ax).copy(),
                        target_coord=np.moveaxis(t3, 0, ax).copy(), vertical_axis=ax, **k)
                rec.add("interpolate_monotonic", f"{tag} {mode} vertical_axis={ax}, vector target",
                        data=np.moveaxis(d3, 0, ax).copy(), coord=np.moveaxis(c3, 0, ax).copy(), target_coord=tv, vertical_axis=ax, **k)
        if dt is np.float32:  # mixed: f32 data with an f64 coordinate (and f64 targets)
            for mode in MODES:
                rec.add("interpolate_monotonic", f"mixed f32 data, f64 coord {mode}", data=d, coord=c.astype(np.float64),
                        target_coord=tf.astype(np.float64), interpolation=mode)


def hybrid_pressure_cases(rec, rng):
    A, B = ref.hybrid_level_parameters(137)
    ncol = 11
    sp64 = rng.uniform(52000.0, 104000.0, ncol)
    sp64[3], sp64[7] = np.nan, np.inf
    d64 = 250.0 + 40.0 * rng.uniform(-1, 1, (137, ncol))
    d64[136, 5], d64[60, 6] = np.nan, np.inf
    std = 100.0 * np.array([1000, 975, 950, 925, 900, 875, 850, 825, 800, 775, 750, 700, 650, 600, 550, 500, 450, 400, 350,
                            300, 250, 225, 200, 175, 150, 125, 100, 70, 50, 30, 20, 10, 7, 5, 3, 2, 1], dtype=np.float64)
    for dt in (np.float64, np.float32):
        tag = "f64" if dt is np.float64 else "f32"
        a, b, sp, d, tv = (x.astype(dt) for x in (A, B, sp64, d64, std))
        p = ref.pressure_on_hybrid_levels(a, b, sp)
        assert p.dtype == dt
        pd = p[::-1]  # descending view, for the per-column targets (rows 2 .. of the 137)
        sel = pd[[0, 1, 2, 40, 80, 134, 135, 136]]
        tf = column_targets(sel, dt)
        surf_d = (288.0 + rng.uniform(-3, 3, ncol)).astype(dt)
        for mode in MODES:
            k = dict(A=a, B=b, sp=sp, interpolation=mode)
            f = "interpolate_hybrid_to_pressure_levels"
            rec.add(f, f"{tag} {mode} 37 standard levels", data=d, target_p=tv, **k)
            rec.add(f, f"{tag} {mode} field targets on and around the levels", data=d, target_p=tf, **k)
            rec.add(f, f"{tag} {mode} scalar target", data=d, target_p=np.asarray(tv[6]), **k)
            rec.add(f, f"{tag} {mode} level subset (bottom 47)", data=d[90:].copy(), target_p=tv, **k)
            rec.add(f, f"{tag} {mode} aux bottom = the surface", data=d, target_p=tv, aux_bottom_data=surf_d, aux_bottom_p=sp, **k)
            rec.add(f, f"{tag} {mode} aux top alone (scalars)", data=d, target_p=tf, aux_top_data=np.asarray(200.0, dt),
                    aux_top_p=np.asarray(0.5, dt), **k)
            rec.add(f, f"{tag} {mode} both aux, arpege", data=d, target_p=tf, aux_bottom_data=surf_d, aux_bottom_p=sp,
                    aux_top_data=np.asarray(200.0, dt), aux_top_p=np.asarray(0.5, dt), alpha_top="arpege", **k)
            rec.add(f, f"{tag} {mode} one column", data=d[:, 0].copy(), target_p=tv, A=a, B=b, sp=np.asarray(sp[0]), interpolation=mode)
            # vertical_axis != 0: the documented meaning (the reference raises a shape error there): recorded on moved arrays
            d3, sp2 = d[:, :10].reshape(137, 2, 5), sp[:10].reshape(2, 5)
            t3 = tf[:, :10].reshape(-1, 2, 5)
            for ax in (1, 2):
                def moved(call, ax=ax):
                    c2 = dict(call)
                    c2["data"] = np.moveaxis(c2["data"], ax, 0)
                    if np.ndim(c2["target_p"]) > 1:
                        c2["target_p"] = np.moveaxis(c2["target_p"], ax, 0)
                    c2["vertical_axis"] = 0
                    return np.moveaxis(ref.interpolate_hybrid_to_pressure_levels(**c2), 0, ax)
                rec.add(f, f"{tag} {mode} vertical_axis={ax} vector target", expected=moved, data=np.moveaxis(d3, 0, ax).copy(),
                        target_p=tv, A=a, B=b, sp=sp2, interpolation=mode, vertical_axis=ax)
                rec.add(f, f"{tag} {mode} vertical_axis={ax} field target", expected=moved, data=np.moveaxis(d3, 0, ax).copy(),
                        target_p=np.moveaxis(t3, 0, ax).copy(), A=a, B=b, sp=sp2, interpolation=mode, vertical_axis=ax)
        if dt is np.float32:  # mixed: the f64 tables with f32 sp and f32 data: the pressure (and the arithmetic) is f64
            for mode in MODES:
                rec.add("interpolate_hybrid_to_pressure_levels", f"mixed f64 tables, f32 sp and data {mode}", data=d, target_p=std,
                        A=A, B=B, sp=sp, interpolation=mode)


def reference_tables(rec):
    for name, rows in load("_monotonic_cases").cases.items():
        for i, (data, coord, target, mode, _expected) in enumerate(rows):
            try:
                rec.add("interpolate_monotonic", f"reference table {name}[{i}]", data=np.asarray(data, dtype=np.float64),
                        coord=np.asarray(coord, dtype=np.float64), target_coord=np.asarray(target, dtype=np.float64),
                        interpolation=mode)
            except Exception as exc:  # a row the reference itself rejects is not a fixture
                print("skipped", name, i, type(exc).__name__)
    pl = load("_pl_data")
    for k in ("t", "z", "p", "p_surf", "z_surf"):
        rec.store[f"plfix.{k}"] = np.asarray(getattr(pl, k), dtype=np.float64)
    # the pressure-level table as a plain monotonic problem: t against p, both orders
    t, p = np.asarray(pl.t, dtype=np.float64), np.asarray(pl.p, dtype=np.float64)
    tv = np.array([100000.0, 92500.0, 60000.0, 12500.0, 10000.0, 9000.0])
    for mode in MODES:
        rec.add("interpolate_monotonic", f"reference _pl_data t on p {mode}", data=t, coord=p, target_coord=tv, interpolation=mode)


def hybrid_height_cases(rec):
    hh = load("_hybrid_height_data")
    A, B, t, q = (np.asarray(getattr(hh, k), dtype=np.float64) for k in ("A", "B", "t", "q"))
    zs, sp = np.asarray(hh.z_surf, dtype=np.float64), np.asarray(hh.p_surf, dtype=np.float64)
    for ht in ("geometric", "geopotential"):
        for hr in ("ground", "sea"):
            h = ref.height_on_hybrid_levels(t, q, zs, A, B, sp, h_type=ht, h_reference=hr)
            lo, hi = h.min(axis=0).max(), h.max(axis=0).min()
            tv = np.array([0.25 * lo, 1.5 * lo, 100.0 + lo, 1000.0 + lo, 5000.0 + lo, 20000.0, 0.9 * hi, 1.2 * hi])
            # no target within 1e-3 relative of any column's end coordinate: the end-to-end check needs no exclusions
            for end in (h[0], h[-1]):
                assert np.all(np.abs(tv[:, None] - end[None, :]) > 1e-3 * np.abs(end[None, :])), (ht, hr)
            for mode in MODES:
                k = dict(t=t, q=q, zs=zs, A=A, B=B, sp=sp, h_type=ht, h_reference=hr, interpolation=mode)
                rec.add("interpolate_hybrid_to_height_levels", f"{ht} {hr} {mode}", data=t, target_h=tv, **k)
            rec.add("interpolate_hybrid_to_height_levels", f"{ht} {hr} linear, both aux", data=t, target_h=tv,
                    aux_bottom_data=np.asarray([285.0, 295.0]), aux_bottom_h=np.asarray(0.1 * lo),
                    aux_top_data=np.asarray(190.0), aux_top_h=np.asarray(1.5 * hi), t=t, q=q, zs=zs, A=A, B=B, sp=sp,
                    h_type=ht, h_reference=hr, interpolation="linear")


def write_npz(path, store):
    """np.savez_compressed with a fixed time stamp on every member: the file regenerates byte for byte."""
    import io
    import zipfile

    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, arr in store.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def pressure_height_cases(rec):
    pl = load("_pl_data")
    t, z = np.asarray(pl.t, dtype=np.float64), np.asarray(pl.z, dtype=np.float64)
    zs = np.asarray(pl.z_surf, dtype=np.float64)
    for dt in (np.float64, np.float32):
        tag = "f64" if dt is np.float64 else "f32"
        t_, z_, zs_ = t.astype(dt), z.astype(dt), zs.astype(dt)
        for ht in ("geometric", "geopotential"):
            for hr in ("ground", "sea"):
                hh = ref.geometric_height_from_geopotential(z_) if ht == "geometric" else ref.geopotential_height_from_geopotential(z_)
                tv = np.array([0.0, 50.0, 1000.0, 5000.0, 10000.0, 0.5 * (hh[-1].min() + hh[-2].max()), 40000.0]).astype(dt)
                for mode in MODES:
                    rec.add("interpolate_pressure_to_height_levels", f"{tag} {ht} {hr} {mode}", data=t_, target_h=tv, z=z_, zs=zs_,
                            h_type=ht, h_reference=hr, interpolation=mode)
                rec.add("interpolate_pressure_to_height_levels", f"{tag} {ht} {hr} linear, ascending pressure, both aux",
                        data=t_[::-1].copy(), target_h=tv, z=z_[::-1].copy(), zs=zs_, h_type=ht, h_reference=hr,
                        interpolation="linear", aux_bottom_data=(t_[0] + dt(1.5)), aux_bottom_h=np.asarray(-400.0, dt),
                        aux_top_data=np.asarray(215.0, dt), aux_top_h=np.asarray(45000.0, dt))


def main():
    rec = Recorder()
    rng = np.random.default_rng(20261017)
    reference_tables(rec)
    new_monotonic_cases(rec, rng)
    hybrid_pressure_cases(rec, rng)
    hybrid_height_cases(rec)
    pressure_height_cases(rec)
    meta = dict(cases=rec.manifest, signatures={f: bare_signature(getattr(ref, f)) for f in FUNCS})
    rec.store["manifest"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "interp_golden.npz")
    write_npz(path, rec.store)
    print(len(rec.manifest), "cases,", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
