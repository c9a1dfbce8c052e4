#!/usr/bin/env python3
"""Golden vectors for stats.GumbelDistribution and the return-period functions, recorded from the REFERENCE (build
container only; stand-ins for the un-vendored packages in tests/golden/_standin, as in gen_golden_quantiles.py).  The
reference's stats/array/extreme_values.py and stats/array/_polyfill.py are loaded by file path, so nothing else of the
package is imported.

Writes tests/golden/gumbel_golden.npz: data only; arrays are stored once and shared between cases; a JSON manifest with
the NumPy and SciPy versions that computed them and the recorded signature strings; the file regenerates byte for byte.

Every `fit` case records three results (mu and sigma each):
  (a) the reference as it runs on the recording host, on the sample's own dtype (with SciPy >= 1.15 installed its
      `lmoment` is scipy.stats.lmoment);
  (b) the reference with `lmoment` replaced by its own polyfill (_polyfill.py), on the sample's own dtype;
  (c) the polyfill path on the sample widened to float64: what the product reproduces bit for bit.
The polyfill takes axis 0 only, so (b) and (c) of a case with another axis are recorded on the sample moved to axis 0;
it refuses fewer than 4 values, so the cases with 2 and 3 values record its exception there (and (a) where SciPy takes
them).  `nonfinite` lists the columns that hold a NaN or an infinity: the comparison of (a) and (b) with (c) leaves out
exactly those.

fit cases, 24 points each unless an axis case: f32 and f64, n in {2, 3, 4, 9, 51, 128} plus 256 for f32; Gumbel-distributed
data, 300 +- 0.05 (l2 is ill-conditioned), tie-heavy clamped precipitation with all-zero columns; special columns (all
equal, a NaN member, +inf, -inf, both); axes 0, 1, 2 and -1 of a (5, 7, 6) array; integer input; the error cases.
cdf / ppf / return-period cases: scalar, 1-D and (2, 3) levels, (mu - x) / sigma from -40 to 4, p in
{0, 1e-12, 0.5, 1 - 1e-12, 1}, numeric and timedelta freq, sigma of 0 and negative, a NaN parameter, f32 parameters with
float64 levels, a scalar and a two-dimensional distribution.
"""
import datetime
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


def load_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_ARRAY = os.path.join(REF, "src", "earthkit", "meteo", "stats", "array")
ref = load_path("_ref_stats_extreme_values", os.path.join(_ARRAY, "extreme_values.py"))
poly = load_path("_ref_stats_polyfill", os.path.join(_ARRAY, "_polyfill.py"))
NATIVE_LMOMENT = ref.lmoment


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


def plain_of(v):
    """A JSON form of a plain argument: a timedelta becomes ["timedelta", seconds]."""
    if isinstance(v, datetime.timedelta):
        return ["timedelta", v.total_seconds()]
    return v


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

    def _fit(self, sample, axis, lmoment):
        ref.lmoment = lmoment
        try:
            dist = ref.GumbelDistribution.fit(sample, axis=axis)
            return dict(mu=self.put(dist.mu), sigma=self.put(dist.sigma), raises=None)
        except Exception as exc:  # the error convention is part of the record
            return dict(mu=None, sigma=None, raises=[type(exc).__name__, str(exc)])
        finally:
            ref.lmoment = NATIVE_LMOMENT

    def add_fit(self, note, sample, axis=0):
        before = sample.copy()
        entry = dict(id=f"c{len(self.manifest):04d}", func="fit", note=note, arrays=dict(sample=self.put(sample)),
                     plain=dict(axis=axis))
        entry["a"] = self._fit(sample, axis, NATIVE_LMOMENT)
        try:
            first = np.ascontiguousarray(np.moveaxis(sample, axis, 0))
            entry["b"] = self._fit(first, 0, poly.lmoment)
            entry["c"] = self._fit(first.astype(F64), 0, poly.lmoment)
            entry["nonfinite"] = self.put((~np.isfinite(first.astype(F64))).any(axis=0).astype(np.uint8))
        except Exception as exc:  # an axis that does not exist: nothing to move
            entry["b"] = entry["c"] = dict(mu=None, sigma=None, raises=[type(exc).__name__, str(exc)])
            entry["nonfinite"] = None
        assert before.tobytes() == sample.tobytes(), "the reference modified its input"
        self.manifest.append(entry)

    def add_call(self, func, note, mu, sigma, freq, arg, deviation=None):
        """func in cdf, ppf, value_to_return_period, return_period_to_value; arg: the levels (a number, an array or a
        timedelta)."""
        entry = dict(id=f"c{len(self.manifest):04d}", func=func, note=note, arrays=dict(mu=self.put(mu), sigma=self.put(sigma)),
                     plain=dict(freq=plain_of(freq)), out=None, raises=None)
        if isinstance(arg, np.ndarray):
            entry["arrays"]["arg"] = self.put(arg)
        else:
            entry["plain"]["arg"] = plain_of(arg)
        dist = ref.GumbelDistribution(mu, sigma, freq=freq)
        try:
            if func in ("cdf", "ppf"):
                out = getattr(dist, func)(arg)
            else:
                out = getattr(ref, func)(dist, arg)
            out = np.asarray(out)
            if out.dtype == object:  # timedelta / float64 array: an array of timedelta objects, stored as seconds
                entry["out_kind"] = "timedelta seconds"
                out = np.array([v.total_seconds() for v in out.reshape(-1)], F64).reshape(out.shape)
            entry["out"] = self.put(out)
        except Exception as exc:
            entry["raises"] = [type(exc).__name__, str(exc)]
        if deviation:
            entry["deviation"] = deviation
        self.manifest.append(entry)


def gumbel(rng, rows, npts, dt):
    return rng.gumbel(20.0, 5.0, (rows, npts)).astype(dt)


def narrow(rng, rows, npts, dt):
    """300 +- 0.05: the second L-moment is a small difference of large sums."""
    return (300.0 + rng.uniform(-0.05, 0.05, (rows, npts))).astype(dt)


def precip(rng, rows, npts, dt):
    """gen_golden_ensemble.precip: gamma-distributed, clamped at zero (many ties), rounded to 1/8; two all-zero columns."""
    a = np.maximum(rng.gamma(1.5, 2.0, (rows, npts)) - 1.5, 0.0)
    a[:, 1:3] = 0.0
    return (np.round(a * 8) / 8).astype(dt)


def special(rng, m, dt):
    a = gumbel(rng, m, NPTS, dt)
    a[:, 0:2] = dt(3.25)                       # all-equal columns
    a[m // 2, 2:4] = np.nan                    # a NaN member
    a[m // 3, 4] = np.inf                      # +inf
    a[m // 3, 5] = -np.inf                     # -inf: -inf * 0 = NaN in the weighted sum
    a[0, 6], a[m - 1, 6] = np.inf, -np.inf     # both
    a[1, 7], a[m - 2, 7] = -np.inf, -np.inf    # two at the bottom
    return a


def fit_cases(rec, rng):
    for dt, tag in ((F64, "f64"), (F32, "f32")):
        for m in (2, 3, 4, 9, 51, 128) + ((256,) if dt is F32 else ()):
            for kind, make in (("gumbel", gumbel), ("narrow", narrow), ("precip", precip)):
                rec.add_fit(f"{tag} n {m} {kind}", make(rng, m, NPTS, dt))
        for m in (9, 51):
            rec.add_fit(f"{tag} n {m} special", special(rng, m, dt))
        cube = gumbel(rng, 5, 42, dt).reshape(5, 7, 6)
        cube[1, 2, 3] = np.nan
        for axis in (0, 1, 2, -1):
            rec.add_fit(f"{tag} cube axis {axis}", cube, axis=axis)
    rec.add_fit("integer input", np.round(gumbel(rng, 9, NPTS, F64)).astype(np.int64))
    # the error cases
    rec.add_fit("error one value", gumbel(rng, 1, NPTS, F64))
    rec.add_fit("error axis out of range", gumbel(rng, 9, NPTS, F64), axis=2)
    rec.add_fit("error scalar sample", np.float64(3.0))


def call_cases(rec, rng):
    mu = 20.0 + rng.normal(0, 3, NPTS)
    sigma = 5.0 * np.exp(rng.normal(0, 0.2, NPTS))
    odd_mu, odd_sigma = mu.copy(), sigma.copy()
    odd_sigma[3], odd_sigma[4], odd_mu[5], odd_sigma[6] = 0.0, -2.0, np.nan, np.nan
    z = np.linspace(-40.0, 4.0, 12)
    x1 = 20.0 - 5.0 * z                                  # (mu - x) / sigma from about -40 to 4
    x23 = np.array([[10.0, 25.0, 31.5], [60.0, 120.0, 220.0]])
    p1 = np.array([0.0, 1e-12, 0.5, 1.0 - 1e-12, 1.0])
    p23 = np.array([[0.01, 0.5, 0.9], [0.99, 0.999, 1.0 - 1e-9]])
    rp1 = np.array([1.0, 2.0, 10.0, 100.0, 1e6, 1e12])
    dists = (("plain", mu, sigma), ("odd sigma", odd_mu, odd_sigma), ("2-d", mu.reshape(4, 6), sigma.reshape(4, 6)),
             ("broadcast", mu.reshape(4, 6)[:, :1], sigma.reshape(4, 6)[:1, :]), ("scalar", np.float64(21.0), np.float64(4.5)),
             ("f32 parameters", mu.astype(F32), sigma.astype(F32)))
    day = datetime.timedelta(days=1)
    for name, m, s in dists:
        for lname, x in (("scalar", 31.5), ("1-d", x1), ("(2, 3)", x23)):
            rec.add_call("cdf", f"{name} levels {lname}", m, s, None, x)
            for fname, freq in (("none", None), ("2.5", 2.5), ("7", 7), ("timedelta", day)):
                rec.add_call("value_to_return_period", f"{name} levels {lname} freq {fname}", m, s, freq, x)
        for lname, p in (("scalar", 0.99), ("1-d", p1), ("(2, 3)", p23)):
            rec.add_call("ppf", f"{name} p {lname}", m, s, None, p)
        for lname, rp in (("scalar", 100.0), ("1-d", rp1)):
            for fname, freq in (("none", None), ("0.5", 0.5)):
                rec.add_call("return_period_to_value", f"{name} return period {lname} freq {fname}", m, s, freq, rp)
        rec.add_call("return_period_to_value", f"{name} return period timedelta freq timedelta", m, s, day,
                     datetime.timedelta(days=3652))
        rec.add_call("return_period_to_value", f"{name} return period timedelta64 1-d freq timedelta", m, s, day,
                     np.array([2, 30, 365, 36525], dtype="timedelta64[D]"))


def main():
    import scipy

    rec = Recorder()
    rng = np.random.default_rng(20261019)
    fit_cases(rec, rng)
    call_cases(rec, rng)
    sigs = {"GumbelDistribution": bare_signature(ref.GumbelDistribution.__init__),
            "fit": bare_signature(ref.GumbelDistribution.fit), "cdf": bare_signature(ref.GumbelDistribution.cdf),
            "ppf": bare_signature(ref.GumbelDistribution.ppf),
            "value_to_return_period": bare_signature(ref.value_to_return_period),
            "return_period_to_value": bare_signature(ref.return_period_to_value)}
    meta = dict(cases=rec.manifest, numpy=np.__version__, scipy=scipy.__version__,
                native_lmoment=NATIVE_LMOMENT.__module__, signatures=sigs)
    rec.store["manifest"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "gumbel_golden.npz")
    write_npz(path, rec.store)
    print(len(rec.manifest), "cases,", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
