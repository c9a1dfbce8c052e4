"""An independent NumPy restatement of the solar functions (reference solar/array/solar.py), the parity bar of the solar
tests with its derivation, and access to tests/golden/solar_golden.npz -- TEST INFRASTRUCTURE.

The restatement evaluates the reference's formula directly -- one cosine of the full hour angle per node and point, no
angle addition -- in extended precision (numpy.longdouble) on the inputs upcast exactly, with the angle reduced modulo
360 degrees first; its own rounding is below 1e-18, so it stands for the exact value of the formula.  Its time nodes
come from its own builder (`nodes`), written from the description of the quadrature, not from ekm_hip.solar.

THE BAR.  Every compared quantity is a cosine in [0, 1] (times isr <= 5.06e6 for the radiation); the bar is absolute.
With u = 2^-53 (unit roundoff of float64) and N time nodes, for |lon| <= 720.  A sine or cosine good to 1 ulp is counted
as 2 u (an ulp of a value in [0.5, 1] is 2^-52); tests/test_solar_cpu.py asserts exactly that of `sol_sincos_deg`:
  the reference's float64 run, against the exact formula
    rad(lat) rounded: |lat_rad| u <= 1.6 u, in sin(lat) and in cos(lat)                                  3.2 u
    sin(lat), cos(lat) (libm, < 1 ulp each)                                                              4   u
    h15 + lon rounded (<= 900 deg: 15.7 u rad), + tc rounded (15.8 u), deg2rad rounded (15.8 u)         47.3 u
    cos of that angle                                                                                    2   u
    sd * sin, cd * cos, * cos, the sum                                                                   4   u
                                                                                                  total 60.5 u
  the product (csrc/solar_point.hpp: exact reduction in degrees), against the exact formula
    sin / cos of lat and of lon (<= 1 ulp each: 8 u), cos(lat) * cos(lon), cos(lat) * sin(lon) (2 u)    10   u
    the node angle a = h15 + tc rounded (<= 184 deg: 3.2 u rad), deg2rad (3.2 u), cos a, sin a (2 u),
    cd * cos a, cd * sin a (1 u): 9.4 u in q and in r                                                   18.8 u
    r * c, the two fma                                                                                   3   u
                                                                                                  total 31.8 u
  clip0 changes no difference; the weights are positive and sum to 1, so a weighted mean of per-node errors is no
  larger.  The accumulation adds, per node, the rounding of w * value (together <= 1 u of the result, both sides: 2 u)
  and of the running sum (u times a partial sum <= the final value <= 1): N/2 u on each side for a linearly growing
  sum, N u for both.
      B(N) = (60.5 + 31.8 + 2 + N) u = (94.3 + N) * 2^-53:  1.06e-14 for one node, 5.3e-14 for 384 nodes (cap: 1e-13).
  The radiation multiplies every term by isr (one more rounding, inside the 2 u above): B(N) * max(isr).
For f32 input the product is judged against the reference's run on the upcast inputs with the same B; the integrated
functions return f32 there, one rounding of the result: B (1 + 2^-24) + 2^-24 |want|.
The restatement is exact to 1e-18, so the same B bounds |restatement - reference| and |product - restatement|."""
import datetime as dt
import functools
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solar_golden.npz")
F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
U = 2.0 ** -53
L = np.longdouble
PI = L("3.14159265358979323846264338327950288419716939937510582")
B_CAP = 1e-13
FUNCS = {"instant": "cos_solar_zenith_angle", "integrated": "cos_solar_zenith_angle_integrated", "toa": "toa_incident_solar_radiation"}


def bar(nnodes):
    b = (94.3 + nnodes) * U
    assert b <= B_CAP
    return b


def allowed(want, nnodes, scale=1.0, f32_result=False):
    """The absolute bound at every point of `want` (float64 values of the reference)."""
    b = bar(nnodes) * scale
    if not f32_result:
        return np.full(np.shape(want), b)
    return b * (1 + 2.0 ** -24) + 2.0 ** -24 * np.nan_to_num(np.abs(np.asarray(want, F64)), nan=0.0)


# ---- time nodes, from the description of the quadrature ----
def _year_fraction(date):
    start = dt.datetime(date.year, 1, 1, tzinfo=date.tzinfo if date.utcoffset() is not None else None)
    d = date - start
    return d.days + d.seconds / 86400.0


def _declination_tc(date):
    g = _year_fraction(date) / 365.25 * np.pi * 2
    c1, s1, c2, s2, c3, s3 = np.cos(g), np.sin(g), np.cos(2 * g), np.sin(2 * g), np.cos(3 * g), np.sin(3 * g)
    dec = float(0.396372 - 22.91327 * c1 + 4.025430 * s1 - 0.387205 * c2 + 0.051967 * s2 - 0.154527 * c3 + 0.084798 * s3)
    tc = float(0.004297 + 0.107029 * c1 - 1.837877 * s1 - 0.837378 * c2 - 2.340475 * s2)
    return dec, tc


def _radiation(date):
    return np.cos(_year_fraction(date) / 365.25 * np.pi * 2) * 165120.0 + 4892416.0


def _rule(order):
    if order == 1:
        return np.array([0.0]), np.array([2.0])
    if order == 2:
        r = np.sqrt(np.asarray(3.0))
        return np.array([-1.0 / r, 1.0 / r]), np.array([1.0, 1.0])
    if order == 3:
        r = np.sqrt(np.asarray(5.0 / 9.0))  # (the reference's abscissa, not sqrt(3/5))
        return np.array([-r, 0.0, r]), np.array([5.0 / 9.0, 8.0 / 9.0, 5.0 / 9.0])
    if order == 4:
        a, b = np.sqrt(np.asarray(6.0 / 5.0)), np.sqrt(np.asarray(30))
        hi, lo = np.sqrt(3.0 / 7.0 + 2.0 / 7.0 * a), np.sqrt(3.0 / 7.0 - 2.0 / 7.0 * a)
        return np.array([-hi, -lo, lo, hi]), np.array([(18 - b) / 36, (18 + b) / 36, (18 + b) / 36, (18 - b) / 36])
    raise ValueError(order)


def nodes(begin, end, intervals_per_hour=1, integration_order=3, radiation=False):
    """dict of float64 vectors sd, cd, h15, tc, w, isr, and the node dates."""
    absc, wts = _rule(integration_order)
    assert intervals_per_hour > 0 and end > begin
    hours = (end - begin).total_seconds() / 3600.0
    pieces = int(hours * intervals_per_hour + 0.5)
    assert pieces > 0
    edges = np.linspace(0, hours, num=pieces + 1)
    dates, w = [], []
    for lo, hi in zip(edges[:-1], edges[1:]):
        half = (hi - lo) / 2.0
        wk = half * wts
        wk /= hours
        tk = half * absc
        tk += (hi + lo) / 2.0
        dates += [begin + dt.timedelta(hours=float(t)) for t in tk]
        w += list(wk)
    return instant_nodes(dates, np.array(w), radiation)


def instant_nodes(dates, w=None, radiation=False):
    dec_tc = [_declination_tc(d) for d in dates]
    dec = np.deg2rad(np.array([x[0] for x in dec_tc]))
    return dict(sd=np.sin(dec), cd=np.cos(dec), h15=np.array([(d.hour - 12) * 15.0 for d in dates]),
                tc=np.array([x[1] for x in dec_tc]), w=np.ones(len(dates)) if w is None else np.asarray(w, F64),
                isr=np.array([_radiation(d) if radiation else 1.0 for d in dates]), dates=dates)


def evaluate(rec, lat, lon):
    """The sum over the nodes of `rec` at broadcast(lat, lon), in extended precision, returned as float64."""
    lat, lon = np.broadcast_arrays(np.asarray(lat).astype(L), np.asarray(lon).astype(L))
    with np.errstate(all="ignore"):
        latr = lat * (PI / 180)
        slat, clat = np.sin(latr), np.cos(latr)
        acc = np.zeros(lat.shape, L)
        for k in range(len(rec["w"])):
            ang = np.fmod(np.fmod(lon, L(360)) + (L(rec["h15"][k]) + L(rec["tc"][k])), L(360)) * (PI / 180)
            z = L(rec["sd"][k]) * slat + L(rec["cd"][k]) * clat * np.cos(ang)
            z = np.where(z < 0, L(0), z)
            acc = acc + L(rec["w"][k]) * (L(rec["isr"][k]) * z)
    return acc.astype(F64)


def call(func, dates, lat, lon, **kwargs):
    """The restatement of one public call; float64 values (the result dtype is not restated)."""
    if func == "instant":
        return evaluate(instant_nodes(list(dates)), lat, lon)
    rec = nodes(dates[0], dates[1], radiation=func == "toa", **kwargs)
    lat = np.asarray(lat)
    return evaluate(rec, lat, np.broadcast_to(np.asarray(lon), lat.shape))


# ---- goldens ----
@functools.lru_cache(maxsize=None)
def _load():
    with np.load(PATH) as z:
        data = {k: z[k] for k in z.files}
    index = json.loads(bytes(data.pop("index")).decode())
    return index, data


def index():
    return _load()[0]


def array(key):
    return _load()[1][key]


def cases():
    return _load()[0]["cases"]


def dates_of(case):
    return [dt.datetime.fromisoformat(s) for s in case["dates"]]


def inputs_of(case):
    if case["lat"] is None:
        return case["lat_value"], case["lon_value"]
    return array(case["lat"]).copy(), array(case["lon"]).copy()


def expected_of(case):
    return array("out." + case["id"])


def is_f32(case):
    return case["lat"] is not None and array(case["lat"]).dtype == F32


def judged_against(case):
    """What the product is held to: the reference's output, for f32 input its run on the upcast inputs."""
    return array("out." + case["id"] + ".up") if is_f32(case) else expected_of(case)


def nnodes_of(case):
    if case["func"] == "instant":
        return 1
    kw = case["kwargs"]
    key = next(k for k, v in index()["nodesets"].items()
               if v["begin"] == case["dates"][0] and v["end"] == case["dates"][1]
               and v["kwargs"] == dict(intervals_per_hour=kw.get("intervals_per_hour", 1), integration_order=kw.get("integration_order", 3)))
    return len(index()["nodesets"][key]["dates"])


def scale_of(case):
    """max(isr) over the case's nodes for the radiation, else 1."""
    if case["func"] != "toa":
        return 1.0
    kw = case["kwargs"]
    for k, v in index()["nodesets"].items():
        if v["begin"] == case["dates"][0] and v["end"] == case["dates"][1] and v["kwargs"] == dict(
                intervals_per_hour=kw.get("intervals_per_hour", 1), integration_order=kw.get("integration_order", 3)):
            return float(array(f"nodes.{k}.isr").max())
    raise KeyError(case["id"])


class Mismatch(AssertionError):
    pass


LEDGER_KIND = "solar absolute bar B(N) (tests/_solar_numpy.py)"


def judge(got, want, bound, what, ledger=None):
    """|got - want| <= bound at every point, the same NaN pattern, no point excluded; the sign of zero is not compared.
    Returns the largest used fraction of the bound."""
    got64, want64 = np.asarray(got, F64), np.asarray(want, F64)
    if got64.shape != want64.shape:
        raise Mismatch(f"{what}: shape {got64.shape} != {want64.shape}")
    if not np.array_equal(np.isnan(got64), np.isnan(want64)):
        i = np.flatnonzero(np.isnan(got64).ravel() != np.isnan(want64).ravel())[:4]
        raise Mismatch(f"{what}: NaN pattern differs at {i}: got {got64.ravel()[i]}, want {want64.ravel()[i]}")
    with np.errstate(all="ignore"):
        err = np.where(np.isnan(want64), 0.0, np.abs(got64 - want64))
    bound = np.broadcast_to(np.asarray(bound, F64), err.shape)
    used = float(np.max(err / bound, initial=0.0))
    if ledger is not None:
        ledger.append((what, LEDGER_KIND, used, 1.0, err.size))
    if not (err <= bound).all():
        i = int(np.argmax(err / bound))
        raise Mismatch(f"{what}: |{got64.ravel()[i]!r} - {want64.ravel()[i]!r}| = {err.ravel()[i]:.3e} > {bound.ravel()[i]:.3e} at {i}")
    return used


def judge_case(case, got, what, ledger=None):
    """A result of the product (or of the host twin) for a recorded case: type, dtype, shape, then the bar."""
    want = expected_of(case)
    if np.asarray(got).dtype != want.dtype or np.shape(got) != want.shape:
        raise Mismatch(f"{what}: {np.asarray(got).dtype}{np.shape(got)} for the reference's {want.dtype}{want.shape}")
    ref = judged_against(case)
    n = nnodes_of(case)
    bound = allowed(ref, n, scale_of(case), f32_result=want.dtype == F32)
    return judge(got, ref, bound, what, ledger)
