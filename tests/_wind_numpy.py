"""`wind` for the tests: a NumPy restatement of the reference's functions (wind/array/wind.py:15-189, :225-328), the
goldens recorded from the reference (tests/golden/wind_polar_golden.npz) and the judges.

The restatement follows the reference operation for operation in the input's dtype, so against the goldens it is held
bit for bit (tests/test_wind_cpu.py); the census of tests/test_gpu_wind.py uses it where nothing is recorded.

THE BARS.  eps is np.finfo(dtype).eps, so one rounding of a value x costs at most eps/2 |x| and "1 ulp" at most eps |x|.
E = eps of float64, e = eps of float32.  Float64 (and integer or mixed) input is computed in double.  float32 fields are
computed in FLOAT arithmetic (csrc/wind_point.hpp); such a result is judged against the reference's float64 run on the
upcast inputs (recorded as `.up`), and its bar is the float64 bar -- the reference's side -- plus the float kernel's own
terms in e, derived below.

speed (relative): the product squares (E/2), adds by fma (E/2), takes the root (halves the 1 E so far, adds E/2): 1 E;
    the scaling by powers of two is exact but for a denormal result (one more rounding: the smallest denormal, absolute).
    The reference's hypot is within 1 ulp: 1 E.  c = 2:  |got - want| <= 2 E |want| + tiny.
    float32: the same three roundings in float, 1 e:  + 1 e |want|.
direction (absolute, degrees, on the circular distance): with d = atan2(v, u), |d| <= pi,
    product: atan2 within 3 ulp of d (csrc/wind_point.hpp: division E/2 on |t| <= 7/16, one rounded denominator E/2,
    polynomial and table 1 ulp, two roundings undoing the octant: measured 2 ulp against libm) = 3 E pi rad = 1.5 E 360;
    the subtraction from 1.5 pi (or the +360) rounds a value up to 2 pi: E/2 360; the product with 180/pi: E/2 360.
    reference: atan2 1 ulp = 0.5 E 360; the same two roundings: E 360.
    c = 2.5 + 1.5 = 4:  dist <= 4 E 360.
    float32: the same count in float (atan2 3 ulp = 1.5 e 360, measured 1 ulp; subtraction e/2 360; product e/2 360) and
    the constants rounded to float: 1.5 pi by at most half an ulp of 4.71 = 2.4e-7 rad = 0.32 e 360, 180/pi by e/2
    relative = 0.5 e 360; 3.32, taken as 3.5:  + 3.5 e 360.
polar_to_xy (absolute): a = the angle in radians, m the magnitude.  The angle 270 - direction is the same IEEE operation
    on the same operands on both sides; the reference then multiplies by pi/180 (E/2 |a|, and the constant's own rounding
    E/2 |a|) and the issue's form allows 1.5 |a| for the angle; cos / sin are 1-Lipschitz, so that is an absolute error
    of the factor.  The reference's cos / sin: 1 ulp <= E; its product: E/2.  The product's own sine / cosine (exact
    reduction in degrees, csrc/solar_point.hpp): 1 ulp <= E; its product: E/2.
    c = 3:  |got - want| <= (3 + 1.5 |a|) E |m|.
    float32: 270 - direction in float rounds the angle, e/2 |a|; the float sine / cosine (exact reduction, float-float
    argument, truncation 0.03 ulp, evaluation and final rounding) 1.5 ulp <= 1.5 e; the product e/2:
    + (2 + 0.5 |a|) e |m|.
coriolis (absolute): the same with m = 2 Omega (the doubling is exact) and a = lat in radians:
    |got - want| <= (3 + 1.5 |a|) E 2 Omega.
    float32: no angle term (the latitude is reduced exactly); sine 1.5 e, 2 Omega rounded to float e/2, product e/2:
    + 2.5 e 2 Omega.
No bar may exceed the project's parity bars, 1e-6 (float64) and 1e-4 (float32) of 360 degrees, |m| or 2 Omega at
|a| <= 100 rad (15 turns; the angle term grows with |a| on both sides): `bar_*` assert it.

A circular match of a direction that is not a plain match (0 against 360) is accepted only where v < 0 and
|u| <= 4 eps |v| (eps of the result's dtype), the neighbourhood of the branch point of the meteorological direction;
anywhere else it is a mismatch.  The NaN pattern must be identical and an infinity the same infinity, except that for
polar_to_xy beside an infinite magnitude NaN and +-inf are not told apart (the exact zeros of the degree
reduction); the non-finite pattern is the reference's everywhere.
The wind rose -- counts, percentages and direction bins -- is compared bit for bit."""
import functools
import json
import os

import numpy as np

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
E64, E32 = float(np.finfo(np.float64).eps), float(np.finfo(np.float32).eps)
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wind_polar_golden.npz")
DEGREE = 180.0 / np.pi
RADIAN = 1.0 / DEGREE
TWO_OMEGA = 2 * 7.292115083046062e-05  # recorded in the goldens' index and checked there (test_wind_cpu.py)
C_SPEED, C_DIRECTION, C_XY = 2.0, 4.0, 3.0
C32_SPEED, C32_DIRECTION, C32_XY, C32_CORIOLIS = 1.0, 3.5, 2.0, 2.5  # the float32 kernels' own terms, in eps32
TILE = {"f32": 1024, "f64": 512}  # points per workgroup of the all-fields kernel: 256 lanes x 16 B


# ---- restatement ----
def speed(u, v):
    return np.hypot(np.asarray(u), np.asarray(v))


def direction(u, v, convention="meteo", to_positive=True):
    u, v = np.asarray(u), np.asarray(v)
    if convention == "meteo":
        minus_pi2 = -np.pi / 2.0
        d = np.asarray(np.arctan2(v, u))
        m = d <= minus_pi2
        d[m] = (minus_pi2 - d[m]) * DEGREE
        m = ~m
        d[m] = (1.5 * np.pi - d[m]) * DEGREE
        return d
    if convention == "polar":
        d = np.arctan2(v, u) * DEGREE
        if to_positive:
            d = np.asarray(d)
            m = d < 0
            d[m] = 360.0 + d[m]
        return d
    raise ValueError(f"direction(): invalid convention={convention}!")


def xy_to_polar(x, y, convention="meteo"):
    return speed(x, y), direction(x, y, convention=convention)


def polar_to_xy(magnitude, direction, convention="meteo"):
    magnitude, direction = np.asarray(magnitude), np.asarray(direction)
    if convention == "meteo":
        a = (270.0 - direction) * RADIAN
    elif convention == "polar":
        a = direction * RADIAN
    else:
        raise ValueError(f"polar_to_xy(): invalid convention={convention}!")
    return magnitude * np.cos(a), magnitude * np.sin(a)


def coriolis(lat):
    return TWO_OMEGA * np.sin(np.asarray(lat) * RADIAN)


def rose_edges(speed_dtype, sectors, speed_bins):
    step = 360.0 / sectors
    return (np.asarray(speed_bins, dtype=speed_dtype),
            np.linspace(int(-step / 2), int(360 + step / 2), int(360 / step) + 2, dtype=speed_dtype))


def _bin_of(x, edges):
    """np.histogramdd's rule: searchsorted on the right, the last edge joins the last bin; 0 and len(edges) are outside."""
    k = np.searchsorted(edges, x, side="right")
    k[x == edges[-1]] -= 1
    return k


def windrose(speed, direction, sectors=16, speed_bins=None, percent=True):
    """The reference's windrose without np.histogram2d: the bin rule above and a bincount."""
    speed_bins = speed_bins if speed_bins is not None else []
    if len(speed_bins) < 2:
        raise ValueError("windrose(): speed_bins must have at least 2 elements!")
    sectors = int(sectors)
    if sectors < 1:
        raise ValueError("windrose(): sectors must be greater than 1!")
    sp, di = np.atleast_1d(speed), np.atleast_1d(direction)
    if sp.ndim != 1 or di.ndim != 1 or sp.shape != di.shape:
        raise ValueError("windrose(): one-dimensional samples of one length")
    se, de = rose_edges(sp.dtype, sectors, speed_bins)
    for e in (se, de):
        if np.any(e[:-1] > e[1:]):
            raise ValueError("bins must be monotonically increasing")
    ks, kd = _bin_of(sp, se), _bin_of(di, de)
    ok = (ks >= 1) & (ks <= len(se) - 1) & (kd >= 1) & (kd <= len(de) - 1)
    rows, cols = len(se) - 1, len(de) - 1
    res = np.bincount((ks[ok] - 1) * cols + (kd[ok] - 1), minlength=rows * cols).reshape(rows, cols).astype(F64)
    res[:, 0] = res[:, 0] + res[:, -1]
    res = res[:, :-1]
    with np.errstate(all="ignore"):
        return ((res * 100.0 / res.sum()) if percent else res), de[:-1]


FUNCS = {"speed": speed, "direction": direction, "xy_to_polar": xy_to_polar, "polar_to_xy": polar_to_xy, "coriolis": coriolis,
         "windrose": windrose}


# ---- goldens ----
@functools.lru_cache(maxsize=None)
def _load():
    with np.load(PATH) as z:
        data = {k: z[k] for k in z.files}
    index = json.loads(bytes(data.pop("index")).decode())
    arrays = {}
    for key, (dt, offset, shape) in index["arrays"].items():  # one blob per dtype: (dtype, offset, shape)
        n = int(np.prod(shape, dtype=np.int64))
        arrays[key] = data["blob" + dt][offset:offset + n].reshape(shape)
    return index, arrays


def index():
    return _load()[0]


def array(key):
    return _load()[1][key]


def cases(kind="elementwise"):
    return [c for c in _load()[0]["cases"] if (c["func"] == "windrose") == (kind == "windrose")]


def cast_inputs(arrays, tag):
    """The inputs of a case from the float64 (or integer) arrays of its set: f64 as stored, f32 cast, mixed = float32
    first operand beside a float64 second, scalar = Python floats of element 0, int as stored."""
    if tag == "f32":
        return [a.astype(F32) for a in arrays]
    if tag == "mixed":
        return [a.astype(F32) if k == 0 else a.copy() for k, a in enumerate(arrays)]
    if tag == "scalar":
        return [float(a.ravel()[0]) for a in arrays]
    return [a.copy() for a in arrays]


def inputs_of(case):
    names = "ab"[:case["nin"]]
    return cast_inputs([array(f"in.{case['set']}.{n}") for n in names], case["tag"])


def expected_of(case, up=False):
    return [array(f"out.{case['id']}.{k}" + (".up" if up else "")) for k in range(case["nout"])]


def judged_against(case):
    return expected_of(case, up=case["tag"] == "f32")


N_CENSUS = 1 << 16


def census_inputs(T, get=None):
    """(u, v, magnitude, direction) of the 65 536-point census, seeded with the goldens' specials, the branch
    neighbourhood and the huge / tiny pairs.  `get(key)` reads an input set (default: the recorded file)."""
    get = array if get is None else get
    rng = np.random.default_rng(41)
    u, v = rng.normal(0, 15, N_CENSUS), rng.normal(0, 15, N_CENSUS)
    k = 0
    for s in ("uvspecial", "uvbranch", "uvhuge", "uvknown"):
        a, b = np.asarray(get(f"in.{s}.a"), F64).ravel(), np.asarray(get(f"in.{s}.b"), F64).ravel()
        u[k:k + a.size], v[k:k + a.size] = a, b
        k += a.size
    m, d = rng.uniform(0, 80, N_CENSUS), rng.uniform(-720, 1080, N_CENSUS)
    a, b = np.asarray(get("in.mdspecial.a"), F64), np.asarray(get("in.mdspecial.b"), F64)
    m[:a.size], d[:a.size] = a, b
    with np.errstate(all="ignore"):
        return [x.astype(T) for x in (u, v, m, d)]


# ---- judges ----
class Mismatch(AssertionError):
    pass


def _eps_out(dtype):
    return E32 if np.dtype(dtype) == F32 else E64


def _is32(dtype):
    return np.dtype(dtype) == F32


def _capped(rel, dtype):
    assert np.all(rel <= (1e-4 if _is32(dtype) else 1e-6)), "a derived bar above the project's parity bar"
    return rel


def bar_speed(want, dtype):
    rel = _capped(C_SPEED * E64 + (C32_SPEED * E32 if _is32(dtype) else 0.0), dtype)
    tiny = float(np.finfo(np.dtype(dtype)).smallest_subnormal)
    return rel * np.abs(np.asarray(want, F64)) + tiny


def bar_direction(dtype):
    return float(_capped(C_DIRECTION * E64 + (C32_DIRECTION * E32 if _is32(dtype) else 0.0), dtype)) * 360.0


def bar_xy(scale, a_rad, dtype, c32=None):
    """c32: the float32 constant, C32_XY (default) or C32_CORIOLIS; the float32 angle term is 0.5 |a| for polar_to_xy
    (the float subtraction 270 - direction) and none for coriolis."""
    a = np.abs(np.asarray(a_rad, F64))
    c32 = C32_XY if c32 is None else c32
    with np.errstate(all="ignore"):
        rel = (C_XY + 1.5 * a) * E64
        if _is32(dtype):
            rel = rel + (c32 + (0.5 * a if c32 == C32_XY else 0.0)) * E32
        _capped(rel[np.isfinite(a) & (a <= 100.0)], dtype)
        tiny = float(np.finfo(np.dtype(dtype)).smallest_subnormal)
        return rel * np.abs(np.asarray(scale, F64)) + tiny


def _same_nan(got, want, what, loose=None):
    g, w = np.isnan(got), np.isnan(want)
    if loose is not None:  # only the non-finite pattern where `loose`
        g = np.where(loose, ~np.isfinite(got), g)
        w = np.where(loose, ~np.isfinite(want), w)
    if not np.array_equal(g, w):
        i = np.flatnonzero(g.ravel() != w.ravel())[:4]
        raise Mismatch(f"{what}: NaN pattern differs at {i}: got {got.ravel()[i]}, want {want.ravel()[i]}")


def _shapes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        raise Mismatch(f"{what}: shape {got.shape} != {want.shape}")
    with np.errstate(all="ignore"):
        w = want.astype(got.dtype) if got.dtype in (F32, F64) else want  # (a float64 reference of a float32 result may overflow to inf)
    return got.astype(F64), want.astype(F64), np.asarray(got == w)


def _verdict(err, bound, what, ledger, kind, got, want):
    bound = np.broadcast_to(np.asarray(bound, F64), err.shape)
    with np.errstate(all="ignore"):
        frac = np.where(err == 0, 0.0, err / bound)
    used = float(np.max(frac, initial=0.0))
    if ledger is not None:
        ledger.append((what, kind, used, 1.0, err.size))
    if not ((err == 0) | (err <= bound)).all():  # (err is 0 where both are the same infinity or NaN, whatever the bound)
        i = int(np.nanargmax(np.where((err == 0) | (err <= bound), 0.0, np.inf)))
        raise Mismatch(f"{what}: |{got.ravel()[i]!r} - {want.ravel()[i]!r}| = {err.ravel()[i]:.3e} > {bound.ravel()[i]:.3e} at {i}")
    return used


def judge_speed(got, want, what, ledger=None):
    g, w, same = _shapes(got, want, what)
    _same_nan(g, w, what)
    with np.errstate(all="ignore"):
        err = np.where(same | np.isnan(w), 0.0, np.abs(g - w))
    return _verdict(err, bar_speed(w, np.asarray(got).dtype), what, ledger, "wind speed: 2 eps relative (tests/_wind_numpy.py)", g, w)


def judge_direction(got, want, u, v, what, ledger=None):
    dtype = np.asarray(got).dtype
    g, w, same = _shapes(got, want, what)
    _same_nan(g, w, what)
    u, v = np.broadcast_to(np.asarray(u, F64), g.shape), np.broadcast_to(np.asarray(v, F64), g.shape)
    with np.errstate(all="ignore"):
        plain = np.where(same | np.isnan(w), 0.0, np.abs(g - w))
        wrapped = np.abs(360.0 - plain)
        at_branch = (v < 0) & (np.abs(u) <= 4 * _eps_out(dtype) * np.abs(v))
        err = np.where(at_branch, np.minimum(plain, wrapped), plain)
    return _verdict(err, bar_direction(dtype), what, ledger, "wind direction: 4 eps 360 circular (tests/_wind_numpy.py)", g, w)


def judge_xy(got, want, magnitude, a_rad, what, ledger=None, scale=None, c32=None):
    g, w, same = _shapes(got, want, what)
    with np.errstate(all="ignore"):
        wc = np.asarray(want).astype(np.asarray(got).dtype).astype(F64)  # the reference in the result's dtype: its overflow is the result's
    m = np.broadcast_to(np.asarray(magnitude, F64), g.shape)
    # the non-finite pattern is the reference's everywhere; NaN against +-inf is let through only beside an infinite
    # magnitude, anywhere else NaN matches NaN and an infinity the same infinity
    bad = np.isfinite(g) != np.isfinite(wc)
    strict = ~np.isinf(m) & ~np.isfinite(wc)
    bad |= strict & ~((np.isnan(g) & np.isnan(wc)) | (g == wc))
    if bad.any():
        i = np.flatnonzero(bad.ravel())[:4]
        raise Mismatch(f"{what}: non-finite pattern differs at {i}: got {g.ravel()[i]}, want {wc.ravel()[i]}")
    with np.errstate(all="ignore"):
        err = np.where(same | ~np.isfinite(wc), 0.0, np.abs(g - w))
    bound = bar_xy(m if scale is None else scale, np.broadcast_to(np.asarray(a_rad, F64), g.shape), np.asarray(got).dtype, c32)
    return _verdict(err, bound, what, ledger, "wind polar_to_xy / coriolis: (3 + 1.5 |a|) eps |m| (tests/_wind_numpy.py)", g, w)


def angle_of(direction, convention):
    d = np.asarray(direction, F64)
    return (270.0 - d) * RADIAN if convention == "meteo" else d * RADIAN


def judge_call(func, kwargs, inputs, got, want, what, ledger=None):
    """The results `got` (a tuple) of one call of an elementwise function against the reference's `want`."""
    got = got if isinstance(got, tuple) else (got,)
    if len(got) != len(want):
        raise Mismatch(f"{what}: {len(got)} results for {len(want)}")
    used = 0.0
    if func in ("speed", "xy_to_polar"):
        used = max(used, judge_speed(got[0], want[0], what + " speed", ledger))
    if func in ("direction", "xy_to_polar"):
        used = max(used, judge_direction(got[-1], want[-1], inputs[0], inputs[1], what + " direction", ledger))
    if func == "polar_to_xy":
        a = angle_of(inputs[1], kwargs.get("convention", "meteo"))
        for k, name in enumerate("xy"):
            used = max(used, judge_xy(got[k], want[k], inputs[0], a, f"{what} {name}", ledger))
    if func == "coriolis":
        a = np.asarray(inputs[0], F64) * RADIAN
        used = max(used, judge_xy(got[0], want[0], np.ones_like(a), a, what, ledger, scale=TWO_OMEGA, c32=C32_CORIOLIS))
    return used


def judge_case(case, got, what, ledger=None):
    """A result of the product (or of the host twin) for a recorded case: count, dtype and shape, then the bars."""
    got = got if isinstance(got, tuple) else (got,)
    want = expected_of(case)
    for g, w in zip(got, want):
        if np.asarray(g).dtype != w.dtype or np.shape(g) != w.shape:
            raise Mismatch(f"{what}: {np.asarray(g).dtype}{np.shape(g)} for the reference's {w.dtype}{w.shape}")
    return judge_call(case["func"], case["kwargs"], inputs_of(case), got, judged_against(case), what, ledger)


def judge_rose(got, want, what):
    """Counts (or percentages) and direction bins bit for bit, dtype and shape included."""
    for name, g, w in zip(("res", "dir_bins"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        if g.dtype != w.dtype or g.shape != w.shape:
            raise Mismatch(f"{what} {name}: {g.dtype}{g.shape} for the reference's {w.dtype}{w.shape}")
        if g.tobytes() != w.tobytes() and not np.array_equal(g, w, equal_nan=True):
            i = np.flatnonzero(~((g == w) | (np.isnan(g) & np.isnan(w))).ravel())[:4]
            raise Mismatch(f"{what} {name}: differs at {i}: got {g.ravel()[i]}, want {w.ravel()[i]}")
        if not np.array_equal(g, w, equal_nan=True):
            raise Mismatch(f"{what} {name}: differs")
