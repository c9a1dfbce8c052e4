"""Access to tests/golden/interp_golden.npz (recorded by tests/golden/gen_golden_interp.py) and the judge the
interpolation tests share -- TEST INFRASTRUCTURE."""
import functools
import json
import os

import numpy as np

import _interp_numpy as inp

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "interp_golden.npz")
EPS = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}  # unit roundoff


@functools.lru_cache(maxsize=1)
def _load():
    with np.load(PATH) as f:
        meta = json.loads(bytes(f["manifest"]).decode())
        arrays = {k: f[k] for k in f.files if k != "manifest"}
    return meta, arrays


def signatures():
    return _load()[0]["signatures"]


def cases(func=None):
    meta, _ = _load()
    return [c for c in meta["cases"] if func is None or c["func"] == func]


def kwargs_of(case):
    _, arrays = _load()
    kw = dict(case["plain"])
    kw.update({k: arrays[key] for k, key in case["arrays"].items()})
    return kw


def expected_of(case):
    return _load()[1][case["out"]]


def case_id(case):
    return f"{case['id']}-{case['note'].replace(' ', '_')}"


def mode_of(case):
    return case["plain"].get("interpolation", "linear")


class Mismatch(AssertionError):
    pass


def judge_exact(got, want, what=""):
    """dtype, shape, NaN positions and every other value bit for bit."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        raise Mismatch(f"{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}")
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        raise Mismatch(f"{what}: NaN pattern differs at {int(np.sum(np.isnan(got) != np.isnan(want)))} points")
    ok = np.isnan(want) | (got == want)
    if not ok.all():
        i = np.flatnonzero(~ok.reshape(-1))[0]
        raise Mismatch(f"{what}: {int((~ok).sum())} of {ok.size} values differ, first {got.reshape(-1)[i]!r} against {want.reshape(-1)[i]!r}")


# `log` mode: rounded operations between the inputs and the result, in units of the unit roundoff u of the arithmetic
# dtype.  The weight is f = (L(tc) - L(cb)) / (L(ct) - L(cb)) with L = log: each of the three logarithms carries the
# error of its implementation -- the device's log is specified to 1 ulp = 2u (fp32: OCML's documented accuracy of logf;
# fp64: log, 1 ulp), NumPy's libm log to 1 ulp = 2u as well -- so one side's numerator and denominator are each off by
# at most 2u(|L(tc)| + |L(cb)|) + u|num| resp. 2u(|L(ct)| + |L(cb)|) + u|den| (two logarithms and one rounded
# subtraction), and the quotient adds u|f|.  With |f| <= 1 inside a bracket, |df| <= [2u(|L(tc)| + |L(ct)| + 2|L(cb)|)
# + 3u|den|] / |den| per side; with S = |L(tc)| + |L(cb)| + |L(ct)| (so |L(tc)| + |L(ct)| + 2|L(cb)| <= 2 S) that is
# |df| <= (4 S / |den| + 3) u per side, (8 S / |den| + 6) u between the two sides.  The blend (1 - f) db + f dt
# = db + f (dt - db) moves by |df| |dt - db|, plus four rounded operations on terms no larger than max(|dt|, |db|)
# per side.  Hence  |got - want| <= 8 u S / |den| |dt - db| + (6 |dt - db| + 8 max(|dt|, |db|)) u
#                                <= C u S / |den| |dt - db| + C u max(|dt|, |db|)   with C = 20
# (6 |dt - db| <= 12 max: 12 + 8 = 20 covers the second term, and 20 >= 8 the first).
LOG_C = 20.0


def log_bound(tc, c_b, c_t, d_b, d_t, dtype):
    u = EPS[np.dtype(dtype)]
    with np.errstate(all="ignore"):
        ltc, lb, lt = (np.abs(np.log(np.asarray(x, np.float64))) for x in (tc, c_b, c_t))
        den = np.abs(np.log(np.asarray(c_t, np.float64)) - np.log(np.asarray(c_b, np.float64)))
        dd = np.abs(np.asarray(d_t, np.float64) - np.asarray(d_b, np.float64))
        return LOG_C * u * (ltc + lb + lt) / den * dd + LOG_C * u * np.maximum(np.abs(d_t), np.abs(d_b)).astype(np.float64)


def judge_log(got, want, bound, what="", ledger=None):
    """`log` mode: dtype, shape and NaN pattern exactly; |got - want| <= bound where both are finite, equal where the
    reference is infinite.  Logs used / allowed (the largest ratio) to the ledger."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        raise Mismatch(f"{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}")
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        raise Mismatch(f"{what}: NaN pattern differs at {int(np.sum(np.isnan(got) != np.isnan(want)))} points")
    fin = np.isfinite(want)
    if not np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]):
        raise Mismatch(f"{what}: infinities differ")
    err = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
    lim = np.broadcast_to(bound, want.shape)[fin]
    with np.errstate(all="ignore"):
        ratio = np.where(err == 0, 0.0, err / lim)
    worst = float(ratio.max()) if ratio.size else 0.0
    if ledger is not None:
        ledger.append((what, "interp log: worst used/allowed in 1e-6", int(round(worst * 1e6)), 1e6, int(fin.sum())))
    if not (worst <= 1.0):
        raise Mismatch(f"{what}: log-mode error {worst:.3g} x the derived bound")
    return worst


def bracket_terms(case, T, kw=None):
    """tc, c_b, c_t, d_b, d_t of every output point of a monotonic / hybrid->pressure golden case (level axis first,
    shaped like the expected output moved to axis 0), from the NumPy restatement's bracket: what log_bound needs.
    `kw`: the call's arguments when they are not the recorded ones."""
    kw = kwargs_of(case) if kw is None else kw
    if case["func"] == "interpolate_pressure_to_height_levels":
        h = inp.height_from_geopotential(kw["z"], kw["zs"], kw.get("h_type", "geometric"), kw.get("h_reference", "ground"))
        kw = dict(data=kw["data"], coord=h, target_coord=kw["target_h"], aux_min_level_data=kw.get("aux_bottom_data"),
                  aux_min_level_coord=kw.get("aux_bottom_h"), aux_max_level_data=kw.get("aux_top_data"),
                  aux_max_level_coord=kw.get("aux_top_h"), vertical_axis=kw.get("vertical_axis", 0))
    ax = kw.get("vertical_axis", 0)
    if case["func"] == "interpolate_hybrid_to_pressure_levels":
        data, target = np.asarray(kw["data"]), np.atleast_1d(kw["target_p"])
        if ax:
            data, target = (np.moveaxis(x, ax, 0) if x.ndim > 1 else x for x in (data, target))
        coord = inp.hybrid_pressure(kw["A"], kw["B"], np.broadcast_to(kw["sp"], data.shape[1:]), data.shape[0], T)
        aux_min, aux_max = (kw.get("aux_top_data"), kw.get("aux_top_p")), (kw.get("aux_bottom_data"), kw.get("aux_bottom_p"))
    else:
        data, coord, target = np.asarray(kw["data"]), np.atleast_1d(kw["coord"]), np.atleast_1d(kw["target_coord"])
        if ax:
            data, coord, target = (np.moveaxis(x, ax, 0) if x.ndim > 1 else x for x in (data, coord, target))
        aux_min = (kw.get("aux_min_level_data"), kw.get("aux_min_level_coord"))
        aux_max = (kw.get("aux_max_level_data"), kw.get("aux_max_level_coord"))
        if coord.shape != data.shape:
            aux_min = aux_max = (None, None)
    nlev, cols = data.shape[0], data.shape[1:]
    n = int(np.prod(cols, dtype=np.int64))
    d = data.reshape(nlev, n).astype(T)
    c = np.broadcast_to(coord.reshape(nlev, -1), (nlev, n)).astype(T)
    if c[0, 0] < c[-1, 0]:
        d, c = d[::-1], c[::-1]
    tc = np.broadcast_to(target.reshape(target.shape[0], -1), (target.shape[0], n)).astype(T)
    idx = inp._place_searchsorted(c, tc)
    top = np.clip(idx, 1, nlev - 1)
    g = lambda a, i: np.take_along_axis(a, i, axis=0)  # noqa: E731
    c_b, c_t, d_b, d_t = g(c, top - 1), g(c, top), g(d, top - 1), g(d, top)
    for outside, side, aux in ((idx == 0, 0, aux_max), (idx == nlev, -1, aux_min)):
        if aux[0] is None or aux[1] is None:
            continue  # no blend outside the column without an aux layer
        ad = np.broadcast_to(np.broadcast_to(np.asarray(aux[0], T), cols if np.size(aux[0]) != 1 else (1,)).reshape(-1), tc.shape)
        ac = np.broadcast_to(np.broadcast_to(np.asarray(aux[1], T), cols if np.size(aux[1]) != 1 else (1,)).reshape(-1), tc.shape)
        ce, de = np.broadcast_to(c[side], tc.shape), np.broadcast_to(d[side], tc.shape)
        if side == 0:
            c_b, c_t, d_b, d_t = (np.where(outside, x, y) for x, y in ((ac, c_b), (ce, c_t), (ad, d_b), (de, d_t)))
        else:
            c_b, c_t, d_b, d_t = (np.where(outside, x, y) for x, y in ((ce, c_b), (ac, c_t), (de, d_b), (ad, d_t)))
    shape = (target.shape[0],) + cols
    return tuple(x.reshape(shape) for x in (tc, c_b, c_t, d_b, d_t))


def judge_case(case, got, what, ledger=None):
    """A golden case through any implementation: linear / nearest bit for bit, log under the derived bound."""
    want = expected_of(case)
    if mode_of(case) != "log":
        return judge_exact(got, want, what)
    kw = kwargs_of(case)
    T = inp.arith_dtype(*[v for v in kw.values() if isinstance(v, np.ndarray)])  # every array of a case has the case's dtype
    ax = kw.get("vertical_axis", 0)
    mv = (lambda x: np.moveaxis(x, ax, 0)) if ax and np.ndim(want) > 1 else (lambda x: x)
    bound = log_bound(*bracket_terms(case, T), T)
    return judge_log(mv(np.asarray(got)), mv(want), bound.reshape(mv(want).shape), what, ledger)


def inp_mode(case):
    return {"linear": 0, "log": 1, "nearest": 2}[mode_of(case)]
