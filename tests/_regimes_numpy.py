"""An independent NumPy restatement of regimes.project, regimes.regime_index and score.pearson_correlation, their
judges, and access to tests/golden/regimes_golden.npz -- TEST INFRASTRUCTURE.

The restatement
  project        C[p] = pattern_p * (weights / weights.sum()) and field @ C.T in the call's dtype (f32 only when field,
                 patterns, modulator and weights are all f32), then the modulator of the field times the sum;
  regime_index   (projection - mean) / std with NumPy's own promotion;
  pearson        along the sample axis moved to the front, ONE ROW AFTER THE OTHER in the call's dtype: mean = (x0 + x1 +
                 ...) / m, centre, norm = sqrt(xc0^2 + xc1^2 + ...), (xc / norm) * (yc / norm) summed in order.  This is
                 what NumPy does when the sample axis is not the contiguous one.

The bars (none is fitted to a result; each judge prints, and files in the ledger, the largest share of its bar used):

  project: |got - exact| <= (K + 4) eps sum_k |f_k p_k w_k|  (+ eps |exact| for ModulatedPatterns), eps the machine
    epsilon of the result's dtype, K the grid points of a pattern, `exact` the sum in numpy.longdouble of the inputs
    widened (w the normalised weights as NumPy forms them in their own dtype, p the modulated pattern).  Every term
    carries at most three roundings before it enters the sum (the modulation of the pattern, and two products -- or one
    product and one fma) and a sum of K terms in ANY order adds at most K - 1 more to each: (1 + eps)^(K + 2) - 1 <=
    (K + 4) eps for K eps < 0.1.  So it holds for the reference (pairwise sums), for the kernel (256 strided fma chains
    and a tree) and for f32 or f64 accumulation alike.  Applying the modulator to the finished sum rounds once more, on
    the result: eps |exact|.  Where `exact` is not finite the result must be the same infinity, or NaN with it.

  pearson, inner > 1 (the sample axis is not the contiguous one): bit for bit with the recording.

  pearson, inner == 1: |got - exact| <= (2 m + 16) eps, absolute (|r| <= 1), `exact` in numpy.longdouble.  With u_i =
    xc_i / |xc| and v_i likewise, r = sum u_i v_i and sum |u_i v_i| <= |u| |v| = 1 (Cauchy-Schwarz).  First order, per
    term: the subtraction x_i - mean (1 rounding, relative to xc_i up to the centring error below), the norm (m
    roundings of squares and sums shared by all terms, halved by the square root: (m + 2) / 2 eps), the division (1),
    the same for v, the product (1) and the final sum of m terms (m - 1): (2 (1 + (m + 2) / 2 + 1) + 1 + m - 1) eps =
    (2 m + 6) eps; 10 eps are left for the rounding of the mean's own division and for second-order terms.  The error
    of the mean, delta <= m eps max|x|, shifts EVERY centred value alike: sum (xc_i + delta) (yc_i + delta') = sum xc_i
    yc_i + m delta delta' because sum xc_i = 0, so it enters at second order, as (m eps max|x| / |xc|)^2.
    `second_order_term` computes that quantity per row and the CPU suite asserts it below 1 eps for every such case:
    the cases are chosen so, the bar is not widened for them.

  regime_index: bit for bit with the recording.
"""
import functools
import json
import os

import numpy as np

from _ensemble_numpy import F32, F64, Mismatch, equal_bits, judge_exact  # noqa: F401

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regimes_golden.npz")
PROJECT_KIND = "regimes project: (K + 4) eps sum |f p w| (tests/_regimes_numpy.py)"
PEARSON_KIND = "pearson along the contiguous axis: (2 m + 16) eps (tests/_regimes_numpy.py)"
LD = np.longdouble


def arith_dtype(*arrays):
    return F32 if all(np.asarray(a).dtype == F32 for a in arrays) else F64


# ---- golden file ----
@functools.lru_cache(maxsize=1)
def _load():
    with np.load(PATH) as f:
        meta = json.loads(bytes(f["manifest"]).decode())
        arrays = {k: f[k] for k in f.files if k != "manifest"}
    for a in arrays.values():
        a.setflags(write=False)
    return meta, arrays


def signatures():
    return _load()[0]["signatures"]


def cases(func):
    return [c for c in _load()[0]["cases"] if c["func"] == func]


def arrays_of(case):
    return {k: _load()[1][key] for k, key in case["arrays"].items()}


def recorded(case):
    """The recorded result: an array (pearson) or {label: array}."""
    out = case["out"]
    if out is None:
        return None
    # (the manifest's keys are sorted; the labels' own order is in `plain`)
    return {k: _load()[1][out[k]] for k in case["plain"]["labels"]} if isinstance(out, dict) else _load()[1][out]


def case_id(case):
    return f"{case['id']}-{case['note'].replace(' ', '_')}"


def grid_of(pshape):
    return {"area": [pshape[0] - 1, 0, 0, pshape[1] - 1], "grid": [1, 1]}


def build_patterns(case, module):
    """(patterns object of `module`'s classes, extra keyword arguments of project) for a project case."""
    a, plain = arrays_of(case), case["plain"]
    labels, grid = plain["labels"], grid_of(plain["pshape"])
    if plain["kind"] == "constant":
        return module.ConstantPatterns(labels, grid, a["patterns"]), {}
    if plain["kind"] == "modulated":
        return module.ModulatedPatterns(labels, grid, a["patterns"], lambda step: step), dict(step=a["modulator"])

    class FieldShapedPatterns(module.Patterns):
        def patterns(self):
            return dict(zip(self.labels, a["patterns"]))

    return FieldShapedPatterns(labels, grid, None), {}


def index_args(case):
    a, plain = arrays_of(case), case["plain"]
    proj = {label: a["proj_" + label] for label in plain["labels"]}
    mean = {label: a.get("mean_" + label, plain["mean"].get(label)) for label in plain["labels"]}
    std = {label: a.get("std_" + label, plain["std"].get(label)) for label in plain["labels"]}
    return proj, mean, std


# ---- project ----
def _project_terms(case):
    """(field [N, K], pattern [P, N or 1, K], normalised weights [K], modulator [N] or None, N-shape) as recorded."""
    a, plain = arrays_of(case), case["plain"]
    pshape = tuple(plain["pshape"])
    k, nd = int(np.prod(pshape)), len(pshape)
    field = a["field"]
    nshape = field.shape[:-nd]
    f = field.reshape(-1, k)
    with np.errstate(all="ignore"):
        wn = (a["weights"] / a["weights"].sum()).reshape(k)
    pats = a["patterns"]
    p = pats.reshape(pats.shape[0], -1, k) if plain["kind"] == "perfield" else pats.reshape(pats.shape[0], 1, k)
    mod = np.broadcast_to(a["modulator"], nshape).reshape(-1) if plain["kind"] == "modulated" else None
    return f, p, wn, mod, nshape


def project_dtype(case):
    a = arrays_of(case)
    return arith_dtype(*(a[k] for k in ("field", "patterns", "weights", "modulator") if k in a))


def project(case):
    """The restatement: {label: array}."""
    f, p, wn, mod, nshape = _project_terms(case)
    T = project_dtype(case)
    with np.errstate(all="ignore"):
        c = p.astype(T) * wn.astype(T)
        res = np.einsum("nk,pnk->pn", f.astype(T), np.broadcast_to(c, (c.shape[0], f.shape[0], c.shape[2])))
        if mod is not None:
            res = mod.astype(T) * res
    return {label: res[i].astype(T).reshape(nshape) for i, label in enumerate(case["plain"]["labels"])}


def project_exact_and_bar(case):
    """({label: longdouble exact}, {label: bar}) of a project case."""
    f, p, wn, mod, nshape = _project_terms(case)
    eps = float(np.finfo(project_dtype(case)).eps)
    k = f.shape[1]
    with np.errstate(all="ignore"):
        terms = f.astype(LD)[None] * p.astype(LD) * wn.astype(LD)  # [P, N, K]
        if mod is not None:
            terms = terms * mod.astype(LD)[None, :, None]
        exact, mag = terms.sum(axis=2), np.abs(terms).sum(axis=2)
        bar = (k + 4) * eps * mag + (eps * np.abs(exact) if mod is not None else 0)
    labels = case["plain"]["labels"]
    return ({label: exact[i].reshape(nshape) for i, label in enumerate(labels)},
            {label: bar[i].reshape(nshape) for i, label in enumerate(labels)})


def _file(ledger, what, kind, used, n):
    print(f"{what}: {used:.3f} of its bar used ({n} values)")
    if ledger is not None:
        ledger.append((what, kind, used, 1.0, n))
    return used


def judge_bar(got, exact, bar, what, kind, ledger=None, dtype=None):
    """|got - exact| <= bar where `exact` is finite; elsewhere the same infinity, or NaN with it.  Returns the share used."""
    got, exact = np.asarray(got), np.asarray(exact)
    if dtype is not None and got.dtype != dtype:
        raise Mismatch(f"{what}: result is {got.dtype}, expected {np.dtype(dtype)}")
    if got.shape != exact.shape:
        raise Mismatch(f"{what}: shape {got.shape} against {exact.shape}")
    fin = np.isfinite(exact)
    if not np.array_equal(np.isnan(got), np.isnan(exact)):
        raise Mismatch(f"{what}: NaN pattern differs at {int(np.sum(np.isnan(got) != np.isnan(exact)))} points")
    inf = np.isinf(exact)
    if not (got[inf].astype(LD) == exact[inf]).all():
        raise Mismatch(f"{what}: an infinite result differs")
    if not np.isfinite(got[fin]).all():
        raise Mismatch(f"{what}: a result is not finite where the exact one is")
    err = np.abs(got[fin].astype(LD) - exact[fin])
    b = np.broadcast_to(np.asarray(bar, dtype=LD), exact.shape)[fin]
    if not (err <= b).all():
        i = int(np.argmax(err - b))
        raise Mismatch(f"{what}: |got - exact| = {float(err[i]):.3e} > bar {float(b[i]):.3e} ({int((err > b).sum())} of {err.size} values)")
    used = float(np.max(err / np.maximum(b, np.finfo(LD).tiny), initial=0.0)) if err.size else 0.0
    return _file(ledger, what, kind, used, int(err.size))


def judge_project(case, got, what, ledger=None):
    """`got`: {label: array}; every label against the exact sum within the bar, in the call's dtype and shape."""
    exact, bar = project_exact_and_bar(case)
    if list(got) != case["plain"]["labels"]:
        raise Mismatch(f"{what}: labels {list(got)} against {case['plain']['labels']}")
    return max(judge_bar(got[label], exact[label], bar[label], f"{what} {label}", PROJECT_KIND, ledger, project_dtype(case))
               for label in exact)


def judge_index(got, want, what):
    if list(got) != list(want):
        raise Mismatch(f"{what}: labels {list(got)} against {list(want)}")
    for label in want:
        judge_exact(got[label], want[label], f"{what} {label}")


# ---- pearson ----
def layout(shape, axis):
    axis %= len(shape)
    return int(np.prod(shape[:axis], dtype=np.int64)), shape[axis], int(np.prod(shape[axis + 1:], dtype=np.int64))


def pearson(x, y, axis=0):
    """The sequential restatement, in the call's dtype."""
    x, y = np.asarray(x), np.asarray(y)
    T = arith_dtype(x, y)
    x, y = np.moveaxis(x.astype(T), axis, 0), np.moveaxis(y.astype(T), axis, 0)
    m = x.shape[0]

    def seq(rows):
        s = rows[0].copy()
        for i in range(1, m):
            s = s + rows[i]
        return s

    with np.errstate(all="ignore"):
        count = np.dtype(T).type(m)
        xc, yc = x - seq(x) / count, y - seq(y) / count
        xn, yn = xc / np.sqrt(seq(xc * xc)), yc / np.sqrt(seq(yc * yc))
        return np.asarray(seq(xn * yn), dtype=T)


def pearson_exact(x, y, axis=0):
    x, y = np.moveaxis(np.asarray(x).astype(LD), axis, 0), np.moveaxis(np.asarray(y).astype(LD), axis, 0)
    with np.errstate(all="ignore"):
        xc, yc = x - x.mean(axis=0), y - y.mean(axis=0)
        return (xc * yc).sum(axis=0) / np.sqrt((xc * xc).sum(axis=0) * (yc * yc).sum(axis=0))


def pearson_bar(m, dtype):
    return (2 * m + 16) * float(np.finfo(dtype).eps)


def second_order_term(x, axis, dtype):
    """(m eps max|x| / |xc|)^2 per point, in units of eps (NaN where the column is not finite or constant)."""
    x = np.moveaxis(np.asarray(x).astype(LD), axis, 0)
    eps = LD(np.finfo(dtype).eps)
    with np.errstate(all="ignore"):
        xc = x - x.mean(axis=0)
        return ((x.shape[0] * eps * np.abs(x).max(axis=0) / np.sqrt((xc * xc).sum(axis=0))) ** 2 / eps).astype(F64)


def judge_pearson(x, y, axis, got, want, what, ledger=None):
    """inner > 1: `got` equals `want` (the recording, or the restatement) bit for bit.  inner == 1: `got` has want's
    dtype, shape and NaN pattern and lies within (2 m + 16) eps of the exact value.  Returns the share of the bar used
    (0 on the bit-for-bit path)."""
    _, m, inner = layout(np.shape(x), axis)
    if inner > 1:
        judge_exact(got, want, what)
        return 0.0
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        raise Mismatch(f"{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}")
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        raise Mismatch(f"{what}: NaN pattern differs at {int(np.sum(np.isnan(got) != np.isnan(want)))} points")
    exact = np.where(np.isnan(want), LD(np.nan), pearson_exact(x, y, axis))
    return judge_bar(got, exact, pearson_bar(m, got.dtype), what, PEARSON_KIND, ledger)
