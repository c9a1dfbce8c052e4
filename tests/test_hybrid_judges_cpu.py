"""The judges of the hybrid-level kernels (tests/_hybrid_exact.py) before they see a GPU result: no GPU needed.

1. The pinned NumPy oracle (oracle/vertical_oracle.py) in float64 stays inside the fp64, libm-form bounds against the
   extended-precision reference, every output and mode: the reference's own arithmetic fits the bar the kernels get.
2. The ladder between the two alpha forms, from values computed here: the oracle run in float32 passes the fp32 libm-form
   bound and is REJECTED by the fp32 series-form alpha bound where |p_hi / dif| > 50 -- the bar of the fp32 kernel is one
   the fp32 reference does not meet.
3. Every bar lands with its mutation (as tests/test_judges_reject.py does for the thermo judges).  The mutations are
   applied to NumPy result arrays only.  What a rounding bound can and cannot see, from the shares printed here:
     * Rd or g0 scaled by 1 + 8 u is rejected where the layer is thick and the top-layer rule supplies alpha (bound about
       6 u); over the thin layers of the 137-level table the same result is INSIDE the bound (printed, not asserted):
       delta = log(p_lo / p_hi) of two rounded pressures is uncertain by about 5 u absolute, hundreds of u of a thin layer's
       delta, whatever the kernel does.
     * re scaled by 1 + 8 u moves a height by 8 u z / (re - z), below 0.1 u for any z the atmosphere has: no bound sees it
       there.  It is rejected where z = 0.9 re, and a 7th-digit error in re is rejected in fp64 on ordinary columns.
     * The running sum handed over a chunk boundary one rounding differently is inside every rounding bound by construction
       (its share is printed); `judge_identical` (chunks against one launch, bit for bit) is the judge that rejects it.
"""
import numpy as np
import pytest

import _compare
import _hybrid_exact as hx
from oracle import vertical_oracle as vo

OUT = ("full", "half", "delta", "alpha")
TYPES = {"f32": np.float32, "f64": np.float64}
NPTS = 1027


def _tables(T):
    from ekm_hip import vertical

    return hx.tables(*vertical.hybrid_level_parameters(137), T)


def _oracle_chain(t, q, zs, A, B, sp, alpha_top):
    out = {"thickness": vo.relative_geopotential_thickness_on_hybrid_levels(t, q, A, B, sp, alpha_top=alpha_top),
           "geopotential": vo.geopotential_on_hybrid_levels(t, q, zs, A, B, sp, alpha_top=alpha_top)}
    for ht in ("geometric", "geopotential"):
        for hr in ("sea", "ground"):
            out[f"h_{ht}_{hr}"] = vo.height_on_hybrid_levels(t, q, zs, A, B, sp, alpha_top=alpha_top, h_type=ht, h_reference=hr)
    return out


def _oracle_all(T, A, B, sp, zs, t, q, alpha_top):
    """Every output of the oracle on inputs of dtype T, cast to T (it keeps delta and alpha in float64 arrays whatever
    the input dtype, as the reference does)."""
    res = dict(zip(OUT, vo.pressure_on_hybrid_levels(A, B, sp, alpha_top=alpha_top, output=OUT)))
    res.update(_oracle_chain(t, q, zs, A, B, sp, alpha_top))
    al, de = res["alpha"].astype(T), res["delta"].astype(T)
    res["from_alpha_delta"] = vo.relative_geopotential_thickness_on_hybrid_levels_from_alpha_delta(t, q, al, de)
    return {k: np.asarray(v).astype(T) for k, v in res.items()}, al, de


def _judge_all(got, al, de, T, A, B, sp, zs, t, q, alpha_top, form, what, ledger):
    P = hx.pressure(A, B, sp, alpha_top)
    E = hx.pressure_bounds(P, T, form)
    shares = {k: hx.judge(got[k], P[k], E[k], f"{what} {k}", ledger, T) for k in OUT}
    ex, eb = hx.chain(A, B, sp, zs, t, q, T, alpha_top, form)
    shares.update({k: hx.judge(got[k], ex[k], eb[k], f"{what} {k}", ledger, T) for k in hx.MODES})
    X = hx.scan(t, q, al, de)
    shares["from_alpha_delta"] = hx.judge(got["from_alpha_delta"], X["dphi"], hx.scan_bounds(X, T), f"{what} from_alpha_delta",
                                          ledger, T)
    return shares


def test_the_reference_is_wider_than_float64_and_the_constants_are_the_packages():
    from ekm_hip import vertical

    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    assert hx.TOA == vertical.PRESSURE_TOA
    assert hx.CONST == dict(Rd=vo.RD, RvRd=vo.RV - vo.RD, g0=vo.G0, re=float(vo.R_EARTH))
    assert hx.ALPHA_TOP == {"ifs": float(np.log(2)), "arpege": 1.0}


@pytest.mark.parametrize("name", ["ifs137", "low24", "low5", "low2", "low1", "thick", "thick_zero_top", "switch"])
def test_float64_oracle_within_the_f64_libm_bounds(name):
    """The tie to the pinned oracle: worst share per output printed, at most 1."""
    T = np.float64
    A, B = _tables(T)[name]
    worst = {}
    for seed, alpha_top in ((1, "ifs"), (2, "arpege")):
        sp, t, q, zs = hx.draw(np.random.default_rng(seed), T, NPTS, A.size - 1)
        got, al, de = _oracle_all(T, A, B, sp, zs, t, q, alpha_top)
        sh = _judge_all(got, al, de, T, A, B, sp, zs, t, q, alpha_top, "libm", f"oracle f64 {name} {alpha_top}", _compare.LEDGER)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in sh.items()}
    print(f"oracle f64 / libm-form bound, {name}: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("name", ["ifs137", "low24", "thick", "switch"])
def test_ladder_between_the_libm_and_the_series_form(name):
    """fp32 oracle: inside the fp32 libm-form bounds; its alpha beyond the series-form bound where |p_hi / dif| > 50."""
    T = np.float32
    A, B = _tables(T)[name]
    sp, t, q, zs = hx.draw(np.random.default_rng(3), T, NPTS, A.size - 1)
    got, al, de = _oracle_all(T, A, B, sp, zs, t, q, "ifs")
    sh = _judge_all(got, al, de, T, A, B, sp, zs, t, q, "ifs", "libm", f"oracle f32 {name}", _compare.LEDGER)
    print(f"oracle f32 / libm-form bound, {name}: " + " ".join(f"{k}={v:.3f}" for k, v in sh.items()))
    P = hx.pressure(A, B, sp, "ifs")
    E = hx.pressure_bounds(P, T, "series")
    thin = np.asarray(E["amp"] > 50)
    if P["top"]:
        thin[0] = False
    if name in ("ifs137", "low24"):
        assert thin.sum() > 1000
        scratch = []
        with pytest.raises(AssertionError):
            hx.judge(got["alpha"][thin], P["alpha"][thin], E["alpha"][thin], "oracle f32 alpha, series form", scratch, T)
        print(f"oracle f32 alpha / series-form bound where |p_hi/dif| > 50, {name}: {scratch[0][2]:.1f} ({int(thin.sum())} elements)")
        assert scratch[0][2] > 1.0
    else:  # thick layers: nothing is amplified, the fp32 reference meets the series form too
        assert thin.sum() == 0
        w = hx.judge(got["alpha"], P["alpha"], E["alpha"], f"oracle f32 {name} alpha, series form", _compare.LEDGER, T)
        print(f"oracle f32 alpha / series-form bound, {name} (no thin layer): {w:.3f}")


# ---- every bar lands with its mutation --------------------------------------------------------------------------------
def _rejects(fn, what):
    marks = len(_compare.LEDGER)
    try:
        with pytest.raises(AssertionError):
            fn()
            pytest.fail(f"the judge ACCEPTED {what}", pytrace=False)
    finally:
        del _compare.LEDGER[marks:]


def _share(got, exact, bound):
    scratch = []
    try:
        hx.judge(got, exact, bound, "probe", scratch)
    except AssertionError:
        pass
    return scratch[0][2]


def _one_thick_layer(T):
    """One layer under a zero-pressure top, alpha_top = 1: dphi = rt, the tightest bound of the chain."""
    return np.zeros(2, T), np.array([0.0, 1.0], T)


@pytest.mark.parametrize("tag", sorted(TYPES))
def test_wrong_constants_are_rejected(tag):
    T = TYPES[tag]
    u = float(hx.unit(T))
    A, B = _one_thick_layer(T)
    sp, t, q, zs = hx.draw(np.random.default_rng(4), T, NPTS, 1)
    ex, eb = hx.chain(A, B, sp, zs, t, q, T, "arpege")
    P = hx.pressure(A, B, sp, "arpege")
    led = []
    for k in hx.MODES:  # the exact result rounded to T passes
        hx.judge(ex[k].astype(T), ex[k], eb[k], k, led, T)

    def wrong(**scaled):
        const = dict(hx.CONST)
        for name, f in scaled.items():
            const[name] = np.longdouble(const[name]) * f
        X = hx.scan(t, q, P["alpha"], P["delta"], const)
        return {k: v.astype(T) for k, v in hx.modes(X["dphi"], zs, const).items()}

    print(f"{tag} one thick layer: share of the rounded exact result {max(x[2] for x in led):.3f}")
    for name, must in (("Rd", ("thickness", "h_geopotential_ground")), ("g0", ("h_geopotential_sea", "h_geopotential_ground"))):
        bad = wrong(**{name: 1 + 8 * u})
        print(f"{tag} one thick layer, {name} (1 + 8u): " + " ".join(f"{k}={_share(bad[k], ex[k], eb[k]):.2f}" for k in hx.MODES))
        for k in must:  # (the surface geopotential, which neither constant touches, dilutes the other modes)
            _rejects(lambda: hx.judge(bad[k], ex[k], eb[k], k, led, T), f"{k} with {name} scaled by 1 + 8u")
    # re: only where z is comparable with it
    k = "h_geometric_sea"
    ordinary = _share(wrong(re=1 + 8 * u)[k], ex[k], eb[k])
    print(f"{tag} re (1 + 8u), ordinary columns, {k}: share {ordinary:.3f} (moves the height by < 0.1 u: inside any bound)")
    zs_far = np.full(NPTS, 0.9 * hx.CONST["re"] * hx.CONST["g0"], T)
    X = hx.scan(t, q, P["alpha"], P["delta"])
    e_far = hx.mode_bounds(X["dphi"], hx.scan_bounds(X, T, hx.pressure_bounds(P, T, "kernel")["delta"],
                                                     hx.pressure_bounds(P, T, "kernel")["alpha"]), zs_far, T)[k]
    x_far = hx.modes(X["dphi"], zs_far)[k]
    hx.judge(x_far.astype(T), x_far, e_far, k, led, T)
    const = dict(hx.CONST, re=np.longdouble(hx.CONST["re"]) * (1 + 8 * u))
    _rejects(lambda: hx.judge(hx.modes(X["dphi"], zs_far, const)[k].astype(T), x_far, e_far, k, led, T),
             "h_geometric_sea at z = 0.9 re with re scaled by 1 + 8u")
    if tag == "f64":
        for k in ("h_geometric_sea", "h_geometric_ground"):
            _rejects(lambda: hx.judge(wrong(re=1 + 1e-7)[k], ex[k], eb[k], k, led, T), f"{k} with re wrong in its 7th digit")
    # the same constants over the thin layers of the 137-level table: what the bound can see there (printed only)
    A, B = _tables(T)["ifs137"]
    sp, t, q, zs = hx.draw(np.random.default_rng(5), T, 64, 137)
    ex, eb = hx.chain(A, B, sp, zs, t, q, T, "ifs")
    P = hx.pressure(A, B, sp, "ifs")
    for f in (8, 64, 512):
        X = hx.scan(t, q, P["alpha"], P["delta"], dict(hx.CONST, Rd=np.longdouble(hx.CONST["Rd"]) * (1 + f * u)))
        print(f"{tag} 137 levels, Rd (1 + {f}u): thickness share {_share(X['dphi'].astype(T), ex['thickness'], eb['thickness']):.2f}")
    if tag == "f64":  # the mistake the fp64 bar of 1e-6 let through: a constant wrong in its 7th digit
        for name in ("Rd", "RvRd", "g0"):
            const = dict(hx.CONST, **{name: np.longdouble(hx.CONST[name]) * (1 + 1e-7)})
            X = hx.scan(t, q, P["alpha"], P["delta"], const)
            k = "h_geopotential_sea" if name == "g0" else "thickness"
            _rejects(lambda: hx.judge(hx.modes(X["dphi"], zs, const)[k].astype(T), ex[k], eb[k], k, led, T),
                     f"137 levels, {k} with {name} wrong in its 7th digit")


@pytest.mark.parametrize("tag", sorted(TYPES))
def test_wrong_rows_and_a_missing_top_layer_rule_are_rejected(tag):
    T = TYPES[tag]
    A, B = _tables(T)["ifs137"]
    sp, t, q, zs = hx.draw(np.random.default_rng(6), T, 67, 137)
    P = hx.pressure(A, B, sp, "ifs")
    E = hx.pressure_bounds(P, T, "kernel")
    led = []
    good = {k: P[k].astype(T) for k in OUT}
    for k in OUT:
        hx.judge(good[k], P[k], E[k], k, led, T)
    # alpha of level k+1 at level k in one column: in the alpha output, and in the thickness built from it
    for k in (1, 60, 135):
        bad = good["alpha"].copy()
        bad[k, 11] = bad[k + 1, 11]
        _rejects(lambda: hx.judge(bad, P["alpha"], E["alpha"], "alpha", led, T), f"alpha of level {k + 1} at level {k}")
        al = P["alpha"].copy()
        al[k, 11] = al[k + 1, 11]
        ex, eb = hx.chain(A, B, sp, zs, t, q, T, "ifs")
        X = hx.scan(t, q, al, P["delta"])
        _rejects(lambda: hx.judge(X["dphi"].astype(T), ex["thickness"], eb["thickness"], "thickness", led, T),
                 f"thickness with alpha of level {k + 1} at level {k}")
    # the top layer without the rule: a zero-pressure top (inf / NaN), and a top half level of 0.05 Pa (finite, wrong)
    no_rule = hx.pressure(A, B, sp, "ifs", top=False)
    for k in ("delta", "alpha"):
        _rejects(lambda: hx.judge(no_rule[k].astype(T), P[k], E[k], k, led, T), f"{k} of a zero-pressure top without the rule")
    A2 = A.copy()
    A2[0] = 0.05
    P2, no_rule = hx.pressure(A2, B, sp, "arpege"), hx.pressure(A2, B, sp, "arpege", top=False)
    assert P2["top"] and np.isfinite(no_rule["delta"]).all()
    E2 = hx.pressure_bounds(P2, T, "kernel")
    for k in ("delta", "alpha"):
        hx.judge(P2[k].astype(T), P2[k], E2[k], k, led, T)
        _rejects(lambda: hx.judge(no_rule[k].astype(T), P2[k], E2[k], k, led, T), f"{k} of a 0.05 Pa top without the rule")
    other = hx.pressure(A2, B, sp, "ifs")["alpha"].astype(T)  # alpha_top = log 2 where 1 was asked for
    _rejects(lambda: hx.judge(other, P2["alpha"], E2["alpha"], "alpha", led, T), "the other alpha_top")


def _scan_in_T(T, t, q, al, de, boundary=None):
    """The kernel's scan in NumPy arithmetic of dtype T; `boundary`: the running sum is handed over that level boundary one
    rounding differently (its neighbour in T) in the ragged tail columns."""
    rd, rvd = T(hx.CONST["Rd"]), T(hx.CONST["RvRd"])
    acc = np.zeros(t.shape[1], T)
    out = np.empty_like(t)
    for k in range(t.shape[0] - 1, -1, -1):
        if k + 1 == boundary:
            acc[-3:] = np.nextafter(acc[-3:], T(np.inf))
        rt = (rd + rvd * q[k]) * t[k]
        out[k] = acc + rt * al[k]
        acc = acc + rt * de[k]
    return out


@pytest.mark.parametrize("tag", sorted(TYPES))
def test_a_running_sum_handed_over_differently_is_rejected_bit_for_bit(tag):
    T = TYPES[tag]
    A, B = _tables(T)["low24"]
    sp, t, q, zs = hx.draw(np.random.default_rng(7), T, 1027, 24)
    P = hx.pressure(A, B, sp, "ifs")
    al, de = P["alpha"].astype(T), P["delta"].astype(T)
    whole, chunked = _scan_in_T(T, t, q, al, de), _scan_in_T(T, t, q, al, de, boundary=12)
    assert whole.dtype == T
    hx.judge_identical(whole.copy(), whole, "the scan against itself")
    _rejects(lambda: hx.judge_identical(chunked, whole, "chunks against one launch"), "a running sum handed over one rounding off")
    X = hx.scan(t, q, al, de)
    e = hx.scan_bounds(X, T)
    print(f"{tag} running sum one rounding off at a chunk boundary: share of the rounding bound {_share(chunked, X['dphi'], e):.3f} "
          f"(unmutated {_share(whole, X['dphi'], e):.3f}): inside it, as any single rounding is")
    hx.judge(whole, X["dphi"], e, "NumPy scan in T, from alpha / delta", _compare.LEDGER, T)


def test_a_float32_result_presented_as_float64_is_rejected():
    T = np.float64
    A, B = _tables(T)["low24"]
    sp, t, q, zs = hx.draw(np.random.default_rng(8), T, 257, 24)
    f32 = [x.astype(np.float32) for x in (A, B, sp, zs, t, q)]
    got, al, de = _oracle_all(np.float32, f32[0], f32[1], f32[2], f32[3], f32[4], f32[5], "ifs")
    got = {k: v.astype(T) for k, v in got.items()}
    P = hx.pressure(A, B, sp, "ifs")
    E = hx.pressure_bounds(P, T, "kernel")
    ex, eb = hx.chain(A, B, sp, zs, t, q, T, "ifs")
    led = []
    for k in OUT:
        _rejects(lambda: hx.judge(got[k], P[k], E[k], k, led, T), f"float32 {k} as float64")
    for k in hx.MODES:
        _rejects(lambda: hx.judge(got[k], ex[k], eb[k], k, led, T), f"float32 {k} as float64")
    _rejects(lambda: hx.judge(got["full"].astype(np.float32), P["full"], E["full"], "full", led, T), "a float32 array for float64")


@pytest.mark.parametrize("tag", sorted(TYPES))
def test_a_number_for_a_nan_and_a_wrong_shape_are_rejected(tag):
    T = TYPES[tag]
    A, B = _tables(T)["low5"]
    sp, t, q, zs = hx.draw(np.random.default_rng(9), T, 19, 5)
    sp[5] = np.nan
    P = hx.pressure(A, B, sp, "ifs")
    E = hx.pressure_bounds(P, T, "kernel")
    ex, eb = hx.chain(A, B, sp, zs, t, q, T, "ifs")
    led = []
    cases = [(P[k], E[k], k) for k in OUT] + [(ex[k], eb[k], k) for k in hx.MODES]
    for exact, bound, k in cases:
        good = exact.astype(T)
        assert np.isnan(good[:, 5]).all() and np.isfinite(np.delete(good, 5, axis=1)).all()
        hx.judge(good, exact, bound, k, led, T)
        bad = good.copy()
        bad[2, 5] = np.delete(good, 5, axis=1)[2].mean()
        _rejects(lambda: hx.judge(bad, exact, bound, k, led, T), f"{k}: a number where the exact value is NaN")
        bad = good.copy()
        bad[1, 3] = np.nan
        _rejects(lambda: hx.judge(bad, exact, bound, k, led, T), f"{k}: a NaN where the exact value is a number")
        bad = good.copy()
        bad[1, 3] = np.inf
        _rejects(lambda: hx.judge(bad, exact, bound, k, led, T), f"{k}: an infinity where the exact value is a number")
        _rejects(lambda: hx.judge(good[:, :-1], exact, bound, k, led, T), f"{k}: a column short")
