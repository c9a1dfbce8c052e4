"""Exact reference and rounding bounds for the hybrid-level kernels of csrc/hybrid.hip (NumPy only, no GPU).

The inputs are taken as they reach the kernel, already rounded to its dtype T; everything below is evaluated on them in
`np.longdouble` (64-bit significand, asserted at import), so an fp64 result is never judged against fp64 arithmetic.
The constants are the oracle's (oracle/vertical_oracle.py) and the package's (ekm_hip.vertical.PRESSURE_TOA).

A BOUND is an array of the output's shape: the sum of named terms, each `count x u x |quantity|` with u = eps(T)/2
the unit roundoff.  A count is the number of roundings the kernel's expression performs on that quantity, read from
hybrid.hip; a constant that the kernel converts with T(c) pays its actual conversion error |T(c) - c| (zero in fp64).
No count is fitted to a result.  Every bound is first order in u and multiplied by 1 + 64 u for the products of
roundings (gamma_n = n u / (1 - n u) with n <= 64 in the per-level expressions).

half   p = A + B sp              u |B sp|  the product                    (absent when contracted to an fma: budgeted)
                               + u |p|     the sum                                                          = E_half
full   p_k + 0.5 (p_k+1 - p_k)   (E_k + E_k+1) / 2   the two half levels
                               + u |p_k+1 - p_k| / 2  the difference (0.5 x is exact)
                               + u |p_full|           the blend (an fma or an addition: one rounding)
delta  log(p_lo / p_hi)          pert = E_k/|p_k| + E_k+1/|p_k+1|  the ratio moved by both half-level errors (d log r = dr / r)
   libm form                   + u                    the division p_lo / p_hi (absolute in delta)
                               + L u |delta|          the logarithm.  L = 2 in fp64: 1 ulp = 2 u (device libm, glibc).  L = 3 in
                                 fp32: the device's logf is v_log_f32 (1 ulp of log2 r: up to 2 u relative) times ln 2 in a
                                 compensated product that rounds once more (read from the kernel's ISA; found on the GPU:
                                 the top layer's log(p_1 / 0.1) = 5.72 was 17.3 u off under a budget of 14.7 u with L = 2)
   series form (fp32, |s| < 0.25: delta = 2 s q(s^2), s = dif rcp(p_lo + p_hi))
                               + (5 / (1 - s^2) + 3) u |delta|:  s pays dif, the sum, v_rcp_f32 at 1 ulp = 2 u and the product
                                 (5 u, carried into 2 atanh s by 1 / (1 - s^2)); q pays its last fma and at most one u for
                                 all that is inside it (it enters times z q' / q <= 0.023); 2 s q pays one product (2 s is exact)
alpha  1 - p_hi / dif * delta = g(r), r = p_lo / p_hi, g(r) = 1 - log r / (r - 1)
                                 h(r) pert, h = |r g'(r)| = |r log r - (r - 1)| / (r - 1)^2 (1/2 for thin layers): both
                                 factors come from the SAME rounded pressures, so their errors enter through g alone
   series form                 + |x| ((5 / (1 - s^2) + 3) u + 4 u), x = p_hi / dif * delta: delta's own roundings, v_rcp_f32 of
                                 dif (2 u) and the two products
                               + u |alpha|            the subtraction from 1
   libm form                   + |p_hi / dif| (u + L u |delta|)  the rounding of the ratio and of the logarithm are independent of
                                 dif and are amplified by p_hi / dif
                               + 3 u |x|              the difference dif, the division p_hi / dif, the product
                               + u |alpha|
top layer, rule on               delta = log(p_1 / 0.1): E_1/|p_1| + |T(0.1) - 0.1| / 0.1 + u + L u |delta|;  alpha = alpha_top:
                                 |T(alpha_top) - alpha_top|
rt     (Rd + (Rv - Rd) q) t      |T(Rd) - Rd| + (|T(Rv-Rd) - (Rv-Rd)| + u |Rv - Rd|) |q| + u |R|, times |t|, + u |rt|   = E_rt
dphi_k sum_{j>k} rt_j delta_j + rt_k alpha_k
                                 sum_{j>k} (|rt_j| bound(delta_j) + E_rt_j |delta_j|) + |rt_k| bound(alpha_k) + E_rt_k |alpha_k|
                               + (terms + 2) u sum |term|   the products and the running sum, bottom-up
       from alpha / delta: the same with bound(delta) = bound(alpha) = 0 (they are inputs).
       The running sum crosses a chunk boundary in an output row of dtype T, which it already has: no term.
modes  + zs: u |dphi + zs|;  / g0: (|T(g0) - g0| / g0 + u) |result|;  geometric height H(z) = re z / (re - z):
       E_z re^2 / (re - z)^2 + |T(re) - re| z^2 / (re - z)^2 + 3 u |H| (product, difference, division);
       above ground: the same for the surface's own height, + u |result| for the subtraction.
"""
import numpy as np

from oracle import vertical_oracle as vo

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, (
    "np.longdouble is no wider than float64 here: evaluate this module's expressions with mpmath at 40 digits instead")

TOA = 0.1  # ekm_hip.vertical.PRESSURE_TOA, checked against the package in tests/test_hybrid_judges_cpu.py
CONST = dict(Rd=vo.RD, RvRd=vo.RV - vo.RD, g0=vo.G0, re=float(vo.R_EARTH))
ALPHA_TOP = {"ifs": float(np.log(2)), "arpege": 1.0}
MODES = ("thickness", "geopotential", "h_geometric_sea", "h_geopotential_sea", "h_geometric_ground", "h_geopotential_ground")
KIND = "hybrid levels: worst |got - exact| / derived rounding bound"


def unit(T):
    return LD(np.finfo(T).eps) / 2


def _second(T):
    return 1 + 64 * unit(T)


def _cerr(T, c):
    """|T(c) - c|: what the kernel's T(c) costs."""
    return abs(LD(np.dtype(T).type(c)) - LD(c))


def draw(rng, T, npts, nfull):
    """sp 520-1040 hPa, t 190-315 K, q log-uniform 1e-6.5 ... 1e-1.7, zs 0 ... 3e4, rounded to T."""
    sp = rng.uniform(52000.0, 104000.0, npts).astype(T)
    t = rng.uniform(190.0, 315.0, (nfull, npts)).astype(T)
    q = (10.0 ** rng.uniform(-6.5, -1.7, (nfull, npts))).astype(T)
    zs = rng.uniform(0.0, 3e4, npts).astype(T)
    return sp, t, q, zs


def tables(A137, B137, T):
    """The level tables of both test files, rounded to T: the 137 IFS levels, their lowest 24 / 5 / 2 / 1 (top half level
    far from 0 Pa, B != 0), two synthetic ones with layer ratios up to 10 (one with a zero-pressure top: the top-layer rule),
    and one with A = 0 whose B[k+1] / B[k] steps through 5/3 from -4 to +4 ulp: s = (r - 1) / (r + 1) on both sides of 0.25,
    the fp32 kernel's switch from its series to libm."""
    A137, B137 = np.asarray(A137, dtype=np.float64), np.asarray(B137, dtype=np.float64)
    tabs = {"ifs137": (A137, B137)}
    for n in (24, 5, 2, 1):
        tabs[f"low{n}"] = (A137[137 - n:], B137[137 - n:])
    thick = np.array([5e-4, 5e-3, 5e-2, 0.2, 0.5, 1.0])
    tabs["thick"] = (np.array([40.0, 30.0, 20.0, 10.0, 0.0, 0.0]), thick)
    tabs["thick_zero_top"] = (np.zeros(7), np.concatenate([[0.0], thick]))
    b = [np.dtype(T).type(0.004)]
    for j in range(-4, 5):
        nxt = np.dtype(T).type(LD(b[-1]) * 5 / 3)
        for _ in range(abs(j)):
            nxt = np.nextafter(nxt, np.dtype(T).type(np.inf if j > 0 else -np.inf))
        b.append(nxt)
    tabs["switch"] = (np.zeros(len(b)), np.array(b, dtype=np.float64))
    return {k: (a.astype(T), b_.astype(T)) for k, (a, b_) in tabs.items()}


# ---- exact values --------------------------------------------------------------------------------------------------
def pressure(A, B, sp, alpha_top="ifs", top=None):
    """Exact half / full / delta / alpha of the table (A, B) over the columns `sp` (1-D), with the intermediates the
    bounds need.  `top`: the top-layer rule; None decides it as the reference does, any(p_half[0] <= 0.1)."""
    A, B, sp = (np.asarray(x).astype(LD) for x in (A, B, sp))
    assert A.ndim == 1 and A.shape == B.shape and sp.ndim == 1
    with np.errstate(all="ignore"):
        bsp = B[:, None] * sp[None, :]
        half = A[:, None] + bsp
        hi, lo = half[:-1], half[1:]
        dif = lo - hi
        full = hi + dif / 2
        ratio = lo / hi
        delta = np.log(ratio)
        x = hi / dif * delta
        alpha = 1 - x
        if top is None:
            top = bool(np.any(half[0] <= LD(TOA)))
        if top:
            delta[0] = np.log(lo[0] / LD(TOA))
            alpha[0] = LD(ALPHA_TOP[alpha_top])
    return dict(half=half, full=full, delta=delta, alpha=alpha, bsp=bsp, dif=dif, ratio=ratio, x=x, top=top,
                alpha_top=ALPHA_TOP[alpha_top])


def scan(t, q, alpha, delta, const=CONST):
    """The bottom-up scan dphi_k = sum_{j>k} rt_j delta_j + rt_k alpha_k on [levels, columns] arrays."""
    t, q, alpha, delta = (np.asarray(v).astype(LD) for v in (t, q, alpha, delta))
    R = LD(const["Rd"]) + LD(const["RvRd"]) * q
    rt = R * t
    td = rt * delta
    below = np.zeros_like(td)
    below[:-1] = np.cumsum(td[:0:-1], axis=0)[::-1]
    ta = rt * alpha
    return dict(q=q, t=t, R=R, rt=rt, td=td, ta=ta, below=below, dphi=below + ta, alpha=alpha, delta=delta)


def _geom(z, const):
    re = LD(const["re"])
    return re * z / (re - z)


def modes(dphi, zs, const=CONST):
    """The six outputs of the chain from the exact thickness and the surface geopotential."""
    g0 = LD(const["g0"])
    zs = np.asarray(zs).astype(LD)[None, :]
    zsum = dphi + zs
    return dict(thickness=dphi, geopotential=zsum, h_geometric_sea=_geom(zsum / g0, const), h_geopotential_sea=zsum / g0,
                h_geometric_ground=_geom(zsum / g0, const) - _geom(zs / g0, const), h_geopotential_ground=dphi / g0)


# ---- bounds -----------------------------------------------------------------------------------------------------------
def pressure_bounds(P, T, form):
    """Bounds of the four outputs.  `form`: "libm" (fp64 kernel, the NumPy oracle), "series" (the fp32 kernel's
    2 atanh s path) or "kernel": libm for fp64; for fp32 series where |s| < 0.25 and libm elsewhere, the larger of the two
    within 16 u of the switch, where the kernel's own rounded s decides (s pays 5 u, and the half-level errors move it
    by 2 u (1 + r) / (r - 1) = 2 u / s = 8 u there)."""
    u, S = unit(T), _second(T)
    lg = (3 if np.dtype(T) == np.float32 else 2) * u  # the logarithm's own relative error (module docstring)
    half, dif, delta, alpha, x, r = (P[k] for k in ("half", "dif", "delta", "alpha", "x", "ratio"))
    with np.errstate(all="ignore"):
        e_half = (u * np.abs(P["bsp"]) + u * np.abs(half)) * S
        e_full = ((e_half[:-1] + e_half[1:]) / 2 + u * np.abs(dif) / 2 + u * np.abs(P["full"])) * S
        pert = e_half[:-1] / np.abs(half[:-1]) + e_half[1:] / np.abs(half[1:])
        s = dif / (half[1:] + half[:-1])
        own = (5 / (1 - s * s) + 3) * u
        h = np.where(np.abs(r - 1) < 1e-5, (1 + np.abs(r - 1)) / 2, np.abs(r * np.log(r) - (r - 1)) / (r - 1) ** 2)
        amp = np.abs(half[:-1] / dif)
        d_libm = (pert + u + lg * np.abs(delta)) * S
        d_series = (pert + own * np.abs(delta)) * S
        a_libm = (h * pert + amp * (u + lg * np.abs(delta)) + 3 * u * np.abs(x) + u * np.abs(alpha)) * S
        a_series = (h * pert + np.abs(x) * (own + 4 * u) + u * np.abs(alpha)) * S
        if form == "kernel" and np.dtype(T) == np.float64:
            form = "libm"
        if form == "libm":
            e_delta, e_alpha = d_libm, a_libm
        elif form == "series":
            e_delta, e_alpha = d_series, a_series
        else:
            assert form == "kernel", form
            lo, hi_ = 0.25 * (1 - 16 * u), 0.25 * (1 + 16 * u)
            inside, outside = np.abs(s) < lo, ~(np.abs(s) < hi_)
            e_delta = np.where(inside, d_series, np.where(outside, d_libm, np.maximum(d_series, d_libm)))
            e_alpha = np.where(inside, a_series, np.where(outside, a_libm, np.maximum(a_series, a_libm)))
        if P["top"]:
            e_delta[0] = (e_half[1] / np.abs(half[1]) + _cerr(T, TOA) / LD(TOA) + u + lg * np.abs(delta[0])) * S
            e_alpha[0] = _cerr(T, P["alpha_top"])
    return dict(half=e_half, full=e_full, delta=e_delta, alpha=e_alpha, amp=amp, s=s)


def scan_bounds(X, T, e_delta=None, e_alpha=None):
    """Bound of the thickness; e_delta / e_alpha None: alpha and delta are inputs (from_alpha_delta)."""
    u, S = unit(T), _second(T)
    e_R = _cerr(T, CONST["Rd"]) + (_cerr(T, CONST["RvRd"]) + u * abs(LD(CONST["RvRd"]))) * np.abs(X["q"]) + u * np.abs(X["R"])
    e_rt = (e_R * np.abs(X["t"]) + u * np.abs(X["rt"])) * S
    zero = np.zeros_like(X["rt"])
    e_td = np.abs(X["rt"]) * (zero if e_delta is None else e_delta) + e_rt * np.abs(X["delta"])
    e_ta = np.abs(X["rt"]) * (zero if e_alpha is None else e_alpha) + e_rt * np.abs(X["alpha"])
    n = X["rt"].shape[0]
    e_below, abs_below = np.zeros_like(e_td), np.zeros_like(e_td)
    e_below[:-1] = np.cumsum(e_td[:0:-1], axis=0)[::-1]
    abs_below[:-1] = np.cumsum(np.abs(X["td"])[:0:-1], axis=0)[::-1]
    terms = (n - np.arange(n)).astype(LD)[:, None]  # the layers below k, and k's own
    return (e_below + e_ta + (terms + 2) * u * (abs_below + np.abs(X["ta"]))) * S


def mode_bounds(dphi, e_dphi, zs, T):
    u, S = unit(T), _second(T)
    g0, re = LD(CONST["g0"]), LD(CONST["re"])
    cg, cre = _cerr(T, CONST["g0"]) / g0, _cerr(T, CONST["re"])
    zs = np.asarray(zs).astype(LD)[None, :]
    zsum = dphi + zs
    e_sum = e_dphi + u * np.abs(zsum)

    def e_geom(z, e_z):
        return (e_z * re * re / (re - z) ** 2 + cre * z * z / (re - z) ** 2 + 3 * u * np.abs(_geom(z, CONST))) * S

    z, z_s = zsum / g0, zs / g0
    e_z = (e_sum / g0 + (cg + u) * np.abs(z)) * S
    e_zs = (cg + u) * np.abs(z_s) * S
    above = _geom(z, CONST) - _geom(z_s, CONST)
    return dict(thickness=e_dphi, geopotential=e_sum * S, h_geopotential_sea=e_z, h_geometric_sea=e_geom(z, e_z),
                h_geopotential_ground=(e_dphi / g0 + (cg + u) * np.abs(dphi / g0)) * S,
                h_geometric_ground=(e_geom(z, e_z) + e_geom(z_s, e_zs) + u * np.abs(above)) * S)


def chain(A, B, sp, zs, t, q, T, alpha_top="ifs", form="kernel", top=None):
    """Exact values and bounds of the six chain outputs for `t.shape[0]` bottom-most levels of the table."""
    A, B = np.asarray(A), np.asarray(B)
    n = t.shape[0]
    A, B = A[A.shape[0] - 1 - n:], B[B.shape[0] - 1 - n:]
    P = pressure(A, B, sp, alpha_top, top)
    E = pressure_bounds(P, T, form)
    X = scan(t, q, P["alpha"], P["delta"])
    e_dphi = scan_bounds(X, T, E["delta"], E["alpha"])
    return modes(X["dphi"], zs), mode_bounds(X["dphi"], e_dphi, zs, T)


# ---- judges -----------------------------------------------------------------------------------------------------------
def judge(got, exact, bound, what, ledger, T=None):
    """dtype, shape, identical NaN / inf pattern, |got - exact| <= bound at EVERY element.  Appends
    (what, kind, worst used / allowed, 1.0, n) to `ledger` and returns the worst share."""
    got = np.asarray(got)
    if T is not None:
        assert got.dtype == np.dtype(T), f"{what}: dtype {got.dtype}, expected {np.dtype(T)}"
    assert got.dtype in (np.dtype(np.float32), np.dtype(np.float64)), f"{what}: dtype {got.dtype}"
    assert got.shape == exact.shape == bound.shape, f"{what}: shapes {got.shape} {exact.shape} {bound.shape}"
    nan_g, nan_e = np.isnan(got), np.isnan(exact)
    assert np.array_equal(nan_g, nan_e), f"{what}: NaN pattern differs at {np.argwhere(nan_g != nan_e)[:4].tolist()}"
    inf_e = np.isinf(exact)
    assert np.array_equal(np.isinf(got), inf_e), f"{what}: inf pattern differs"
    assert np.array_equal(got[inf_e].astype(LD), exact[inf_e]), f"{what}: inf signs differ"
    fin = ~(nan_e | inf_e)
    err = np.abs(got[fin].astype(LD) - exact[fin])
    b = bound[fin]
    with np.errstate(all="ignore"):
        share = np.where(err == 0, LD(0), err / b)
    share = np.where(np.isfinite(share) | (err == 0), share, LD(np.inf))  # a NaN or zero bound under an error: rejected
    worst = float(share.max()) if share.size else 0.0
    ledger.append((what, KIND, worst, 1.0, int(got.size)))
    if not worst <= 1.0:
        i = int(np.argmax(share))
        idx = np.argwhere(fin)[i].tolist()
        raise AssertionError(f"{what}: |got - exact| = {float(err[i]):.3e} is {worst:.3f} x the bound {float(b[i]):.3e} "
                             f"at {idx} (got {got[fin][i]!r}, exact {float(exact[fin][i])!r}); "
                             f"{int((share > 1).sum())} of {got.size} elements beyond it")
    return worst


def judge_identical(got, want, what):
    """Two launch shapes of the same arithmetic (level chunks against one launch, rows against columns): every bit.
    One rounding more or less in a value handed from one launch to the next is inside any rounding bound by
    construction; this is the judge that sees it."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} / {want.dtype} {want.shape}"
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    assert same.all(), f"{what}: {int((~same).sum())} of {got.size} elements differ, first at {np.argwhere(~same)[0].tolist()}"
