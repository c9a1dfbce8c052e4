"""Ensemble reductions (efi, sot, sot_func, crps_from_ensemble) without a GPU: the independent NumPy restatement and
the host twin of the kernels' per-point routines (csrc/ensemble_point.hpp) against the results recorded from the
reference (tests/golden/ensemble_golden.npz), the public signatures and error conventions, and the judges themselves.

Parity: bit for bit, no point excluded -- efi and crps for f32 and f64 input, sot_func, and sot for f64 AND f32 input
(numpy.percentile's f32 arithmetic is reproduced: quantile, virtual index and gamma are all formed in f32).  The one
bound is the documented mixed-dtype deviation of efi (clim f32, ens f64), derived in _ensemble_numpy.mixed_efi_bound."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import _compare
import _ensemble_numpy as en
from ekm_hip import extreme, score  # noqa: F401  (the modules under test: absent before this feature)
import _hosttwin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUE_CASES = [c for c in en.cases() if not c["raises"]]
ERROR_CASES = [c for c in en.cases() if c["raises"]]


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def twin(func, kw):
    """One golden call through the host twin: the argument handling of ekm_hip.extreme / ekm_hip.score restated for the
    twin's C entry points (dtype choice, flattening, row pointers, coefficient tables)."""
    lib = _hosttwin.lib()
    if func == "efi":
        clim, ens = np.asarray(kw["clim"]), np.asarray(kw["ens"])
        T = en.arith_dtype(clim, ens)
        clim, ens = np.ascontiguousarray(clim, T), np.ascontiguousarray(ens, T)
        tabs = [np.ascontiguousarray(t) for t in kw.get("tables") or en.efi_tables(clim.shape[0])]
        tabs = [t if t.size else np.zeros(1) for t in tabs]
        out = np.full(clim.shape[1], 7.0)
        fn = getattr(lib, f"ekm_host_efi_{'f32' if T == en.F32 else 'f64'}")
        fn.restype = C.c_int
        rc = fn(_vp(clim), _vp(ens), C.c_uint(clim.shape[0]), C.c_uint(ens.shape[0]), C.c_size_t(clim.shape[1]),
                C.c_double(kw.get("eps", -0.1)), _vp(tabs[0]), _vp(tabs[1]), _vp(tabs[2]), _vp(out))
        assert rc == 0
        return out
    if func == "sot":
        clim, ens, perc = np.asarray(kw["clim"]), np.asarray(kw["ens"]), kw["perc"]
        T = en.arith_dtype(clim, ens)
        pts = clim.shape[1:]
        clim = np.ascontiguousarray(clim, T).reshape(101, -1)
        ens = np.ascontiguousarray(ens, T).reshape(ens.shape[0], -1)
        qc, tail = np.ascontiguousarray(clim[perc]), np.ascontiguousarray(clim[99 if perc > 50 else 1])
        out = np.full(clim.shape[1], 7, T)
        fn = getattr(lib, f"ekm_host_sot_{'f32' if T == en.F32 else 'f64'}")
        fn.restype = C.c_int
        rc = fn(_vp(qc), _vp(tail), _vp(ens), C.c_uint(ens.shape[0]), C.c_size_t(clim.shape[1]), C.c_int(perc),
                C.c_double(kw.get("eps", -1e4)), _vp(out))
        assert rc == 0
        return out.reshape(pts)
    if func == "sot_func":
        arrs = [np.asarray(kw[k]) for k in ("qc_tail", "qc", "qf")]
        T = en.arith_dtype(*arrs)
        arrs = [np.ascontiguousarray(a, T) for a in np.broadcast_arrays(*arrs)]
        out = np.full(arrs[0].shape, 7, T)
        fn = getattr(lib, f"ekm_host_sot_func_{'f32' if T == en.F32 else 'f64'}")
        fn.restype = C.c_int
        rc = fn(_vp(arrs[0]), _vp(arrs[1]), _vp(arrs[2]), C.c_size_t(out.size), C.c_double(kw.get("eps", -1e-4)),
                C.c_double(kw.get("lower_bound", -10)), C.c_double(kw.get("upper_bound", 10)), _vp(out))
        assert rc == 0
        return out
    x, y = np.asarray(kw["x"]), np.asarray(kw["y"])
    T = en.arith_dtype(x, y)
    n = x.shape[0]
    x, yf = np.ascontiguousarray(x, T).reshape(n, -1), np.ascontiguousarray(y, T).reshape(-1)
    p = np.arange(n + 1) / float(n)
    p2, q2 = np.ascontiguousarray(p**2), np.ascontiguousarray((1 - p) ** 2)
    out, missing = np.full(yf.size, 7.0), np.full(yf.size, 9, np.uint8)
    fn = getattr(lib, f"ekm_host_crps_from_ensemble_{'f32' if T == en.F32 else 'f64'}")
    fn.restype = C.c_int
    rc = fn(_vp(x), _vp(yf), C.c_uint(n), C.c_size_t(yf.size), _vp(p2), _vp(q2), _vp(out), _vp(missing))
    assert rc == 0
    assert set(np.unique(missing)) <= {0, 1}
    policy = kw.get("nan_policy", "propagate")
    if policy == "omit":
        return out[missing == 0]
    assert policy == "propagate" or not missing.any()
    return out.reshape(y.shape)


def _tables_note(nclim):
    """The EFI coefficients depend on this host's arccos and sqrt: equal to the recorded ones -> judge against the
    recorded result; another libm -> say so and judge against the restatement with this host's tables, still in bits."""
    if str(nclim) not in en._load()[0]["efi_tables"]:
        return True
    return all(np.array_equal(a, b) for a, b in zip(en.efi_tables(nclim), en.recorded_tables(nclim)))


def judge(case, got, what):
    if case["func"] == "efi" and not en.is_mixed_efi(case):
        kw = en.kwargs_of(case)
        if not _tables_note(kw["clim"].shape[0]):
            want = en.efi(**kw)
            return en.judge_exact(got, want, what + " [this host's arccos/sqrt give other EFI coefficients than the "
                                  "recorded ones: judged against the restatement with this host's tables]")
    return en.judge_case(case, got, what, _compare.LEDGER)


@pytest.mark.parametrize("case", VALUE_CASES, ids=en.case_id)
def test_restatement_against_the_recorded_reference(case):
    judge(case, en.RESTATEMENT[case["func"]](**en.kwargs_of(case)), en.case_id(case))


@pytest.mark.parametrize("case", VALUE_CASES, ids=en.case_id)
def test_host_twin_against_the_recorded_reference(case):
    judge(case, twin(case["func"], en.kwargs_of(case)), en.case_id(case))


def test_known_answers_of_the_reference_tests():
    seen = 0
    for case in VALUE_CASES:
        if "known" in case and case["note"].startswith("f64"):  # the reference's tests state them for f64 input
            got = twin(case["func"], en.kwargs_of(case))
            tol = 1e-4 if case["func"] == "efi" else 1e-5  # the reference's own allclose tolerances (rtol / default)
            assert abs(float(got.reshape(-1)[0]) - case["known"]) <= tol * abs(case["known"]) + 1e-8, en.case_id(case)
            seen += 1
    assert seen == 7


def test_every_case_the_issue_names_is_recorded():
    notes = [c["note"] for c in en.cases()]
    for shape in ("101x51", "101x50", "11x7", "2x1", "101x128"):
        for eps in ("-0.1", "0.0", "0.0001", "1.0"):
            for tag in ("f32", "f64"):
                assert f"{tag} {shape} eps {eps}" in notes
    for perc in (2, 10, 33, 49, 51, 90, 98):
        assert any(f"perc {perc} eps" in n for n in notes)
    for policy in ("propagate", "raise", "omit"):
        assert any(n.endswith(f"nens 1 clean {policy}") for n in notes)


# ---- the public interface: signatures and errors, no GPU involved ----
def _product():
    sys.path.insert(0, os.path.join(ROOT, "earthkit-meteo_amd"))
    from ekm_hip import extreme, score
    return {"efi": extreme.efi, "sot": extreme.sot, "sot_func": extreme.sot_func,
            "crps_from_ensemble": score.crps_from_ensemble}


def test_signatures_are_the_references():
    fns = _product()
    assert sorted(en.signatures()) == sorted(fns)
    for name, recorded in en.signatures().items():
        assert str(inspect.signature(fns[name])) == recorded, name


@pytest.mark.parametrize("case", ERROR_CASES, ids=en.case_id)
def test_error_conventions(case):
    kind, message = case["raises"]
    exc = {"Exception": Exception, "ValueError": ValueError}[kind]
    with pytest.raises(exc) as info:
        _product()[case["func"]](**en.kwargs_of(case))
    assert type(info.value) is exc and str(info.value) == message


def test_efi_shape_errors():
    efi = _product()["efi"]
    with pytest.raises(AssertionError):  # efi.py:45
        efi(np.zeros((101, 4)), np.zeros((51, 5)))
    with pytest.raises(ValueError):      # efi.py:43: a shape that does not unpack into two
        efi(np.zeros(101), np.zeros((51, 5)))
    with pytest.raises(ValueError):
        efi(np.zeros((101, 2, 2)), np.zeros((51, 2, 2)))


def test_product_tables_are_the_references_expression():
    sys.path.insert(0, os.path.join(ROOT, "earthkit-meteo_amd"))
    from ekm_hip import extreme, score
    for nclim in (2, 11, 101):
        for a, b in zip(extreme.efi_coefficients(nclim), en.efi_tables(nclim)):
            assert np.array_equal(a, b)
    for a, b in zip(score.crps_weights(51), ((np.arange(52) / 51.0) ** 2, (1 - np.arange(52) / 51.0) ** 2)):
        assert np.array_equal(a, b)


# ---- the judges reject what they must ----
def _flip(a, i):
    b = np.array(a, copy=True)
    b.reshape(-1).view(np.uint32 if b.dtype == en.F32 else np.uint64)[i] ^= 1
    return b


@pytest.mark.parametrize("func", ["efi", "sot", "sot_func", "crps_from_ensemble"])
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_judge_exact_rejects_one_flipped_bit_and_one_wrong_nan(func, tag):
    case = next(c for c in VALUE_CASES if c["func"] == func and c["note"].startswith(tag) and en.expected_of(c).size > 4)
    want = en.expected_of(case)
    en.judge_exact(want, want)
    i = int(np.flatnonzero(~np.isnan(want.reshape(-1)))[-1])
    with pytest.raises(en.Mismatch):
        en.judge_exact(_flip(want, i), want)
    bad = want.copy()
    bad.reshape(-1)[i] = np.nan
    with pytest.raises(en.Mismatch):
        en.judge_exact(bad, want)
    with pytest.raises(en.Mismatch):
        en.judge_exact(want.astype(np.float32 if want.dtype == en.F64 else np.float64), want)
    with pytest.raises(en.Mismatch):
        en.judge_exact(-np.zeros(3), np.zeros(3))


def test_one_count_off_by_one_is_caught():
    """A rank that is off by one member at one climate row moves efi by far more than a bit."""
    case = next(c for c in VALUE_CASES if c["note"] == "f64 101x51 eps -0.1")
    kw = en.kwargs_of(case)
    ens = kw["ens"].copy()
    j = 5
    row = kw["clim"][50, j]
    k = int(np.argmax(ens[:, j] > row))  # one member just above climate row 50 drops onto it: its count grows by one
    assert ens[k, j] > row
    ens[k, j] = row
    with pytest.raises(en.Mismatch):
        en.judge_case(case, en.efi(kw["clim"], ens, kw["eps"]), "off by one")


def test_judge_bound_rejects_beyond_the_bound():
    case = next(c for c in VALUE_CASES if en.is_mixed_efi(c))
    kw, want = en.kwargs_of(case), en.expected_of(case)
    bound = en.mixed_efi_bound(kw["clim"], kw["ens"], kw["eps"])
    assert 0 < bound.max() < 1e-5
    en.judge_bound(want, want, bound)
    bad = want.copy()
    bad[3] += 2 * bound[3]
    with pytest.raises(en.Mismatch):
        en.judge_bound(bad, want, bound)
    bad = want.copy()
    bad[3] = np.nan
    with pytest.raises(en.Mismatch):
        en.judge_bound(bad, want, bound)


def test_mixed_dtype_deviation_measured_against_its_bound():
    """The reference's own f32-frac and f64-frac runs on 20 000 gamma-distributed points at 101 x 51 (restatement with
    dtype f32 for frac is what the reference does when only clim is f32): measured 2.1e-8, inside the derived bound."""
    rng = np.random.default_rng(7)
    clim = np.sort(rng.gamma(1.5, 2.0, (101, 20000)), axis=0).astype(np.float32)
    ens = rng.gamma(1.5, 2.0, (51, 20000))
    c64 = clim.astype(np.float64)
    f64 = en.efi(c64, ens, -0.1)
    # frac in f32, everything else as in f64: the comparison ens <= clim is exact in both
    T = en.F32
    total = np.zeros(20000)
    acosdiff, proddiff, acoef = en.efi_tables(101)
    f0 = en._frac(c64[0], ens, T)
    for icl in range(100):
        f1 = en._frac(c64[icl + 1], ens, T)
        total = total + ((T.type(2) * f0 - T.type(1)).astype(np.float64) * acosdiff[icl]
                         + acoef[icl] * ((f1 - f0) * T.type(100)).astype(np.float64) - proddiff[icl])
        f0 = f1
    f32 = total * (2.0 / np.pi)
    used = np.abs(f32 - f64)
    bound = en.mixed_efi_bound(c64, ens, -0.1)
    print(f"mixed-dtype efi deviation: measured max {used.max():.2e}, bound max {bound.max():.2e}")
    _compare.LEDGER.append(("efi mixed dtype 20000 points", "efi mixed-dtype bound", float((used / bound).max()), 1.0, 20000))
    assert (used <= bound).all()


@pytest.mark.skipif(not os.path.exists(_hosttwin.ASAN_PATH), reason="ASan host twin not built (make twin-asan)")
def test_golden_cases_through_the_sanitized_host_twin():
    if os.environ.get("EKM_HOSTTWIN_LIB") == _hosttwin.ASAN_PATH:
        pytest.skip("already inside the sanitized run")
    out = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    ub = subprocess.run(["gcc", "-print-file-name=libubsan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(out) and os.path.exists(out)):
        pytest.skip("libasan.so not found next to gcc")
    env = dict(os.environ, EKM_HOSTTWIN_LIB=_hosttwin.ASAN_PATH,
               LD_PRELOAD=":".join(x for x in (out, ub) if os.path.isabs(x) and os.path.exists(x)),
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               OMP_NUM_THREADS="1", PYTHONMALLOC="malloc")
    cmd = [sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", os.path.abspath(__file__), "-k", "host_twin_against"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    tail = r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0, tail
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, tail
    assert " passed" in r.stdout, tail
