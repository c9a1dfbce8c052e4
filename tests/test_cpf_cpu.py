"""Crossing Point Forecast (extreme.cpf) without a GPU: the independent NumPy restatement (tests/_cpf_numpy.py) and the
host twin of the kernel's per-point routine (cpf_point / cpf_value in csrc/ensemble_point.hpp) against the results
recorded from the reference (tests/golden/cpf_golden.npz), the public signature and error conventions, and the judge.

Parity: dtype, bits and NaN pattern, no point excluded, for f32 and f64 input and every option.  The one bound is the
documented mixed-dtype deviation (clim f32, ens f64), derived in _cpf_numpy.mixed_cpf_bound."""
import ctypes as C
import inspect

import numpy as np
import pytest

import _compare
import _cpf_numpy as cn
import _ensemble_numpy as en
import _hosttwin
from ekm_hip import extreme

CASES = cn.cases()


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def twin(clim, ens, sort_clim=True, sort_ens=True, epsilon=None, symmetric=False, from_zero=False, dtype=None):
    """One call through the host twin: the argument handling of ekm_hip.extreme.cpf restated for ekm_host_cpf_*."""
    clim, ens = np.asarray(clim), np.asarray(ens)
    T = np.dtype(dtype) if dtype is not None else cn.arith_dtype(clim, ens)
    clim, ens = np.ascontiguousarray(clim, T), np.ascontiguousarray(ens, T)
    out = np.full(clim.shape[1], 7, np.float32)
    fn = getattr(_hosttwin.lib(), f"ekm_host_cpf_{'f32' if T == cn.F32 else 'f64'}")
    fn.restype = C.c_int
    use_eps = epsilon is not None and not symmetric
    rc = fn(_vp(clim), _vp(ens), C.c_uint(clim.shape[0]), C.c_uint(ens.shape[0]), C.c_size_t(clim.shape[1]),
            C.c_int(bool(sort_clim)), C.c_int(bool(sort_ens)), C.c_int(bool(from_zero)), C.c_int(bool(symmetric)),
            C.c_int(use_eps), C.c_double(epsilon if use_eps else 0.0), _vp(out))
    assert rc == 0
    return out


def judge(case, got, what):
    want = cn.expected_of(case)
    if not cn.is_mixed_clim_f32(case):
        return en.judge_exact(got, want, what)
    kw = cn.kwargs_of(case)
    bound = cn.mixed_cpf_bound(kw["clim"], kw["ens"], **cn.options_of(case))
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), what
    err = np.where(np.isnan(want), 0.0, np.abs(got.astype(np.float64) - want.astype(np.float64)))
    used = float(np.max(err / np.maximum(bound, 1e-300), initial=0.0))
    print(f"{what}: max |reference - product| {err.max():.3e}, bound max {bound.max():.3e}, {int((err > 0).sum())} points differ")
    _compare.LEDGER.append((what, "cpf mixed-dtype bound", used, 1.0, err.size))
    if not (err <= bound).all():
        i = int(np.argmax(err - bound))
        raise en.Mismatch(f"{what}: |{got[i]!r} - {want[i]!r}| = {err[i]:.3e} > {bound[i]:.3e}")


# One test walks all recorded cases (a failure names its case): 441 parametrised items would cost the suite more in
# per-item overhead than the comparisons themselves take.
def test_restatement_against_the_recorded_reference():
    for case in CASES:
        judge(case, cn.cpf(**cn.kwargs_of(case)), "restatement " + cn.case_id(case))


def test_host_twin_against_the_recorded_reference():
    for case in CASES:
        judge(case, twin(**cn.kwargs_of(case)), "host twin " + cn.case_id(case))


def test_known_answers_of_the_reference_tests():
    seen = 0
    for case in CASES:
        if "known" in case:
            known = cn._load()[1][case["known"]]
            assert np.allclose(twin(**cn.kwargs_of(case)), known), cn.case_id(case)  # the reference's own tolerance
            assert np.allclose(cn.cpf(**cn.kwargs_of(case)), known), cn.case_id(case)
            seen += 1
    assert seen == 8


def test_every_case_the_issue_names_is_recorded():
    notes = [c["note"] for c in CASES]
    for shape in ("101x51", "101x50", "11x7", "3x1", "3x2", "5x3", "101x3", "11x128"):
        for tag in ("f32", "f64"):
            for kind in ("gamma", "normal"):
                for option in ("default", "from_zero", "symmetric", "symmetric from_zero", "epsilon 0.5", "sorts off presorted",
                               "sorts off unsorted", "sort_clim off", "sort_ens off"):
                    assert f"{tag} {shape} {kind} {option}" in notes
    assert any("equal above below nan inf" in n for n in notes)
    assert any(n.startswith("mixed clim f32 ens f64") for n in notes) and any(n.startswith("mixed clim f64 ens f32") for n in notes)
    for case in CASES:
        assert cn.kwargs_of(case)["clim"].shape[1] == cn.expected_of(case).shape[0]


def test_the_goldens_tell_f32_from_f64_arithmetic():
    """The same values run in the other dtype's arithmetic give other bits somewhere: the goldens do decide the dtype rules."""
    for case in CASES:
        kw = cn.kwargs_of(case)
        if case["note"].startswith("f32 101x51") and kw["clim"].dtype == cn.F32:
            if np.any(cn.cpf(**kw, dtype=cn.F64) != cn.expected_of(case)):
                return
    raise AssertionError("no recorded f32 case tells f32 from f64 arithmetic")


def test_nan_columns_do_give_crossings():
    """numpy.sort puts a NaN last and the scan compares as usual: a column with a NaN is not NaN."""
    hits = 0
    for case in CASES:
        if "nan everywhere" in case["note"]:
            want = cn.expected_of(case)
            assert not np.isnan(want).any()
            hits += int((want != 0).sum())
    assert hits > 0


# ---- the public interface: signature and errors, no GPU involved ----
def test_signature_is_the_references():
    assert str(inspect.signature(extreme.cpf)) == cn.signature()
    assert cn.signature() == "(clim, ens, sort_clim=True, sort_ens=True, epsilon=None, symmetric=False, from_zero=False)"
    assert str(inspect.signature(cn.cpf)).startswith(cn.signature()[:-1])


def test_cpf_shape_errors():
    with pytest.raises(AssertionError):  # cpf.py:138
        extreme.cpf(np.zeros((101, 4)), np.zeros((51, 5)))
    with pytest.raises(ValueError):      # cpf.py:136: a shape that does not unpack into two
        extreme.cpf(np.zeros(101), np.zeros((51, 5)))
    with pytest.raises(ValueError):
        extreme.cpf(np.zeros((101, 2, 2)), np.zeros((51, 2, 2)))
    with pytest.raises(AssertionError):
        cn.cpf(np.zeros((101, 4)), np.zeros((51, 5)))
    with pytest.raises(ValueError):
        cn.cpf(np.zeros(101), np.zeros((51, 5)))


# ---- the judge rejects what it must ----
@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_judge_exact_rejects_one_flipped_bit_and_one_wrong_nan(tag):
    case = next(c for c in CASES if c["note"] == f"{tag} 101x51 normal default")
    want = cn.expected_of(case)
    en.judge_exact(want, want)
    i = int(np.flatnonzero(want != 0)[-1])
    bad = want.copy()
    bad.view(np.uint32)[i] ^= 1
    with pytest.raises(en.Mismatch):
        en.judge_exact(bad, want)
    bad = want.copy()
    bad[i] = np.nan
    with pytest.raises(en.Mismatch):
        en.judge_exact(bad, want)
    with pytest.raises(en.Mismatch):
        en.judge_exact(want.astype(np.float64), want)
    with pytest.raises(en.Mismatch):
        en.judge_exact(-np.zeros(3, np.float32), np.zeros(3, np.float32))


def test_mixed_bound_rejects_beyond_the_bound():
    case = next(c for c in CASES if c["note"] == "mixed clim f32 ens f64 from_zero")
    kw = cn.kwargs_of(case)
    bound = cn.mixed_cpf_bound(kw["clim"], kw["ens"], **cn.options_of(case))
    assert 0 < bound.max() <= 3 * cn.U32 * (1 + 2.0 ** -19) and (bound == 0).any()
    want = cn.expected_of(case)
    i = int(np.argmax(bound))
    bad = want.copy()
    bad[i] += np.float32(4 * bound[i])
    with pytest.raises(en.Mismatch):
        judge(case, bad, "beyond the bound")
    bad = want.copy()
    j = int(np.argmin(bound))
    bad.view(np.uint32)[j] ^= 1  # a point that no interpolation decided has no allowance at all
    with pytest.raises(en.Mismatch):
        judge(case, bad, "one bit at a point without allowance")
    _compare.LEDGER[:] = [e for e in _compare.LEDGER if e[0] not in ("beyond the bound", "one bit at a point without allowance")]


# ---- inputs and dtypes ----
@pytest.mark.parametrize("options", [dict(), dict(symmetric=True, from_zero=True), dict(sort_clim=False, sort_ens=False, epsilon=0.5)],
                         ids=["default", "symmetric", "unsorted"])
def test_inputs_are_unchanged_after_a_call(options):
    case = next(c for c in CASES if c["note"] == "f32 11x7 normal sorts off unsorted")
    kw = cn.kwargs_of(case)
    clim, ens = kw["clim"].copy(), kw["ens"].copy()
    assert not (np.sort(clim, axis=0) == clim).all() and not (np.sort(ens, axis=0) == ens).all()
    twin(clim, ens, **options)
    cn.cpf(clim, ens, **options)
    assert np.array_equal(clim, kw["clim"]) and np.array_equal(ens, kw["ens"])


def test_mixed_dtypes_compute_in_f64_on_the_upcast_columns():
    mixed = [c for c in CASES if c["note"].startswith(("mixed", "integer"))]
    assert len(mixed) == 9
    for case in mixed:
        kw = cn.kwargs_of(case)
        up = dict(kw, clim=kw["clim"].astype(np.float64), ens=kw["ens"].astype(np.float64))
        en.judge_exact(twin(**kw), twin(**up, dtype=cn.F64), cn.case_id(case))
        en.judge_exact(twin(**kw), cn.cpf(**up), cn.case_id(case))


def test_mixed_dtype_deviation_stays_inside_its_bound():
    """Only clim f32: the reference rounds climate-row differences to f32, the product does not.  The recorded reference
    output is nowhere further from the f64 computation than the bound; the number of points that differ at all is
    printed (0 on the recorded cases)."""
    differing = 0
    for case in CASES:
        if cn.is_mixed_clim_f32(case):
            got = twin(**cn.kwargs_of(case))
            differing += int(np.sum(got != cn.expected_of(case)))
            judge(case, got, "cpf " + case["note"])
    print(f"mixed-dtype cpf: {differing} recorded points differ from the f64 computation")
