"""extreme.long_cpf without a GPU: the host twin of `long_cpf_tiles` (the kernel's whole-number keys, std::sort where a
flag asks for it, then cpf_value_running of csrc/ensemble_point.hpp) against what the reference gave on columns the short
`cpf` refuses (tests/golden/long_cpf_golden.npz), against the host twin of the short kernel on a census (the running
maximum of cpf_point_running against the quadratic priming loop of cpf_point) and against the NumPy restatement
`_cpf_numpy.cpf`, imported unchanged, at two shapes beyond the recorded ones; the public signature, the errors that
need no device, the C signatures and the one host body.

Parity: bit for bit, with identical NaN pattern and result dtype (float32), no point excluded, f32 and f64."""
import inspect
import os
import re

import numpy as np
import pytest

import _cpf_numpy as cn
import _long_cpf as lc
from ekm_hip import _ffi, extreme

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = pytest.mark.parametrize("T", [lc.F32, lc.F64], ids=["f32", "f64"])


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_host_twin_against_the_recorded_reference(tag):
    cases = lc.cases(tag)
    assert len(cases) == 72
    for case in cases:
        lc.judge_case(case, lc.twin(**lc.kwargs_of(case)), "twin " + lc.case_id(case))


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_restatement_against_the_recorded_reference(tag):
    """This is what makes the restatement the reference at shapes that are not recorded."""
    for case in lc.cases(tag):
        lc.judge_case(case, cn.cpf(**lc.kwargs_of(case)), "restatement " + lc.case_id(case))


def test_every_case_the_issue_names_is_recorded():
    notes = [c["note"] for c in lc.cases()]
    assert len(notes) == len(set(notes)) == 144
    for nclim, nens in lc.SHAPES:
        for tag in ("f32", "f64"):
            for option in lc.OPTION_NOTES:
                assert f"{tag} {nclim}x{nens} {option}" in notes
    kinds, reversed_used = set(), False
    for case in lc.cases():
        kw, want = lc.kwargs_of(case), lc.expected_of(case)
        clim, ens = kw["clim"], kw["ens"]
        T = lc.F32 if case["dtype"] == "f32" else lc.F64
        assert clim.dtype == ens.dtype == T and want.dtype == np.float32 and want.shape == (24,) == clim.shape[1:] == ens.shape[1:]
        assert clim.shape[0] + ens.shape[0] > lc.SHORT_ROWS[lc.F32]  # the short function refuses it when it sorts the climate
        assert lc.no_column_mixes_the_zeros(clim) and lc.no_column_mixes_the_zeros(ens)
        assert not np.isnan(want[16:18]).any()  # a NaN column does not give NaN (an infinite one may: inf - inf)
        if case["perm"]:  # the unsorted climate is unsorted, the unsorted ensemble is
            assert not (np.diff(clim[:, :12], axis=0) >= 0).all(axis=0).any()
        if not case["presort_ens"]:
            assert not (np.diff(ens[:, :12], axis=0) >= 0).all(axis=0).any()
        # the special columns of gen_golden_long_cpf.py
        assert np.isnan(clim[:, 16]).sum() == 1 and np.isnan(ens[:, 17]).sum() == 1
        assert ens[:, 18].max() == np.inf and ens[:, 19].min() == -np.inf and clim[:, 20].min() == -np.inf and clim[:, 20].max() == np.inf
        assert np.unique(clim[:, 12]).size == 1 and np.unique(ens[:, 12]).size == 1 and (clim[:, 13] == 0).all()
        assert np.nanmax(ens[:, 14]) < np.nanmin(clim[:, 14]) and np.nanmin(ens[:, 15]) > np.nanmax(clim[:, 15])
        assert all(np.unique(ens[:, j]).size < ens.shape[0] for j in range(8, 12))  # ties
        _, kind, rev = cn.cpf_with_kinds(**kw)
        kinds |= {(int(k), bool(kw.get("from_zero"))) for k in kind}
        reversed_used = reversed_used or bool(rev.any())
    # every kind of write decides a recorded point; the lower-tail interpolation is reached with from_zero
    assert {k for k, _ in kinds} == {cn.NONE, cn.LOWER, cn.PLAIN, cn.UPPER} and (cn.LOWER, True) in kinds and reversed_used


CENSUS_SHAPES = ((101, 51), (11, 7), (3, 1), (3, 2), (5, 3), (101, 3), (200, 20), (200, 120), (40, 280), (280, 40), (17, 64), (2, 5))


@TYPES
def test_running_maximum_scan_is_the_quadratic_scan_on_a_census(T):
    """cpf_point_running against cpf_point, through the two host twins, bit for bit: 12 shapes with nens + nclim <= 320,
    1800 random columns each (21600 per dtype: ties on a 1/8 grid, NaN, +inf and -inf columns, constant columns), every
    one under the 12 option sets -- sorted and as-given columns, `symmetric`, `from_zero`, `epsilon`.  The census reaches
    every kind of write."""
    rng = np.random.default_rng(20261023)
    kinds, columns = set(), 0
    for nclim, nens in CENSUS_SHAPES:
        assert nclim + nens <= 320
        clim, ens = lc.fields(rng, nclim, nens, 1800, T)
        assert lc.no_column_mixes_the_zeros(clim) and lc.no_column_mixes_the_zeros(ens)
        columns += clim.shape[1]
        for options in lc.OPTION_SETS:
            lc.judge_exact(lc.twin(clim, ens, **options), lc.short_twin(clim, ens, **options), f"{nclim}x{nens} {options}")
        for from_zero in (False, True):
            kinds |= {int(k) for k in np.unique(cn.cpf_with_kinds(clim, ens, from_zero=from_zero)[1])}
    assert columns >= 20000 and kinds == {cn.NONE, cn.LOWER, cn.PLAIN, cn.UPPER}
    assert len(lc.OPTION_SETS) == 12 and any(not o.get("sort_ens", True) for o in lc.OPTION_SETS)


@pytest.mark.parametrize("T,nclim,nens", [(lc.F32, 4097, 4097), (lc.F64, 8192, 33)], ids=["f32-4097x4097", "f64-8192x33"])
def test_twin_against_the_restatement_beyond_the_recorded_shapes(T, nclim, nens):
    rng = np.random.default_rng(nclim + nens)
    clim, ens = lc.fields(rng, nclim, nens, 12, T)
    for options in (dict(), dict(symmetric=True, from_zero=True), dict(sort_clim=False, sort_ens=False, from_zero=True),
                    dict(sort_ens=False, epsilon=0.5)):
        lc.judge_exact(lc.twin(clim, ens, **options), cn.cpf(clim, ens, **options), f"{nclim}x{nens} {options}")


def test_twin_refuses_what_the_entry_points_refuse():
    import ctypes as C

    import _hosttwin

    for T in (lc.F32, lc.F64):
        fn = getattr(_hosttwin.lib(), f"ekm_host_long_cpf_{lc.TAG[T]}")
        fn.restype = C.c_int
        a, out = np.zeros(4, T), np.zeros(1, np.float32)
        for nclim, nens in ((0, 3), (3, 0), (lc.CAP[T] + 1, 3), (3, lc.CAP[T] + 1)):
            rc = fn(C.c_void_p(a.ctypes.data), C.c_void_p(a.ctypes.data), C.c_uint(nclim), C.c_uint(nens), C.c_size_t(1),
                    C.c_int(1), C.c_int(1), C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.0), C.c_void_p(out.ctypes.data))
            assert rc == -2, (nclim, nens)


def test_signature_is_the_references_and_the_short_siblings():
    assert str(inspect.signature(extreme.long_cpf)) == lc.signature() == cn.signature() == str(inspect.signature(extreme.cpf))


def test_argument_errors_need_no_device():
    clim, ens = np.zeros((700, 4)), np.zeros((700, 4))
    with pytest.raises(ValueError, match="must be 2-D"):
        extreme.long_cpf(clim[0], ens)
    with pytest.raises(ValueError, match="must be 2-D"):
        extreme.long_cpf(clim.reshape(700, 2, 2), ens.reshape(700, 2, 2))
    with pytest.raises(ValueError, match="at least one row each"):
        extreme.long_cpf(clim[:0], ens)
    with pytest.raises(ValueError, match="at least one row each"):
        extreme.long_cpf(clim, ens[:0])
    with pytest.raises(AssertionError):  # cpf.py:138
        extreme.long_cpf(clim, ens[:, :3])


def _c_arguments(text, name):
    """The argument types of one EKM_API declaration, reduced to what ctypes tells apart."""
    decl = re.search(r"EKM_API\s+int\s+" + name + r"\s*\(([^;]*?)\)\s*;", text).group(1)
    kinds = []
    for arg in decl.split(","):
        arg = " ".join(arg.split())
        ctype = arg.rsplit(" ", 1)[0]
        kinds.append("ptr" if "*" in arg else ctype.replace("const ", ""))
    return kinds


def test_header_and_binding_agree_on_the_entry_points():
    import ctypes as C

    text = open(os.path.join(ROOT, "include", "ekm_thermo.h")).read()
    names = {C.c_int: "int", C.c_void_p: "ptr", C.c_uint32: "uint32_t", C.c_size_t: "size_t", C.c_double: "double"}
    for tag in ("f32", "f64"):
        long_args, short_args = _c_arguments(text, f"ekm_long_cpf_{tag}"), _c_arguments(text, f"ekm_cpf_{tag}")
        assert long_args == short_args and len(long_args) == 14
        fn = getattr(_ffi.lib(), f"ekm_long_cpf_{tag}")
        assert [names[a] for a in fn.argtypes] == long_args and fn.restype is C.c_int
        assert f"ekm_long_cpf_{tag}" in _ffi.declared_symbols()
    assert int(re.search(r"#define EKM_ABI_VERSION (\d+)", text).group(1)) == 5  # an addition: the version stays


def test_long_and_short_share_their_host_code(monkeypatch):
    """One body: `long_cpf` and `cpf` differ in the family of entry points they name, nothing else."""
    seen = []
    monkeypatch.setattr(extreme, "_cpf", lambda *a: seen.append(a[2:]) or "r")
    a = np.zeros((3, 2))
    assert extreme.cpf(a, a, False, True, 0.5, True, True) == extreme.long_cpf(a, a, False, True, 0.5, True, True) == "r"
    assert extreme.cpf(a, a) == extreme.long_cpf(a, a) == "r"
    assert seen == [(False, True, 0.5, True, True, "ekm_cpf_"), (False, True, 0.5, True, True, "ekm_long_cpf_"),
                    (True, True, None, False, False, "ekm_cpf_"), (True, True, None, False, False, "ekm_long_cpf_")]


def test_the_docs_no_longer_deny_a_long_form():
    assert "no long form" not in extreme.__doc__
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "long_cpf" in design and "long_cpf" in extreme.__doc__
