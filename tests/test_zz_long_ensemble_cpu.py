"""extreme.long_efi, extreme.long_sot, score.long_crps_from_ensemble and stats.GumbelDistribution.long_fit without a GPU:
the host twins of the kernels (std::sort on the kernel's whole-number keys, then efi_point / sot_point / crps_point /
gumbel_fit_point of csrc/ensemble_point.hpp) and the NumPy restatements of `_ensemble_numpy` / `_gumbel_numpy`, imported
unchanged, against what the reference gave on member axes of 257 to 1980 values
(tests/golden/long_ensemble_golden.npz); the public signatures and the errors that need no device.

Parity: bit for bit, with identical NaN pattern and result dtype, no point excluded, f32 and f64."""
import inspect

import numpy as np
import pytest

import _long_ensemble as le
from ekm_hip import extreme, score, stats

GROUPS = [(func, tag) for func in le.FUNCS for tag in ("f32", "f64")]
COUNT = {"efi": 20, "sot": 20, "crps_from_ensemble": 5, "fit": 5}  # recorded cases per dtype


@pytest.mark.parametrize("func,tag", GROUPS)
def test_host_twin_against_the_recorded_reference(func, tag):
    cases = le.cases(func, tag)
    assert len(cases) == COUNT[func]
    for case in cases:
        le.judge_case(case, le.twin_case(case), "twin " + le.case_id(case))


@pytest.mark.parametrize("func,tag", GROUPS)
def test_restatement_against_the_recorded_reference(func, tag):
    """This is what makes the restatements the reference of the GPU tests at member counts that are not recorded."""
    for case in le.cases(func, tag):
        le.judge_case(case, le.restate_case(case), "restatement " + le.case_id(case))


def test_every_case_the_issue_names_is_recorded():
    notes = {(c["func"], c["note"]) for c in le.cases()}
    for tag in ("f32", "f64"):
        for m in le.MS:
            for eps in (-0.1, 0.5):
                for kind in ("sorted", "unsorted"):
                    assert ("efi", f"{tag} m {m} {kind} clim eps {eps}") in notes
            for perc in (10, 90):
                for eps in (-1e4, 0.75):
                    assert ("sot", f"{tag} m {m} perc {perc} eps {eps}") in notes
            assert ("crps_from_ensemble", f"{tag} m {m}") in notes and ("fit", f"{tag} m {m}") in notes
    assert len(notes) == len(le.cases()) == 100
    for case in le.cases():
        kw = le.kwargs_of(case)
        ens = kw["ens" if "ens" in kw else "x" if "x" in kw else "sample"]
        T = le.F32 if case["note"].startswith("f32") else le.F64
        assert ens.dtype == T and ens.shape[0] > 256 and ens.shape[1] >= 24  # beyond both short caps, a few dozen points
        assert all(v.dtype == T for v in kw.values() if isinstance(v, np.ndarray))
        # the columns: smooth (distinct but for chance), heavy ties, one NaN, +inf, -inf
        distinct = np.array([np.unique(ens[:, j]).size for j in range(ens.shape[1])])
        assert (distinct[:10] >= 0.9 * ens.shape[0]).all() and (distinct[10:20] < ens.shape[0] // 4).all()
        assert np.isnan(ens[:, 20]).sum() == 1 and ens[:, 21].max() == np.inf and ens[:, 22].min() == -np.inf
        for v in kw.values():  # no column mixes the two zeros
            if isinstance(v, np.ndarray) and v.ndim == 2:
                assert le.no_column_mixes_the_zeros(v)
        if case["func"] in ("efi", "sot"):
            assert kw["clim"].shape == (101, ens.shape[1])
            is_sorted = bool((np.diff(kw["clim"], axis=0) >= 0).all())
            assert is_sorted == ("unsorted" not in case["note"])
        want = le.expected_of(case)
        if case["func"] == "fit":
            assert np.isnan(want[0][20]) and np.isnan(want[1][20]) and np.isfinite(want[0][:20]).all()
        elif case["func"] != "sot":
            assert np.isnan(want[20]) and np.isfinite(want[:9]).all()
        else:
            assert np.isnan(want[20])
    eps_pos = le.expected_of(next(c for c in le.cases("sot") if c["note"] == "f64 m 300 perc 10 eps 0.75"))
    eps_neg = le.expected_of(next(c for c in le.cases("sot") if c["note"] == "f64 m 300 perc 10 eps -10000.0"))
    assert np.isfinite(eps_pos[10:15]).all() and np.isfinite(eps_neg[10:15]).all()
    assert (eps_pos[10:15] != eps_neg[10:15]).all()  # the positive eps is not a no-op on the tie columns


def test_signatures_are_the_short_siblings():
    for long_fn, short_fn in ((extreme.long_efi, extreme.efi), (extreme.long_sot, extreme.sot),
                              (score.long_crps_from_ensemble, score.crps_from_ensemble),
                              (stats.GumbelDistribution.long_fit, stats.GumbelDistribution.fit)):
        assert str(inspect.signature(long_fn)) == str(inspect.signature(short_fn))
    assert inspect.ismethod(stats.GumbelDistribution.long_fit) and stats.GumbelDistribution.long_fit.__self__ is stats.GumbelDistribution


def test_argument_errors_need_no_device():
    clim, ens = np.zeros((101, 4)), np.zeros((300, 4))
    with pytest.raises(ValueError, match="must be 2-D"):
        extreme.long_efi(clim[0], ens)
    with pytest.raises(AssertionError):
        extreme.long_efi(clim, ens[:, :3])
    for perc in (1, 99, 90.0):
        with pytest.raises(Exception, match="Percentile value should be and Integer between 2 and 98"):
            extreme.long_sot(clim, ens, perc)
    with pytest.raises(Exception, match="cannot be 50"):
        extreme.long_sot(clim, ens, 50)
    with pytest.raises(Exception, match="should contain 101 percentiles"):
        extreme.long_sot(clim[:100], ens, 90)
    with pytest.raises(ValueError, match="point dimensions differ"):
        extreme.long_sot(clim, ens[:, :3], 90)
    with pytest.raises(ValueError, match="nan_policy must be 'raise', 'propagate', or 'omit'"):
        score.long_crps_from_ensemble(ens, ens[0], nan_policy="drop")
    with pytest.raises(ValueError, match=r"must be \(n_ens,\) \+ the shape of y"):
        score.long_crps_from_ensemble(ens, ens[0, :3])
    bad = ens.copy()
    bad[7, 1] = np.nan
    with pytest.raises(ValueError, match="Missing values present in input and nan_policy=raise"):
        score.long_crps_from_ensemble(bad, ens[0], nan_policy="raise")
    with pytest.raises(ValueError, match="at least two values"):
        stats.GumbelDistribution.long_fit(np.zeros((1, 4)))
    with pytest.raises(ValueError, match="at least one dimension"):
        stats.GumbelDistribution.long_fit(np.float64(3.0))
    with pytest.raises(np.exceptions.AxisError):
        stats.GumbelDistribution.long_fit(ens, axis=2)


def test_no_result_without_work_needs_no_device():
    dist = stats.GumbelDistribution.long_fit(np.zeros((700, 0)), freq=2.0)
    assert isinstance(dist, stats.GumbelDistribution) and dist.shape == (0,) and dist.freq == 2.0


def test_long_and_short_share_their_host_code(monkeypatch):
    """One body each: a long function and its short sibling differ in the family of entry points they name, nothing else."""
    seen = []
    monkeypatch.setattr(extreme, "_efi", lambda *a: seen.append(a[2:]) or "r")
    monkeypatch.setattr(extreme, "_sot", lambda *a: seen.append(a[2:]) or "r")
    monkeypatch.setattr(score, "_crps_from_ensemble", lambda *a: seen.append(a[2:]) or "r")
    monkeypatch.setattr(stats.GumbelDistribution, "_fit", classmethod(lambda cls, *a: seen.append(a[1:]) or "r"))
    a = np.zeros((3, 2))
    assert extreme.efi(a, a, 0.5) == extreme.long_efi(a, a, 0.5) == "r"
    assert extreme.sot(a, a, 90, 0.5) == extreme.long_sot(a, a, 90, 0.5) == "r"
    assert score.crps_from_ensemble(a, a[0], "omit") == score.long_crps_from_ensemble(a, a[0], "omit") == "r"
    assert stats.GumbelDistribution.fit(a, 1, 3.0) == stats.GumbelDistribution.long_fit(a, 1, 3.0) == "r"
    assert seen == [(0.5, "ekm_efi_"), (0.5, "ekm_long_efi_"), (90, 0.5, "ekm_sot_"), (90, 0.5, "ekm_long_sot_"),
                    ("omit", "ekm_crps_from_ensemble_"), ("omit", "ekm_long_crps_from_ensemble_"),
                    (1, 3.0, "ekm_gumbel_fit_"), (1, 3.0, "ekm_long_gumbel_fit_")]


@pytest.mark.parametrize("T", [le.F32, le.F64], ids=["f32", "f64"])
def test_twin_of_a_short_axis_is_the_short_twins(T):
    """Short axes go through the same arithmetic: the long twins equal the restatements at member counts the short kernels
    take, the shortest included."""
    rng = np.random.default_rng(5)
    for nens in (1, 2, 33, le.SHORT_CAP[T]):
        ens, clim = le.field(rng, nens, 9, T), le.climate(rng, 9, T)
        for eps in (-0.1, 0.5):
            le.judge_exact(le.twin_efi(clim, ens, eps), le.restate("efi", clim=clim, ens=ens, eps=eps), f"efi {nens} {eps}")
        for eps in (-1e4, 0.75):
            le.judge_exact(le.twin_sot(clim, ens, 90, eps), le.restate("sot", clim=clim, ens=ens, perc=90, eps=eps), f"sot {nens} {eps}")
        y = ens[0] + T.type(0.5)
        le.judge_exact(le.twin_crps(ens, y), le.restate("crps_from_ensemble", x=ens, y=y), f"crps {nens}")
        if nens >= 2:
            got, want = le.twin_fit(ens), le.restate("fit", sample=ens)
            le.judge_exact(got[0], want[0], f"fit mu {nens}")
            le.judge_exact(got[1], want[1], f"fit sigma {nens}")
