"""The wind judges of tests/_wind_numpy.py must reject what they exist to catch: each case below hands a judge a
result that is wrong in one way and expects `Mismatch`."""
import numpy as np
import pytest

import _wind_numpy as wn

U = np.array([3.0, -2.0, 0.5, 1e-3, -7.0, 4.0])
V = np.array([1.0, 5.0, -0.25, -2.0, -7.0, 0.0])


@pytest.mark.parametrize("dtype", [wn.F32, wn.F64], ids=["f32", "f64"])
def test_a_direction_off_by_twice_the_bar(dtype):
    want = wn.direction(U, V)
    ok = (want + 0.5 * wn.bar_direction(dtype)).astype(dtype)
    wn.judge_direction(ok, ok.astype(wn.F64) - 0.5 * wn.bar_direction(dtype), U, V, "half the bar")
    bad = want.copy()
    bad[2] += 2 * wn.bar_direction(dtype)
    if dtype == wn.F32:
        bad = bad.astype(dtype)
        want = bad.astype(wn.F64)
        want[2] -= 2 * wn.bar_direction(dtype)
    with pytest.raises(wn.Mismatch):
        wn.judge_direction(bad, want, U, V, "twice the bar")


def test_a_wrap_away_from_the_branch_point():
    u, v = np.array([1.0, 0.0, 1e-3]), np.array([-1.0, -1.0, -1.0])
    want = np.array([315.0, 0.0, 359.9427042395855])
    wn.judge_direction(np.array([315.0, 360.0, 359.9427042395855]), want, u, v, "a wrap at the branch point")
    with pytest.raises(wn.Mismatch):  # 0 against 360 where u is not within 4 eps of 0
        wn.judge_direction(np.array([315.0, 0.0, 360.0]), np.array([315.0, 0.0, 0.0]), u, v, "a wrap elsewhere")
    with pytest.raises(wn.Mismatch):  # ... or where v > 0
        wn.judge_direction(np.array([360.0]), np.array([0.0]), np.array([0.0]), np.array([1.0]), "a wrap at v > 0")


def test_a_nan_moved():
    want = wn.direction(U, V)
    got = want.copy()
    got[1] = np.nan
    with pytest.raises(wn.Mismatch):
        wn.judge_direction(got, want, U, V, "a NaN too many")
    sp = wn.speed(U, V)
    sp_want = sp.copy()
    sp_want[0], sp[1] = np.nan, np.nan
    with pytest.raises(wn.Mismatch):
        wn.judge_speed(sp, sp_want, "a NaN moved")
    m, d = np.array([2.0, np.inf]), np.array([90.0, 90.0])
    a = wn.angle_of(d, "meteo")
    wn.judge_xy(np.array([-2.0, np.nan]), np.array([-2.0, -np.inf]), m, a, "NaN for inf beside an infinite magnitude")
    with pytest.raises(wn.Mismatch):
        wn.judge_xy(np.array([np.nan, -np.inf]), np.array([-2.0, -np.inf]), m, a, "a NaN beside a finite magnitude")
    with pytest.raises(wn.Mismatch):
        wn.judge_xy(np.array([-2.0, 1.0]), np.array([-2.0, -np.inf]), m, a, "a finite value for an infinite one")


def test_an_infinity_for_a_finite_value_beside_a_finite_magnitude():
    m, a = np.array([2.0]), wn.angle_of(np.array([45.0]), "polar")
    with pytest.raises(wn.Mismatch):
        wn.judge_xy(np.array([np.inf]), np.array([-1.414]), m, a, "inf for a finite value")
    with pytest.raises(wn.Mismatch):
        wn.judge_xy(np.array([1.0]), np.array([np.inf]), m, a, "a finite value for inf")
    with pytest.raises(wn.Mismatch):
        wn.judge_xy(np.array([-np.inf]), np.array([np.inf]), m, a, "the other infinity")
    with pytest.raises(wn.Mismatch):
        wn.judge_xy(np.array([np.nan]), np.array([np.inf]), m, a, "NaN for inf beside a finite magnitude")
    wn.judge_xy(np.array([np.inf], np.float32), np.array([1e39]), np.array([1e30]), a, "the float32 overflow of the float64 reference")
    with pytest.raises(wn.Mismatch):
        wn.judge_xy(np.array([np.inf]), np.array([0.5]), np.array([1.0]), a, "coriolis-like", scale=wn.TWO_OMEGA, c32=wn.C32_CORIOLIS)


def test_a_speed_and_a_component_off_by_twice_the_bar():
    want = wn.speed(U, V)
    with pytest.raises(wn.Mismatch):
        wn.judge_speed(want * (1 + 4 * wn.E64), want, "speed")
    m, d = np.array([10.0]), np.array([225.0])
    a = wn.angle_of(d, "meteo")
    x, _ = wn.polar_to_xy(m, d)
    with pytest.raises(wn.Mismatch):
        wn.judge_xy(x + 2 * wn.bar_xy(m, a, wn.F64), x, m, a, "x")


def test_counts_moved_or_off_by_one():
    rng = np.random.default_rng(5)
    want = wn.windrose(rng.uniform(0, 12, 500), rng.uniform(0, 360, 500), sectors=8, speed_bins=[0, 3, 6, 12], percent=False)
    wn.judge_rose((want[0].copy(), want[1].copy()), want, "the same")
    moved = want[0].copy()
    moved[1, 2] -= 1
    moved[1, 3] += 1  # the neighbouring sector, the sum unchanged
    with pytest.raises(wn.Mismatch):
        wn.judge_rose((moved, want[1]), want, "one count moved")
    off = want[0].copy()
    off[0, 0] += 1
    with pytest.raises(wn.Mismatch):
        wn.judge_rose((off, want[1]), want, "a count off by one")
    with pytest.raises(wn.Mismatch):
        wn.judge_rose((want[0], want[1].astype(np.float32)), want, "direction bins in another dtype")
