"""Solar functions without a GPU: the independent restatement (tests/_solar_numpy.py) and the host twin of the kernel's
per-point routine (csrc/solar_point.hpp) against the results recorded from the reference
(tests/golden/solar_golden.npz), the node-record builder against the reference's recorded intermediate dates, weights
and host scalars (bit for bit), the sine / cosine in degrees, and the public signatures, result types and errors.

Parity: the absolute bar B(N) derived in tests/_solar_numpy.py, the same NaN pattern, no point excluded; the sign of
zero is not compared.  For f32 input the judge is the reference's run on the upcast inputs; the distance to its f32 run
is printed as a usage figure."""
import ctypes as C
import datetime as dt
import inspect

import numpy as np
import pytest

import _compare
import _hosttwin
import _solar_numpy as sn
from ekm_hip import _engine, _ffi, solar

CASES = sn.cases()
FN = {"instant": solar.cos_solar_zenith_angle, "integrated": solar.cos_solar_zenith_angle_integrated,
      "toa": solar.toa_incident_solar_radiation}


def records_of(func, dates, kwargs):
    if func == "instant":
        return solar.node_records(dates)
    d, w = solar.node_dates(dates[0], dates[1], **kwargs)
    return solar.node_records(d, w, func == "toa")


def twin_raw(tag, lat, lon, rec, n):
    """ekm_host_solar_<tag> on operands given as (array, (mode, len, inner)); the flat result in the entry's own dtype."""
    out = np.full(n, 7, np.float32 if tag == "f32" else np.float64)
    fn = getattr(_hosttwin.lib(), f"ekm_host_solar_{tag}")
    fn.restype = C.c_int
    args = []
    for a, cls in (lat, lon):
        args += [C.c_void_p(a.ctypes.data), C.c_int(cls[0]), C.c_ulonglong(cls[1]), C.c_ulonglong(cls[2])]
    rec = np.ascontiguousarray(rec, np.float64)
    assert fn(*args, C.c_void_p(rec.ctypes.data), C.c_uint(rec.shape[0]), C.c_void_p(out.ctypes.data), C.c_size_t(n)) == 0
    return out


def twin(func, dates, lat, lon, **kwargs):
    """One call through the host twin: the argument handling of ekm_hip.solar restated for ekm_host_solar_*."""
    lat, lon = np.asarray(lat), np.asarray(lon)
    rec = solar.kernel_records(records_of(func, dates, kwargs))
    both32 = lat.dtype == sn.F32 and lon.dtype == sn.F32
    if func == "instant":
        shape, T, out_dtype = np.broadcast_shapes(lat.shape, lon.shape), sn.F32 if both32 else sn.F64, sn.F64
    else:
        shape, T, out_dtype = lat.shape, sn.F32 if both32 else sn.F64, lat.dtype
    Out = out_dtype if T == out_dtype or (T, out_dtype) == (sn.F32, sn.F64) else sn.F64
    tag = "f32_f64" if (T, Out) == (sn.F32, sn.F64) else "f32" if T == sn.F32 else "f64"
    ops = []
    for a in (lat, lon):
        cls = _engine.classify(a.shape, shape)
        if cls is None:
            a, cls = np.broadcast_to(a, shape), (_ffi.FIELD, 0, 0)
        ops.append((np.ascontiguousarray(a, T), cls))
    out = twin_raw(tag, ops[0], ops[1], rec, int(np.prod(shape, dtype=np.int64))).reshape(shape)
    return out.astype(out_dtype)


# One test walks all recorded cases (a failure names its case), as the CPF tests do.
def test_restatement_against_the_recorded_reference():
    worst = 0.0
    for case in CASES:
        lat, lon = sn.inputs_of(case)
        got = sn.call(case["func"], sn.dates_of(case), lat, lon, **case["kwargs"])
        ref = sn.judged_against(case)
        used = sn.judge(got, ref, sn.allowed(ref, sn.nnodes_of(case), sn.scale_of(case)), "restatement " + case["id"], _compare.LEDGER)
        worst = max(worst, used)
    print(f"restatement against the reference: largest use of B(N) {worst:.3f}")


def test_host_twin_against_the_recorded_reference():
    worst = far32 = 0.0
    for case in CASES:
        lat, lon = sn.inputs_of(case)
        got = twin(case["func"], sn.dates_of(case), lat, lon, **case["kwargs"])
        worst = max(worst, sn.judge_case(case, got, "host twin " + case["id"], _compare.LEDGER))
        if sn.is_f32(case):  # usage figure, not judged: the distance to the reference's own f32 run
            want = sn.expected_of(case).astype(np.float64)
            with np.errstate(all="ignore"):
                far32 = max(far32, float(np.nanmax(np.abs(got.astype(np.float64) - want) / sn.scale_of(case), initial=0.0)))
    print(f"host twin against the reference: largest use of B(N) {worst:.3f}; distance to the reference's f32 run (not judged, "
          f"per unit of isr): {far32:.3e}")


def test_known_answers_of_the_reference_tests():
    known = sn.index()["known"]
    for iso, value in known["julian_day"]:
        assert np.isclose(solar.julian_day(dt.datetime.fromisoformat(iso)), value)
    for iso, (dec, tc) in known["declination"]:
        got = solar.solar_declination_angle(dt.datetime.fromisoformat(iso))
        assert np.isclose(got[0], dec) and np.isclose(got[1], tc)
    for iso, value in known["isr"]:
        assert np.isclose(solar.incoming_solar_radiation(dt.datetime.fromisoformat(iso)), value)
    day = [dt.datetime(2024, 4, 22), dt.datetime(2024, 4, 23)]
    assert np.allclose(twin("instant", [dt.datetime(2024, 4, 22, 12)], 40.0, 18.0), known["cos_sza"])
    for order in (1, 2, 3, 4):
        assert np.allclose(twin("integrated", day, 40.0, 18.0, integration_order=order), known["integrated"])
        assert np.allclose(sn.call("integrated", day, 40.0, 18.0, integration_order=order), known["integrated"])
    assert np.allclose(twin("toa", day, 40.0, 18.0), known["toa"])


def test_host_scalars_are_the_references_bit_for_bit():
    for name, s in sn.index()["scalars"].items():
        d = dt.datetime.fromisoformat(s["date"])
        dec, tc = solar.solar_declination_angle(d)
        assert float(solar.julian_day(d)).hex() == s["julian_day"], name
        assert (float(dec).hex(), float(tc).hex()) == (s["declination"], s["time_correction"]), name
        assert float(solar.incoming_solar_radiation(d)).hex() == s["isr"], name
        assert isinstance(dec, float) and isinstance(tc, float)


def test_node_records_are_the_references_bit_for_bit():
    """Dates, weights, julian days, declinations, time corrections, radiation and hours of every recorded node set:
    the product's builder and the restatement's own builder, both bit for bit."""
    sets = sn.index()["nodesets"]
    assert len(sets) == 48 and {len(v["dates"]) for v in sets.values()} >= {1, 3, 4, 72, 384}
    for key, v in sets.items():
        begin, end = dt.datetime.fromisoformat(v["begin"]), dt.datetime.fromisoformat(v["end"])
        dates, w = solar.node_dates(begin, end, **v["kwargs"])
        assert [d.isoformat() for d in dates] == v["dates"], key
        assert np.array_equal(w, sn.array(f"nodes.{key}.w")), key
        rec = solar.node_records(dates, w, radiation=True)
        own = sn.nodes(begin, end, radiation=True, **v["kwargs"])
        assert [d.isoformat() for d in own["dates"]] == v["dates"], key
        dec = np.deg2rad(sn.array(f"nodes.{key}.decl"))
        for r in (rec, own):
            assert np.array_equal(r["w"], sn.array(f"nodes.{key}.w")), key
            assert np.array_equal(r["sd"], np.sin(dec)) and np.array_equal(r["cd"], np.cos(dec)), key
            assert np.array_equal(r["tc"], sn.array(f"nodes.{key}.tc")), key
            assert np.array_equal(r["isr"], sn.array(f"nodes.{key}.isr")), key
            assert np.array_equal(r["h15"], (sn.array(f"nodes.{key}.hour") - 12) * 15.0), key
        assert np.array_equal([solar.julian_day(d) for d in dates], sn.array(f"nodes.{key}.jd")), key
        assert abs(w.sum() - 1.0) < 1e-14


def test_the_hour_angle_is_a_step_function_within_the_hour():
    a = solar.node_records([dt.datetime(2023, 7, 15, 9, 0), dt.datetime(2023, 7, 15, 9, 59, 59)])
    assert a["h15"][0] == a["h15"][1] == -45.0 and a["tc"][0] != a["tc"][1]


def test_every_case_the_issue_names_is_recorded():
    ids = [c["id"] for c in CASES]
    for tag in ("f64", "f32"):
        for n in (1, 63, 64, 65, 257):
            assert any(f".pts{n}.{tag}" in i for i in ids), (n, tag)
        assert f"instant.minutes.grid.{tag}" in ids and sn.expected_of(next(c for c in CASES if c["id"] == f"instant.minutes.grid.{tag}")).shape == (5, 67)
        for when in ("minutes90min", "midnight3h", "newyear3h", "tz1h", "known24h", "feb29_24h"):
            for iph, order in ((1, 3), (1, 1), (2, 2), (4, 4)):
                assert f"integrated.{when}.pts65.{tag}.int{order}.int{iph}" in ids
                assert f"toa.{when}.pts65.{tag}.int{order}.int{iph}" in ids
    lat, lon = sn.array("in.pts65.f64.lat"), sn.array("in.pts65.f64.lon")
    assert lat.max() == 90 and lat.min() == -90 and lon.min() == -360 and lon.max() == 720
    slat, slon = sn.array("in.special.f64.lat"), sn.array("in.special.f64.lon")
    assert np.isnan(slat).any() and np.isinf(slat).any() and np.isnan(slon).any() and np.isinf(slon).any()
    assert all((c["lat"] is None) or sn.is_f32(c) == (("out." + c["id"] + ".up") in sn._load()[1]) for c in CASES)


def test_nan_pattern_is_the_references():
    seen = 0
    for case in CASES:
        if ".special." in case["id"]:
            lat, lon = sn.inputs_of(case)
            want = sn.expected_of(case)
            bad = ~(np.isfinite(lat) & np.isfinite(lon))
            assert np.array_equal(np.isnan(want), bad), case["id"]  # the reference: NaN exactly at non-finite coordinates
            got = twin(case["func"], sn.dates_of(case), lat, lon, **case["kwargs"])
            assert np.array_equal(np.isnan(got), bad), case["id"]
            seen += 1
    assert seen >= 30


# ---- the sine and cosine in degrees ----
def _sincos_deg(x):
    x = np.ascontiguousarray(x, np.float64)
    s, c = np.empty_like(x), np.empty_like(x)
    fn = _hosttwin.lib().ekm_host_sincos_deg
    fn.restype = None
    fn(C.c_void_p(x.ctypes.data), C.c_void_p(s.ctypes.data), C.c_void_p(c.ctypes.data), C.c_size_t(x.size))
    return s, c


def test_sine_and_cosine_in_degrees_are_good_to_an_ulp():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-720, 720, 200000), rng.uniform(-1e6, 1e6, 20000), np.arange(-720.0, 721.0, 15.0),
                        rng.uniform(-1e-3, 1e-3, 1000), [1e15, -3e15, 2.0 ** 52, 2.0 ** 60 + 2.0 ** 8, 1e300, -1.7e308]])
    s, c = _sincos_deg(x)
    xl = x.astype(sn.L)
    if np.finfo(sn.L).eps < 1e-18:
        big = np.abs(x) >= 2.0 ** 52
        red = np.where(big, 0, np.fmod(xl, sn.L(360)))
        red[big] = [int(abs(v)) % 360 * (1 if v > 0 else -1) for v in x[big]]
        es, ec = np.sin(red * (sn.PI / 180)).astype(np.float64), np.cos(red * (sn.PI / 180)).astype(np.float64)
        err = max(np.abs(s - es).max(), np.abs(c - ec).max())
        print(f"sin / cos in degrees: largest absolute error {err:.3e} ({err / sn.U:.2f} u)")
        assert err <= 2 * sn.U  # 1 ulp of a value in [0.5, 1]: what the derivation of B(N) counts for every sine and cosine
    assert np.all(np.abs(s) <= 1) and np.all(np.abs(c) <= 1)
    # exact at the multiples of 90 degrees
    s, c = _sincos_deg(np.array([0.0, 90.0, 180.0, 270.0, 360.0, -90.0, 720.0, 450.0]))
    assert np.array_equal(np.abs(s), [0, 1, 0, 1, 0, 1, 0, 1]) and np.array_equal(np.abs(c), [1, 0, 1, 0, 1, 0, 1, 0])
    assert s[1] == 1 and s[3] == -1 and c[2] == -1 and s[5] == -1 and s[7] == 1
    s, c = _sincos_deg(np.array([np.nan, np.inf, -np.inf]))
    assert np.isnan(s).all() and np.isnan(c).all()


# ---- the public interface: signatures, result types and errors, no GPU involved ----
def test_signatures_are_the_references():
    assert str(inspect.signature(solar.cos_solar_zenith_angle)) == "(date, latitudes, longitudes)"
    want = "(begin_date, end_date, latitudes, longitudes, *, intervals_per_hour=1, integration_order=3)"
    assert str(inspect.signature(solar.cos_solar_zenith_angle_integrated)) == want
    assert str(inspect.signature(solar.toa_incident_solar_radiation)) == want
    for name in ("julian_day", "solar_declination_angle", "incoming_solar_radiation"):
        assert str(inspect.signature(getattr(solar, name))) == "(date)"
    import ekm_hip

    assert solar.array is solar and ekm_hip.solar is solar


def test_recorded_result_types():
    """What the goldens pin: float64 for the instantaneous function whatever the input, latitudes' dtype and shape for the
    integrated ones, a NumPy float64 scalar for Python scalars."""
    for case in CASES:
        want = sn.expected_of(case)
        if case["func"] == "instant":
            assert want.dtype == sn.F64, case["id"]
        elif case["lat"] is not None:
            assert want.dtype == sn.array(case["lat"]).dtype and want.shape == sn.array(case["lat"]).shape, case["id"]
    scalar = next(c for c in CASES if c["id"] == "instant.known.scalar.py")
    assert scalar["result_type"] == "float64" and scalar["shape"] == []


B0, B1 = dt.datetime(2024, 4, 22), dt.datetime(2024, 4, 23)


@pytest.mark.parametrize("fn", [solar.cos_solar_zenith_angle_integrated, solar.toa_incident_solar_radiation], ids=["integrated", "toa"])
def test_errors_of_the_integrated_functions(fn):
    lat, lon = np.zeros(4), np.zeros(4)
    for order in (0, 5, -1):
        with pytest.raises(ValueError):
            fn(B0, B1, lat, lon, integration_order=order)
    for iph in (0, -1):
        with pytest.raises(AssertionError):
            fn(B0, B1, lat, lon, intervals_per_hour=iph)
    with pytest.raises(AssertionError):
        fn(B1, B0, lat, lon)
    with pytest.raises(AssertionError):
        fn(B0, B0, lat, lon)
    with pytest.raises(AssertionError):  # 20 minutes at one interval per hour: int(1/3 + 0.5) = 0 sub-intervals
        fn(B0, B0 + dt.timedelta(minutes=20), lat, lon)
    with pytest.raises(TypeError):
        fn(B0, B1, np.array([1, 2, 3]), np.zeros(3))
    with pytest.raises(TypeError):
        fn(B0, B1, np.zeros(3, np.float16), np.zeros(3))
    with pytest.raises(ValueError):  # longitudes must broadcast TO latitudes' shape
        fn(B0, B1, np.zeros((5, 1)), np.zeros((1, 67)))
    with pytest.raises(ValueError):
        fn(B0, B1, np.zeros(3), np.zeros(4))
    with pytest.raises(TypeError):  # keyword-only
        fn(B0, B1, lat, lon, 2)


def test_errors_of_the_instantaneous_function():
    with pytest.raises(ValueError):
        solar.cos_solar_zenith_angle(B0, np.zeros(3), np.zeros(4))
    with pytest.raises(TypeError):
        solar.cos_solar_zenith_angle(B0, np.array(["a"]), np.zeros(1))


# ---- the judge rejects what it must ----
def test_judge_rejects_beyond_the_bar_a_wrong_nan_and_a_wrong_dtype():
    case = next(c for c in CASES if c["id"] == "integrated.known24h.pts257.f64")
    want = sn.expected_of(case)
    sn.judge_case(case, want.copy(), "the reference itself")
    bad = want.copy()
    bad[7] += 2 * sn.bar(72)
    with pytest.raises(sn.Mismatch):
        sn.judge_case(case, bad, "beyond the bar")
    bad = want.copy()
    bad[7] = np.nan
    with pytest.raises(sn.Mismatch):
        sn.judge_case(case, bad, "a NaN too many")
    with pytest.raises(sn.Mismatch):
        sn.judge_case(case, want.astype(np.float32), "wrong dtype")
    assert sn.bar(1) < 1.1e-14 and sn.bar(384) < 6e-14 <= sn.B_CAP
