"""Host logic of ekm_hip that needs no GPU: operand classification (what is handed to the
kernels as a field / scalar / level vector), dtype promotion, sharding, error conventions."""
import os
import numpy as np
import pytest

from ekm_hip import _engine, _ffi, _streamed
from ekm_hip.device import shard_bounds

F, S, MAJ, MIN = _ffi.FIELD, _ffi.SCALAR, _ffi.LEVEL_MAJOR, _ffi.LEVEL_MINOR


@pytest.mark.parametrize("shape,out,expect", [
    ((137, 1800, 3600), (137, 1800, 3600), (F, 0, 0)),
    ((), (137, 10), (S, 0, 0)),
    ((1,), (137, 10), (S, 0, 0)),
    ((1, 1), (137, 10), (S, 0, 0)),
    ((137, 1, 1), (137, 1800, 3600), (MAJ, 137, 1800 * 3600)),
    ((137, 1), (137, 10), (MAJ, 137, 10)),
    ((5, 7, 1), (5, 7, 9), (MAJ, 35, 9)),
    ((137,), (10, 137), (MIN, 137, 0)),
    ((1, 137), (10, 137), (MIN, 137, 0)),
    ((7, 9), (5, 7, 9), (MIN, 63, 0)),
    ((137, 1), (137, 2), None),          # inner < 4: materialised
    ((3,), (10, 3), None),               # len < 4: materialised
    ((5, 1, 9), (5, 7, 9), None),        # hole in the middle: materialised
    ((1, 7, 1), (5, 7, 9), None),        # middle axis only: materialised
    ((1,), (1,), (F, 0, 0)),
])
def test_classify(shape, out, expect):
    assert _engine.classify(shape, out) == expect


def test_classify_matches_numpy_broadcast_indexing():
    rng = np.random.default_rng(0)
    for shape, out in [((6, 1, 1), (6, 4, 5)), ((4, 5), (6, 4, 5)), ((6, 4, 1), (6, 4, 8)), ((8,), (3, 8))]:
        a = rng.normal(size=shape)
        full = np.broadcast_to(a.reshape((1,) * (len(out) - a.ndim) + a.shape), out).ravel()
        mode, ln, inner = _engine.classify(shape, out)
        i = np.arange(full.size)
        idx = i // inner if mode == MAJ else i % ln
        assert np.array_equal(a.ravel()[idx], full)


def test_result_dtype_follows_numpy_weak_scalars():
    f32, f64 = np.float32, np.float64
    r = _engine._result_dtype
    assert r([np.zeros(3, f32), 1.5]) == (np.dtype(f32), np.dtype(f32))
    assert r([np.zeros(3, f32), np.zeros(3, f64)]) == (np.dtype(f64), np.dtype(f64))
    assert r([np.zeros(3, np.int32), 2]) == (np.dtype(f64), np.dtype(f64))
    assert r([[1.0, 2.0], 3]) == (np.dtype(f64), np.dtype(f64))
    assert r([264.12, 85000.0]) == (np.dtype(f64), np.dtype(f64))
    assert r([np.zeros(3, np.float16), 1.0]) == (np.dtype(np.float16), np.dtype(f32))
    with pytest.raises(TypeError):
        r([np.zeros(3, np.complex64)])


@pytest.mark.parametrize("n,k", [(887760000, 8), (887760000, 2), (1038240, 4), (17, 4), (0, 3), (5, 8), (16, 1)])
def test_shard_bounds_partition(n, k):
    b = shard_bounds(n, k)
    assert len(b) == k and b[0][0] == 0 and b[-1][1] == n
    for (lo, hi), (lo2, _) in zip(b, b[1:]):
        assert hi == lo2 and lo <= hi
    assert all(lo % 16 == 0 for lo, hi in b if lo < n)  # 64-B aligned shard starts keep the float4 path


def test_error_conventions_raise_before_any_gpu_work():
    from ekm_hip import thermo

    t = np.array([280.0])
    p = np.array([9e4])
    assert thermo.saturation_vapour_pressure(t, phase="bogus") is None
    assert thermo.saturation_vapour_pressure_slope(t, phase="bogus") is None
    with pytest.raises(KeyError) as ei:
        thermo.ept_from_dewpoint(t, t - 2, p, method="bogus")
    assert ei.value.args == ("bogus",)
    with pytest.raises(ValueError, match="temperature_on_moist_adiabat: invalid t_method=bogus specified!"):
        thermo.temperature_on_moist_adiabat(t, p, t_method="bogus")
    with pytest.raises(ValueError, match="temperature_on_moist_adiabat: invalid t_method=direct specified!"):
        thermo.wet_bulb_temperature_from_dewpoint(t, t - 2, p, t_method="direct")
    with pytest.raises(ValueError, match="lcl_temperature: invalid method=bogus specified!"):
        thermo.lcl(t, t - 2, p, method="bogus")
    for f, args in ((thermo.specific_humidity_from_vapour_pressure, (t, p)),
                    (thermo.mixing_ratio_from_vapour_pressure, (t, p)),
                    (thermo.saturation_mixing_ratio_slope, (t, p)),
                    (thermo.saturation_specific_humidity_slope, (t, p))):
        with pytest.raises(ValueError, match=r"\(\): eps=-1 must be > 0"):
            f(*args, eps=-1)


def test_signatures_match_the_reference():
    """Names, argument order and defaults of the 39 reference functions."""
    import inspect
    import json

    from _golden import golden
    from ekm_hip import thermo
    from oracle import thermo_oracle as orc

    sigs = json.loads(bytes(golden()["signatures"]).decode())  # recorded from the reference by gen_golden.py
    assert sorted(sigs) == sorted(orc.ALL_FUNCTIONS) and len(sigs) == 39
    for name, sig in sigs.items():
        assert str(inspect.signature(getattr(thermo, name))) == sig, name
        assert str(inspect.signature(getattr(orc, name))) == sig, name


@pytest.mark.parametrize("n0,k", [(137, 8), (137, 1), (721, 4), (8, 8), (9, 8), (3, 2)])
def test_leading_axis_bounds(n0, k):
    b = _streamed.leading_axis_bounds(n0, k)
    assert len(b) == k and b[0][0] == 0 and b[-1][1] == n0
    assert all(hi == lo2 for (_, hi), (lo2, _) in zip(b, b[1:]))
    sizes = [hi - lo for lo, hi in b]
    assert max(sizes) - min(sizes) <= 1


def test_bisection_lattice_is_exact_in_fp32():
    """The LDS table of the IFS bisection (csrc/thermo_math.hpp::kBisectLattice, the search tree) relies on this: the
    reference's accumulated fp32 temperature (thermo.py:1055-1079: t = 253.16; dt /= 2; t += sign*dt) equals
    253.16f + M*120/2048 bit for bit at each of the 12 evaluations, for EVERY one of the 2^11 sign paths."""
    t0 = np.float32(273.16 - 20)
    step = np.float32(120.0 / 2048)
    paths = np.arange(2 ** 11, dtype=np.int64)
    t = np.full(paths.size, t0, np.float32)
    m = np.zeros(paths.size, np.int64)
    dt = np.float32(120.0)
    for it in range(12):
        lattice = (m.astype(np.float32) * step + t0).astype(np.float32)  # what the kernel's table is filled with
        assert lattice.dtype == np.float32 and np.array_equal(lattice, t), it
        assert np.array_equal(lattice.astype(np.float64), np.float64(t0) + m * (120.0 / 2048))  # exactly representable
        dt = np.float32(dt / np.float32(2))
        s = np.where((paths >> min(it, 10)) & 1, 1, -1)
        t = (t + s.astype(np.float32) * dt).astype(np.float32)
        m = m + s * (2048 >> (it + 1))
    assert -2048 < m.min() and m.max() < 2048


def test_foreign_device_arrays_are_adopted_implicitly(monkeypatch):
    """VERDICT r2 item 7 (reference: array_namespace(*inputs), thermo/array/thermo.py:826): an argument whose
    __dlpack_device__ says kDLROCM goes through from_dlpack without the caller asking; the result goes back through
    the producing library's from_dlpack only when EVERY array argument came from that one library.  Host logic only
    (the GPU side is tests/_dlpack_torch_child.py)."""
    import sys
    import types

    from ekm_hip import _engine, dlpack
    from ekm_hip.device import DeviceArray

    class Foreign:  # stands for a torch / cupy device tensor
        def __init__(self, tag, dev_type=10):
            self.tag, self.dev_type = tag, dev_type

        def __dlpack_device__(self):
            return (self.dev_type, 0)

        def __dlpack__(self, stream=None):
            raise AssertionError("from_dlpack is stubbed in this test")

        def __array__(self, dtype=None, copy=None):
            return np.array([1.0, 2.0])

    Foreign.__module__ = "fakelib.tensor"
    wrapped = []
    monkeypatch.setattr(dlpack, "from_dlpack", lambda x: wrapped.append(x.tag) or DeviceArray(None, 0, (2,), np.float32, 0))
    args, mod = _engine._adopt_foreign((Foreign("t"), Foreign("q"), 85000.0))
    assert wrapped == ["t", "q"] and mod == ("fakelib", "device") and all(isinstance(a, DeviceArray) for a in args[:2]) and args[2] == 85000.0
    _, mod = _engine._adopt_foreign((Foreign("t"), np.ones(2)))          # a NumPy array among them: our own types out
    assert mod is None
    _, mod = _engine._adopt_foreign((Foreign("t"), DeviceArray(None, 0, (2,), np.float32, 0)))
    assert mod is None
    # a HOST array of a foreign library (kDLCPU): viewed as NumPy (this one refuses the DLPack export: its own conversion),
    # and -- the reference returns the caller's type for every backend, CPU tensors included -- handed back through the library
    cpu = Foreign("c", dev_type=1)
    args, mod = _engine._adopt_foreign((cpu, 2.0))
    assert isinstance(args[0], np.ndarray) and args[0].tolist() == [1.0, 2.0] and mod == ("fakelib", "host")
    _, mod = _engine._adopt_foreign((cpu, Foreign("t")))                  # host and device arrays of one library mixed
    assert mod is None
    # handing back: through the library the CALLER imported, never imported here
    fake = types.ModuleType("fakelib")
    fake.from_dlpack = lambda r: ("fakelib tensor", r)
    fake.asarray = lambda r: ("fakelib scalar", r)
    monkeypatch.setitem(sys.modules, "fakelib", fake)
    r = DeviceArray(None, 0, (2,), np.float32, 0)
    assert _engine._hand_back((r,), ("fakelib", "device")) == (("fakelib tensor", r),)
    assert _engine._hand_back((r,), ("not_imported_lib", "device")) == (r,)
    h = np.arange(3.0)
    back = _engine._hand_back((h, np.float64(2.5)), ("fakelib", "host"))
    assert back[0][0] == "fakelib tensor" and back[0][1] is h and back[1] == ("fakelib scalar", np.float64(2.5))
    assert _engine._hand_back((h,), ("not_imported_lib", "host")) == (h,)


def test_array_namespaces_as_in_the_reference():
    """earthkit.meteo.{thermo,vertical,wind}.array.<name> is where the reference keeps its array-level functions
    (thermo/array/__init__.py:14, vertical/array/__init__.py:14-15, wind/array/__init__.py): the same names resolve here."""
    import ekm_hip

    assert ekm_hip.thermo.array.potential_temperature is ekm_hip.thermo.potential_temperature
    assert ekm_hip.vertical.array.pressure_on_hybrid_levels is ekm_hip.vertical.pressure_on_hybrid_levels
    assert ekm_hip.vertical.array.hybrid_level_parameters is ekm_hip.vertical.hybrid_level_parameters
    assert ekm_hip.vertical.array.height_on_hybrid_levels is ekm_hip.vertical.height_on_hybrid_levels
    assert ekm_hip.wind.array.w_from_omega is ekm_hip.wind.w_from_omega


def test_results_are_typed_as_the_reference_types_them():
    """ekm_hip/_dtype_rules.py (recorded from the reference by tests/golden/gen_dtype_rules.py) applied to what a NumPy call
    returns: a Python scalar is float64 where the reference passes that operand through asarray, weak elsewhere; theta_w
    "direct" is float64 from float32 arrays; temperature_on_moist_adiabat follows theta_e; lcl's t_lcl follows (t, td) in type
    and shape.  No GPU: the rule is applied to stand-in results."""
    import numpy as np

    from ekm_hip import _engine as e
    from ekm_hip._dtype_rules import RULES
    from ekm_hip.thermo import EPT_METHOD, LCL_METHOD, T_METHOD

    f = np.ones((3, 2), np.float32)
    d = np.ones((3, 2), np.float64)
    typed = lambda name, ints, args, outs: [(np.shape(o), np.asarray(o).dtype.char) for o in e._as_the_reference_types_them(name, ints, args, outs)]  # noqa: E731
    assert typed("potential_temperature", (), (280.0, f), (f.copy(),)) == [((3, 2), "d")]
    assert typed("potential_temperature", (), (f, f), (f.copy(),)) == [((3, 2), "f")]
    assert typed("relative_humidity_from_specific_humidity", (), (f, f, 9e4), (f.copy(),)) == [((3, 2), "f")]
    assert typed("relative_humidity_from_specific_humidity", (), (280.0, f, f), (f.copy(),)) == [((3, 2), "d")]
    direct = (EPT_METHOD["ifs"], T_METHOD["direct"])
    assert typed("wet_bulb_potential_temperature_from_specific_humidity", direct, (f, f, f), (f.copy(),)) == [((3, 2), "d")]
    bis = (EPT_METHOD["ifs"], T_METHOD["bisect"])
    assert typed("temperature_on_moist_adiabat", bis, (f, d), (d.copy(),)) == [((3, 2), "f")]
    lcl = (LCL_METHOD["davies"],)
    assert typed("lcl", lcl, (f[:, :1], f[:1, :1], d), (d.copy(), d.copy())) == [((3, 1), "f"), ((3, 2), "d")]
    assert typed("lcl", lcl, (f, f, d), (d.copy(), d.copy())) == [((3, 2), "f"), ((3, 2), "d")]
    assert typed("lcl", lcl, (f, f, f), (f.copy(), f.copy())) == [((3, 2), "f"), ((3, 2), "f")]
    # the reference's bisection runs on atleast_1d(theta_e): 0-d operands come back with shape (1,); Newton's stay 0-d
    assert typed("temperature_on_moist_adiabat", bis, (320.0, 9e4), (np.float64(290.0),)) == [((1,), "d")]
    assert typed("temperature_on_moist_adiabat", (EPT_METHOD["ifs"], T_METHOD["newton"]), (320.0, 9e4), (np.float64(290.0),)) == [((), "d")]
    # a DeviceArray-like operand (anything that is not NumPy / a Python scalar) leaves the results alone
    assert typed("potential_temperature", (), (object(), 280.0), (f.copy(),)) == [((3, 2), "f")]
    # the table is data: entry points the library has, kinds of the right length, float32 / float64 only
    from ekm_hip._optable import OPS
    for (name, ints), rules in RULES.items():
        nin, nout = len(OPS[name][0]), len(OPS[name][1])
        assert len(ints) == len(OPS[name][2])
        for kinds, chars in rules.items():
            assert len(kinds) == nin and set(kinds) <= set("fds") and len(chars) == nout
            assert set(chars) <= (set("dpa") if set(kinds) == {"s"} else set("fd"))
    # calls on Python scalars alone: a Python float where the reference's function is plain arithmetic, a 0-d array where it
    # fills a result buffer (saturation_vapour_pressure, phase "mixed"), np.float64 otherwise
    from ekm_hip.thermo import PHASE
    out = e._as_the_reference_types_them("celsius_to_kelvin", (), (7.0,), (np.float64(280.16),))
    assert type(out[0]) is float
    out = e._as_the_reference_types_them("saturation_vapour_pressure", (PHASE["mixed"],), (280.0,), (np.float64(991.0),))
    assert isinstance(out[0], np.ndarray) and out[0].shape == () and out[0].dtype == np.float64
    out = e._as_the_reference_types_them("potential_temperature", (), (280.0, 9e4), (np.float64(288.0),))
    assert type(out[0]) is np.float64


def test_the_typing_table_regenerates_from_the_reference(tmp_path):
    """ekm_hip/_dtype_rules.py is what tests/golden/gen_dtype_rules.py derives, byte for byte, from the result dtypes
    recorded from the reference (tests/golden/dtype_rules_recorded.json) and today's entry-point mapping of the package."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "rules.py"
    subprocess.run([sys.executable, os.path.join(root, "tests", "golden", "gen_dtype_rules.py"), str(out)], check=True, capture_output=True, timeout=600)
    assert out.read_text() == open(os.path.join(root, "earthkit-meteo_amd", "ekm_hip", "_dtype_rules.py")).read()


def test_pinned_pool_bound_follows_the_memory_cgroup(tmp_path):
    """MemAvailable is host-wide; page-locked memory is charged to the container's cgroup and cannot be
    reclaimed, so the pool's default bound is clamped by the cgroup's headroom (v2 memory.max, v1 memory.limit_in_bytes)."""
    from ekm_hip.device import _PinnedPool

    assert _PinnedPool._cgroup_headroom(str(tmp_path)) is None  # no controller files: no finite limit
    (tmp_path / "memory.max").write_text("max\n")
    (tmp_path / "memory.current").write_text("123\n")
    assert _PinnedPool._cgroup_headroom(str(tmp_path)) is None
    (tmp_path / "memory.max").write_text(f"{8 << 30}\n")
    (tmp_path / "memory.current").write_text(f"{3 << 30}\n")
    assert _PinnedPool._cgroup_headroom(str(tmp_path)) == 5 << 30
    (tmp_path / "memory").mkdir()
    (tmp_path / "memory" / "memory.limit_in_bytes").write_text("9223372036854771712\n")  # v1's "unlimited"
    (tmp_path / "memory" / "memory.usage_in_bytes").write_text("1\n")
    assert _PinnedPool._cgroup_headroom(str(tmp_path)) == 5 << 30
    (tmp_path / "memory" / "memory.limit_in_bytes").write_text(f"{4 << 30}\n")
    (tmp_path / "memory" / "memory.usage_in_bytes").write_text(f"{1 << 30}\n")
    assert _PinnedPool._cgroup_headroom(str(tmp_path)) == 3 << 30
    assert 0 <= _PinnedPool.machine_limit() <= 16 << 30


def test_pinned_pool_does_not_flush_its_cache_for_a_request_that_cannot_fit():
    """take() used to evict every cached block of the other sizes before noticing that the request could not fit
    beside what the callers hold."""
    from ekm_hip.device import _PinnedPool

    pool = _PinnedPool()
    pool.limit = pool.live_limit = 64 << 20
    pool.free = {8 << 20: [0xdead0000]}      # one cached 8-MiB block (never dereferenced: nothing below allocates or frees)
    pool.cached = 8 << 20
    pool.handed_out = 40 << 20               # the callers hold 40 MiB
    ptr, b = pool.take(32 << 20)             # 40 + 32 > 64: cannot fit whatever is evicted
    assert ptr is None and b == 32 << 20
    assert pool.cached == 8 << 20 and pool.free[8 << 20] == [0xdead0000]
