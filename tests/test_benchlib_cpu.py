"""tools/_benchlib.py without a GPU: the call sequence of the event timer, the copy helper, the derived fields and the
final write, against a stub library that records every call and hands back a chosen elapsed time.

The checks are walked inside one test, not one test each (as tests/test_nanaverage_cpu.py walks its cases): a failure
names its check in the traceback."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

import _benchlib as bl  # noqa: E402

DEV = 0


class StubLib:
    """Every ekm_* call lands in `calls` as (name, arguments); ekm_event_elapsed_ms hands out `elapsed` in turn."""

    def __init__(self, elapsed=(5.0,)):
        self.calls, self.elapsed, self.handles = [], list(elapsed), 0

    def __getattr__(self, name):
        if not name.startswith("ekm_"):
            raise AttributeError(name)

        def call(*args):
            if name == "ekm_event_create":
                self.handles += 1
                args[1]._obj.value = 0x1000 * self.handles
            if name == "ekm_event_elapsed_ms":
                args[3]._obj.value = self.elapsed.pop(0)
            if name == "ekm_stream_mix":  # the pointer arrays as plain lists
                args = args[:2] + (list(args[2]), args[3], list(args[4])) + args[5:]
            self.calls.append((name, tuple(a.value if isinstance(a, C.c_void_p) else a for a in args)))
            return 0

        return call

    def names(self):
        return [name for name, _ in self.calls]


def window(steps):
    return ["ekm_event_record"] + ["launch"] * steps + ["ekm_event_record", "ekm_event_sync", "ekm_event_elapsed_ms"]


def check_single_timing_is_warmup_then_one_window(warmup, steps):
    lib = StubLib([5.0])
    with bl.EventTimer(lib, DEV, steps, warmup) as timer:
        assert lib.names() == ["ekm_event_create"] * 2
        e0, e1 = 0x1000, 0x2000
        del lib.calls[:]
        ms = timer.mean(lambda: lib.calls.append(("launch", ())))
        assert lib.names() == ["launch"] * warmup + window(steps)
        assert lib.names().count("launch") == warmup + steps
        # event 0 before the steps and event 1 after them, on the null stream; the sync and the elapsed time on that pair
        assert [a[:3] for n, a in lib.calls if n != "launch"] == [(DEV, e0, None), (DEV, e1, None), (DEV, e1), (DEV, e0, e1)]
        assert ms == 5.0 / steps


def check_repeated_timing_warms_up_once():
    elapsed = [5.0, 7.0, 6.0, 9.0]
    lib = StubLib(elapsed)
    with bl.EventTimer(lib, DEV, 10, 3) as timer:
        del lib.calls[:]
        out = timer.repeated(lambda: lib.calls.append(("launch", ())), 4)
    assert lib.names()[:-2] == ["launch"] * 3 + window(10) * 4
    assert out == [C.c_float(t).value / 10 for t in elapsed] and len(set(out)) == 4


def check_copy_rounds_down_to_16_bytes_and_passes_the_pointers_on():
    lib = StubLib([4.0, 4.0, 8.0, 2.0])
    with bl.EventTimer(lib, DEV, 2, 1) as timer:
        assert timer.copy([0xA0], [0xB0], 1000) == 2.0
        assert timer.copy([0xA0, 0xA4], [0xB0], 4096) == 2.0
        assert timer.copy([0xA0], [0xB0, 0xB4], 1000, reps=2) == [4.0, 1.0]
    mixes = [a for n, a in lib.calls if n == "ekm_stream_mix"]
    assert mixes[:3] == [(DEV, None, [0xA0], 1, [0xB0], 1, 992)] * 3
    assert mixes[3:6] == [(DEV, None, [0xA0, 0xA4], 2, [0xB0], 1, 4096)] * 3
    assert mixes[6:] == [(DEV, None, [0xA0], 1, [0xB0, 0xB4], 2, 992)] * 5
    assert bl.whole_words(1000) == 992 and bl.whole_words(992) == 992 and bl.whole_words(15) == 0


def check_derived_fields():
    d = bl.derived(2.0, 8e9, 5e12, 1e6)
    want = dict(bytes_per_s=4e12, copy_bytes_per_s=5e12, copy_ms_same_bytes=1.6, frac_copy_rate=0.8, frac_hbm_peak=0.5, points_per_s=5e8)
    assert list(d) == ["bytes_per_s", "copy_bytes_per_s", "copy_ms_same_bytes", "frac_copy_rate", "frac_hbm_peak", "points_per_s"]
    assert d == pytest.approx(want, rel=1e-15)
    assert bl.HBM_PEAK == 8.0e12
    assert list(bl.derived(2.0, 8e9, 5e12)) == list(d)[:-1]
    assert bl.derived(2.0, 8e9, None, 1e6) == pytest.approx(dict(bytes_per_s=4e12, frac_hbm_peak=0.5, points_per_s=5e8), rel=1e-15)


def check_emit_appends_and_prints_one_line(capsys):
    result = dict(elementwise=[], windrose=[])
    run = dict(call="speed", kernel_ms=1.5)
    bl.emit(result, "windrose", run)
    assert result == dict(elementwise=[], windrose=[run])
    assert capsys.readouterr().out == json.dumps(run) + "\n"


def check_write_creates_the_directory_and_sorts_keys(tmp_path):
    path = tmp_path / "missing" / "deeper" / "x_bench.json"
    result = dict(steps=10, device="d", runs=[dict(kernel_ms=1.0, dtype="f32")])
    bl.write(str(path), result)
    assert path.read_text() == json.dumps(result, indent=1, sort_keys=True)
    assert path.read_text().index('"device"') < path.read_text().index('"runs"') < path.read_text().index('"steps"')


def check_events_are_destroyed_on_exit_and_when_a_launch_raises():
    lib = StubLib()
    with bl.EventTimer(lib, DEV, 10, 3) as timer:
        timer.mean(lambda: None)
    assert lib.calls[-2:] == [("ekm_event_destroy", (DEV, 0x1000)), ("ekm_event_destroy", (DEV, 0x2000))]

    def failing():
        raise RuntimeError("launch failed")

    lib = StubLib()
    with pytest.raises(RuntimeError, match="launch failed"):
        with bl.EventTimer(lib, DEV, 10, 3) as timer:
            timer.mean(failing)
    assert lib.calls[-2:] == [("ekm_event_destroy", (DEV, 0x1000)), ("ekm_event_destroy", (DEV, 0x2000))]
    assert lib.names().count("ekm_event_destroy") == 2


def check_parser_flags_and_tag():
    args = bl.parser("x_bench.json").parse_args([])
    assert (args.steps, args.warmup, args.out) == (10, 3, os.path.join(bl.ROOT, "profiles", "x_bench.json"))
    import numpy as np

    assert [bl.tag(t) for t in (np.float32, np.dtype("float32"), np.float64)] == ["f32", "f32", "f64"]


def check_import_loads_no_library():
    env = dict(os.environ, EKM_THERMO_LIB="/nonexistent/libekm_thermo.so")
    code = "import sys; sys.path.insert(0, %r); import _benchlib; assert 'ekm_hip' not in sys.modules" % TOOLS
    subprocess.run([sys.executable, "-c", code], env=env, check=True)


def test_benchlib(capsys, tmp_path):
    check_single_timing_is_warmup_then_one_window(3, 10)
    check_single_timing_is_warmup_then_one_window(0, 1)
    check_repeated_timing_warms_up_once()
    check_copy_rounds_down_to_16_bytes_and_passes_the_pointers_on()
    check_derived_fields()
    check_emit_appends_and_prints_one_line(capsys)
    check_write_creates_the_directory_and_sorts_keys(tmp_path)
    check_events_are_destroyed_on_exit_and_when_a_launch_raises()
    check_parser_flags_and_tag()
    check_import_loads_no_library()
