#!/usr/bin/env python3
"""Record the REFERENCE's result dtypes for every function x variant x operand kind and write the deviations from plain
weak-scalar promotion as data into the package (earthkit-meteo_amd/ekm_hip/_dtype_rules.py).

Two steps.  Where the reference is importable, `python tests/golden/gen_dtype_rules.py --record` calls it for every case and
stores what it returned, as data, in tests/golden/dtype_rules_recorded.json.  `python tests/golden/gen_dtype_rules.py [OUT]`
derives the rules from that recording and writes them (default: the package's _dtype_rules.py); it needs no reference, so
tests/test_engine_host.py replays it.

The reference's result dtype is not one rule: a Python float is weak where a function uses the operand as it comes and
float64 where it passes it through `xp.asarray` first (potential_temperature(280.0, p_f32) is float64,
relative_humidity_from_specific_humidity(t_f32, q_f32, 9e4) float32); two Python floats divided by each other feed
`power` and come back as a float64 scalar; theta_w "direct" is float64 even from float32 arrays (the float64 coefficient
lists of polyval); temperature_on_moist_adiabat takes its dtype from theta_e alone; lcl's first output depends on (t, td)
only.  Operand kinds: f = float32 array, d = float64 array (and whatever NumPy turns into one: ints, lists), s = Python
scalar.  Only data is written: (entry point, enum arguments) -> {kinds: result dtype characters}; for a call on Python scalars alone: p = Python float, a = 0-d array (d = np.float64, not stored)."""
import itertools
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("EKM_REFERENCE", "/root/reference")
RECORDED = os.path.join(HERE, "dtype_rules_recorded.json")
sys.path[:0] = [HERE, ROOT, os.path.join(ROOT, "earthkit-meteo_amd"), os.path.join(ROOT, "tests")]

import _fuzz  # noqa: E402
from ekm_hip import _engine, thermo  # noqa: E402

warnings.simplefilter("ignore")
np.seterr(all="ignore")


class _Seen(Exception):
    pass


def entry_of(func, operands, kwargs):
    """(entry point, enum arguments) that ekm_hip.thermo.<func> launches for these keyword arguments."""
    seen = []

    def fake(name, args, ints=(), eps=None, dtype=None):
        seen.append((name, tuple(int(i) for i in ints)))
        raise _Seen()

    real, _engine.run = _engine.run, fake
    try:
        getattr(thermo, func)(*operands, **kwargs)
    except _Seen:
        pass
    finally:
        _engine.run = real
    assert len(seen) == 1, (func, kwargs, seen)
    return seen[0]


def _mk(kind, key, shape=(3,)):
    v = _fuzz.TYPICAL[key]
    return float(v) if kind == "s" else np.full(shape, v, np.float32 if kind == "f" else np.float64)


def _key(func, kw, kinds):
    return f"{func}|{json.dumps(kw, sort_keys=True)}|{kinds}"


def record():
    """Call the reference for every case x operand kinds; {case key: what it returned, or null where it raised}.  Calls
    on Python scalars alone give p = Python float, a = 0-d array, d = np.float64, ? = anything else; the others the
    dtype characters of their outputs."""
    sys.path[:0] = [os.path.join(HERE, "_standin"), os.path.join(REF, "src")]
    from earthkit.meteo.thermo import array as ref

    seen = {}
    for func, keys, kw in _fuzz._case_table():
        for kinds in itertools.product("fds", repeat=len(keys)):
            got = None
            if all(k == "s" for k in kinds):
                try:
                    out = getattr(ref, func)(*[_mk("s", key) for key in keys], **kw)
                except Exception:
                    out = None
                if out is not None:
                    out = out if isinstance(out, tuple) else (out,)
                    got = "".join("p" if type(o) is float else ("a" if isinstance(o, np.ndarray) and o.ndim == 0 else
                                                               ("d" if isinstance(o, np.float64) else "?")) for o in out)
            else:
                try:
                    out = getattr(ref, func)(*[_mk(k, key) for k, key in zip(kinds, keys)], **kw)
                except Exception:
                    # the reference raises on N-d operands of these kinds (a mask index into what a Python scalar made 0-d);
                    # with 0-d arrays the same call may go through: that typing then (the N-d call has none to compare with)
                    try:
                        out = getattr(ref, func)(*[_mk(k, key, ()) for k, key in zip(kinds, keys)], **kw)
                    except Exception:
                        out = None
                if out is not None:
                    out = out if isinstance(out, tuple) else (out,)
                    got = "".join(np.asarray(o).dtype.char for o in out)
            seen[_key(func, kw, "".join(kinds))] = got
    return seen


def main():
    if sys.argv[1:] == ["--record"]:
        seen = record()
        with open(RECORDED, "w") as f:
            json.dump(seen, f, indent=0, sort_keys=True)
            f.write("\n")
        print(f"{RECORDED}: {len(seen)} calls of the reference")
        return
    with open(RECORDED) as f:
        seen = json.load(f)
    rules = {}
    for func, keys, kw in _fuzz._case_table():
        entry = entry_of(func, [_mk("d", k) for k in keys], {k: v for k, v in kw.items() if k != "eps"})
        dev = rules.setdefault(entry, {})
        for kinds in itertools.product("fds", repeat=len(keys)):
            got = seen[_key(func, kw, "".join(kinds))]
            if got is None:
                continue  # the reference raised: no rule, the library's own promotion stands
            if all(k == "s" for k in kinds):
                # every operand a Python scalar: np.float64 mostly; a Python float where the function is plain arithmetic
                # ('p'), a 0-d array where it fills a result buffer ('a': saturation_vapour_pressure, phase "mixed")
                if "?" not in got and set(got) != {"d"}:
                    dev["".join(kinds)] = got
                continue
            assert set(got) <= {"f", "d"}, (func, kw, kinds, got)
            plain = ("d" if "d" in kinds else "f") * len(got)
            if got != plain:
                dev["".join(kinds)] = got
    rules = {k: v for k, v in rules.items() if v}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "earthkit-meteo_amd", "ekm_hip", "_dtype_rules.py")
    with open(path, "w") as f:
        f.write('"""GENERATED by tests/golden/gen_dtype_rules.py from the reference: where its result dtype is NOT the plain promotion of\n'
                'the operands with Python scalars weak.  (entry point, enum arguments) -> {operand kinds: result dtype per output};\n'
                'kinds: f = float32 array, d = float64 array (ints, lists), s = Python scalar.  Data only."""\n\nRULES = {\n')
        for k in sorted(rules):
            f.write(f"    {k!r}: {dict(sorted(rules[k].items()))!r},\n")
        f.write("}\n")
    print(f"{path}: {len(rules)} entries, {sum(len(v) for v in rules.values())} deviations")


if __name__ == "__main__":
    main()
