"""The launch-shape knobs of csrc/map_kernel.hpp::launch_map -- ekm_set_tuning(tiles_per_block, unroll), the tuning
parameters table_tiles, lev_per_wg and hybrid_band_kb, and the size heuristics (ntile >= 4096) -- reach kernel bodies
and grids no other test runs: map_fields<Op, T, 2> for every family, tiles per workgroup between 1 and the census's 16,
level walks of other lengths than 4, band counts that do not divide the row.  The sweep runs in ONE fresh child process
(tests/_launch_shapes_child.py says why and what it asserts); this test starts it, waits, and checks that it printed a
line for every family x knob value."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_launch_shape_sweep_in_a_child_process(ek):
    import _launch_shapes_child as child  # (the tables only: nothing of it runs in this process)

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_launch_shapes_child.py")
    r = subprocess.run([sys.executable, path], capture_output=True, text=True, timeout=1500)
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    bad = [ln for ln in lines if ln.get("ok") is False]
    assert r.returncode == 0 and not bad, f"{bad[:2]}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
    assert lines and lines[-1] == {"done": True}, r.stdout[-1500:]
    seen = {(ln["family"], ln["tag"], ln["mode"], ln["knob"], str(ln["value"])) for ln in lines if "knob" in ln}
    fams = {f: (child.MODES if len(child.OPS[name][0]) > 1 else ("field",)) for f, name, _ in child.FAMILIES}
    missing = []
    for fam, modes in fams.items():
        for tag in ("f32", "f64"):
            for ntile in (4095, 4096, 4097):
                for knob, value in (("default", f"ntile={ntile}"), ("tiles_per_block,unroll", f"1,1 ntile={ntile}"),
                                    ("tiles_per_block,unroll", f"2,2 ntile={ntile}")):
                    missing += [(fam, tag, "field", knob, value)] if (fam, tag, "field", knob, value) not in seen else []
            for mode in modes:
                want = [("default", "moderate")] + [("tiles_per_block,unroll", f"{t},{u}") for t in child.TILES for u in child.UNROLL]
                want += [("table_tiles", str(v)) for v in child.TABLE_TILES]
                if mode == "hybrid":
                    want += [("hybrid_band_kb", str(v)) for v in child.BAND_KB]
                missing += [(fam, tag, mode) + w for w in want if (fam, tag, mode) + w not in seen]
    for fam in ("two-in", "three-in three-out"):
        for tag in ("f32", "f64"):
            missing += [(fam, tag, "hybrid", "lev_per_wg", f"{v} levels={nlev}") for v in child.LEV_PER_WG for nlev in (1, 5, 137)
                        if (fam, tag, "hybrid", "lev_per_wg", f"{v} levels={nlev}") not in seen]
    for fam in ("tree ifs", "tree bolton35", "tree bolton39"):
        missing += [(fam, "f32", "field", "table_tiles (large)", str(v)) for v in (0,) + child.TABLE_TILES
                    if (fam, "f32", "field", "table_tiles (large)", str(v)) not in seen]
    missing += [("two-in", "f32", "hybrid", "hybrid_band_kb (large)", str(v)) for v in (8192, 64, 1 << 20)
                if ("two-in", "f32", "hybrid", "hybrid_band_kb (large)", str(v)) not in seen]
    assert not missing, missing[:10]
    notes = [ln for ln in lines if ln.get("note")]
    print(f"\nlaunch-shape sweep: {len(lines) - 1} cases in the child, {len(seen)} distinct (family, dtype, mode, knob, value)")
    for ln in notes[:6]:
        print("  note:", ln["family"], ln["tag"], ln["value"], ln["note"])
