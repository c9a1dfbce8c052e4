"""The build switches of the kernel sources (-DEKM_*): the set in the code is the set documented in DESIGN.md section 4,
and every one of them still compiles with its non-default value (gfx950 front end only, no code generation)."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "earthkit-meteo_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")

# helper macros that appear in preprocessor conditions but are set by the sources themselves, never on the command line
INTERNAL = {"EKM_HD", "EKM_FD", "EKM_ANY", "EKM_WAVE_MASK", "EKM_TIE_NOINLINE", "EKM_HAVE_FDOUBLE_FAST", "EKM_OP_TABLE",
            "EKM_LEV_LAUNCH", "EKM_GEO_LAUNCH", "EKM_HIP"}
# translation unit (under csrc/) and non-default values; independent switches share one compiler run
CASES = [
    ("gen/entries_basic_f64.hip", ["-DEKM_F64_LIBM"]),
    ("gen/entries_basic_f64.hip", ["-DEKM_F64_TWO_PASS=0"]),
    ("gen/entries_wbpt_f32.hip", ["-DEKM_NO_TIE", "-DEKM_NO_WAVE_SKIP", "-DEKM_WALK_DEPTH=6", "-DEKM_TREE_WAVES=4",
                                  "-DEKM_TREE_THREADS=256"]),
    ("gen/entries_basic_f32.hip", ["-DEKM_NT_LOAD=0", "-DEKM_NT_STORE=0", "-DEKM_WAVES_PER_EU=2",
                                   "-DEKM_THREADS_DEFAULT=512"]),
    ("gen/entries_pipeline_f32.hip", ["-DEKM_P5_WAVES=4"]),
    ("hybrid.hip", ["-DEKM_GEO_THREADS=128"]),
]
KEPT = {re.match(r"-D(EKM_[A-Z0-9_]+)", d).group(1) for _, defs in CASES for d in defs}


def makefile_hipflags():
    with open(os.path.join(ROOT, "earthkit-meteo_amd", "Makefile")) as f:
        mk = f.read()
    flags = re.search(r"^HIPFLAGS\s*\?=\s*(.*)$", mk, re.M).group(1)
    return flags.replace("$(ARCH)", re.search(r"^ARCH\s*\?=\s*(\S+)", mk, re.M).group(1)).split()


def test_the_switches_in_the_sources_are_the_documented_ones():
    files = glob.glob(os.path.join(CSRC, "*.hpp")) + glob.glob(os.path.join(CSRC, "*.hip")) + [os.path.join(CSRC, "host_twin.cpp")]
    found = set()
    for path in files:
        with open(path) as f:
            for line in f:
                if re.match(r"\s*#\s*(ifn?def|if|elif)\b.*\bEKM_[A-Z0-9_]+", line):
                    found.update(re.findall(r"\bEKM_[A-Z0-9_]+", line.split("//")[0]))
    assert found - INTERNAL == KEPT
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    assert not [name for name in sorted(KEPT) if not re.search(r"`" + name + r"`", design)]


@pytest.mark.parametrize("unit,defs", CASES, ids=[" ".join(d) for _, d in CASES])
def test_every_switch_compiles_with_its_non_default_value(unit, defs):
    cmd = [HIPCC] + makefile_hipflags() + defs + ["-fsyntax-only", os.path.join(CSRC, unit)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
