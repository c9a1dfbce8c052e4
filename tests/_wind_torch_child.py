"""Child process of tests/test_gpu_wind.py::test_torch_device_tensors.

torch (a FOREIGN ROCm array library; test infrastructure only, the product never imports it) is imported and
initialised first, then ekm_hip, as in tests/_solar_torch_child.py.  Exit code 77 = torch has no ROCm device here."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, ROOT, os.path.join(ROOT, "earthkit-meteo_amd")]

import numpy as np  # noqa: E402

try:
    import torch
except ImportError:
    print("torch is not installed")
    sys.exit(77)
if not torch.cuda.is_available():
    print("torch sees no ROCm device")
    sys.exit(77)
torch.zeros(1, device="cuda").cpu()  # initialise torch's HIP context before the other library loads

import ekm_hip as ek  # noqa: E402

import _wind_numpy as wn  # noqa: E402
from test_wind_cpu import rose_inputs  # noqa: E402

np.seterr(all="ignore")
dev = torch.device("cuda", ek.current_device())
TDT = {wn.F32: torch.float32, wn.F64: torch.float64}

count = 0
for case in wn.cases():
    if case["tag"] not in ("f32", "f64", "mixed"):
        continue
    ins = wn.inputs_of(case)
    tens = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in ins]
    got = getattr(ek.wind, case["func"])(*tens, **case["kwargs"])
    got = got if isinstance(got, tuple) else (got,)
    for g, w in zip(got, wn.expected_of(case)):
        assert isinstance(g, torch.Tensor) and g.device == dev and g.dtype == TDT[w.dtype] and tuple(g.shape) == w.shape, (case["id"], type(g))
    wn.judge_case(case, tuple(g.cpu().numpy() for g in got), "torch " + case["id"])
    assert all(np.array_equal(t.cpu().numpy(), a, equal_nan=True) for t, a in zip(tens, ins)), case["id"]
    count += 1
for case in wn.cases("windrose"):
    sp, di, bins = rose_inputs(case)
    if case["scalar"] or np.asarray(sp).dtype not in TDT or np.asarray(di).dtype not in TDT or np.asarray(sp).size == 0:
        continue
    t_sp, t_di = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (sp, di))
    got = ek.wind.windrose(t_sp, t_di, sectors=case["sectors"], speed_bins=bins, percent=case["percent"])
    assert all(isinstance(g, torch.Tensor) and g.device == dev for g in got), case["id"]
    wn.judge_rose(tuple(g.cpu().numpy() for g in got), wn.expected_of(dict(case, nout=2)), "torch " + case["id"])
    count += 1
assert count > 150, count
torch.cuda.synchronize()
ek.synchronize()
print("WIND_TORCH_OK:", count, "cases")
