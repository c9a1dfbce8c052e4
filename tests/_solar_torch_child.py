"""Child process of tests/test_gpu_solar.py::test_torch_device_tensors.

torch (a FOREIGN ROCm array library; test infrastructure only, the product never imports it) is imported and
initialised first, then ekm_hip, as in tests/_cpf_torch_child.py.  Exit code 77 = torch has no ROCm device here."""
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

import _solar_numpy as sn  # noqa: E402

np.seterr(all="ignore")
dev = torch.device("cuda", ek.current_device())
TDT = {sn.F32: torch.float32, sn.F64: torch.float64}

count = 0
for case in sn.cases():
    if case["lat"] is None or sn.array(case["lat"]).dtype not in TDT:
        continue
    lat, lon = sn.inputs_of(case)
    t_lat, t_lon = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (lat, lon))
    fn = getattr(ek.solar, sn.FUNCS[case["func"]])
    got = fn(*sn.dates_of(case), t_lat, t_lon, **case["kwargs"])
    want = sn.expected_of(case)
    assert isinstance(got, torch.Tensor) and got.device == dev and got.dtype == TDT[want.dtype] and tuple(got.shape) == want.shape, \
        (case["id"], type(got))
    sn.judge_case(case, got.cpu().numpy(), "torch " + case["id"])
    assert np.array_equal(t_lat.cpu().numpy(), lat, equal_nan=True) and np.array_equal(t_lon.cpu().numpy(), lon, equal_nan=True), case["id"]
    count += 1
    del t_lat, t_lon, got
assert count > 250, count
torch.cuda.synchronize()
ek.synchronize()
print("SOLAR_TORCH_OK:", count, "cases")
