"""Child process of tests/test_gpu_interp.py::test_torch_device_tensors_through_the_four_functions.

torch (a FOREIGN ROCm array library; test infrastructure only, the product never imports it) is imported and
initialised first, then ekm_hip, as in tests/_dlpack_torch_child.py.  Exit code 77 = torch has no ROCm device here."""
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

import _interp_golden as gold  # noqa: E402
import _interp_numpy as inp  # noqa: E402

np.seterr(all="ignore")
dev = torch.device("cuda", ek.current_device())
TDT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}


def is_field(k, v):
    return isinstance(v, np.ndarray) and k not in ("A", "B") and v.ndim > 0 and v.dtype in TDT


count = {}
for case in gold.cases():
    kw = gold.kwargs_of(case)
    if kw.get("vertical_axis"):
        continue  # device tensors are level-major
    tens = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if is_field(k, v) else v) for k, v in kw.items()}
    fn = getattr(ek.vertical, case["func"])
    got = fn(**tens)
    want = gold.expected_of(case)
    arith = inp.arith_dtype(*[v for k, v in kw.items() if isinstance(v, np.ndarray)])
    assert isinstance(got, torch.Tensor) and got.device == dev and tuple(got.shape) == want.shape, (case["id"], type(got))
    assert got.dtype == TDT[np.dtype(arith)], (case["id"], got.dtype)  # device results stay in the arithmetic dtype
    host = got.cpu().numpy().astype(want.dtype)
    if case["func"] == "interpolate_hybrid_to_height_levels":
        # the height field is the GPU's own: the same bits as the DeviceArray path, which test_gpu_interp.py judges
        devs = {k: (ek.to_device(v) if is_field(k, v) else v) for k, v in kw.items()}
        same = fn(**devs)
        assert isinstance(same, ek.DeviceArray) and inp.same_bits(got.cpu().numpy(), same.to_host()), case["id"]
    else:
        gold.judge_case(case, host, "torch " + case["note"])  # linear / nearest: bit for bit against the recorded reference
    count[case["func"]] = count.get(case["func"], 0) + 1
    del tens, got
assert len(count) == 4 and all(count.values()), count
torch.cuda.synchronize()
ek.synchronize()
print("INTERP_TORCH_OK:", ", ".join(f"{k} {v}" for k, v in sorted(count.items())))
