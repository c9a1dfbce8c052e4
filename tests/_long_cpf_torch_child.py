"""Child process of tests/test_gpu_long_cpf.py::test_torch_device_tensors.

torch (a FOREIGN ROCm array library; test infrastructure only, the product never imports it) is imported and
initialised first, then ekm_hip, as in tests/_long_ensemble_torch_child.py.  Exit code 77 = torch has no ROCm device here."""
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

import _long_cpf as lc  # noqa: E402

np.seterr(all="ignore")
dev = torch.device("cuda", ek.current_device())
count = 0
for case in lc.cases():
    if "1980x51" not in case["note"]:  # one shape, both dtypes, the 12 option sets
        continue
    kw = lc.kwargs_of(case)
    tens = {k: (torch.from_numpy(np.array(v)).to(dev) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    before = {k: v.clone() for k, v in tens.items() if isinstance(v, torch.Tensor)}
    got = ek.extreme.long_cpf(**tens)
    assert isinstance(got, torch.Tensor) and got.device == dev and got.dtype == torch.float32, (case["id"], type(got))
    lc.judge_case(case, got.cpu().numpy(), "torch " + case["note"])
    assert all(torch.equal(before[k].view(torch.uint8), tens[k].view(torch.uint8)) for k in before), case["id"]  # inputs unwritten
    count += 1
    del tens, got, before
assert count == 24, count
torch.cuda.synchronize()
ek.synchronize()
print("LONG_CPF_TORCH_OK:", count, "cases")
