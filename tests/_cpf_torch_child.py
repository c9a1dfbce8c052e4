"""Child process of tests/test_gpu_cpf.py::test_torch_device_tensors.

torch (a FOREIGN ROCm array library; test infrastructure only, the product never imports it) is imported and
initialised first, then ekm_hip, as in tests/_ensemble_torch_child.py.  Exit code 77 = torch has no ROCm device here."""
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

import _cpf_numpy as cn  # noqa: E402
import _ensemble_numpy as en  # noqa: E402

np.seterr(all="ignore")
dev = torch.device("cuda", ek.current_device())
TDT = {cn.F32: torch.float32, cn.F64: torch.float64}

count = 0
for case in cn.cases():
    kw = cn.kwargs_of(case)
    tens = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) and v.dtype in TDT else v)
            for k, v in kw.items()}
    got = ek.extreme.cpf(**tens)
    want = cn.expected_of(case)
    if all(v.dtype in TDT for v in kw.values() if isinstance(v, np.ndarray)):
        assert isinstance(got, torch.Tensor) and got.device == dev and got.dtype == torch.float32 and tuple(got.shape) == want.shape, \
            (case["id"], type(got))
        host = got.cpu().numpy()
    else:  # an integer array stays a NumPy argument beside the tensors: the result is not handed back to torch
        assert isinstance(got, ek.DeviceArray), (case["id"], type(got))
        host = got.to_host()
    for k, v in tens.items():  # the inputs are never written
        if isinstance(v, torch.Tensor):
            assert np.array_equal(v.cpu().numpy(), kw[k], equal_nan=True), (case["id"], k)
    if cn.is_mixed_clim_f32(case):
        bound = cn.mixed_cpf_bound(kw["clim"], kw["ens"], **cn.options_of(case))
        assert (np.abs(host.astype(np.float64) - want.astype(np.float64)) <= bound).all(), case["id"]
    else:
        en.judge_exact(host, want, "torch " + case["note"])
    count += 1
    del tens, got
assert count == len(cn.cases()) and count > 400
torch.cuda.synchronize()
ek.synchronize()
print("CPF_TORCH_OK:", count, "cases")
