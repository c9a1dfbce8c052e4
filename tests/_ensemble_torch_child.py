"""Child process of tests/test_gpu_ensemble.py::test_torch_device_tensors.

torch (a FOREIGN ROCm array library; test infrastructure only, the product never imports it) is imported and
initialised first, then ekm_hip, as in tests/_interp_torch_child.py.  Exit code 77 = torch has no ROCm device here."""
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

import _ensemble_numpy as en  # noqa: E402

np.seterr(all="ignore")
dev = torch.device("cuda", ek.current_device())
TDT = {en.F32: torch.float32, en.F64: torch.float64}
FUNCS = {"efi": ek.extreme.efi, "sot": ek.extreme.sot, "sot_func": ek.extreme.sot_func,
         "crps_from_ensemble": ek.score.crps_from_ensemble}

count = {}
for case in en.cases():
    if case["raises"]:
        continue
    kw = en.kwargs_of(case)
    tens = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) and v.dtype in TDT else v)
            for k, v in kw.items()}
    got = FUNCS[case["func"]](**tens)
    want = en.expected_of(case)
    if all(v.dtype in TDT for v in kw.values() if isinstance(v, np.ndarray)):
        assert isinstance(got, torch.Tensor) and got.device == dev and tuple(got.shape) == want.shape, (case["id"], type(got))
        host = got.cpu().numpy()
    else:  # an integer array stays a NumPy argument beside the tensors: the result is not handed back to torch
        assert isinstance(got, ek.DeviceArray), (case["id"], type(got))
        host = got.to_host()
    if case["func"] == "efi" and not en.is_mixed_efi(case):
        nclim = kw["clim"].shape[0]
        own = ek.extreme.efi_coefficients(nclim)
        if not all(np.array_equal(a, b) for a, b in zip(own, en.recorded_tables(nclim))):
            want = en.efi(**kw, tables=own)  # another libm: the restatement with the product's own tables, still in bits
            en.judge_exact(host, want, "torch " + case["note"] + " [other EFI coefficients than recorded]")
            continue
    en.judge_case(case, host, "torch " + case["note"])
    count[case["func"]] = count.get(case["func"], 0) + 1
    del tens, got
assert len(count) == 4 and all(count.values()), count
torch.cuda.synchronize()
ek.synchronize()
print("ENSEMBLE_TORCH_OK:", ", ".join(f"{k} {v}" for k, v in sorted(count.items())))
