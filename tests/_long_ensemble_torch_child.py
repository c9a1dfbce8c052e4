"""Child process of tests/test_gpu_long_ensemble.py::test_torch_device_tensors.

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

import _long_ensemble as le  # noqa: E402

np.seterr(all="ignore")
dev = torch.device("cuda", ek.current_device())
FUNCS = {"efi": ek.extreme.long_efi, "sot": ek.extreme.long_sot, "crps_from_ensemble": ek.score.long_crps_from_ensemble,
         "fit": ek.stats.GumbelDistribution.long_fit}
own = ek.extreme.efi_coefficients(101)
same_libm = all(np.array_equal(a, b) for a, b in zip(own, le.recorded_tables()))

count = {}
for case in le.cases():
    kw = le.kwargs_of(case)
    tens = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    got = FUNCS[case["func"]](**tens)
    if case["func"] == "fit":
        assert isinstance(got, ek.stats.GumbelDistribution), (case["id"], type(got))
        assert all(isinstance(v, torch.Tensor) and v.device == dev and v.dtype == torch.float64 for v in (got.mu, got.sigma)), case["id"]
        host = (got.mu.cpu().numpy(), got.sigma.cpu().numpy())
        if case["note"].endswith("m 300"):  # the class's functions on the fitted tensors: torch out
            cdf = got.cdf([290.0, 300.0])
            assert isinstance(cdf, torch.Tensor) and tuple(cdf.shape) == (2,) + tuple(got.mu.shape)
    else:
        assert isinstance(got, torch.Tensor) and got.device == dev, (case["id"], type(got))
        host = got.cpu().numpy()
    if case["func"] == "efi" and not same_libm:  # another libm: the restatement with the product's own tables, still in bits
        le.judge_exact(host, le.restate_case(case, tables=own), "torch " + case["note"] + " [other EFI coefficients than recorded]")
    else:
        le.judge_case(case, host, "torch " + case["note"])
    count[case["func"]] = count.get(case["func"], 0) + 1
    del tens, got
assert count == {"efi": 40, "sot": 40, "crps_from_ensemble": 10, "fit": 10}, count
torch.cuda.synchronize()
ek.synchronize()
print("LONG_ENSEMBLE_TORCH_OK:", ", ".join(f"{k} {v}" for k, v in sorted(count.items())))
