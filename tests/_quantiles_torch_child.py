"""Child process of tests/test_gpu_quantiles.py::test_torch_device_tensors.

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

import _quantiles_numpy as qn  # noqa: E402

np.seterr(all="ignore")
dev = torch.device("cuda", ek.current_device())
TDT = {qn.F32: torch.float32, qn.F64: torch.float64}

count = 0
for case in qn.value_cases():
    kw = qn.kwargs_of(case)
    if kw["arr"].dtype not in TDT or not case["rows"]:  # integer input stays NumPy; no rows: nothing to hand back
        continue
    kw["arr"] = torch.from_numpy(np.ascontiguousarray(kw["arr"])).to(dev)
    got = ek.stats.quantiles(**kw)
    assert isinstance(got, torch.Tensor) and got.device == dev, (case["id"], type(got))
    qn.judge_case(case, got.cpu().numpy(), "torch " + case["note"])
    if case["note"].endswith("cube axis 1 numpy which 4"):
        rows = list(ek.stats.iter_quantiles(**kw))
        assert len(rows) == 5 and all(isinstance(r, torch.Tensor) and tuple(r.shape) == (4, 5) for r in rows)
        qn.judge_case(case, torch.stack(rows).cpu().numpy(), "torch rows " + case["note"])
        # a view that is not contiguous: the same samples with the axes swapped
        swapped = kw["arr"].permute(1, 0, 2)
        assert not swapped.is_contiguous()
        qn.judge_case(case, ek.stats.quantiles(swapped, 4, 0, "numpy").cpu().numpy(), "torch permuted " + case["note"])
        count += 100000
    count += 1
    del kw, got
assert count > 200000 + 600, count
torch.cuda.synchronize()
ek.synchronize()
print("QUANTILES_TORCH_OK:", count % 100000, "cases")
