"""Child process of tests/test_gpu_long_quantiles.py::test_torch_device_tensors.

torch (a FOREIGN ROCm array library; test infrastructure only, the product never imports it) is imported and
initialised first, then ekm_hip, as in tests/_quantiles_torch_child.py.  Exit code 77 = torch has no ROCm device here."""
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

import _long_quantiles as lq  # noqa: E402

np.seterr(all="ignore")
dev = torch.device("cuda", ek.current_device())

count = rows_checked = 0
for case in lq.cases():
    kw = lq.kwargs_of(case)
    kw["arr"] = torch.from_numpy(np.ascontiguousarray(kw["arr"])).to(dev)
    got = ek.stats.long_quantiles(**kw)
    assert isinstance(got, torch.Tensor) and got.device == dev, (case["id"], type(got))
    lq.judge_case(case, got.cpu().numpy(), "torch " + case["note"])
    if case["note"].endswith("special axis middle numpy which 1"):
        rows = list(ek.stats.iter_long_quantiles(**kw))
        assert len(rows) == 2 and all(isinstance(r, torch.Tensor) and tuple(r.shape) == (2, 4) for r in rows)
        lq.judge_case(case, torch.stack(rows).cpu().numpy(), "torch rows " + case["note"])
        swapped = kw["arr"].permute(1, 0, 2)  # a view that is not contiguous: the same samples with the axes swapped
        assert not swapped.is_contiguous()
        lq.judge_case(case, ek.stats.long_quantiles(swapped, 1, 0, "numpy").cpu().numpy().reshape(2, 2, 4), "torch permuted " + case["note"])
        rows_checked += 1
    count += 1
    del kw, got
assert count == 234 and rows_checked == 2, (count, rows_checked)
torch.cuda.synchronize()
ek.synchronize()
print("LONG_QUANTILES_TORCH_OK:", count, "cases")
