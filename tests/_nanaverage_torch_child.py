"""Child process of tests/test_gpu_nanaverage.py::test_torch_device_tensors.

torch (a FOREIGN ROCm array library; test infrastructure only, the product never imports it) is imported and
initialised first, then ekm_hip, as in tests/_regimes_torch_child.py.  Exit code 77 = torch has no ROCm device here."""
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
from ekm_hip import stats  # noqa: E402

import _nanaverage_numpy as nn  # noqa: E402

np.seterr(all="ignore")
dev = torch.device("cuda", ek.current_device())


def to_torch(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


plain = weighted = 0
for case in nn.cases():
    d, w, kw = nn.call_of(case)
    if case["raises"] or case["product_raises"] or d.dtype not in (nn.F32, nn.F64) or d.ndim == 0 or d.size == 0:
        continue
    axis, keepdims, want = kw.get("axis"), kw.get("keepdims", False), nn.recorded(case)
    if want.ndim == 0:  # (a tensor result has at least one axis on the way back)
        continue
    t = to_torch(d)
    tw = to_torch(w) if w is not None and w.dtype in (nn.F32, nn.F64) and w.ndim else w  # (a 0-d weight stays a NumPy scalar)
    got = stats.nanaverage(t, tw, **kw)
    assert isinstance(got, torch.Tensor) and got.device == dev and tuple(got.shape) == want.shape, (case["id"], type(got), np.shape(got))
    nn.judge(d, w, axis, got.cpu().numpy(), want, "torch " + case["note"], None, keepdims)
    nn.judge_exact(got.cpu().numpy(), np.asarray(stats.nanaverage(d, w, **kw)), "torch against numpy input " + case["note"])
    assert np.array_equal(t.cpu().numpy(), d, equal_nan=True), "the tensor came back changed"
    plain += w is None
    weighted += w is not None
assert plain >= 30 and weighted >= 40, (plain, weighted)
torch.cuda.synchronize()
ek.synchronize()
print("NANAVERAGE_TORCH_OK:", plain, "plain and", weighted, "weighted means")
