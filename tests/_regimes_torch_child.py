"""Child process of tests/test_gpu_regimes.py::test_torch_device_tensors.

torch (a FOREIGN ROCm array library; test infrastructure only, the product never imports it) is imported and
initialised first, then ekm_hip, as in tests/_gumbel_torch_child.py.  Exit code 77 = torch has no ROCm device here."""
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
from ekm_hip import regimes, score  # noqa: E402

import _regimes_numpy as rn  # noqa: E402

np.seterr(all="ignore")
dev = torch.device("cuda", ek.current_device())


def to_torch(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


projects = indices = pearsons = 0
for case in rn.cases("project"):
    a = rn.arrays_of(case)
    if case["raises"] or a["field"].ndim <= 2:
        continue
    patterns, extra = rn.build_patterns(case, regimes)
    t = to_torch(a["field"])
    got = regimes.project(t, patterns, a["weights"], **extra)
    assert all(isinstance(v, torch.Tensor) and v.device == dev for v in got.values()), case["id"]
    host = {k: v.cpu().numpy() for k, v in got.items()}
    rn.judge_project(case, host, "torch " + case["note"])
    rn.judge_index(host, regimes.project(a["field"], patterns, a["weights"], **extra), "torch against numpy input")
    assert np.array_equal(t.cpu().numpy(), a["field"], equal_nan=True)
    idx = regimes.regime_index(got, {k: 1.0 for k in got}, {k: 2.0 for k in got})
    assert all(isinstance(v, torch.Tensor) for v in idx.values())
    rn.judge_index({k: v.cpu().numpy() for k, v in idx.items()}, {k: (v - v.dtype.type(1.0)) / v.dtype.type(2.0) for k, v in host.items()}, "torch index")
    projects += 1
for case in rn.cases("regime_index"):
    proj, mean, std = rn.index_args(case)
    got = regimes.regime_index({k: to_torch(v) for k, v in proj.items()}, mean, std)
    assert all(isinstance(v, torch.Tensor) for v in got.values())
    rn.judge_index({k: v.cpu().numpy() for k, v in got.items()}, rn.recorded(case), "torch " + case["note"])
    indices += 1
for case in rn.cases("pearson_correlation"):
    a = rn.arrays_of(case)
    if case["raises"] or a["x"].dtype not in (rn.F32, rn.F64):
        continue
    axis = case["plain"]["axis"]
    x, y = to_torch(a["x"]), to_torch(a["y"])
    got = score.pearson_correlation(x, y, axis=axis)
    assert isinstance(got, torch.Tensor) and got.device == dev, case["id"]
    rn.judge_pearson(a["x"], a["y"], axis, got.cpu().numpy(), rn.recorded(case), "torch " + case["note"])
    if a["x"].ndim == 3 and axis == 1:  # a view that is not contiguous: the same samples with the axes swapped
        xs, ys = x.permute(1, 0, 2), y.permute(1, 0, 2)
        assert not xs.is_contiguous()
        rn.judge_exact(score.pearson_correlation(xs, ys, 0).cpu().numpy(), got.cpu().numpy(), "torch permuted")
        pearsons += 1000
    pearsons += 1
assert projects >= 15 and indices >= 12 and pearsons > 2000 + 50, (projects, indices, pearsons)
torch.cuda.synchronize()
ek.synchronize()
print("REGIMES_TORCH_OK:", projects, "projections,", indices, "indices,", pearsons % 1000, "correlations")
