"""Child process of tests/test_gpu_gumbel.py::test_torch_device_tensors.

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
from ekm_hip import stats  # noqa: E402

import _gumbel_numpy as gn  # noqa: E402

np.seterr(all="ignore")
dev = torch.device("cuda", ek.current_device())
TDT = {gn.F32: torch.float32, gn.F64: torch.float64}

fits = calls = 0
for case in gn.fit_cases():
    sample, axis = gn.sample_of(case), case["plain"]["axis"]
    if sample.dtype not in TDT:  # integer input stays NumPy
        continue
    t = torch.from_numpy(np.ascontiguousarray(sample)).to(dev)
    d = stats.GumbelDistribution.fit(t, axis=axis)
    assert isinstance(d.mu, torch.Tensor) and isinstance(d.sigma, torch.Tensor) and d.mu.device == dev, (case["id"], type(d.mu))
    assert d.mu.dtype == torch.float64 and tuple(d.mu.shape) == d.shape
    want = gn.recorded_fit(case, "c") or gn.fit(sample, axis)
    gn.judge_fit_exact((d.mu.cpu().numpy(), d.sigma.cpu().numpy()), want, "torch " + case["note"])
    assert np.array_equal(t.cpu().numpy(), sample, equal_nan=True)
    if case["note"].endswith("cube axis 1"):  # a view that is not contiguous: the same samples with the axes swapped
        swapped = t.permute(1, 0, 2)
        assert not swapped.is_contiguous()
        d2 = stats.GumbelDistribution.fit(swapped, 0)
        gn.judge_fit_exact((d2.mu.cpu().numpy(), d2.sigma.cpu().numpy()), want, "torch permuted " + case["note"])
        x = d.cdf([25.0, 40.0])  # a fitted distribution answers in the caller's library
        assert isinstance(x, torch.Tensor) and tuple(x.shape) == (2,) + d.shape
        fits += 1000
    fits += 1

for case in gn.call_cases("cdf", "ppf", "value_to_return_period", "return_period_to_value"):
    kw = gn.call_args(case)
    if gn.is_timedelta_case(case) or kw["mu"].ndim == 0:
        continue
    mu, sigma = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (kw["mu"], kw["sigma"]))
    dist = stats.GumbelDistribution(mu, sigma, freq=kw["freq"])
    assert isinstance(dist.mu, torch.Tensor) and dist.mu.dtype == torch.float64
    got = getattr(dist, case["func"])(kw["arg"]) if case["func"] in ("cdf", "ppf") else getattr(stats, case["func"])(dist, kw["arg"])
    assert isinstance(got, torch.Tensor) and got.device == dev, (case["id"], type(got))
    gn.judge_call(case, got.cpu().numpy(), "torch " + gn.case_id(case))
    calls += 1
assert fits > 2000 + 50 and calls > 80, (fits, calls)
torch.cuda.synchronize()
ek.synchronize()
print("GUMBEL_TORCH_OK:", fits % 1000, "fits,", calls, "calls")
