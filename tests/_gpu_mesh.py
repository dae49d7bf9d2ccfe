"""What the GPU tests of the mesh queries share: tensors to and from the device, equality of bits, and the derived tolerance of a
winding number against tests/_winding_ref.py (test_gpu_winding.py states where it comes from)."""
import numpy as np
import torch

import _winding_ref as ref

f32, f64 = np.float32, np.float64


def dev():
    return torch.device("cuda:0")


def T(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(dev())


def N(x):
    return x.detach().cpu().numpy()


def bits_equal(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    if a.dtype == torch.float64:
        return torch.equal(a.view(torch.int64), b.view(torch.int64))
    return torch.equal(a, b)


def check_w(got, want, terms, label):
    """got: the kernel's fp32 w; want: the restatement's dict; terms: F or the visits per point"""
    from conftest import report_worst
    got = N(got)
    assert got.dtype == f32 and got.shape == want["w"].shape
    nan = np.isnan(want["w"])
    assert np.array_equal(np.isnan(got), nan), label
    w64 = want["S"][~nan] / ref.FOUR_PI
    tol = np.spacing(np.abs(w64).astype(f32)).astype(f64) + np.broadcast_to(np.asarray(terms, f64), nan.shape)[~nan] * 2.0 ** -50
    err = np.abs(got[~nan].astype(f64) - w64)
    worst = float((err / tol).max()) if err.size else 0.0
    print(f"{label}: {err.size} points, worst |dw| {err.max() if err.size else 0.0:.2e} = {worst:.2f} of its tolerance")
    report_worst("winding number vs the fp64 restatement, share of ulp32 + n 2^-50", worst)
    assert worst <= 1.0, (label, worst)
