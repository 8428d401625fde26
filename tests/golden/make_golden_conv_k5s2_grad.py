#!/usr/bin/env python3
"""Generate tests/golden/op_conv_k5s2_grad.npz by RUNNING THE REFERENCE's 5x5 stride-2 blocks under fp32 autograd on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_conv_k5s2_grad.py <path of the reference checkout>

Imports networks/module.py of the reference (read-only, never copied).  For every case of tests/conv_k5s2_grad_ref.GOLDEN_CASES it
builds the reference's block -- ``Conv2d(8, 16, 5, stride=2, padding=2)`` or ``Conv2d(16, 32, 5, stride=2, padding=2)``
(FeatureNet's conv1.0 / conv2.0, module.py:289, :295): layer + TRAIN-mode BatchNorm + ReLU --, loads the case's weight and BatchNorm
gamma / beta, runs it on the input and back-propagates the upstream gradient.  Stored per case, data only: x, w, gamma, beta, gy, the
block's output and the gradients for x, w, gamma and beta.

Asserted on every case before it is stored (the tests re-assert it on the stored data): no BatchNorm output within 1e-5 of the ReLU
kink (tests/conv_k5s2_grad_ref.kink_violations).  Printed per case: ``e_ref``, the distance of the reference's fp32 results to the
float64 restatement, normalised by the tensor's max-abs.  The file is asserted to stay under the repository's limit for a committed
file (1 MiB).
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "networks", "module.py")):
    sys.exit(__doc__)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, sys.argv[1])
warnings.filterwarnings("ignore")

import conv_k5s2_grad_ref as R  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    from networks import module as ref_module  # noqa: E402

torch.set_num_threads(8)


def run_reference(case):
    Cb = case["Cb"]
    block = ref_module.Conv2d(Cb, 2 * Cb, 5, stride=2, padding=2)
    assert block.conv.bias is None and block.bn is not None and block.relu
    assert tuple(block.conv.weight.shape) == tuple(case["w"].shape)
    with torch.no_grad():
        block.conv.weight.copy_(case["w"])
        block.bn.weight.copy_(case["gamma"])
        block.bn.bias.copy_(case["beta"])
    block.train()
    x = case["x"].clone().requires_grad_(True)
    out = block(x)
    assert out.shape == case["gy"].shape, (out.shape, case["gy"].shape)
    out.backward(case["gy"])
    return dict(out=out.detach(), g_x=x.grad, g_w=block.conv.weight.grad, g_gamma=block.bn.weight.grad, g_beta=block.bn.bias.grad)


def main():
    arrs = {}
    for name, kw in R.GOLDEN_CASES.items():
        case = R.make_case(**kw)
        assert R.kink_violations(case) == 0, (name, "a BatchNorm output sits on the ReLU kink: pick another seed")
        ref = run_reference(case)
        f64 = R.block_f64(case)
        e = {k: R.rel_dist(ref[k], f64[k]) for k in ("out", "g_x", "g_w", "g_gamma", "g_beta")}
        print(f"{name}: e_ref " + "  ".join(f"{k} {v:.2e}" for k, v in e.items()))
        assert max(e.values()) < 1e-5, (name, e)   # sanity only: the same function, not a test bound
        for k in ("x", "w", "gamma", "beta", "gy"):
            arrs[f"{name}.{k}"] = case[k].numpy()
        for k, v in ref.items():
            arrs[f"{name}.{k}"] = v.contiguous().numpy()
    path = os.path.join(HERE, "op_conv_k5s2_grad.npz")
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    print(f"op_conv_k5s2_grad.npz: {size / 1024:.1f} KB, keys={len(arrs)}")
    assert size < (1 << 20)


if __name__ == "__main__":
    main()
