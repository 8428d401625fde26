#!/usr/bin/env python3
"""Generate tests/golden/op_featurenet_grad.npz by RUNNING THE REFERENCE's FeatureNet(8) in train mode under fp32 autograd on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_featurenet_grad.py <path of the reference checkout> [seeds to try]

Imports networks/module.py of the reference (read-only, never copied).  Per case of tests/featurenet_grad_ref.GOLDEN_CASES (B = 2 at
16 x 24; B = 1 at 20 x 36, which gives odd extents 5 x 9 at the conv2 level) it builds the inputs of featurenet_grad_ref.make_net_case,
loads the state dict into the reference's network with strict=True, runs it on x and back-propagates the fixed upstream gradients on
all six outputs.  Stored, data only: the state dict (one for both cases) and per case x, the six upstream gradients, the six outputs and
the gradient of every learnable parameter.

The fixture carries a condition, asserted here before a case is stored and re-asserted by the tests on the stored data: in the float64
restatement (featurenet_grad_ref.run_net) no BatchNorm output lies within KINK_MARGIN = 1e-4 of the ReLU kink -- a flipped kink would
dominate every gradient.  The seed is the first one for which that holds in both cases; it is printed, and GOLDEN_SEED must name it.

Printed per case: the largest ``e_ref`` of the stored tensors, the distance of the reference's fp32 results to the float64 run
normalised by the tensor's max-abs.  The file is asserted to stay under the largest existing op_*_grad.npz fixture.
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
if len(sys.argv) not in (2, 3) or not os.path.isfile(os.path.join(sys.argv[1], "networks", "module.py")):
    sys.exit(__doc__)
SEEDS = int(sys.argv[2]) if len(sys.argv) == 3 else 200
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, sys.argv[1])
warnings.filterwarnings("ignore")

import featurenet_grad_ref as R  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    from networks import module as ref_module  # noqa: E402

torch.set_num_threads(8)
MAX_BYTES = 782997   # op_conv_grad.npz, the largest op_*_grad.npz


def run_reference(case):
    net = ref_module.FeatureNet(8)
    net.load_state_dict(case["sd"], strict=True)
    net.train()
    outs = net(case["x"])
    assert tuple(outs) == R.OUT_KEYS
    params = dict(net.named_parameters())
    assert list(params) == R.param_keys()
    grads = torch.autograd.grad([outs[k] for k in R.OUT_KEYS], list(params.values()), [case["gys"][k] for k in R.OUT_KEYS])
    return {k: v.detach() for k, v in outs.items()}, dict(zip(params, grads))


def main():
    arrs = {}
    for seed in range(SEEDS):
        cases = {name: R.make_net_case(kw["B"], kw["H"], kw["W"], seed) for name, kw in R.GOLDEN_CASES.items()}
        f64s = {name: R.run_net(case) for name, case in cases.items()}
        if all(f["nearest_kink"] > R.KINK_MARGIN for f in f64s.values()):
            break
    else:
        sys.exit(f"no seed below {SEEDS} keeps every BatchNorm output of both cases off the ReLU kink")
    assert seed == R.GOLDEN_SEED, f"the first clean seed is {seed}; featurenet_grad_ref.GOLDEN_SEED names {R.GOLDEN_SEED}"
    for name, case in cases.items():
        f64 = f64s[name]
        out, grads = run_reference(case)
        e = {**{f"out.{k}": R.rel_dist(out[k], f64["out"][k]) for k in R.OUT_KEYS},
             **{f"g.{k}": R.rel_dist(grads[k], f64["g"][k]) for k in grads}}
        print(f"{name}: seed {seed}, nearest kink {f64['nearest_kink']:.2e}; e_ref max {max(e.values()):.2e} ({max(e, key=e.get)})")
        assert max(e.values()) < 1e-4, (name, e)   # sanity only: the same function, not a test bound
        arrs[f"{name}.x"] = case["x"].numpy()
        for k, v in case["sd"].items():
            arrs[f"sd.{k}"] = v.numpy()   # (the same for both cases: stored once)
        for k in R.OUT_KEYS:
            arrs[f"{name}.gy.{k}"], arrs[f"{name}.out.{k}"] = case["gys"][k].numpy(), out[k].contiguous().numpy()
        for k, v in grads.items():
            arrs[f"{name}.g.{k}"] = v.contiguous().numpy()
    path = os.path.join(HERE, "op_featurenet_grad.npz")
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    print(f"op_featurenet_grad.npz: {size / 1024:.1f} KB, keys={len(arrs)}")
    assert size <= MAX_BYTES


if __name__ == "__main__":
    main()
