#!/usr/bin/env python3
"""Generate tests/golden/op_regnet_grad.npz by RUNNING THE REFERENCE's CostRegNet_part and CostRegNet_part_refine in train mode under
fp32 autograd on the CPU.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_regnet_grad.py <path of the reference checkout> [seeds to try]

Imports networks/module.py of the reference (read-only, never copied).  Per case of tests/regnet_grad_ref.GOLDEN_NETS (batch 2; the full
part at 8 x 16 x 24, the refine part at 4 x 16 x 24) it builds the reference's network (2, 8), loads the weights dmvsnet_amd.synth makes
for the case's seed (they are not stored), runs it on x and back-propagates gy.  Stored per case, data only: the seed, x, gy, the output,
g_x, every BatchNorm's g_gamma / g_beta and g_w of conv0, conv1, conv2, conv11 and prob (the large layers' weight gradients are left to
the float64 comparison).

The fixture carries a condition, asserted here on every case before it is stored and re-asserted by the tests on the stored data:

  1. in the float64 run (tests/regnet_grad_ref.PlainPart*) no BatchNorm output lies within KINK_MARGIN = 1e-4 of the ReLU kink;
  2. the reference's fp32 run has the same ReLU masks as the float64 run at every block.

The seed is the first one of the range tried for which both hold.  Where the range has none -- the full part has 145 920 BatchNorm
outputs, about 15 of them inside the margin for any seed, so a clean seed is a one-in-millions event; the refine part has half as many
values and about 7 inside -- the case takes seed 0 and moves the BatchNorm biases instead: block by block in forward order, every
channel that has a value inside the margin gets the smallest shift of its beta that puts the kink into a gap of the channel's values
at least 4 margins wide (a shift of the order of 1e-3 on a beta of the order of 0.1; later blocks are re-run on the shifted earlier
ones).  Such a case stores its BatchNorm biases (``<case>.beta.<block>``, [C] each) and regnet_grad_ref.net_weights puts them in place of
the recipe's; everything else is the recipe's.  Both conditions are then asserted like for any other case.

Printed per case: ``e_ref`` of every stored tensor, the distance of the reference's fp32 results to the float64 run, normalised by the
tensor's max-abs.  The file is asserted to stay under the repository's limit for a committed file (1 MiB).
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
SEEDS = int(sys.argv[2]) if len(sys.argv) == 3 else 2000
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, sys.argv[1])
warnings.filterwarnings("ignore")

import regnet_grad_ref as R  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    from networks import module as ref_module  # noqa: E402

torch.set_num_threads(8)


def run_f64(name, sd, x, gy):
    return R.run_part(R.plain_net(name, sd, torch.float64), x, gy)


def run_reference(name, sd, x, gy):
    net = (ref_module.CostRegNet_part_refine if R.GOLDEN_NETS[name]["refine"] else ref_module.CostRegNet_part)(2, 8)
    net.load_state_dict(sd, strict=True)
    return R.run_part(net, x, gy)


def clean(name, sd, x, gy):
    """Both conditions; returns (ok, float64 run, reference run or None)."""
    f64 = run_f64(name, sd, x, gy)
    if R.kink_violations(f64[2]):
        return False, f64, None
    ref = run_reference(name, sd, x, gy)
    return R.same_masks(ref[2], f64[2]), f64, ref


def centre_betas(name, seed, x, gy):
    """The BatchNorm biases of the case with the kink moved into a gap of every channel's values, block by block in forward order."""
    beta = {}
    for blk in R.BLOCKS:
        pre = run_f64(name, R.net_weights(name, seed, beta), x, gy)[2][blk]
        C = pre.shape[1]
        vals = pre.transpose(0, 1).reshape(C, -1)
        b = R.net_weights(name, seed, beta)[f"{blk}.bn.bias"].double()
        half = 2 * R.KINK_MARGIN
        for c in range(C):
            v = torch.sort(vals[c]).values
            if (v.abs() > R.KINK_MARGIN).all():
                continue
            edges = torch.cat((v.new_tensor([-1e9]), v, v.new_tensor([1e9])))
            lo, hi = edges[:-1] + half, edges[1:] - half          # the kink may sit at t in [lo, hi] of a gap wide enough
            ok = hi >= lo
            t = torch.clamp(torch.zeros_like(lo), min=lo, max=hi)[ok]
            t = t[t.abs().argmin()]
            b[c] -= t                                             # values v - t: the kink of the shifted channel is at v = t
        beta[blk] = b.float().numpy()
    return beta


def main():
    arrs = {}
    for name in R.GOLDEN_NETS:
        beta = None
        for seed in range(SEEDS):
            x, gy = R.net_inputs(name, seed)
            ok, f64, ref = clean(name, R.net_weights(name, seed), x, gy)
            if ok:
                break
        else:
            seed = 0
            x, gy = R.net_inputs(name, seed)
            beta = centre_betas(name, seed, x, gy)
            ok, f64, ref = clean(name, R.net_weights(name, seed, beta), x, gy)
            print(f"{name}: no clean seed below {SEEDS}; seed 0 with centred BatchNorm biases, largest shift "
                  f"{max(float(np.abs(beta[b] - R.net_weights(name, seed)[f'{b}.bn.bias'].numpy()).max()) for b in R.BLOCKS):.2e}")
        assert ok and R.kink_violations(f64[2]) == 0 and R.same_masks(ref[2], f64[2]), name
        (o64, g64, _), (oref, gref, _) = f64, ref
        keep = ["x"] + [k for k in gref if k.endswith("bn.weight") or k.endswith("bn.bias") or k in R.STORED_WEIGHT_GRADS]
        e = {"out": R.rel_dist(oref, o64), **{k: R.rel_dist(gref[k], g64[k]) for k in keep}}
        print(f"{name}: seed {seed}; e_ref max {max(e.values()):.2e} ({max(e, key=e.get)}), out {e['out']:.2e}, g_x {e['x']:.2e}")
        assert max(e.values()) < 1e-4, (name, e)   # sanity only: the same function, not a test bound
        arrs[f"{name}.seed"] = np.array(seed)
        arrs[f"{name}.x"], arrs[f"{name}.gy"], arrs[f"{name}.out"] = x.numpy(), gy.numpy(), oref.numpy()
        for k in keep:
            arrs[f"{name}.g.{k}"] = gref[k].contiguous().numpy()
        for blk, b in (beta or {}).items():
            arrs[f"{name}.beta.{blk}"] = b
    path = os.path.join(HERE, "op_regnet_grad.npz")
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    print(f"op_regnet_grad.npz: {size / 1024:.1f} KB, keys={len(arrs)}")
    assert size < (1 << 20)


if __name__ == "__main__":
    main()
