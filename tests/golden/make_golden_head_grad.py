#!/usr/bin/env python3
"""Generate tests/golden/op_head_grad.npz by RUNNING THE REFERENCE's DepthNet and mvs_loss under fp32 autograd (build container
only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_head_grad.py

Imports /root/reference/networks and /root/reference/loss.py (read-only, never copied).  For every case of
tests/head_grad_ref.GOLDEN_CASES it runs ``DepthNet.forward`` -> ``.refine`` (on the main pass's ``depth_values_c``, not
detached) -> ``mvs_loss(mode="regression", dlossw=[w])`` and stores the inputs (logits, hypotheses, refine logits, ground truth,
mask, weight, interval), the outputs (depth_sub_plus, depth_values_c, depth_sub_plus_refine, depth, loss) and the gradients with
respect to both logit volumes; for the refine pass alone (its hypotheses a detached leaf) also the gradient with respect to
``depth_values_c``.  Data only.

Asserted on every case before it is stored (tests/head_grad_ref.condition_violations; the tests re-assert them on the stored data):
(a) the depths of each pair differ by more than MARGIN, (b) no smooth-L1 argument within MARGIN of the knee or of 0 and no tie of
the two |. - gt| of a pair, (c) the reference's cell mask drops no all-valid cell.  Printed per case: ``e_ref``, the distance of
the reference's fp32 gradients to the float64 restatement, normalised by the tensor's max-abs.
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
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")
warnings.filterwarnings("ignore")

import head_grad_ref as R  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    from networks import mvsnet as ref_mvsnet  # noqa: E402
    import loss as ref_loss  # noqa: E402

torch.set_num_threads(8)


def run_reference(case, refine_alone=False):
    net = ref_mvsnet.DepthNet()
    L = case["logits"].clone().requires_grad_(True)
    Lr = case["rlogits"].clone().requires_grad_(True)
    itv = torch.tensor(case["interval"], dtype=torch.float32)
    main = net(L, case["hyp"], L.shape[2], itv)
    c = main["depth_values_c"]
    if refine_alone:
        c = c.detach().requires_grad_(True)
    refine = net.refine(Lr, c, 4, itv)
    stage = {**refine, **main}
    loss = ref_loss.mvs_loss({"stage1": stage}, {"stage1": case["gt"]}, {"stage1": case["mask"]}, "regression",
                             dlossw=[case["weight"]])
    if refine_alone:
        return torch.autograd.grad(loss, c)[0]
    g_L, g_Lr = torch.autograd.grad(loss, [L, Lr])
    return stage, loss.detach(), g_L, g_Lr


def main():
    arrs = {}
    for name, kw in R.GOLDEN_CASES.items():
        case = R.make_case(**kw)
        bad = R.condition_violations(case)
        assert not bad, (name, bad)
        stage, loss, g_L, g_Lr = run_reference(case)
        g_c = run_reference(case, refine_alone=True)
        f64 = R.chain_f64(case)
        assert abs(loss.item() - f64["loss"].item()) <= 1e-4 * abs(f64["loss"].item()), (name, loss.item(), f64["loss"].item())
        e = {k: R.rel_dist(v, f64[k]) for k, v in (("g_logits", g_L), ("g_rlogits", g_Lr), ("g_c", g_c))}
        no_edge = R.rel_dist(g_L, R.chain_f64(case, edge=False)["g_logits"])
        print(f"{name}: loss {loss.item():.6f}  e_ref " + "  ".join(f"{k} {v:.2e}" for k, v in e.items())
              + f"  (without the hypotheses edge g_logits would be off by {no_edge:.2e})")
        # sanity only (no test bound): fp32 rounding of a ~600 mm expectation is ~1e-4 mm, which the quadratic branch of the smooth-L1
        # turns into a gradient error of that size; a wrong term or a dropped edge is off by orders of magnitude more
        assert max(e.values()) < 2e-3 and no_edge > 0.05, (name, e, no_edge)
        for k in ("logits", "hyp", "rlogits", "gt", "mask"):
            arrs[f"{name}.{k}"] = case[k].numpy()
        arrs[f"{name}.weight"] = np.array(case["weight"], dtype=np.float64)
        arrs[f"{name}.interval"] = np.array(case["interval"], dtype=np.float64)
        for k in ("depth_sub_plus", "depth_values_c", "depth_sub_plus_refine", "depth"):
            arrs[f"{name}.{k}"] = stage[k].detach().numpy()
        arrs[f"{name}.loss"] = np.array(loss.item(), dtype=np.float32)
        arrs[f"{name}.g_logits"] = g_L.numpy()
        arrs[f"{name}.g_rlogits"] = g_Lr.numpy()
        arrs[f"{name}.g_c"] = g_c.numpy()
    path = os.path.join(HERE, "op_head_grad.npz")
    np.savez_compressed(path, **arrs)
    size, limit = os.path.getsize(path), os.path.getsize(os.path.join(HERE, "op_costagg_grad.npz"))
    print(f"op_head_grad.npz: {size / 1024:.1f} KB (limit {limit / 1024:.1f} KB), keys={len(arrs)}")
    assert size <= limit


if __name__ == "__main__":
    main()
