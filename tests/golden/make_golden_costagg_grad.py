#!/usr/bin/env python3
"""Generate tests/golden/op_costagg_grad.npz by RUNNING THE REFERENCE's CostAgg under autograd (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_costagg_grad.py

Imports /root/reference/networks (read-only, never copied).  For every case of tests/costagg_grad_ref.GOLDEN_CASES it stores
the inputs, the similarity volume and the gradients of L = <gsim, sim> with respect to every feature map, computed in train
mode; eval mode is run as well and must give the same bits (stored as ``<case>.train_eq_eval``).  Also per case: the share of
samples with a tap outside the image (kept between 5 % and 50 %) and ``e_oracle`` -- the max-abs distance of the reference's
fp32 gradients to the float64 restatement, per gradient tensor.  Data only.
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

import costagg_grad_ref as R  # noqa: E402

with contextlib.redirect_stdout(io.StringIO()):
    from networks import mvsnet as ref_mvsnet  # noqa: E402

torch.set_num_threads(8)


def run(agg, feats, cams, depth, gsim):
    return R.grads_of(lambda f, p, d: agg(f, p, d, 0), feats, cams, depth, gsim)


def main():
    arrs = {}
    for name, kw in R.GOLDEN_CASES.items():
        feats, cams, depth, gsim = R.make_case(**kw)
        agg = ref_mvsnet.CostAgg("variance")
        agg.train()
        sim, grads = run(agg, feats, cams, depth, gsim)
        agg.eval()
        sim_e, grads_e = run(agg, feats, cams, depth, gsim)
        same = torch.equal(sim, sim_e) and all(torch.equal(a, b) for a, b in zip(grads, grads_e))
        assert same, f"{name}: train and eval mode differ"
        share = R.outside_share(cams, depth)
        assert 0.05 <= share <= 0.50, (name, share)
        _, g64 = R.grads_f64(feats, cams, depth, gsim)
        e = np.array([(a.double() - b).abs().max().item() for a, b in zip(grads, g64)])
        mag = np.array([a.abs().max().item() for a in grads])
        assert all(a.abs().max() > 0 for a in grads), name
        print(f"{name}: outside share {share:.3f}; |grad| max {mag.min():.2f}..{mag.max():.2f}; e_oracle {e.min():.2e}..{e.max():.2e}")
        arrs[f"{name}.proj"] = cams.numpy()
        arrs[f"{name}.depth"] = depth.numpy()
        arrs[f"{name}.gsim"] = gsim.numpy()
        arrs[f"{name}.sim"] = sim.numpy()
        arrs[f"{name}.train_eq_eval"] = np.array(same)
        arrs[f"{name}.outside_share"] = np.array(share)
        arrs[f"{name}.e_oracle"] = e
        for v in range(len(feats)):
            arrs[f"{name}.feat{v}"] = feats[v].numpy()
            arrs[f"{name}.grad{v}"] = grads[v].numpy()
    path = os.path.join(HERE, "op_costagg_grad.npz")
    np.savez_compressed(path, **arrs)
    print(f"op_costagg_grad.npz: {os.path.getsize(path) / 1024:.1f} KB, keys={len(arrs)}")


if __name__ == "__main__":
    main()
