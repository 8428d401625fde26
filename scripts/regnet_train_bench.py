#!/usr/bin/env python
"""Time K2g (the weight gradient of the regularisation U-Nets' 2-channel ends conv0 2 -> 8 and prob 8 -> 2, ops.conv3d_wgrad_c2)
against ATen's weight gradient of the same layer (aten::convolution_backward with only the weight's output asked for -- what autograd
of F.conv3d runs for the weight) on the same MI355X, at the config-2 volumes of the two layers: 64 x 296 x 400, 32 x 592 x 800 and
8 x 1184 x 1600 (the three main passes) and 4 x 1184 x 1600 (the refine pass).  Then forward + backward time and peak memory of a
whole ``DiffCostRegNet`` against the same stack on nn.Conv3d / nn.ConvTranspose3d / nn.BatchNorm3d + ReLU, train mode, batch 1.

Both arms run in one process on one GPU, on the same tensors; every arm is warmed, and the timed windows come in pairs whose order is
swapped every pair.  Per row and arm: device events around --reps repetitions, per repetition; the median
over the pairs, with min and max.  K2g's time is also given as a multiple of its floors, scaled with the voxels from their values at
15.16 M voxels (432 MAC and 40 B per voxel): 0.115 ms on packed VALU FMA (113.7 TFLOP/s; the kernel is the VALU form), 0.083 ms on the
fp32 MFMA (157.3 TFLOP/s), 0.076 ms on HBM (8 TB/s).
One JSON line; --md writes the table of profiles/regnet_train.md.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

VOLUMES = (("c2.s1", (64, 296, 400)), ("c2.s2", (32, 592, 800)), ("c2.s3", (8, 1184, 1600)), ("c2.s3.refine", (4, 1184, 1600)))
LAYERS = (("conv0", 2, 8), ("prob", 8, 2))
FLOOR_VOXELS = 32 * 592 * 800
FLOORS_MS = dict(valu=0.115, mfma=0.083, hbm=0.076)   # at FLOOR_VOXELS


def spread(ts):
    return dict(min=min(ts), median=float(np.median(ts)), max=max(ts), n=len(ts))


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def ab(arms, reps, pairs):
    """{"hip": fn, "aten": fn} -> times: every arm warmed, the windows in pairs with the order swapped every pair."""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for w in range(pairs):
        for k in (("hip", "aten") if w % 2 == 0 else ("aten", "hip")):
            ms[k].append(window(arms[k], reps))
    r = {k + "_ms": spread(v) for k, v in ms.items()}
    r["aten_over_hip"] = r["aten_ms"]["median"] / r["hip_ms"]["median"]
    return r


class _Block(nn.Module):
    def __init__(self, conv):
        super().__init__()
        self.conv, self.bn = conv, nn.BatchNorm3d(conv.out_channels)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


class _AtenPart(nn.Module):
    """CostRegNet_part on stock layers, with the reference's child names (loads a DiffCostRegNetPart's state dict)."""

    def __init__(self, b=8):
        super().__init__()
        c3 = lambda ci, co, s=1: _Block(nn.Conv3d(ci, co, 3, stride=s, padding=1, bias=False))   # noqa: E731
        t3 = lambda ci, co: _Block(nn.ConvTranspose3d(ci, co, 3, stride=2, padding=1, output_padding=1, bias=False))   # noqa: E731
        self.conv0 = c3(2, b)
        self.conv1, self.conv2 = c3(b, 2 * b, 2), c3(2 * b, 2 * b)
        self.conv3, self.conv4 = c3(2 * b, 4 * b, 2), c3(4 * b, 4 * b)
        self.conv5, self.conv6 = c3(4 * b, 8 * b, 2), c3(8 * b, 8 * b)
        self.conv7, self.conv9, self.conv11 = t3(8 * b, 4 * b), t3(4 * b, 2 * b), t3(2 * b, b)
        self.prob = nn.Conv3d(b, 2, 3, stride=1, padding=1, bias=False)

    def forward(self, x):
        conv0 = self.conv0(x)
        conv2 = self.conv2(self.conv1(conv0))
        conv4 = self.conv4(self.conv3(conv2))
        x = self.conv6(self.conv5(conv4))
        x = conv4 + self.conv7(x)
        x = conv2 + self.conv9(x)
        x = conv0 + self.conv11(x)
        return self.prob(x)


class _AtenNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.cosR_small, self.cosR_huge = _AtenPart(), _AtenPart()

    def forward(self, x):
        return torch.cat((self.cosR_small(x), self.cosR_huge(x)), dim=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=5, help="timed (hip, aten) window pairs per row, at least 5")
    ap.add_argument("--net-volume", default="32,592,800", help="D,H,W of the whole-network row (multiples of 8); empty: skip it")
    ap.add_argument("--md", default=None, help="also write the result table (markdown) to this file")
    args = ap.parse_args()
    assert args.pairs >= 5

    from dmvsnet_amd import DiffCostRegNet, ops
    assert torch.cuda.is_available(), "the benchmark needs the MI355X"
    dev = torch.device("cuda:0")
    out = dict(bench="regnet_train", device=torch.cuda.get_device_name(0), reps=args.reps, pairs=args.pairs, rows={}, net=None)
    for vname, (D, H, W) in VOLUMES:
        for lname, cin, cout in LAYERS:
            g = torch.Generator(device="cpu").manual_seed(cin + D)
            x = torch.randn((cin, D, H, W), generator=g).to(dev)
            gy = torch.randn((cout, D, H, W), generator=g).to(dev)
            w = torch.randn((cout, cin, 3, 3, 3), generator=g).to(dev)
            gw = torch.empty_like(w)
            x5, gy5 = x.unsqueeze(0), gy.unsqueeze(0)
            hip = lambda: ops.conv3d_wgrad_c2(x, gy, out=gw)   # noqa: E731
            aten = lambda: torch.ops.aten.convolution_backward(gy5, x5, w, None, [1, 1, 1], [1, 1, 1], [1, 1, 1], False, [0, 0, 0], 1,   # noqa: E731
                                                               [False, True, False])[1]
            agree = ((hip() - aten()).abs().max() / aten().abs().max()).item()
            r = ab({"hip": hip, "aten": aten}, args.reps, args.pairs)
            vox = D * H * W
            t = r["hip_ms"]["median"]
            r.update(cin=cin, cout=cout, D=D, H=H, W=W, gradients_rel_diff=agree, tflops=2.0 * 432 * vox / (t * 1e-3) / 1e12,
                     **{f"over_{k}_floor": t / (v * vox / FLOOR_VOXELS) for k, v in FLOORS_MS.items()})
            out["rows"][f"{vname}.{lname}"] = r
            print(f"# {vname}.{lname}: K2g {t:.3f} ms [{r['hip_ms']['min']:.3f}, {r['hip_ms']['max']:.3f}]  aten "
                  f"{r['aten_ms']['median']:.3f} ms [{r['aten_ms']['min']:.3f}, {r['aten_ms']['max']:.3f}]  {r['tflops']:.1f} TF  "
                  f"x{r['over_valu_floor']:.1f} VALU floor  gradients differ by {agree:.1e}", file=sys.stderr, flush=True)
            del x, gy, w, gw, x5, gy5
    if args.md:   # (the rows alone first: the whole-network row below is the long one)
        with open(args.md, "w") as f:
            f.write(markdown(out))
    if args.net_volume:
        D, H, W = (int(n) for n in args.net_volume.split(","))
        g = torch.Generator(device="cpu").manual_seed(D)
        x = (0.3 * torch.randn((1, 2, D, H, W), generator=g)).to(dev).requires_grad_(True)
        gy = torch.randn((1, 4, D, H, W), generator=g).to(dev)
        hip_net = DiffCostRegNet(2, 8).to(dev).train()
        aten_net = _AtenNet().to(dev).train()
        aten_net.load_state_dict(hip_net.state_dict(), strict=True)

        def arm(m):
            params = [x] + list(m.parameters())
            return lambda: torch.autograd.grad(m(x), params, gy)

        gh, ga = arm(hip_net)(), arm(aten_net)()
        agree = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(gh, ga))
        del gh, ga
        r = ab({"hip": arm(hip_net), "aten": arm(aten_net)}, 1, args.pairs)
        r.update({k + "_peak_mb": peak_mb(fn) for k, fn in (("hip", arm(hip_net)), ("aten", arm(aten_net)))})
        r.update(D=D, H=H, W=W, gradients_rel_diff=agree)
        out["net"] = r
        print(f"# DiffCostRegNet {D} x {H} x {W}: hip {r['hip_ms']['median']:.1f} ms  aten {r['aten_ms']['median']:.1f} ms  peak "
              f"{r['hip_peak_mb']:.0f} / {r['aten_peak_mb']:.0f} MB  gradients differ by {agree:.1e}", file=sys.stderr, flush=True)
    print(json.dumps(out))
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(out))


def markdown(out):
    lines = ["# conv0 / prob weight gradient (K2g) against ATen, and a whole CostRegNet forward + backward", "",
             f"`scripts/regnet_train_bench.py` on {out['device']}, one process, arms alternating; median [min, max] of {out['pairs']} window "
             f"pairs of {out['reps']} repetitions, per sample.  Times in ms.  ATen: `aten::convolution_backward` for the weight alone.  "
             "Floors (432 MAC and 40 B per voxel, scaled with the voxels): packed VALU FMA 113.7 TFLOP/s (the form K2g has), fp32 MFMA "
             "157.3 TFLOP/s, HBM 8 TB/s -- 0.115 / 0.083 / 0.076 ms at 15.16 M voxels.", "",
             "| pass.layer | in -> out | D x H x W | K2g | ATen wgrad | ATen / K2g | K2g TFLOP/s | x VALU floor | x MFMA floor | x HBM floor | max rel. diff |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, r in out["rows"].items():
        h, a = r["hip_ms"], r["aten_ms"]
        lines.append(f"| {name} | {r['cin']} -> {r['cout']} | {r['D']} x {r['H']} x {r['W']} | {h['median']:.3f} [{h['min']:.3f}, {h['max']:.3f}] | "
                     f"{a['median']:.3f} [{a['min']:.3f}, {a['max']:.3f}] | {r['aten_over_hip']:.2f} | {r['tflops']:.1f} | "
                     f"{r['over_valu_floor']:.1f} | {r['over_mfma_floor']:.1f} | {r['over_hbm_floor']:.1f} | {r['gradients_rel_diff']:.1e} |")
    n = out.get("net")
    if n:
        h, a = n["hip_ms"], n["aten_ms"]
        lines += ["", f"Whole network, train mode, batch 1, {n['D']} x {n['H']} x {n['W']}, forward + backward (gradients for the input and "
                  "every parameter); peak: allocated over one step above what was allocated before it, in MB.", "",
                  "| network | fwd+bwd | peak MB | gradients, max rel. diff |", "|---|---|---|---|",
                  f"| `DiffCostRegNet` (K2 / K2g / K3 / K3g / K3h / K5) | {h['median']:.1f} [{h['min']:.1f}, {h['max']:.1f}] | {n['hip_peak_mb']:.0f} | "
                  f"{n['gradients_rel_diff']:.1e} |",
                  f"| the same stack on nn.Conv3d / nn.ConvTranspose3d / nn.BatchNorm3d + ReLU | {a['median']:.1f} [{a['min']:.1f}, {a['max']:.1f}] | "
                  f"{n['aten_peak_mb']:.0f} | |"]
    lines.append("")
    return "\n".join(lines)


if __name__ == "__main__":
    main()
