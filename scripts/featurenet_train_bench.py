#!/usr/bin/env python
"""Time forward + backward of FeatureNet's six rectangular stride-1 layers on ``DiffFeatureConv2d`` (K3 forward and data gradient, K3f
weight and bias gradient) and of a whole ``DiffFeatureNet`` against the same layers / network on stock nn.Conv2d / nn.BatchNorm2d (ATen)
built from the same state dict, on the same MI355X, train mode.  Shapes: the DTU training size 512 x 640 at batch 1 and 2, and the
benchmark's 1184 x 1600 at batch 1; each layer runs at its own pyramid level (out1 at 1/4, inner1 at 1/2, the others at full size).

Both arms run in one process on one GPU, on the same tensors; every arm is warmed, and the timed windows come in pairs whose order is
swapped every pair.  Per row and arm: device events around --reps repetitions, per repetition; the median
over the pairs, with min and max.  Peak memory: allocated over one step above what was allocated before it.  The two arms' gradients
are compared at the size they are timed at.  One JSON line; --md writes the table of profiles/featurenet_train.md.
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

SIZES = (("dtu.b1", 1, 512, 640), ("dtu.b2", 2, 512, 640), ("bench.b1", 1, 1184, 1600))
# (name, Cin, Cout, kernel, bias, pyramid level: the layer's input is H / level x W / level)
LAYERS = (("conv0.0", 3, 8, 3, False, 1), ("conv0.1", 8, 8, 3, False, 1), ("out1", 32, 64, 1, False, 4), ("inner1", 16, 32, 1, True, 2),
          ("inner2", 8, 32, 1, True, 1), ("out3", 32, 16, 3, False, 1))


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
    r.update({k + "_peak_mb": peak_mb(fn) for k, fn in arms.items()})
    return r


class _Block(nn.Module):
    def __init__(self, cin, cout, k, stride=1):
        super().__init__()
        self.conv, self.bn = nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=False), nn.BatchNorm2d(cout)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


class _AtenFeatureNet(nn.Module):
    """FeatureNet(8) on stock layers, with the reference's child names (loads a DiffFeatureNet's state dict)."""

    def __init__(self, b=8):
        super().__init__()
        self.conv0 = nn.Sequential(_Block(3, b, 3), _Block(b, b, 3))
        self.conv1 = nn.Sequential(_Block(b, 2 * b, 5, 2), _Block(2 * b, 2 * b, 3), _Block(2 * b, 2 * b, 3))
        self.conv2 = nn.Sequential(_Block(2 * b, 4 * b, 5, 2), _Block(4 * b, 4 * b, 3), _Block(4 * b, 4 * b, 3))
        self.out1 = nn.Conv2d(4 * b, 8 * b, 1, bias=False)
        self.inner1, self.inner2 = nn.Conv2d(2 * b, 4 * b, 1, bias=True), nn.Conv2d(b, 4 * b, 1, bias=True)
        self.out2 = nn.Conv2d(4 * b, 4 * b, 3, padding=1, bias=False)
        self.out3 = nn.Conv2d(4 * b, 2 * b, 3, padding=1, bias=False)

    def forward(self, x):
        conv0 = self.conv0(x)
        conv1 = self.conv1(conv0)
        conv2 = self.conv2(conv1)
        o1 = self.out1(conv2)
        intra = F.interpolate(conv2, scale_factor=2, mode="nearest") + self.inner1(conv1)
        o2 = self.out2(intra)
        intra = F.interpolate(intra, scale_factor=2, mode="nearest") + self.inner2(conv0)
        return o1, o2, self.out3(intra)


def rel_diff(gh, ga):
    return max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(gh, ga))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=5, help="timed (hip, aten) window pairs per row, at least 5")
    ap.add_argument("--sizes", default=",".join(s[0] for s in SIZES), help="comma-separated subset of the sizes")
    ap.add_argument("--md", default=None, help="also write the result table (markdown) to this file")
    args = ap.parse_args()
    assert args.pairs >= 5

    from dmvsnet_amd import DiffFeatureConv2d, DiffFeatureNet
    assert torch.cuda.is_available(), "the benchmark needs the MI355X"
    dev = torch.device("cuda:0")
    out = dict(bench="featurenet_train", device=torch.cuda.get_device_name(0), reps=args.reps, pairs=args.pairs, rows={}, nets={})
    for sname, B, H, W in (s for s in SIZES if s[0] in args.sizes.split(",")):
        for lname, cin, cout, k, bias, lvl in LAYERS:
            g = torch.Generator(device="cpu").manual_seed(cin + H)
            h, w = H // lvl, W // lvl
            x = torch.randn((B, cin, h, w), generator=g).to(dev).requires_grad_(cin != 3)
            gy = torch.randn((B, cout, h, w), generator=g).to(dev)
            hip_m = DiffFeatureConv2d(cin, cout, k, padding=k // 2, bias=bias).to(dev)
            aten_m = nn.Conv2d(cin, cout, k, padding=k // 2, bias=bias).to(dev)
            aten_m.load_state_dict(hip_m.state_dict(), strict=True)

            def arm(m):
                leaves = ([x] if x.requires_grad else []) + list(m.parameters())
                return lambda: torch.autograd.grad(m(x), leaves, gy)

            agree = rel_diff(arm(hip_m)(), arm(aten_m)())
            r = ab({"hip": arm(hip_m), "aten": arm(aten_m)}, args.reps, args.pairs)
            r.update(cin=cin, cout=cout, k=k, B=B, H=h, W=w, gradients_rel_diff=agree)
            out["rows"][f"{sname}.{lname}"] = r
            print(f"# {sname}.{lname}: hip {r['hip_ms']['median']:.3f} ms [{r['hip_ms']['min']:.3f}, {r['hip_ms']['max']:.3f}]  aten "
                  f"{r['aten_ms']['median']:.3f} ms [{r['aten_ms']['min']:.3f}, {r['aten_ms']['max']:.3f}]  peak {r['hip_peak_mb']:.0f} / "
                  f"{r['aten_peak_mb']:.0f} MB  gradients differ by {agree:.1e}", file=sys.stderr, flush=True)
            del x, gy, hip_m, aten_m
        g = torch.Generator(device="cpu").manual_seed(H)
        x = torch.randn((B, 3, H, W), generator=g).to(dev)
        hip_net = DiffFeatureNet(8).to(dev).train()
        aten_net = _AtenFeatureNet().to(dev).train()
        aten_net.load_state_dict(hip_net.state_dict(), strict=True)
        gys = [torch.randn(s, generator=g).to(dev) for s in ((B, 64, H // 4, W // 4), (B, 32, H // 2, W // 2), (B, 16, H, W))]

        def hip_arm():
            o = hip_net(x)
            outs = [torch.cat((o[f"stage{i}"], o[f"stage{i}_c"]), 1) for i in (1, 2, 3)]
            return torch.autograd.grad(outs, list(hip_net.parameters()), gys)

        def aten_arm():
            return torch.autograd.grad(list(aten_net(x)), list(aten_net.parameters()), gys)

        agree = rel_diff(hip_arm(), aten_arm())
        r = ab({"hip": hip_arm, "aten": aten_arm}, 1, args.pairs)
        r.update(B=B, H=H, W=W, gradients_rel_diff=agree)
        out["nets"][sname] = r
        print(f"# {sname} DiffFeatureNet: hip {r['hip_ms']['median']:.2f} ms  aten {r['aten_ms']['median']:.2f} ms  peak "
              f"{r['hip_peak_mb']:.0f} / {r['aten_peak_mb']:.0f} MB  gradients differ by {agree:.1e}", file=sys.stderr, flush=True)
        del x, gys, hip_net, aten_net
        if args.md:   # (after every size: a run that is cut short keeps what it measured)
            with open(args.md, "w") as f:
                f.write(markdown(out))
    print(json.dumps(out))


def markdown(out):
    cell = lambda t: f"{t['median']:.3f} [{t['min']:.3f}, {t['max']:.3f}]"   # noqa: E731
    lines = ["# FeatureNet's rectangular layers and the whole FeatureNet, forward + backward, against ATen", "",
             f"`scripts/featurenet_train_bench.py` on {out['device']}, one process, arms alternating; median [min, max] of {out['pairs']} "
             f"window pairs of {out['reps']} repetitions (whole network: 1).  Times in ms per forward + backward of the batch (gradients for "
             "the input, where the layer has one, and every parameter).  hip: `DiffFeatureConv2d` (K3 forward and data gradient, K3f weight "
             "and bias gradient); ATen: `nn.Conv2d` with the same parameters.  Peak: allocated over one step above what was allocated before "
             "it, in MB.  The parent commit has no differentiable path for these layers, so ATen is the baseline.", "",
             "| size.layer | in -> out, k | B x H x W | hip | ATen | ATen / hip | peak MB hip / ATen | gradients, max rel. diff |",
             "|---|---|---|---|---|---|---|---|"]
    for name, r in out["rows"].items():
        lines.append(f"| {name} | {r['cin']} -> {r['cout']}, {r['k']} | {r['B']} x {r['H']} x {r['W']} | {cell(r['hip_ms'])} | {cell(r['aten_ms'])} | "
                     f"{r['aten_over_hip']:.2f} | {r['hip_peak_mb']:.0f} / {r['aten_peak_mb']:.0f} | {r['gradients_rel_diff']:.1e} |")
    lines += ["", "Whole network, train mode, forward + backward (gradients for every parameter): `DiffFeatureNet` (K3 / K3f / K3g / K3k / K3d / "
              "K5) against the same network on nn.Conv2d / nn.BatchNorm2d + ReLU, loaded from the same state dict.", "",
              "| size | B x H x W | hip | ATen | ATen / hip | peak MB hip / ATen | gradients, max rel. diff |", "|---|---|---|---|---|---|---|"]
    for name, r in out["nets"].items():
        lines.append(f"| {name} | {r['B']} x {r['H']} x {r['W']} | {cell(r['hip_ms'])} | {cell(r['aten_ms'])} | {r['aten_over_hip']:.2f} | "
                     f"{r['hip_peak_mb']:.0f} / {r['aten_peak_mb']:.0f} | {r['gradients_rel_diff']:.1e} |")
    lines.append("")
    return "\n".join(lines)


if __name__ == "__main__":
    main()
