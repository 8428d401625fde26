#!/usr/bin/env python
"""Time and size forward + backward of the differentiable dual-depth head and loss (dmvsnet_amd.DiffDepthNet: K4 + K4b,
dmvsnet_amd.diff_mvs_loss: N6 + N6b) against the same op sequence written with ATen ops, at the shapes of config 2
(1184 x 1600: D = 64 / 4 at 296 x 400, 32 / 4 at 592 x 800, 8 / 4 at 1184 x 1600), per sample (batch 1).

The ATen arm restates the reference's sequence op for op (softmax over D, p * depth summed, min / max of the pairs, the
where-chain of the checkerboard, the smooth-L1 terms on index-selected pixels, four grid_sample calls per cell-centre term);
autograd keeps what it keeps there.  Both arms run in one process on one GPU, on the same tensors; every arm is warmed, and the
timed windows alternate with the order swapped every round.  Per row and arm:
  ms        device events around --reps repetitions, per repetition; median over the windows (min / max in the JSON)
  peak_mb   torch.cuda.max_memory_allocated over one forward + backward, minus what was allocated before it
Rows: per stage "head + loss" (main pass -> refine pass on depth_values_c -> the stage's loss -> backward to both logit volumes);
per pass the head alone (random upstream gradients on its differentiable outputs) with K4b apart: its time, its achieved bytes/s
against 32 N bytes (N = D H W: the logit volume read and its gradient written once) and the fraction of the 8 TB/s HBM
roofline; the three-stage loss alone.  One JSON line; --md writes the table of profiles/head_train.md.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

STAGES = (("s1", 64, 296, 400, 0.5), ("s2", 32, 592, 800, 1.0), ("s3", 8, 1184, 1600, 2.0))   # name, D, h, w, dlossw
HBM_TB_S = 8.0


# ------------------------------------------------------------------------------------------------ the ATen arm
def _coors(H, W, dev):
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    return yy[None], xx[None]


def aten_forward(cost_reg, depth_values):
    """DepthNet.forward as ATen ops: -> (depth_sub_plus, depth_values_c)."""
    prob = F.softmax(cost_reg, dim=2)
    dsp = torch.sum(prob * depth_values.unsqueeze(1), 2)
    small, huge = dsp.split([2, 2], dim=1)
    smin, smax, hmin, hmax = small.min(1)[0], small.max(1)[0], huge.min(1)[0], huge.max(1)[0]
    hmin_d, hmax_d, smin_d, smax_d = 2 * hmin - hmax, 2 * hmax - hmin, 2 * smin - smax, 2 * smax - smin

    def six(lo, hi):
        return torch.stack((3 * lo - 2 * hi, 2 * lo - hi, lo, hi, 2 * hi - lo, 3 * hi - 2 * lo), 1)
    stacks = (six(smin, smax), six(hmin, hmax), six(smin_d, smax_d), six(hmin_d, hmax_d))
    yy, xx = _coors(dsp.shape[2], dsp.shape[3], dsp.device)
    out = torch.zeros_like(dsp)
    for q in range(4):
        for c in range(2):
            m = ((yy % 4 == q) & (xx % 2 == c)).unsqueeze(1)
            first = (c == 0) == (q % 2 == 0)
            out = torch.where(m, stacks[q][:, :-2] if first else stacks[q][:, 2:], out)
    return dsp, out


def aten_refine(cost_reg, depth_values, alpha=5):
    """DepthNet.refine as ATen ops: -> (depth_sub_plus_refine, depth)."""
    prob = F.softmax(cost_reg * alpha, dim=2)
    dsp = torch.sum(prob * depth_values.unsqueeze(1), 2)
    small, huge = dsp.split([2, 2], dim=1)
    smin, smax, hmin, hmax = small.min(1)[0], small.max(1)[0], huge.min(1)[0], huge.max(1)[0]
    yy, xx = _coors(dsp.shape[2], dsp.shape[3], dsp.device)
    depth = torch.zeros_like(dsp[:, 0])
    for (r, c), v in (((0, 0), smin), ((0, 1), smax), ((1, 0), hmax), ((1, 1), hmin)):
        depth = torch.where((yy % 2 == r) & (xx % 2 == c), v, depth)
    return dsp, depth


def _regression(est, gt, mask, weight):
    return (F.smooth_l1_loss(est[mask], gt[mask], reduction="none") * weight[mask]).mean()


def _centre_loss(est, gt, mask, weight):
    B, h, w = gt.shape
    y, x = torch.meshgrid(torch.arange(0, h - 1, dtype=torch.float32, device=gt.device),
                          torch.arange(0, w - 1, dtype=torch.float32, device=gt.device), indexing="ij")
    grid = torch.stack(((x + 0.5) / ((w - 1) / 2) - 1, (y + 0.5) / ((h - 1) / 2) - 1), 2).unsqueeze(0).repeat(B, 1, 1, 1)
    s = [F.grid_sample(t.unsqueeze(1), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
         for t in (gt, est, weight, mask.float())]
    return _regression(s[1], s[0], s[3] >= 1.0, s[2])


def aten_loss_set(dsp, gt, mask, w):
    mask = mask > 0.5
    small, huge = dsp.split([2, 2], dim=1)
    ones = torch.ones_like(gt) * w
    total = 0
    for pair in (small, huge):
        e = gt.unsqueeze(1).expand_as(pair)
        total = total + 2 * _regression(pair, e, mask.unsqueeze(1).expand_as(pair), torch.ones_like(pair) * w)
    yy, xx = _coors(gt.shape[1], gt.shape[2], gt.device)
    cm = (yy % 2) == (xx % 2)
    for pair in (small, huge):
        a0, a1 = (pair[:, 0] - gt).abs(), (pair[:, 1] - gt).abs()
        total = total + _regression((pair[:, 0] - pair[:, 1]).abs(), torch.where(a0 < a1, a1, a0), mask, ones)
    for pair in (small, huge):
        mn, mx = pair.min(1)[0], pair.max(1)[0]
        total = total + _centre_loss(torch.where(cm, mn, mx), gt, mask, ones) + _centre_loss(torch.where(~cm, mn, mx), gt, mask, ones)
    return total


# ------------------------------------------------------------------------------------------------ measuring
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


def ab(arms, reps, windows):
    """{"fused": fn, "aten": fn} -> row: every arm warmed, windows alternating with the order swapped every round."""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for w in range(windows):
        for k in (("fused", "aten") if w % 2 == 0 else ("aten", "fused")):
            ms[k].append(window(arms[k], reps))
    r = {k + "_ms": spread(v) for k, v in ms.items()}
    r.update({k + "_peak_mb": peak_mb(fn) for k, fn in arms.items()})
    r["aten_over_fused"] = r["aten_ms"]["median"] / r["fused_ms"]["median"]
    r["peak_aten_over_fused"] = r["aten_peak_mb"] / max(r["fused_peak_mb"], 1e-9)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--stages", default="s1,s2,s3")
    ap.add_argument("--md", default=None, help="also write the result table (markdown) to this file")
    args = ap.parse_args()

    from dmvsnet_amd import DiffDepthNet, diff_mvs_loss, ops
    assert torch.cuda.is_available(), "the benchmark needs the MI355X"
    dev = torch.device("cuda:0")
    net = DiffDepthNet("regression", prob_volume=False)
    out = dict(bench="head_train", device=torch.cuda.get_device_name(0), reps=args.reps, windows=args.windows, stages={}, passes={})
    planes = {}
    for name, D, h, w, dlossw in STAGES:
        if name not in args.stages.split(","):
            continue
        g = torch.Generator(device="cpu").manual_seed(D)
        gt = (600.0 + 40.0 * torch.sin(0.01 * torch.arange(h).view(1, h, 1)) + 30.0 * torch.cos(0.008 * torch.arange(w).view(1, 1, w))).to(dev)
        mask = (torch.rand(1, h, w, generator=g) > 0.15).float().to(dev)
        hyp = (gt.unsqueeze(1) + 8.0 * (torch.rand(1, 1, h, w, generator=g).to(dev) - 0.5)
               + (torch.arange(D, dtype=torch.float32, device=dev).view(1, D, 1, 1) - (D - 1) / 2) * (16.0 / (D - 1))).contiguous()
        L = (3.0 * torch.randn(1, 4, D, h, w, generator=g)).to(dev).requires_grad_(True)
        Lr = torch.randn(1, 4, 4, h, w, generator=g).to(dev).requires_grad_(True)
        itv = torch.tensor(16.0 / (D - 1), device=dev)
        gts, masks = {"stage1": gt}, {"stage1": mask}

        def fused():
            main_ = net(L, hyp, D, itv)
            ref_ = net.refine(Lr, main_["depth_values_c"], 4, itv)
            loss = diff_mvs_loss({"stage1": {**ref_, **main_}}, gts, masks, "regression", dlossw=[dlossw])
            return torch.autograd.grad(loss, [L, Lr])

        def aten():
            dsp, c = aten_forward(L, hyp)
            dsp_r, _ = aten_refine(Lr, c)
            loss = aten_loss_set(dsp, gt, mask, dlossw) + aten_loss_set(dsp_r, gt, mask, dlossw)
            return torch.autograd.grad(loss, [L, Lr])

        gf, ga = fused(), aten()
        agree = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(gf, ga))
        r = ab({"fused": fused, "aten": aten}, args.reps, args.windows)
        r.update(D=D, h=h, w=w, gradients_rel_diff=agree)
        out["stages"][name] = r
        print(f"# {name} head + loss: fused {r['fused_ms']['median']:.3f} ms  aten {r['aten_ms']['median']:.3f} ms  peak "
              f"{r['fused_peak_mb']:.0f} / {r['aten_peak_mb']:.0f} MB  gradients differ by {agree:.1e}", file=sys.stderr, flush=True)
        del gf, ga

        # the two passes apart, with K4b alone
        with torch.no_grad():
            hyps = net(L.detach(), hyp, D, itv)["depth_values_c"]
        for pname, lg, hp, alpha, mode in ((name + ".main", L, hyp, 1.0, 0), (name + ".refine", Lr, hyps.detach(), 5.0, 1)):
            Dp = lg.shape[2]
            g_dsp = torch.randn(1, 4, h, w, generator=g).to(dev)
            g_sel = torch.randn((1, 4, h, w) if mode == 0 else (1, h, w), generator=g).to(dev)
            hp_leaf = hp.clone().requires_grad_(mode == 1)   # the refine pass's hypotheses carry the edge
            wrt = [lg] + ([hp_leaf] if mode == 1 else [])

            def fused_pass():
                o = net(lg, hp_leaf, Dp, itv) if mode == 0 else net.refine(lg, hp_leaf, Dp, itv)
                outs = (o["depth_sub_plus"], o["depth_values_c"]) if mode == 0 else (o["depth_sub_plus_refine"], o["depth"])
                return torch.autograd.grad(outs, wrt, (g_dsp, g_sel))

            def aten_pass():
                outs = aten_forward(lg, hp_leaf) if mode == 0 else aten_refine(lg, hp_leaf)
                return torch.autograd.grad(outs, wrt, (g_dsp, g_sel))

            p = ab({"fused": fused_pass, "aten": aten_pass}, args.reps, args.windows)
            with torch.no_grad():
                dsp, _, _, _ = ops.depth_regress(lg.detach()[0], hp[0], itv.reshape(1), alpha, mode, False)
                gl = torch.empty_like(lg.detach()[0])
                gh = torch.empty_like(hp[0]) if mode == 1 else None
                k4b = lambda: ops.depth_regress_backward(lg.detach()[0], hp[0], alpha, mode, dsp, g_dsp[0], g_sel[0], mode == 1, gl, gh)  # noqa: E731
                k4 = lambda: ops.depth_regress(lg.detach()[0], hp[0], itv.reshape(1), alpha, mode, False)   # noqa: E731
                k4b()
                p["k4b_ms"] = float(np.median([window(k4b, args.reps) for _ in range(args.windows)]))
                p["k4_ms"] = float(np.median([window(k4, args.reps) for _ in range(args.windows)]))
            p["k4b_bytes"] = 32 * Dp * h * w
            p["k4b_tb_per_s"] = p["k4b_bytes"] / (p["k4b_ms"] * 1e-3) / 1e12
            p["k4b_roofline_fraction"] = p["k4b_tb_per_s"] / HBM_TB_S
            p.update(D=Dp, h=h, w=w)
            out["passes"][pname] = p
            print(f"# {pname}: fused {p['fused_ms']['median']:.3f} ms  aten {p['aten_ms']['median']:.3f} ms  K4b {p['k4b_ms']:.3f} ms "
                  f"= {p['k4b_tb_per_s']:.2f} TB/s", file=sys.stderr, flush=True)
            del gl, gh, dsp
        with torch.no_grad():
            planes[name] = (net(L.detach(), hyp, D, itv)["depth_sub_plus"], net.refine(Lr.detach(), hyps, 4, itv)["depth_sub_plus_refine"],
                            gt, mask, dlossw)
        del L, Lr, hyp, hyps

    if len(planes) == len(STAGES):   # the three-stage loss alone
        keys = ["stage1", "stage2", "stage3"]
        leaves = {k: (planes[n][0].clone().requires_grad_(True), planes[n][1].clone().requires_grad_(True)) for k, n in zip(keys, planes)}
        gts = {k: planes[n][2] for k, n in zip(keys, planes)}
        masks = {k: planes[n][3] for k, n in zip(keys, planes)}
        ws = [planes[n][4] for n in planes]
        flat = [t for k in keys for t in leaves[k]]

        def fused_loss():
            inputs = {k: {"depth_sub_plus": leaves[k][0], "depth_sub_plus_refine": leaves[k][1]} for k in keys}
            return torch.autograd.grad(diff_mvs_loss(inputs, gts, masks, "regression", dlossw=ws), flat)

        def aten_loss():
            total = sum(aten_loss_set(leaves[k][i], gts[k], masks[k], w_) for k, w_ in zip(keys, ws) for i in range(2))
            return torch.autograd.grad(total, flat)

        out["loss3"] = ab({"fused": fused_loss, "aten": aten_loss}, args.reps, args.windows)
        print(f"# three-stage loss: fused {out['loss3']['fused_ms']['median']:.3f} ms  aten {out['loss3']['aten_ms']['median']:.3f} ms",
              file=sys.stderr, flush=True)
    print(json.dumps(out))
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(out))


def markdown(out):
    lines = ["# Dual-depth head and loss, forward + backward: fused (K4 + K4b, N6 + N6b) against the ATen op sequence", "",
             f"`scripts/head_train_bench.py` on {out['device']}, one process, arms alternating; median of {out['windows']} windows of "
             f"{out['reps']} repetitions, per sample (batch 1), config-2 shapes.  Times in ms, memory in MB (peak allocated over one "
             "forward + backward, above what was allocated before).", "",
             "## Per stage: main pass -> refine pass -> the stage's loss -> backward to both logit volumes", "",
             "| stage | D | h x w | fused | ATen | ATen / fused | fused peak | ATen peak | peak ATen / fused | gradients, max rel. diff |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for name, r in out["stages"].items():
        lines.append(f"| {name} | {r['D']} / 4 | {r['h']} x {r['w']} | {r['fused_ms']['median']:.3f} | {r['aten_ms']['median']:.3f} | "
                     f"{r['aten_over_fused']:.1f} | {r['fused_peak_mb']:.0f} | {r['aten_peak_mb']:.0f} | {r['peak_aten_over_fused']:.1f} | "
                     f"{r['gradients_rel_diff']:.1e} |")
    lines += ["", "## Per pass: the head alone (random upstream gradients), and K4b apart", "",
              "| pass | D | h x w | fused fwd+bwd | ATen fwd+bwd | ATen / fused | fused peak | ATen peak | K4 | K4b | K4b TB/s (32 N bytes) | of 8 TB/s |",
              "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, p in out["passes"].items():
        lines.append(f"| {name} | {p['D']} | {p['h']} x {p['w']} | {p['fused_ms']['median']:.3f} | {p['aten_ms']['median']:.3f} | "
                     f"{p['aten_over_fused']:.1f} | {p['fused_peak_mb']:.0f} | {p['aten_peak_mb']:.0f} | {p['k4_ms']:.3f} | {p['k4b_ms']:.3f} | "
                     f"{p['k4b_tb_per_s']:.2f} | {p['k4b_roofline_fraction']:.2f} |")
    if "loss3" in out:
        r = out["loss3"]
        lines += ["", "## The three-stage loss alone (N6 + N6b against ATen), forward + backward", "",
                  "| fused | ATen | ATen / fused | fused peak | ATen peak |", "|---|---|---|---|---|",
                  f"| {r['fused_ms']['median']:.3f} | {r['aten_ms']['median']:.3f} | {r['aten_over_fused']:.1f} | {r['fused_peak_mb']:.1f} | "
                  f"{r['aten_peak_mb']:.0f} |"]
    lines.append("")
    return "\n".join(lines)


if __name__ == "__main__":
    main()
