#!/usr/bin/env python
"""Time and size forward + backward of train-mode BatchNorm + ReLU on the product's kernels (dmvsnet_amd.DiffBatchNormReLU3d /
DiffBatchNormReLU2d: K5) against ``F.relu(F.batch_norm(..., training=True))`` on ATen on the same MI355X, at the block output volumes
of the regularisation U-Nets: per stage the 8-channel blocks (conv0, conv11) work at the stage's full volume, the 16-channel ones
(conv1, conv2, conv9) at 1/2, the 32-channel ones (conv3, conv4, conv7) at 1/4 and the 64-channel ones (conv5, conv6) at 1/8; the
refine net's 2D bottleneck is a 64-channel image.  Volumes: the reference's training recipe (scripts/train.sh: 512 x 640, ndepths
48 / 32 / 8; rows "train.*") and the config-2 stage passes (1184 x 1600, ndepths 64 / 32 / 8; rows "c2.*"), batch 1.

Both arms run in one process on one GPU, on the same tensors; every arm is warmed, and the timed windows alternate with the order
swapped every round.  Per row and arm:
  ms        device events around --reps repetitions, per repetition; median over the windows (min / max in the JSON)
  peak_mb   torch.cuda.max_memory_allocated over one forward + backward, minus what was allocated before it
  GB/s      the ALGORITHMIC bytes of the fused operator -- 3 passes forward (x twice, y once), 5 backward (x and gy twice, gx once),
            4 bytes each -- over the time, next to the 6.3 TB/s achievable HBM rate.  Where the backward's working set (x, gy and gx:
            three tensors) is under about 256 MB the Infinity Cache may serve re-reads between passes: the column "IC" marks those.
One JSON line; --md writes the table of profiles/bn_train.md.

--sync replaces the ATen arm by the synchronised-statistics launch sequence of ``DiffSyncBatchNormReLU*`` with R = 1 and no collective:
local moments (statistics + fold), the rank's own [1, C, 3] moments fed back as the gathered buffer, the sync apply; backward sums
(reduce + fold), its own [1, C, 2] pair fed back, the sync backward apply -- the four ``ops.bn_sync_*`` wrappers under one autograd
Function.  Against plain K5 it prices the two extra fold launches, the fp64 combine in the apply prologues and the read-back of the
counts (one stream synchronisation per forward); what a collective itself costs is not in it.  --md then writes the sync table.
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

HBM_GBS = 6300.0
PASSES = 8   # 3 forward + 5 backward

# (stage, full volume (D, H, W) of the stage)
STAGES = (("train.s1", (48, 128, 160)), ("train.s2", (32, 256, 320)), ("train.s3", (8, 512, 640)),
          ("c2.s1", (64, 296, 400)), ("c2.s2", (32, 592, 800)), ("c2.s3", (8, 1184, 1600)))
LEVELS = ((8, 1, "conv0/11"), (16, 2, "conv1/2/9"), (32, 4, "conv3/4/7"), (64, 8, "conv5/6"))


def rows():
    """(row, C, number of spatial dimensions, spatial shape)"""
    out = []
    for stage, (D, H, W) in STAGES:
        for C, div, layers in LEVELS:
            out.append((f"{stage}.{layers}", C, 3, (D // div, H // div, W // div)))
    out.append(("train.s3.refine.conv6", 64, 2, (64, 80)))
    out.append(("c2.s3.refine.conv6", 64, 2, (148, 200)))
    return out


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
    """{"hip": fn, other: fn} -> row: every arm warmed, windows alternating with the order swapped every round."""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    other = next(k for k in arms if k != "hip")
    for w in range(windows):
        for k in (("hip", other) if w % 2 == 0 else (other, "hip")):
            ms[k].append(window(arms[k], reps))
    r = {k + "_ms": spread(v) for k, v in ms.items()}
    r.update({k + "_peak_mb": peak_mb(fn) for k, fn in arms.items()})
    r[other + "_over_hip"] = r[other + "_ms"]["median"] / r["hip_ms"]["median"]
    return r


def sync_function():
    """The sync launch sequence with R = 1 under autograd: every gathered buffer is this process's own row."""
    from dmvsnet_amd import ops

    class SyncLoop(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, weight, bias, rm, rv, momentum, eps):
            xd = x.detach()
            y, mean, invstd, N = ops.bn_sync_forward(xd, weight.detach(), bias.detach(), rm, rv, ops.bn_sync_moments(xd)[None], momentum,
                                                     eps, True)
            ctx.save_for_backward(xd, weight, bias, mean, invstd)
            ctx.N = N
            return y

        @staticmethod
        def backward(ctx, gy):
            x, weight, bias, mean, invstd = ctx.saved_tensors
            gy, w, b = gy.contiguous(), weight.detach(), bias.detach()
            sums, g_gamma, g_beta = ops.bn_sync_backward_sums(x, gy, w, b, mean, invstd, True)
            return ops.bn_sync_backward_apply(x, gy, w, b, mean, invstd, sums[None], ctx.N, True), g_gamma, g_beta, None, None, None, None

    return SyncLoop


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--rows", default="", help="comma-separated substrings: only the rows that contain one of them")
    ap.add_argument("--md", default=None, help="also write the result table (markdown) to this file")
    ap.add_argument("--sync", action="store_true", help="second arm: the synchronised-statistics launch sequence with R = 1, not ATen")
    args = ap.parse_args()

    from dmvsnet_amd import DiffBatchNormReLU2d, DiffBatchNormReLU3d
    assert torch.cuda.is_available(), "the benchmark needs the MI355X"
    dev = torch.device("cuda:0")
    other = "sync" if args.sync else "aten"
    sync_fn = sync_function() if args.sync else None
    out = dict(bench="bn_train_sync" if args.sync else "bn_train", device=torch.cuda.get_device_name(0), reps=args.reps, windows=args.windows, rows={})
    want = [s for s in args.rows.split(",") if s]
    for name, C, nd, spatial in rows():
        if want and not any(s in name for s in want):
            continue
        g = torch.Generator(device="cpu").manual_seed(C + nd + spatial[0])
        shape = (1, C) + tuple(spatial)
        x = torch.randn(shape, generator=g).to(dev).requires_grad_(True)
        gy = torch.randn(shape, generator=g).to(dev)
        hip = (DiffBatchNormReLU3d if nd == 3 else DiffBatchNormReLU2d)(C).to(dev).train()
        with torch.no_grad():
            hip.weight.copy_(1.0 + 0.2 * torch.randn(C, generator=g))
            hip.bias.copy_(0.2 * torch.randn(C, generator=g))
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)

        def hip_arm():
            return torch.autograd.grad(hip(x), [x, hip.weight, hip.bias], gy)

        def aten_arm():
            return torch.autograd.grad(F.relu(F.batch_norm(x, rm, rv, hip.weight, hip.bias, True, 0.1, hip.eps)), [x, hip.weight, hip.bias], gy)

        def sync_arm():
            return torch.autograd.grad(sync_fn.apply(x, hip.weight, hip.bias, rm, rv, 0.1, hip.eps), [x, hip.weight, hip.bias], gy)

        other_arm = sync_arm if args.sync else aten_arm
        gh, ga = hip_arm(), other_arm()
        # the two arms round the statistics differently: an element whose pre-activation lies within that rounding of the ReLU kink
        # gets the other mask, and its g_x differs by a whole gy * scale.  Such elements are counted, not averaged away.
        dx = (gh[0] - ga[0]).abs() / ga[0].abs().max()
        flipped = dx > 1e-3
        n_flipped = int(flipped.sum())
        agree = max([dx[~flipped].max().item()] + [((a - b).abs().max() / b.abs().max()).item() for a, b in zip(gh[1:], ga[1:])])
        del gh, ga, dx, flipped
        r = ab({"hip": hip_arm, other: other_arm}, args.reps, args.windows)
        nbytes = 4.0 * x.numel()
        r.update(C=C, shape=" x ".join(str(n) for n in spatial), tensor_mb=nbytes / 2 ** 20, gradients_rel_diff=agree, kink_flips=n_flipped,
                 hip_gbs=PASSES * nbytes / (r["hip_ms"]["median"] * 1e-3) / 1e9)
        r[other + "_gbs"] = PASSES * nbytes / (r[other + "_ms"]["median"] * 1e-3) / 1e9
        out["rows"][name] = r
        print(f"# {name}: hip {r['hip_ms']['median']:.3f} ms ({r['hip_gbs']:.0f} GB/s)  {other} {r[other + '_ms']['median']:.3f} ms  peak "
              f"{r['hip_peak_mb']:.0f} / {r[other + '_peak_mb']:.0f} MB  gradients differ by {agree:.1e} ({n_flipped} kink flips)", file=sys.stderr, flush=True)
        del x, gy, hip
    print(json.dumps(out))
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown_sync(out) if args.sync else markdown(out))


def markdown(out):
    lines = ["# Train-mode BatchNorm + ReLU, forward + backward: K5 against ATen", "",
             f"`scripts/bn_train_bench.py` on {out['device']}, one process, arms alternating; median of {out['windows']} windows of "
             f"{out['reps']} repetitions, batch 1.  Times in ms, memory in MB (peak allocated over one forward + backward, above what was "
             "allocated before).  GB/s: the algorithmic bytes of the fused operator (3 passes forward, 5 backward, 4 bytes per element) "
             "over the time of the arm, to be read against the 6.3 TB/s achievable HBM rate -- it is a rate of the whole forward + "
             "backward call (launch gaps and autograd's host work included), not of a kernel.  Column `IC`: yes where the backward's working set (x, gy "
             "and gx, three times `tensor MB`) is under about 256 MB, so that the Infinity Cache may serve re-reads between passes and the "
             "GB/s can exceed what HBM delivers.  gradients: the largest "
             "distance between the two arms over g_x, g_gamma and g_beta, each over its max-abs; `kink flips` counts the elements of g_x left "
             "out of it because the arms, which round the statistics differently, put them on different sides of the ReLU kink (more than "
             "1e-3 of max |g_x| apart).", "",
             "| blocks | C | volume | tensor MB | IC | hip fwd+bwd | ATen fwd+bwd | ATen / hip | hip GB/s | ATen GB/s | hip of 6.3 TB/s | hip peak | ATen peak | gradients, max rel. diff | kink flips |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, r in out["rows"].items():
        lines.append(f"| {name} | {r['C']} | {r['shape']} | {r['tensor_mb']:.1f} | {'yes' if 3 * r['tensor_mb'] < 256 else 'no'} | "
                     f"{r['hip_ms']['median']:.3f} | {r['aten_ms']['median']:.3f} | {r['aten_over_hip']:.2f} | {r['hip_gbs']:.0f} | "
                     f"{r['aten_gbs']:.0f} | {r['hip_gbs'] / HBM_GBS:.2f} | {r['hip_peak_mb']:.0f} | {r['aten_peak_mb']:.0f} | "
                     f"{r['gradients_rel_diff']:.1e} | {r['kink_flips']} |")
    lines.append("")
    return "\n".join(lines)


def markdown_sync(out):
    lines = ["## Synchronised statistics: the sync launch sequence against plain K5", "",
             f"`scripts/bn_train_bench.py --sync` on {out['device']}, one process, arms alternating; median of {out['windows']} windows of "
             f"{out['reps']} repetitions, batch 1, forward + backward, times in ms.  `sync`: local moments (statistics + fold), the "
             "rank's own moments fed back as the gathered buffer (R = 1, no collective), sync apply; backward sums (reduce + fold), fed "
             "back, sync backward apply.  `sync - hip` is the price of the two extra fold launches, the fp64 combine in the two apply "
             "prologues and the read-back of the counts (one stream synchronisation per forward).  The collectives themselves are not "
             "in it: their latency over RCCL between GPUs is unmeasured.", "",
             "| blocks | C | volume | tensor MB | hip fwd+bwd | sync fwd+bwd | sync - hip | sync / hip | outputs, max rel. diff |",
             "|---|---|---|---|---|---|---|---|---|"]
    for name, r in out["rows"].items():
        h, s = r["hip_ms"]["median"], r["sync_ms"]["median"]
        lines.append(f"| {name} | {r['C']} | {r['shape']} | {r['tensor_mb']:.1f} | {h:.3f} | {s:.3f} | {s - h:.3f} | {s / h:.2f} | "
                     f"{r['gradients_rel_diff']:.1e} |")
    lines.append("")
    return "\n".join(lines)


if __name__ == "__main__":
    main()
