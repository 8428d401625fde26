#!/usr/bin/env python
"""Time one whole DMVSNet training step -- forward, dual-depth loss, backward, Adam -- on ``dmvsnet_amd.DiffMVSNet`` against the same
model on stock ATen layers (``StockMVSNet(float32)`` of tests/train_step_ref.py: the same wiring function over nn.Conv / nn.BatchNorm,
``grid_sample`` and torch softmax / min / max, moved to the GPU), built from the same state dict, on the same MI355X.  Sizes: the
reference's DTU training recipe (scripts/train.sh: 512 x 640, 5 views, 48 / 32 / 8 planes, ratios 4 / 2 / 1, inverse depth, loss weights
0.5 / 1 / 2, Adam at 1e-3) at batch 1 and 2.  The hypothesis planes of both arms come from the product's kernels (the stock helper
computes them on the CPU); they are two small launches per stage and sample.

Both arms run in one process on one GPU on the same batch; every arm is warmed with two steps, and the timed windows come in pairs whose
order is swapped every pair.  Per arm: device events around one step, the median over the pairs with min and max.  Peak memory:
allocated over one step above what was allocated before it (weights, gradients and Adam's moments are there already).  Then ONE more
HIP step runs under ``ops.KernelTimer``: per kernel family the launches and the sum of their durations, and as a line of its own what
is left of the step's device time -- the ATen glue (36 skip additions and their gradient fan-in, the channel ``cat`` / ``split``, two
nearest up-samplings), autograd's accumulations, Adam, and idle gaps between launches.  The timer's own events add host work to that
step, so the step time quoted beside the split is the timed windows' median, and the remainder is what is left of THAT.  One JSON line;
--md writes profiles/train_step.md.  Nothing here is asserted by a test.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

RECIPE = dict(H=512, W=640, V=5, ndepths=(48, 32, 8), ratios=(4, 2, 1), inverse=True, dlossw=(0.5, 1.0, 2.0), lr=1e-3)
SIZES = (("dtu.b1", 1), ("dtu.b2", 2))


def spread(ts):
    return dict(min=min(ts), median=float(np.median(ts)), max=max(ts), n=len(ts))


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=5, help="timed (hip, aten) window pairs per size, at least 5")
    ap.add_argument("--sizes", default=",".join(s[0] for s in SIZES), help="comma-separated subset of the sizes")
    ap.add_argument("--height", type=int, default=RECIPE["H"])
    ap.add_argument("--width", type=int, default=RECIPE["W"])
    ap.add_argument("--md", default=None, help="also write the result table (markdown) to this file")
    args = ap.parse_args()
    assert args.pairs >= 5

    import train_step_ref as T
    import dmvsnet_amd as da
    from dmvsnet_amd import ops, train
    assert torch.cuda.is_available(), "the benchmark needs the MI355X"
    H, W, V = args.height, args.width, RECIPE["V"]
    sd = T.synth.synth_state_dict(T.StockMVSNet(RECIPE["ndepths"], RECIPE["ratios"]).state_dict(), 0)
    sd = {k: (v / 20 if k.endswith("prob.weight") else v) for k, v in sd.items()}
    out = dict(bench="train_step", device=torch.cuda.get_device_name(0), pairs=args.pairs, recipe={**RECIPE, "H": H, "W": W}, sizes={})
    for name, B in (s for s in SIZES if s[0] in args.sizes.split(",")):
        imgs, proj, dv = T.make_inputs(B, V, H, W)
        gt, mask = T.make_ground_truth(B, H, W)
        sample = {"imgs": imgs.cuda(), "proj_matrices": {k: v.cuda() for k, v in proj.items()}, "depth_values": dv.cuda(),
                  "depth": {k: v.cuda() for k, v in gt.items()}, "mask": {k: v.cuda() for k, v in mask.items()}}
        hip = da.DiffMVSNet(list(RECIPE["ndepths"]), list(RECIPE["ratios"]), inverse_depth=RECIPE["inverse"])
        hip.load_state_dict(sd, strict=True)
        hip = hip.cuda().train()
        hip_opt = torch.optim.Adam(hip.parameters(), lr=RECIPE["lr"])
        stock = T.stock_model(sd, torch.float32, RECIPE["ndepths"], RECIPE["ratios"]).cuda()
        stock.inverse_depth = RECIPE["inverse"]
        stock.hypotheses = (train._hypotheses_first, train._hypotheses_next)
        stock_opt = torch.optim.Adam(stock.parameters(), lr=RECIPE["lr"])
        losses = {"hip": [], "aten": []}

        def hip_step():
            losses["hip"].append(da.train_step(hip, hip_opt, sample, RECIPE["dlossw"])["loss"])

        def aten_step():
            loss = T.stock_loss(stock(sample["imgs"], sample["proj_matrices"], sample["depth_values"]), sample["depth"], sample["mask"],
                                RECIPE["dlossw"])
            stock_opt.zero_grad()
            loss.backward()
            stock_opt.step()
            losses["aten"].append(loss.detach())

        arms = {"hip": hip_step, "aten": aten_step}
        for fn in arms.values():
            fn(), fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for w in range(args.pairs):
            for k in (("hip", "aten") if w % 2 == 0 else ("aten", "hip")):
                ms[k].append(window(arms[k]))
        r = {k + "_ms": spread(v) for k, v in ms.items()}
        r["aten_over_hip"] = r["aten_ms"]["median"] / r["hip_ms"]["median"]
        r.update({k + "_peak_mb": peak_mb(fn) for k, fn in arms.items()})
        r["first_losses"] = {k: [float(v) for v in vs[:3]] for k, vs in losses.items()}
        # the per-family split of one more HIP step
        ops.timer = ops.KernelTimer()
        ops.timer.reserve(4096)
        try:
            hip_step()
            torch.cuda.synchronize()
            fam = ops.timer.summary()
        finally:
            ops.timer = None
        r["families"] = {k: dict(launches=v["launches"], sum_ms=v["sum_ms"]) for k, v in sorted(fam.items(), key=lambda kv: -kv[1]["sum_ms"])}
        r["kernels_sum_ms"] = sum(v["sum_ms"] for v in fam.values())
        r["rest_ms"] = r["hip_ms"]["median"] - r["kernels_sum_ms"]
        r.update(B=B, H=H, W=W, V=V)
        out["sizes"][name] = r
        print(f"# {name}: hip {r['hip_ms']['median']:.1f} ms [{r['hip_ms']['min']:.1f}, {r['hip_ms']['max']:.1f}]  aten {r['aten_ms']['median']:.1f} ms "
              f"[{r['aten_ms']['min']:.1f}, {r['aten_ms']['max']:.1f}]  peak {r['hip_peak_mb']:.0f} / {r['aten_peak_mb']:.0f} MB  kernels "
              f"{r['kernels_sum_ms']:.1f} ms  rest {r['rest_ms']:.1f} ms  losses {r['first_losses']}", file=sys.stderr, flush=True)
        del hip, stock, hip_opt, stock_opt, sample
        if args.md:   # (after every size: a run that is cut short keeps what it measured)
            with open(args.md, "w") as f:
                f.write(markdown(out))
    print(json.dumps(out))


def markdown(out):
    cell = lambda t: f"{t['median']:.1f} [{t['min']:.1f}, {t['max']:.1f}]"   # noqa: E731
    rc = out["recipe"]
    lines = ["# One whole training step: `DiffMVSNet` against the same model on stock ATen layers", "",
             f"`scripts/train_step_bench.py` on {out['device']}, one process, arms alternating; median [min, max] of {out['pairs']} window pairs "
             f"of one step.  A step is forward + `diff_mvs_loss` + backward + Adam on the reference's DTU training recipe: {rc['H']} x {rc['W']}, "
             f"{rc['V']} views, {' / '.join(map(str, rc['ndepths']))} planes, ratios {' / '.join(map(str, rc['ratios']))}, inverse depth.  hip: "
             "`dmvsnet_amd.DiffMVSNet` + `train_step`; ATen: `StockMVSNet(float32)` of tests/train_step_ref.py on the GPU (nn.Conv / nn.BatchNorm, "
             "`grid_sample`, torch softmax / min / max; the same wiring function, the same state dict).  Times in ms per step of the batch.  Peak: "
             "allocated over one step above what was allocated before it, in MB.  The parent commit has no training model, so ATen is the "
             "baseline.", "",
             "The ATen arm is stock PyTorch as it comes: whatever the library picks for fp32 3D convolutions, transposed convolutions and their "
             "gradients at these volumes, `grid_sample` with its materialised warped volumes, boolean-mask indexing in the loss (which synchronises).  "
             "Nothing in it was tuned (no channels-last, no convolution search), so ATen / hip says what a user gains over the unpatched reference on "
             "this GPU, not how far the HIP kernels are from a well-tuned library.  Both arms' first three losses are in the JSON line: the first step's "
             "agree to four digits, after which the two trajectories drift apart as fp32 training runs do.", "",
             "| size | B | hip | ATen | ATen / hip | peak MB hip / ATen |", "|---|---|---|---|---|---|"]
    for name, r in out["sizes"].items():
        lines.append(f"| {name} | {r['B']} | {cell(r['hip_ms'])} | {cell(r['aten_ms'])} | {r['aten_over_hip']:.2f} | {r['hip_peak_mb']:.0f} / {r['aten_peak_mb']:.0f} |")
    for name, r in out["sizes"].items():
        lines += ["", f"## Where the HIP step's time goes, {name}", "",
                  f"One more step under `ops.KernelTimer`: launches and summed kernel durations per family.  The last line is what is left of the "
                  f"step's median above ({r['hip_ms']['median']:.1f} ms): the ATen glue (skip additions and their gradient fan-in, channel `cat` / "
                  "`split`, two nearest up-samplings), autograd's accumulations, Adam, the launches the timer does not record (layout glue, hypothesis "
                  "planes, K1b, the loss) and idle gaps between launches while the host prepares the next one.", "",
                  "| family | launches | sum of kernel durations, ms | share of the step |", "|---|---|---|---|"]
        for fam, v in r["families"].items():
            lines.append(f"| {fam} | {v['launches']} | {v['sum_ms']:.2f} | {v['sum_ms'] / r['hip_ms']['median']:.1%} |")
        lines.append(f"| all kernels | {sum(v['launches'] for v in r['families'].values())} | {r['kernels_sum_ms']:.2f} | "
                     f"{r['kernels_sum_ms'] / r['hip_ms']['median']:.1%} |")
        lines.append(f"| ATen glue, Adam, gaps (the remainder) | | {r['rest_ms']:.2f} | {r['rest_ms'] / r['hip_ms']['median']:.1%} |")
    lines.append("")
    return "\n".join(lines)


if __name__ == "__main__":
    main()
