#!/usr/bin/env python
"""Time and size forward + backward of the six stride-1 square convolutions on the product's kernels (dmvsnet_amd.DiffConv3d /
DiffConv2d: K3 forward and data gradient, K3g weight gradient) against nn.Conv3d / nn.Conv2d on ATen (MIOpen) on the same MI355X, per
sample (batch 1); and of the eight stride-2 / transposed layers between them (DiffConv3d / DiffConv2d at stride 2,
DiffConvTranspose3d / DiffConvTranspose2d: K3 in both stride-2 modes, K3h weight gradient) against nn.Conv3d / nn.ConvTranspose3d and
the 2D forms; and of FeatureNet's two 5x5 stride-2 layers conv1.0 / conv2.0 (DiffConv2d at kernel 5: K3 forward, K3d data gradient, K3k
weight gradient; rows "*.feature.conv1.0" / "*.feature.conv2.0", D x H x W their coarse output) against nn.Conv2d.  A strided row is named after its layer (conv1 / 3 / 5 going down, conv7 / 9 / 11 going up, the refine net's 2D conv5 /
conv7); its coarse volume is the volume of the square layer it sits next to (conv1 and conv11: conv2's, ...), its fine one twice that.

Volumes per layer: the layer's volumes in the reference's training recipe (scripts/train.sh: 512 x 640, ndepths 48 / 32 / 8; rows
"train.*") and in the config-2 stage passes (1184 x 1600, ndepths 64 / 32 / 8; rows "c2.*"): conv2 works at 1/2 of a stage's volume,
conv4 at 1/4, conv6 at 1/8; the refine net has 4 hypotheses and a 2D bottleneck; FeatureNet's conv1.x / conv2.x work at 1/2 and 1/4 of
the image.

Both arms run in one process on one GPU, on the same tensors; every arm is warmed, and the timed windows alternate with the order
swapped every round.  Per row and arm:
  ms        device events around --reps repetitions, per repetition; median over the windows (min / max in the JSON)
  peak_mb   torch.cuda.max_memory_allocated over one forward + backward, minus what was allocated before it
and the weight-gradient kernel alone (K3g, or K3h on the strided rows): its time and its fraction of the 157 TFLOP/s fp32 MFMA peak at
2 * 9 * kd * Cout * Cin * (output voxels of the GEMM's reduction: D * H * W, coarse for K3h) FLOP.
On the 5x5 rows also K3d alone and both kernels' fraction of the HBM floor (the bytes of their tensors at 8 TB/s).
One JSON line; --md writes the table of profiles/conv_train.md.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

PEAK_TF = 157.0
HBM_TBS = 8.0

# FeatureNet's 5x5 stride-2 layers: (row, Cb, fine (H, W)) -- conv1.0 reads the image-sized conv0 output, conv2.0 half of it
ROWS_K5S2 = (("train.feature.conv1.0", 8, (512, 640)), ("train.feature.conv2.0", 16, (256, 320)),
             ("c2.feature.conv1.0", 8, (1184, 1600)), ("c2.feature.conv2.0", 16, (592, 800)))

# (row, C, kdepth, (D, H, W))
ROWS = (
    ("train.s1.conv2", 16, 3, (24, 64, 80)), ("train.s2.conv2", 16, 3, (16, 128, 160)), ("train.s3.conv2", 16, 3, (4, 256, 320)),
    ("train.s1.conv4", 32, 3, (12, 32, 40)), ("train.s2.conv4", 32, 3, (8, 64, 80)), ("train.s3.conv4", 32, 3, (2, 128, 160)),
    ("train.s1.conv6", 64, 3, (6, 16, 20)), ("train.s2.conv6", 64, 3, (4, 32, 40)), ("train.s3.conv6", 64, 3, (1, 64, 80)),
    ("train.s3.refine.conv6", 64, 1, (1, 64, 80)),
    ("train.feature.conv1.x", 16, 1, (1, 256, 320)), ("train.feature.conv2.x", 32, 1, (1, 128, 160)),
    ("c2.s1.conv2", 16, 3, (32, 148, 200)), ("c2.s2.conv2", 16, 3, (16, 296, 400)), ("c2.s3.conv2", 16, 3, (4, 592, 800)),
    ("c2.s1.conv4", 32, 3, (16, 74, 100)), ("c2.s2.conv4", 32, 3, (8, 148, 200)), ("c2.s3.conv4", 32, 3, (2, 296, 400)),
    ("c2.s1.conv6", 64, 3, (8, 37, 50)), ("c2.s2.conv6", 64, 3, (4, 74, 100)), ("c2.s3.conv6", 64, 3, (1, 148, 200)),
    ("c2.s3.refine.conv6", 64, 1, (1, 148, 200)),
    ("c2.feature.conv1.x", 16, 1, (1, 592, 800)), ("c2.feature.conv2.x", 32, 1, (1, 296, 400)),
)


# the strided neighbours of a square row: (suffix of the square layer, stride-2 conv going down, transposed conv going up)
NEIGHBOURS = (("refine.conv6", "refine.conv5", "refine.conv7"), (".conv2", ".conv1", ".conv11"), (".conv4", ".conv3", ".conv9"),
              (".conv6", ".conv5", ".conv7"))


def strided_rows():
    """(row, mode, Ca, kdepth, coarse (D, H, W)) of the eight layers at every volume of ROWS they occur at."""
    rows = []
    for name, C, kd, vol in ROWS:
        if "feature" in name:
            continue
        for suffix, down, up in NEIGHBOURS:
            if name.endswith(suffix):
                stem = name[:-len(suffix)]
                rows += [(stem + down, "conv", C, kd, vol), (stem + up, "deconv", C, kd, vol)]
                break
    return rows


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
    """{"hip": fn, "aten": fn} -> row: every arm warmed, windows alternating with the order swapped every round."""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for w in range(windows):
        for k in (("hip", "aten") if w % 2 == 0 else ("aten", "hip")):
            ms[k].append(window(arms[k], reps))
    r = {k + "_ms": spread(v) for k, v in ms.items()}
    r.update({k + "_peak_mb": peak_mb(fn) for k, fn in arms.items()})
    r["aten_over_hip"] = r["aten_ms"]["median"] / r["hip_ms"]["median"]
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--rows", default="", help="comma-separated substrings: only the rows that contain one of them")
    ap.add_argument("--md", default=None, help="also write the result table (markdown) to this file")
    args = ap.parse_args()

    from dmvsnet_amd import DiffConv2d, DiffConv3d, ops
    assert torch.cuda.is_available(), "the benchmark needs the MI355X"
    dev = torch.device("cuda:0")
    out = dict(bench="conv_train", device=torch.cuda.get_device_name(0), reps=args.reps, windows=args.windows, rows={})
    want = [s for s in args.rows.split(",") if s]
    for name, C, kd, (D, H, W) in ROWS:
        if want and not any(s in name for s in want):
            continue
        g = torch.Generator(device="cpu").manual_seed(C + kd + D)
        shape = (1, C, D, H, W) if kd == 3 else (1, C, H, W)
        x = torch.randn(shape, generator=g).to(dev).requires_grad_(True)
        gy = torch.randn(shape, generator=g).to(dev)
        hip = (DiffConv3d if kd == 3 else DiffConv2d)(C, C, 3, stride=1, padding=1, bias=False).to(dev)
        aten = (nn.Conv3d if kd == 3 else nn.Conv2d)(C, C, 3, stride=1, padding=1, bias=False).to(dev)
        aten.load_state_dict(hip.state_dict())

        def arm(m):
            return lambda: torch.autograd.grad(m(x), [x, m.weight], gy)

        gh, ga = arm(hip)(), arm(aten)()
        agree = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(gh, ga))
        r = ab({"hip": arm(hip), "aten": arm(aten)}, args.reps, args.windows)
        x4, gy4 = x.detach().reshape(C, D, H, W), gy.reshape(C, D, H, W)
        gw = torch.empty_like(hip.weight)
        k3g = lambda: ops.conv3d_wgrad(x4, gy4, kd, out=gw)   # noqa: E731
        k3g()
        r["k3g_ms"] = float(np.median([window(k3g, args.reps) for _ in range(args.windows)]))
        r["k3g_tflops"] = 2.0 * 9 * kd * C * C * D * H * W / (r["k3g_ms"] * 1e-3) / 1e12
        r["k3g_peak_fraction"] = r["k3g_tflops"] / PEAK_TF
        r.update(C=C, kd=kd, D=D, H=H, W=W, gradients_rel_diff=agree)
        out["rows"][name] = r
        print(f"# {name}: hip {r['hip_ms']['median']:.3f} ms  aten {r['aten_ms']['median']:.3f} ms  peak {r['hip_peak_mb']:.0f} / "
              f"{r['aten_peak_mb']:.0f} MB  K3g {r['k3g_ms']:.3f} ms = {r['k3g_tflops']:.1f} TF  gradients differ by {agree:.1e}",
              file=sys.stderr, flush=True)
        del x, gy, gh, ga, hip, aten, gw
    from dmvsnet_amd import DiffConvTranspose2d, DiffConvTranspose3d
    for name, mode, Ca, kd, (D, H, W) in strided_rows():
        if want and not any(s in name for s in want):
            continue
        Cb = Ca // 2
        g = torch.Generator(device="cpu").manual_seed(Ca + kd + D + 1)
        cshape = (1, Ca, D, H, W) if kd == 3 else (1, Ca, H, W)
        fshape = (1, Cb, 2 * D, 2 * H, 2 * W) if kd == 3 else (1, Cb, 2 * H, 2 * W)
        xshape, yshape = (fshape, cshape) if mode == "conv" else (cshape, fshape)
        x = torch.randn(xshape, generator=g).to(dev).requires_grad_(True)
        gy = torch.randn(yshape, generator=g).to(dev)
        if mode == "conv":
            hip = (DiffConv3d if kd == 3 else DiffConv2d)(Cb, Ca, 3, stride=2, padding=1, bias=False).to(dev)
            aten = (nn.Conv3d if kd == 3 else nn.Conv2d)(Cb, Ca, 3, stride=2, padding=1, bias=False).to(dev)
        else:
            hip = (DiffConvTranspose3d if kd == 3 else DiffConvTranspose2d)(Ca, Cb, 3, stride=2, padding=1, output_padding=1, bias=False).to(dev)
            aten = (nn.ConvTranspose3d if kd == 3 else nn.ConvTranspose2d)(Ca, Cb, 3, stride=2, padding=1, output_padding=1, bias=False).to(dev)
        aten.load_state_dict(hip.state_dict())

        def arm(m):
            return lambda: torch.autograd.grad(m(x), [x, m.weight], gy)

        gh, ga = arm(hip)(), arm(aten)()
        agree = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(gh, ga))
        r = ab({"hip": arm(hip), "aten": arm(aten)}, args.reps, args.windows)
        coarse, fine = (gy, x.detach()) if mode == "conv" else (x.detach(), gy)
        c4, f4 = coarse.reshape(Ca, D, H, W), fine.reshape(Cb, 2 * D if kd == 3 else D, 2 * H, 2 * W)
        gw = torch.empty_like(hip.weight)
        k3h = lambda: ops.conv3d_wgrad_s2(c4, f4, kd, out=gw)   # noqa: E731
        k3h()
        r["k3g_ms"] = float(np.median([window(k3h, args.reps) for _ in range(args.windows)]))
        r["k3g_tflops"] = 2.0 * 9 * kd * Ca * Cb * D * H * W / (r["k3g_ms"] * 1e-3) / 1e12
        r["k3g_peak_fraction"] = r["k3g_tflops"] / PEAK_TF
        r.update(C=f"{Cb}->{Ca}" if mode == "conv" else f"{Ca}->{Cb}", kd=kd, D=D, H=H, W=W, gradients_rel_diff=agree, kernel="K3h")
        out["rows"][name] = r
        print(f"# {name}: hip {r['hip_ms']['median']:.3f} ms  aten {r['aten_ms']['median']:.3f} ms  peak {r['hip_peak_mb']:.0f} / "
              f"{r['aten_peak_mb']:.0f} MB  K3h {r['k3g_ms']:.3f} ms = {r['k3g_tflops']:.1f} TF  gradients differ by {agree:.1e}",
              file=sys.stderr, flush=True)
        del x, gy, gh, ga, hip, aten, gw
    for name, Cb, (Hf, Wf) in ROWS_K5S2:
        if want and not any(s in name for s in want):
            continue
        Ca, Hc, Wc = 2 * Cb, (Hf + 1) // 2, (Wf + 1) // 2
        g = torch.Generator(device="cpu").manual_seed(Ca + Hf)
        x = torch.randn((1, Cb, Hf, Wf), generator=g).to(dev).requires_grad_(True)
        gy = torch.randn((1, Ca, Hc, Wc), generator=g).to(dev)
        hip = DiffConv2d(Cb, Ca, 5, stride=2, padding=2, bias=False).to(dev)
        aten = nn.Conv2d(Cb, Ca, 5, stride=2, padding=2, bias=False).to(dev)
        aten.load_state_dict(hip.state_dict())

        def arm(m):
            return lambda: torch.autograd.grad(m(x), [x, m.weight], gy)

        gh, ga = arm(hip)(), arm(aten)()
        agree = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(gh, ga))
        r = ab({"hip": arm(hip), "aten": arm(aten)}, args.reps, args.windows)
        x4, gy4, w = x.detach().reshape(Cb, 1, Hf, Wf), gy.reshape(Ca, 1, Hc, Wc), hip.weight.detach()
        gw, gx = torch.empty_like(w), torch.empty_like(x4)
        k3k = lambda: ops.conv2d_k5s2_wgrad(x4, gy4, out=gw)             # noqa: E731
        k3d = lambda: ops.conv2d_k5s2_dgrad(gy4, w, (Hf, Wf), out=gx)    # noqa: E731
        k3k(), k3d()
        flop, floor_ms = 2.0 * 25 * Ca * Cb * Hc * Wc, 4.0 * (x4.numel() + gy4.numel() + w.numel()) / (HBM_TBS * 1e12) * 1e3
        r["k3g_ms"] = float(np.median([window(k3k, args.reps) for _ in range(args.windows)]))
        r["k3d_ms"] = float(np.median([window(k3d, args.reps) for _ in range(args.windows)]))
        r["k3g_tflops"], r["k3d_tflops"] = flop / (r["k3g_ms"] * 1e-3) / 1e12, flop / (r["k3d_ms"] * 1e-3) / 1e12
        r["k3g_peak_fraction"], r["k3d_peak_fraction"] = r["k3g_tflops"] / PEAK_TF, r["k3d_tflops"] / PEAK_TF
        r["k3g_hbm_fraction"], r["k3d_hbm_fraction"] = floor_ms / r["k3g_ms"], floor_ms / r["k3d_ms"]
        r.update(C=f"{Cb}->{Ca}", kd=1, D=1, H=Hc, W=Wc, gradients_rel_diff=agree, kernel="K3k")
        out["rows"][name] = r
        print(f"# {name}: hip {r['hip_ms']['median']:.3f} [{r['hip_ms']['min']:.3f}, {r['hip_ms']['max']:.3f}] ms  aten "
              f"{r['aten_ms']['median']:.3f} [{r['aten_ms']['min']:.3f}, {r['aten_ms']['max']:.3f}] ms  peak {r['hip_peak_mb']:.0f} / "
              f"{r['aten_peak_mb']:.0f} MB  K3k {r['k3g_ms']:.3f} ms = {r['k3g_tflops']:.2f} TF, {r['k3g_hbm_fraction']:.2f} of the HBM floor  "
              f"K3d {r['k3d_ms']:.3f} ms = {r['k3d_tflops']:.2f} TF, {r['k3d_hbm_fraction']:.2f} of the HBM floor  gradients differ by "
              f"{agree:.1e}", file=sys.stderr, flush=True)
        del x, gy, gh, ga, hip, aten, gw, gx
    print(json.dumps(out))
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(out))


def markdown(out):
    lines = ["# Regularisation and feature convolutions, forward + backward: K3 + K3g / K3h against ATen", "",
             f"`scripts/conv_train_bench.py` on {out['device']}, one process, arms alternating; median of {out['windows']} windows of "
             f"{out['reps']} repetitions, per sample (batch 1).  Times in ms, memory in MB (peak allocated over one forward + backward, "
             "above what was allocated before).  wgrad: the weight-gradient kernel alone (K3g; K3h on the stride-2 / transposed rows, "
             "whose C is in -> out and whose D x H x W is the coarse volume), its time and its fraction of the 157 TFLOP/s fp32 MFMA peak.", "",
             "| layer | C | kd | D x H x W | hip fwd+bwd | ATen fwd+bwd | ATen / hip | hip peak | ATen peak | wgrad | wgrad TFLOP/s | of 157 | gradients, max rel. diff |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, r in out["rows"].items():
        lines.append(f"| {name} | {r['C']} | {r['kd']} | {r['D']} x {r['H']} x {r['W']} | {r['hip_ms']['median']:.3f} | "
                     f"{r['aten_ms']['median']:.3f} | {r['aten_over_hip']:.2f} | {r['hip_peak_mb']:.0f} | {r['aten_peak_mb']:.0f} | "
                     f"{r['k3g_ms']:.3f} | {r['k3g_tflops']:.1f} | {r['k3g_peak_fraction']:.2f} | {r['gradients_rel_diff']:.1e} |")
    k5 = {n: r for n, r in out["rows"].items() if r.get("kernel") == "K3k"}
    if k5:
        lines += ["", "The 5x5 stride-2 rows: median [min, max] of both arms, and K3k / K3d alone (fraction of the 157 TFLOP/s fp32 MFMA peak; "
                  f"HBM floor = the bytes of the kernel's tensors at {HBM_TBS:.0f} TB/s over its time).", "",
                  "| layer | hip fwd+bwd | ATen fwd+bwd | K3k ms | K3k of 157 | K3k HBM floor / time | K3d ms | K3d of 157 | K3d HBM floor / time |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for name, r in k5.items():
            h, a = r["hip_ms"], r["aten_ms"]
            lines.append(f"| {name} | {h['median']:.3f} [{h['min']:.3f}, {h['max']:.3f}] | {a['median']:.3f} [{a['min']:.3f}, {a['max']:.3f}] | "
                         f"{r['k3g_ms']:.3f} | {r['k3g_peak_fraction']:.3f} | {r['k3g_hbm_fraction']:.2f} | {r['k3d_ms']:.3f} | "
                         f"{r['k3d_peak_fraction']:.3f} | {r['k3d_hbm_fraction']:.2f} |")
    lines.append("")
    return "\n".join(lines)


if __name__ == "__main__":
    main()
