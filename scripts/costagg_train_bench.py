#!/usr/bin/env python
"""Time forward + backward of the differentiable cost aggregation (dmvsnet_amd.cost_agg: K1 + K1b) against the same operator
as ATen ops with grid_sample, for the six cost-aggregation passes of a training step, per sample (batch 1).

Recipes: DTU training (512 x 640, 5 views, 48 / 32 / 8 planes + three 4-plane refine passes; scripts/train.sh) and BlendedMVS
fine-tuning (576 x 768, 7 views; scripts/blendedmvs_finetune.sh).  Both arms run in one process on one GPU, on the same
tensors; every arm is warmed, and the timed windows alternate with the order swapped every round (the K1 run-order lesson,
DESIGN.md section 7 item 5).  Per pass and arm:
  ms               forward + backward (gradients to every feature map), device events around --reps repetitions, per
                   repetition; min / median / max over the windows
  peak_mb          torch.cuda.max_memory_allocated over one forward + backward, minus what was allocated before it
and for the fused arm alone the two backward kernels apart (bwd_ref_ms, bwd_src_ms: dmvs_warp_corr_backward with one output
switched off), with the atomic payload of the source-gradient kernel (4 taps * C * 4 B per sample, all samples counted, as
the sizing in docs/kernels/K1b_warp_corr_backward.md does) over its time; for the ATen arm grid_sample's backward alone
(aten_grid_bwd_ms, all source views).  One JSON line; --md writes the table of profiles/costagg_train.md.

--deterministic adds a third arm, cost_agg(..., deterministic=True) (K1b's fixed-point source gradients,
csrc/warp_corr_bwd_det.h), to the same alternating windows, and for it: det_bwd_src_ms (dmvs_warp_corr_backward_det with the
reference gradient switched off: clear + pre-pass + scatter + finalize), its workspace bytes, the added bytes of its 8-byte integer
atomics (4 taps * C * 8 B per sample) over the scatter kernel's time, and the four steps apart -- from the device times of
torch.profiler where it records them (det_parts_ms: clear, prepass, scatter, finalize), and always by difference
(det_bwd_src_zero_gsim_ms: the same launch on gsim = 0, where the scatter exits at once, and det_clear_ms: a memset of the workspace).

--presum (implies --deterministic) adds a fourth and a fifth arm, cost_agg(..., presum=True) in the atomic and in the deterministic mode
(csrc/warp_corr_bwd_presum.h: the scatter pre-summed in LDS windows), to the same alternating windows, and per pass the four source-
gradient launches alone in alternating windows of their own (presum_src_ms: atomic, presum, det, presum_det; the reference gradient
switched off), with the share of workgroups that took the window, fell back to global adds per tap or had no tap inside
(presum_paths, from the entry's path_counts in one extra launch per sink outside every timed window).
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

RECIPES = {"dtu_512x640_5v": (512, 640, 5), "blendedmvs_576x768_7v": (576, 768, 7)}
PASSES = (("s1.main", 32, 48, 4), ("s1.refine", 32, 4, 4), ("s2.main", 16, 32, 2), ("s2.refine", 16, 4, 2),
          ("s3.main", 8, 8, 1), ("s3.refine", 8, 4, 1))   # name, C, D, image size divisor


def aten_grid(pairs, v, depth):
    """The reference's sampling grid of source view v (module.py:222-243), built without a graph."""
    with torch.no_grad():
        B, D, H, W = depth.shape
        comp = lambda p: torch.cat((p[:, 1, :3, :3] @ p[:, 0, :3, :4], p[:, 0, 3:]), 1)   # noqa: E731
        P = comp(pairs[:, v]) @ torch.inverse(comp(pairs[:, 0]))
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=depth.device),
                                torch.arange(W, dtype=torch.float32, device=depth.device), indexing="ij")
        xyz = torch.stack((xx.reshape(-1), yy.reshape(-1), torch.ones_like(xx.reshape(-1))))
        pts = (P[:, :3, :3] @ xyz).unsqueeze(2) * depth.view(B, 1, D, H * W) + P[:, :3, 3].view(B, 3, 1, 1)
        z = torch.where(pts[:, 2] == 0, pts[:, 2] + 1e-5, pts[:, 2])
        return torch.stack((pts[:, 0] / z / ((W - 1) / 2) - 1, pts[:, 1] / z / ((H - 1) / 2) - 1), 3).view(B, D * H, W, 2)


def aten_cost_agg(feats, pairs, depth):
    """CostAgg.forward in train mode (mvsnet.py:111-153): one warped volume and one grid per source view stay alive."""
    B, C, H, W = feats[0].shape
    D = depth.shape[1]
    total = 0
    for v in range(1, len(feats)):
        warped = F.grid_sample(feats[v], aten_grid(pairs, v, depth), mode="bilinear", padding_mode="zeros", align_corners=True)
        total = total + (warped.view(B, C // 2, 2, D, H, W) * feats[0].view(B, C // 2, 2, 1, H, W)).mean(1)
    return total


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--recipes", default=",".join(RECIPES))
    ap.add_argument("--md", default=None, help="also write the result table (markdown) to this file")
    ap.add_argument("--deterministic", action="store_true", help="add the deterministic arm (fixed-point dSrc) beside the others")
    ap.add_argument("--presum", action="store_true", help="add the two pre-summed arms (atomic and deterministic); implies --deterministic")
    args = ap.parse_args()
    args.deterministic = args.deterministic or args.presum

    from dmvsnet_amd import cost_agg, ops, synth
    assert torch.cuda.is_available(), "the benchmark needs the MI355X"
    dev = torch.device("cuda:0")
    out = dict(bench="costagg_train", device=torch.cuda.get_device_name(0), reps=args.reps, windows=args.windows,
               deterministic=args.deterministic, presum=args.presum, recipes={})
    for recipe in args.recipes.split(","):
        Hf, Wf, V = RECIPES[recipe]
        cams = synth.synth_cameras(Hf, Wf, V)
        rows = {}
        for ipass, (name, C, D, div) in enumerate(PASSES):
            H, W = Hf // div, Wf // div
            g = torch.Generator(device="cpu").manual_seed(100 * V + ipass)
            feats = [torch.randn(1, C, H, W, generator=g).to(dev).requires_grad_(True) for _ in range(V)]
            pairs = cams["stage{}".format({4: 1, 2: 2, 1: 3}[div])].to(dev)
            # main passes: planes across the depth range; refine passes: 4 planes around a smooth prior
            step = (240.0 / D) if D > 4 else 2.65 * div
            depth = (560.0 + step * torch.arange(D, dtype=torch.float32).view(1, D, 1, 1) + 5.0 * torch.randn(1, D, H, W, generator=g)).to(dev)
            gsim = torch.randn(1, 2, D, H, W, generator=g).to(dev)

            def fused():
                torch.autograd.grad(cost_agg(feats, pairs, depth), feats, gsim)

            def aten():
                torch.autograd.grad(aten_cost_agg(feats, pairs, depth), feats, gsim)

            def det():
                torch.autograd.grad(cost_agg(feats, pairs, depth, deterministic=True), feats, gsim)

            def presum():
                torch.autograd.grad(cost_agg(feats, pairs, depth, deterministic=False, presum=True), feats, gsim)

            def presum_det():
                torch.autograd.grad(cost_agg(feats, pairs, depth, deterministic=True, presum=True), feats, gsim)

            arms = {"fused": fused, "aten": aten}
            if args.deterministic:
                arms["det"] = det
            if args.presum:
                arms.update(presum=presum, presum_det=presum_det)
            for fn in arms.values():
                fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in arms}
            for w in range(args.windows):
                for k in (list(arms) if w % 2 == 0 else list(arms)[::-1]):
                    ms[k].append(window(arms[k], args.reps))
            r = {k + "_ms": spread(v) for k, v in ms.items()}
            r.update({k + "_peak_mb": peak_mb(fn) for k, fn in arms.items()})
            r["aten_over_fused"] = r["aten_ms"]["median"] / r["fused_ms"]["median"]
            if args.deterministic:
                r["det_over_fused"] = r["det_ms"]["median"] / r["fused_ms"]["median"]

            # the fused arm's kernels apart
            with torch.no_grad():
                q4 = [ops.nchw_to_q4(f[0]) for f in feats]
                proj12 = ops.relative_proj(pairs[0].contiguous())
                gref = torch.empty((C, H, W), device=dev)
                gsrc = [torch.zeros((C, H, W), device=dev) for _ in range(V - 1)]
                none = [None] * (V - 1)
                parts = {"fwd_ms": lambda: ops.warp_corr(q4[0], q4[1:], proj12, depth[0], layout="q4"),
                         "bwd_ref_ms": lambda: ops.warp_corr_backward(q4[0], q4[1:], proj12, depth[0], gsim[0], gref, none),
                         "bwd_src_ms": lambda: ops.warp_corr_backward(q4[0], q4[1:], proj12, depth[0], gsim[0], None, gsrc)}
                for k, fn in parts.items():
                    fn()
                    r[k] = float(np.median([window(fn, args.reps) for _ in range(args.windows)]))
                if args.deterministic:
                    r.update(det_parts(ops, q4, proj12, depth[0], gsim[0], V, C, H, W, args))
                if args.presum:
                    r.update(presum_parts(ops, q4, proj12, depth[0], gsim[0], V, C, H, W, args))
            payload = (V - 1) * D * H * W * 4 * C * 4
            r["bwd_src_atomic_bytes"] = payload
            r["bwd_src_atomic_tb_per_s"] = payload / (r["bwd_src_ms"] * 1e-3) / 1e12
            if args.deterministic:
                # the scatter alone: the profiler's kernel time, else the difference to the launch whose scatter exits at once
                scatter = (r["det_parts_ms"] or {}).get("scatter") or (r["det_bwd_src_ms"]["median"] - r["det_bwd_src_zero_gsim_ms"])
                r["det_scatter_ms"] = scatter
                r["det_atomic_bytes"] = 2 * payload
                r["det_atomic_tb_per_s"] = 2 * payload / (scatter * 1e-3) / 1e12
                r["det_src_over_atomic_src"] = r["det_bwd_src_ms"]["median"] / r["bwd_src_ms"]
            # ATen's grid_sample backward alone (all source views)
            grids = [aten_grid(pairs, v, depth) for v in range(1, V)]
            warped = [F.grid_sample(feats[v], grids[v - 1], mode="bilinear", padding_mode="zeros", align_corners=True) for v in range(1, V)]
            gw = torch.randn_like(warped[0])

            def grid_bwd():
                for v in range(1, V):
                    torch.autograd.grad(warped[v - 1], feats[v], gw, retain_graph=True)
            grid_bwd()
            r["aten_grid_bwd_ms"] = float(np.median([window(grid_bwd, args.reps) for _ in range(args.windows)]))
            r["activation_estimate_mb"] = (V - 1) * (C + 2) * D * H * W * 4 / 2 ** 20   # the issue's arithmetic: warped + grid per view
            del warped, gw, grids, gref, gsrc, q4
            rows[name] = dict(C=C, D=D, H=H, W=W, **r)
            print(f"# {recipe} {name}: fused {r['fused_ms']['median']:.3f} ms  aten {r['aten_ms']['median']:.3f} ms  "
                  f"peak {r['fused_peak_mb']:.0f} / {r['aten_peak_mb']:.0f} MB", file=sys.stderr, flush=True)
        tot = {k: sum(rw[k]["median"] for rw in rows.values()) for k in ("fused_ms", "aten_ms") + (("det_ms",) if args.deterministic else ())}
        if args.deterministic:
            tot.update({k: sum(rw[k] for rw in rows.values()) for k in ("det_scatter_ms", "det_workspace_bytes", "det_atomic_bytes")})
            tot["det_bwd_src_ms"] = sum(rw["det_bwd_src_ms"]["median"] for rw in rows.values())
        if args.presum:
            tot.update({k: sum(rw[k]["median"] for rw in rows.values()) for k in ("presum_ms", "presum_det_ms")})
            tot["presum_src_ms"] = {arm: {q: sum(rw["presum_src_ms"][arm][q] for rw in rows.values()) for q in ("min", "median", "max")}
                                    for arm in PRESUM_ARMS}
        tot.update({k: sum(rw[k] for rw in rows.values()) for k in ("bwd_src_ms", "bwd_ref_ms", "fwd_ms", "aten_grid_bwd_ms", "bwd_src_atomic_bytes")})
        out["recipes"][recipe] = dict(views=V, passes=rows, per_sample=tot)
    print(json.dumps(out))
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(out))


def det_parts(ops, q4, proj12, depth, gsim, V, C, H, W, args):
    """The deterministic source-gradient launch alone and its steps apart (see the module docstring)."""
    dev = depth.device
    none = [None] * (V - 1)
    gsrc = [torch.empty((C, H, W), device=dev) for _ in range(V - 1)]
    nbytes = ops.warp_corr_backward_det_workspace(C, H, W, V - 1)
    ws = torch.empty((nbytes // 8,), dtype=torch.int64, device=dev)
    zero = torch.zeros_like(gsim)
    run = lambda g=gsim: ops.warp_corr_backward_det(q4[0], q4[1:], proj12, depth, g, None, gsrc, workspace=ws)   # noqa: E731
    run()
    r = dict(det_workspace_bytes=nbytes, det_bwd_src_ms=spread([window(run, args.reps) for _ in range(args.windows)]))
    r["det_bwd_src_zero_gsim_ms"] = float(np.median([window(lambda: run(zero), args.reps) for _ in range(args.windows)]))
    r["det_clear_ms"] = float(np.median([window(ws.zero_, args.reps) for _ in range(args.windows)]))
    parts = None
    try:   # device times per kernel; None where the profiler records no device activity
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(args.reps):
                run()
            torch.cuda.synchronize()
        # the scatter is warp_corr_bwd_src_kernel<..., FixedSink>: the sink's name is in the mangled and in the demangled form
        keys = {"prepass": "det_absmax", "scatter": "FixedSink", "finalize": "det_finalize", "clear": "emset"}
        acc = {k: 0.0 for k in keys}
        for ev in prof.key_averages():
            t = getattr(ev, "device_time_total", None)
            t = getattr(ev, "cuda_time_total", 0.0) if t is None else t
            for k, pat in keys.items():
                if pat in ev.key or (k == "clear" and "fillBuffer" in ev.key):
                    acc[k] += t / 1e3 / args.reps
        parts = acc if acc["scatter"] > 0 else None
    except Exception as e:   # the break-out is optional; the arm's times above are not
        print(f"# torch.profiler break-out not available: {e!r}", file=sys.stderr)
    r["det_parts_ms"] = parts
    del gsrc, ws
    return r


PRESUM_ARMS = ("atomic", "presum", "det", "presum_det")


def presum_parts(ops, q4, proj12, depth, gsim, V, C, H, W, args):
    """The four source-gradient launches alone (reference gradient off), windows alternating, and the paths the pre-summed
    scatter's workgroups took (one extra launch per sink, outside the timed windows)."""
    dev = depth.device
    gsrc = [torch.zeros((C, H, W), device=dev) for _ in range(V - 1)]
    ws = torch.empty((ops.warp_corr_backward_det_workspace(C, H, W, V - 1) // 8,), dtype=torch.int64, device=dev)
    head = (q4[0], q4[1:], proj12, depth, gsim, None, gsrc)
    runs = {"atomic": lambda: ops.warp_corr_backward(*head),
            "presum": lambda: ops.warp_corr_backward_presum(*head),
            "det": lambda: ops.warp_corr_backward_det(*head, workspace=ws),
            "presum_det": lambda: ops.warp_corr_backward_presum(*head, deterministic=True, workspace=ws)}
    for fn in runs.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for w in range(args.windows):
        for k in (list(runs) if w % 2 == 0 else list(runs)[::-1]):
            ms[k].append(window(runs[k], args.reps))
    r = dict(presum_src_ms={k: spread(v) for k, v in ms.items()}, presum_paths={}, presum_cap={})
    for key, det in (("presum", False), ("presum_det", True)):
        counts = torch.zeros((3,), dtype=torch.int32, device=dev)
        ops.warp_corr_backward_presum(*head, deterministic=det, workspace=ws if det else None, path_counts=counts)
        torch.cuda.synchronize()
        r["presum_paths"][key] = dict(zip(("windowed", "direct", "empty"), counts.tolist()))
        r["presum_cap"][key] = ops.warp_corr_backward_presum_cap(C, det)
    del gsrc, ws
    return r


def markdown(out):
    lines = ["# Cost aggregation, forward + backward: fused (K1 + K1b) against ATen grid_sample", "",
             f"`scripts/costagg_train_bench.py` on {out['device']}, one process, arms alternating; median of {out['windows']} windows of "
             f"{out['reps']} repetitions, per sample (batch 1).  Times in ms, memory in MB (peak allocated over one forward + "
             "backward, above what was allocated before).", ""]
    for recipe, r in out["recipes"].items():
        lines += [f"## {recipe} ({r['views']} views)", "",
                  "| pass | C | D | H x W | fused fwd+bwd | ATen fwd+bwd | ATen / fused | K1 fwd | dRef kernel | dSrc kernel | ATen grid_sample bwd | dSrc atomics TB/s | fused peak | ATen peak |",
                  "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for name, p in r["passes"].items():
            lines.append(f"| {name} | {p['C']} | {p['D']} | {p['H']} x {p['W']} | {p['fused_ms']['median']:.3f} | {p['aten_ms']['median']:.3f} | "
                         f"{p['aten_over_fused']:.2f} | {p['fwd_ms']:.3f} | {p['bwd_ref_ms']:.3f} | {p['bwd_src_ms']:.3f} | {p['aten_grid_bwd_ms']:.3f} | "
                         f"{p['bwd_src_atomic_tb_per_s']:.2f} | {p['fused_peak_mb']:.0f} | {p['aten_peak_mb']:.0f} |")
        if out.get("deterministic"):
            lines += ["", "Deterministic mode (`cost_agg(..., deterministic=True)`: fixed-point dSrc) against the atomic arm, same windows; min / "
                          "median / max over the windows:", "",
                      "| pass | fused fwd+bwd | deterministic fwd+bwd | det / fused | dSrc atomic | dSrc deterministic | det / atomic | clear | pre-pass | "
                      "scatter | finalize | scatter 8-byte atomics TB/s | workspace MB |",
                      "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
            sp = lambda x: f"{x['min']:.3f} / {x['median']:.3f} / {x['max']:.3f}"   # noqa: E731
            for name, p in r["passes"].items():
                parts = p["det_parts_ms"]
                cells = [f"{parts[k]:.3f}" for k in ("clear", "prepass", "scatter", "finalize")] if parts else \
                        [f"{p['det_clear_ms']:.3f} (memset alone)", "n/a", f"{p['det_scatter_ms']:.3f} (by difference)", "n/a"]
                lines.append(f"| {name} | {sp(p['fused_ms'])} | {sp(p['det_ms'])} | {p['det_over_fused']:.2f} | {p['bwd_src_ms']:.3f} | "
                             f"{sp(p['det_bwd_src_ms'])} | {p['det_src_over_atomic_src']:.2f} | {' | '.join(cells)} | "
                             f"{p['det_atomic_tb_per_s']:.2f} | {p['det_workspace_bytes'] / 2 ** 20:.1f} |")
            t = r["per_sample"]
            lines += ["", f"Per sample: deterministic {t['det_ms']:.2f} ms against fused {t['fused_ms']:.2f} ms ({t['det_ms'] / t['fused_ms']:.2f}x); "
                          f"deterministic dSrc launches {t['det_bwd_src_ms']:.2f} ms against {t['bwd_src_ms']:.2f} ms atomic "
                          f"({t['det_bwd_src_ms'] / t['bwd_src_ms']:.2f}x); scatter kernels {t['det_scatter_ms']:.2f} ms for "
                          f"{t['det_atomic_bytes'] / 1e9:.2f} GB of 8-byte integer atomics "
                          f"({t['det_atomic_bytes'] / 1e9 / t['det_scatter_ms']:.2f} TB/s)."]
        if out.get("presum"):
            sp = lambda x: f"{x['median']:.3f} ({x['min']:.3f} - {x['max']:.3f})"   # noqa: E731
            share = lambda c: f"{100.0 * c['windowed'] / max(1, sum(c.values())):.1f} / {100.0 * c['direct'] / max(1, sum(c.values())):.1f} / " \
                              f"{100.0 * c['empty'] / max(1, sum(c.values())):.1f}"   # noqa: E731
            lines += ["", "Pre-summed scatter (`cost_agg(..., presum=True)`: the scatter's adds summed in LDS windows first) against the plain "
                          "scatter of the same mode.  The source-gradient launches alone, four arms alternating in windows of their own, "
                          "median (min - max); paths: % of workgroups windowed / direct (box above the capacity) / empty:", "",
                      "| pass | dSrc atomic | dSrc presum | presum / atomic | paths (cap " + str(next(iter(r['passes'].values()))['presum_cap']['presum']) +
                      ") | dSrc deterministic | dSrc presum det | presum / det | paths (cap " +
                      str(next(iter(r['passes'].values()))['presum_cap']['presum_det']) + ") | fused fwd+bwd | presum fwd+bwd | det fwd+bwd | presum det fwd+bwd |",
                      "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
            for name, p in r["passes"].items():
                m, c = p["presum_src_ms"], p["presum_paths"]
                lines.append(f"| {name} | {sp(m['atomic'])} | {sp(m['presum'])} | {m['presum']['median'] / m['atomic']['median']:.2f} | {share(c['presum'])} | "
                             f"{sp(m['det'])} | {sp(m['presum_det'])} | {m['presum_det']['median'] / m['det']['median']:.2f} | {share(c['presum_det'])} | "
                             f"{sp(p['fused_ms'])} | {sp(p['presum_ms'])} | {sp(p['det_ms'])} | {sp(p['presum_det_ms'])} |")
            t = r["per_sample"]
            m = t["presum_src_ms"]
            lines += ["", "Per sample, dSrc launches summed over the passes, median (sum of minima - sum of maxima): " +
                      "; ".join(f"{k} {sp(m[k])} ms" for k in PRESUM_ARMS) +
                      f".  Forward + backward: fused {t['fused_ms']:.2f}, presum {t['presum_ms']:.2f}, deterministic {t['det_ms']:.2f}, "
                      f"presum deterministic {t['presum_det_ms']:.2f} ms."]
        t = r["per_sample"]
        lines += ["", f"Per sample: fused {t['fused_ms']:.2f} ms, ATen {t['aten_ms']:.2f} ms ({t['aten_ms'] / t['fused_ms']:.2f}x); "
                      f"dSrc kernels {t['bwd_src_ms']:.2f} ms for {t['bwd_src_atomic_bytes'] / 1e9:.2f} GB of atomic payload, "
                      f"dRef kernels {t['bwd_ref_ms']:.2f} ms, ATen grid_sample backward {t['aten_grid_bwd_ms']:.2f} ms.", ""]
    return "\n".join(lines)


if __name__ == "__main__":
    main()
