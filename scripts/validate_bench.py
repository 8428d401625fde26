#!/usr/bin/env python
"""Time validation mode (dmvsnet_amd.validate, N6) on the MI355X and compare it with the same arithmetic as ATen ops.

One JSON line.  Per size (512 x 640: the validation size; 1184 x 1600: the eval size), all three stages (1/4, 1/2, full):
  fused_ms        the loss pass (three dmvs_dual_depth_loss calls = six launches, the last with the metrics), device events
                  around --reps back-to-back passes after warm-up, per pass; min / median / max over the windows
  aten_ms         tests/validate_ref.py::mvs_loss_ref + metrics on the same device tensors: the reference's op classes
                  (boolean-index selection, elementwise ops, reductions; the host synchronisations boolean indexing implies
                  included, as in the reference), timed in the same run, windows alternating with the fused ones
  bytes           the planes the pass must read: (8 + 2 [+ 1]) * h * w * 4 per stage; over fused time = achieved bytes / s,
                  against the 6.29 TB/s a float4 copy reaches from HBM on this GPU
  equal           fused total against the restatement on the device, relative difference
and ``run_validate`` on synth.synth_val_scene (6 maps: 3 views x 2 lights, 512 x 640, 3 views per sample): maps / s and the
phase split, default path and feature cache.  Kernel times by name come from a separate run under
``rocprofv3 --kernel-trace --stats -- python scripts/validate_bench.py --no-aten --no-run-validate``.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HBM_COPY_BPS = 6.29e12   # measured float4 copy rate of the MI355X (8.0 TB/s spec)
DLOSSW = (0.5, 1.0, 2.0)


def spread(ts):
    return dict(min=min(ts), median=float(np.median(ts)), max=max(ts), n=len(ts))


def stage_planes(H, W, B, dev):
    import validate_ref as ref
    inputs, gts, masks, depth = {}, {}, {}, None
    for s, div in enumerate((4, 2, 1)):
        h, w = H // div, W // div
        per = [ref.synth_planes(h, w, 3, (0.3, 3.0)[b % 2], f"bench.{b}") + (ref.ragged_mask(h, w, 3 + b),) for b in range(B)]
        key = "stage{}".format(s + 1)
        gts[key] = torch.from_numpy(np.stack([p[0] for p in per])).to(dev)
        masks[key] = torch.from_numpy(np.stack([p[4] for p in per])).to(dev)
        inputs[key] = {"depth_sub_plus": torch.from_numpy(np.stack([p[1] for p in per])).to(dev),
                       "depth_sub_plus_refine": torch.from_numpy(np.stack([p[2] for p in per])).to(dev)}
        depth = torch.from_numpy(np.stack([p[3] for p in per])).to(dev)
    return inputs, gts, masks, depth


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=200, help="fused passes per timed window")
    ap.add_argument("--aten-reps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--no-aten", action="store_true")
    ap.add_argument("--no-run-validate", action="store_true")
    args = ap.parse_args()

    from dmvsnet_amd import MVSNet, synth, validate
    import validate_ref as ref
    assert torch.cuda.is_available(), "the benchmark needs the MI355X"
    dev = torch.device("cuda:0")
    out = dict(bench="validate", device=torch.cuda.get_device_name(0), batch=args.batch, sizes={})
    for H, W in ((512, 640), (1184, 1600)):
        inputs, gts, masks, depth = stage_planes(H, W, args.batch, dev)
        buf = torch.zeros(5, dtype=torch.float32, device=dev)

        def fused():
            buf.zero_()
            validate._loss_into(buf[0:1], inputs, gts, masks, {"dlossw": list(DLOSSW)}, depth=depth, depth_key="stage3",
                                metrics4=buf[1:5])

        def aten():
            loss = ref.mvs_loss_ref(inputs, gts, masks, DLOSSW, device=dev)
            return loss, ref.metrics_ref(depth, gts["stage3"], masks["stage3"])

        for _ in range(3):
            fused()
        torch.cuda.synchronize()
        f_ms, a_ms = [], []
        want = None
        if not args.no_aten:
            want, _ = aten()
            torch.cuda.synchronize()
        for _ in range(args.windows):
            f_ms.append(window(fused, args.reps))
            if not args.no_aten:
                a_ms.append(window(aten, args.aten_reps))
        nbytes = sum((8 + 2 + (1 if d == 1 else 0)) * (H // d) * (W // d) * 4 * args.batch for d in (4, 2, 1))
        fused()
        got = buf[0].item()
        r = dict(fused_ms=spread(f_ms), launches=6, bytes=nbytes, fused_bytes_per_s=nbytes / (np.median(f_ms) * 1e-3),
                 share_of_hbm_copy_rate=nbytes / (np.median(f_ms) * 1e-3) / HBM_COPY_BPS,
                 hbm_floor_ms=nbytes / HBM_COPY_BPS * 1e3, loss=got)
        if not args.no_aten:
            r.update(aten_ms=spread(a_ms), aten_over_fused=float(np.median(a_ms) / np.median(f_ms)),
                     rel_diff_vs_restatement=abs(got - want.item()) / abs(want.item()))
        out["sizes"][f"{H}x{W}"] = r

    if not args.no_run_validate:
        with tempfile.TemporaryDirectory() as root:
            info = synth.synth_val_scene(root, seed=0)
            net = MVSNet([48, 32, 8], [4, 2, 1], verbose=False)
            net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=0))
            net = net.to(dev)
            net.return_prob_volume = False
            runs = {}
            for name, cache in (("default", False), ("feature_cache", True)):
                for _ in range(2):   # the first run warms every shape up
                    stats = {}
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    scalars = validate.run_validate(net, root, info["listfile"], nviews=3, dlossw=DLOSSW, lights=info["lights"],
                                                    feature_cache=cache, stats=stats)
                    torch.cuda.synchronize()
                    wall = time.perf_counter() - t0
                runs[name] = dict(maps=stats["maps"], wall_s=wall, maps_per_s=stats["maps"] / wall, phases_s=stats["phases_s"],
                                  scalars=scalars, **({k: stats[k] for k in ("images", "encodes", "hits", "misses")} if cache else {}))
            out["run_validate"] = dict(scene="synth_val_scene: 1 scan, 3 views x 2 lights, 512x640, nviews 3, ndepths 48/32/8", **runs)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
