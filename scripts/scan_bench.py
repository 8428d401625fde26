"""Scan-level eval throughput: the default ``eval_io.save_depth_maps`` (per-sample loader: V decodes + host resizes and a
FeatureNet pass over all V views per depth map) against ``feature_cache=True`` (every image decoded, ingested on the GPU and
encoded once per scan; ``MVSNet.forward_features`` per depth map).

A synthetic scene is written to a temporary directory: N JPEGs (synth images) at the source size, synth cameras and a
DTU-like pair.txt (the 10 nearest views along the camera path).  Both paths run with the same network and settings; their output files must
be byte-equal.  Prints one JSON line: maps, wall seconds and maps/s per path, the cached path's phase split (decode,
h2d_ingest, encode, forward, d2h, write -- device phases from events, host phases summed over threads, so they overlap),
encodes vs distinct images, peak cache bytes, and the GPU-only ms per map of forward vs forward_features (events, after a
warm-up, the two arms alternated call by call).

    python scripts/scan_bench.py                       # DTU recipe: 49 x 1600x1200 -> 864x1152, 5 views, 48/32/8, inverse
    python scripts/scan_bench.py --src 1184 1600 --max 1184 1600 --ndepths 64 32 8 --ratios 3 2 1 --linear   # config 2
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dmvsnet_amd import MVSNet, eval_io, synth  # noqa: E402


def write_scene(root, scan, n, H, W, neighbours=10):
    from PIL import Image
    os.makedirs(os.path.join(root, scan, "cams"))
    os.makedirs(os.path.join(root, scan, "images"))
    cams = synth.synth_cameras(H, W, n)["stage3"][0].numpy()
    for v in range(n):
        img = synth.synth_images(H, W, 1, seed=v)[0, 0]
        Image.fromarray((img.permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(
            os.path.join(root, scan, "images", f"{v:08d}.jpg"), quality=95)
        with open(os.path.join(root, scan, "cams", f"{v:08d}_cam.txt"), "w") as f:
            f.write("extrinsic\n")
            for r in range(4):
                f.write(" ".join(repr(float(x)) for x in cams[v, 0, r]) + "\n")
            f.write("\nintrinsic\n")
            for r in range(3):
                f.write(" ".join(repr(float(x)) for x in cams[v, 1, r, :3]) + "\n")
            f.write("\n425.0 2.5\n")
    k = min(neighbours, n - 1)
    with open(os.path.join(root, scan, "pair.txt"), "w") as f:
        f.write(f"{n}\n")
        for v in range(n):
            srcs = sorted((u for u in range(n) if u != v), key=lambda u: (abs(u - v), u))[:k]
            f.write(f"{v}\n{k} " + " ".join(f"{u} {100.0 - i}" for i, u in enumerate(srcs)) + "\n")


def files(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--images", type=int, default=49)
    ap.add_argument("--src", type=int, nargs=2, default=[1200, 1600], metavar=("H", "W"))
    ap.add_argument("--max", type=int, nargs=2, default=[864, 1152], metavar=("H", "W"))
    ap.add_argument("--views", type=int, default=5)
    ap.add_argument("--ndepths", type=int, nargs="+", default=[48, 32, 8])
    ap.add_argument("--ratios", type=float, nargs="+", default=[4, 2, 1])
    ap.add_argument("--linear", action="store_true", help="linear depth sampling (default: --inverse_depth, the DTU recipe)")
    ap.add_argument("--reps", type=int, default=20, help="timed calls per arm of the GPU-only comparison")
    ap.add_argument("--tag", default="dtu")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scan_bench.py needs the MI355X")
    inverse = not args.linear
    net = MVSNet(args.ndepths, args.ratios, inverse_depth=inverse, verbose=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed=0))
    net = net.cuda()
    net.return_prob_volume = False
    kw = dict(numdepth=192, inverse_depth=inverse)
    res = dict(tag=args.tag, images=args.images, src=args.src, size_max=args.max, views=args.views, ndepths=args.ndepths,
               inverse_depth=inverse)
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "data")
        t0 = time.perf_counter()
        write_scene(data, "warm", 4, *args.src)
        write_scene(data, "scan1", args.images, *args.src)
        res["scene_write_s"] = round(time.perf_counter() - t0, 2)
        # warm-up of both paths (code objects, K1 autotune, allocator) on a small scene of the same size
        eval_io.save_depth_maps(net, data, ["warm"], os.path.join(tmp, "w0"), args.views, *args.max, **kw)
        eval_io.save_depth_maps(net, data, ["warm"], os.path.join(tmp, "w1"), args.views, *args.max, feature_cache=True, **kw)
        torch.cuda.synchronize()
        walls, stats = {}, {}
        for name, fc in (("default", None), ("cached", True)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = eval_io.save_depth_maps(net, data, ["scan1"], os.path.join(tmp, name), args.views, *args.max,
                                          feature_cache=fc, stats=stats if fc else None, **kw)
            torch.cuda.synchronize()
            walls[name] = time.perf_counter() - t0
            res["maps"] = len(out)
        fa, fb = files(os.path.join(tmp, "default")), files(os.path.join(tmp, "cached"))
        res["files_equal"] = sorted(fa) == sorted(fb) and all(fa[k] == fb[k] for k in fa)
        res["files"] = len(fa)
        for name in walls:
            res[f"{name}_wall_s"] = round(walls[name], 3)
            res[f"{name}_maps_per_s"] = round(res["maps"] / walls[name], 3)
        res["wall_speedup"] = round(walls["default"] / walls["cached"], 3)
        res["phases_s"] = {k: round(v, 3) for k, v in stats["phases_s"].items()}
        for k in ("encodes", "images", "hits", "misses", "evictions", "peak_bytes", "budget"):
            res[k] = stats[k]

        # GPU-only per map: forward (FeatureNet over all V views) vs forward_features (cached views), alternated
        ds = eval_io.MVSDataset(data, ["scan1"], "test", args.views, 192, 1.06, inverse_depth=inverse,
                                max_h=args.max[0], max_w=args.max[1])
        s = ds[0]
        imgs = torch.from_numpy(s["imgs"])[None].cuda()
        proj = {k: torch.from_numpy(v)[None].cuda() for k, v in s["proj_matrices"].items()}
        dv = torch.from_numpy(s["depth_values"])[None].cuda()
        views = net.encode_views(imgs[0])
        ms = {"forward": [], "forward_features": [], "encode_per_image": []}
        arms = (("forward", lambda: net(imgs, proj, dv)), ("forward_features", lambda: net.forward_features(views, proj, dv)),
                ("encode_per_image", lambda: net.encode_views(imgs[0])))
        for _ in range(3):
            for _, fn in arms:
                fn()
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for name, fn in arms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / (imgs.shape[1] if name == "encode_per_image" else 1))
        for name, v in ms.items():
            res[f"gpu_ms_{name}"] = round(statistics.median(v), 4)
        amort = res["gpu_ms_forward_features"] + res["gpu_ms_encode_per_image"] * res["encodes"] / res["maps"]
        res["gpu_ms_cached_per_map_amortised"] = round(amort, 4)
        res["gpu_only_speedup"] = round(res["gpu_ms_forward"] / amort, 4)
    print(json.dumps(res))
    return 0 if res["files_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
