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

``--fusion pcd|dypcd`` adds step 2 of Model.test (the fusion filter) under the key "fusion":
  (a) fusion alone on ``synth.synth_fusion_scene`` (864x1152 for pcd, 1056x2048 for dypcd; --images views, the 10 nearest
      views as sources): ``fusion.fuse_scene`` on the files against ``fusion.ScanFusion`` on device maps -- wall time of
      each, GPU ms per view from events (per-pair launches + finish vs the fused kernels), the host split (mask PNGs, JPEG
      decode, PLY, D2H) and how speckled the masks are;
  (b) end to end on the scan above: ``run_test(feature_cache=True)`` against ``run_test(feature_cache=True,
      resident_fusion=True)`` -- wall, maps/s, files_equal (mask PNGs compared as pixels, xyz within 1 ulp).
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


def _same_run_outputs(a, b):
    """run_test output folders: every file byte-equal except mask PNGs (same pixels) and the PLY (header, count and colours
    equal, xyz within 1 ulp or fp64 rounding of the point's scale).  -> (equal, xyz values that differ)."""
    import io
    from PIL import Image
    fa, fb = files(a), files(b)
    if sorted(fa) != sorted(fb):
        return False, None
    ndiff = 0
    for k in fa:
        if k.endswith(".png"):
            if not np.array_equal(np.array(Image.open(io.BytesIO(fa[k]))), np.array(Image.open(io.BytesIO(fb[k])))):
                return False, None
        elif k.endswith(".ply"):
            (ha, ba), (hb, bb) = fa[k].split(b"end_header\n"), fb[k].split(b"end_header\n")
            dt = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")]
            va, vb = np.frombuffer(ba, dt), np.frombuffer(bb, dt)
            if ha != hb or len(va) != len(vb) or any(not np.array_equal(va[c], vb[c]) for c in "rgb"):
                return False, None
            xa = np.stack([va[c] for c in "xyz"], 1).astype(np.float64)
            xb = np.stack([vb[c] for c in "xyz"], 1).astype(np.float64)
            ulp = np.spacing(np.maximum(np.abs(xa), np.abs(xb)).astype(np.float32)).astype(np.float64)
            scale = np.maximum(np.abs(xa).max(1, keepdims=True), 1.0) if len(xa) else 1.0
            if not np.all((np.abs(xa - xb) <= ulp) | (np.abs(xa - xb) <= 1e-12 * scale)):
                return False, None
            ndiff += int((xa != xb).sum())
        elif fa[k] != fb[k]:
            return False, None
    return True, ndiff


def fusion_alone(method, n, tmp):
    """Leg (a): fuse_scene on files vs ScanFusion on device maps, the same synthetic scene."""
    import io
    from PIL import Image
    from dmvsnet_amd import fusion
    dynamic = method == "dypcd"
    H, W = (1056, 2048) if dynamic else (864, 1152)
    t0 = time.perf_counter()
    cams, depths, confs, imgs = synth.synth_fusion_scene(H, W, n, seed=0)
    imgs = [(im * 255).astype(np.uint8) for im in imgs]
    pairs = [(v, sorted((u for u in range(n) if u != v), key=lambda u: (abs(u - v), u))[:min(10, n - 1)]) for v in range(n)]
    root = os.path.join(tmp, "fz_" + method)
    for sub in ("cams", "images", "depth_est", "confidence"):
        os.makedirs(os.path.join(root, sub))
    for v in range(n):
        eval_io.write_cam(os.path.join(root, "cams/{:0>8}_cam.txt".format(v)), cams[v])
        Image.fromarray(imgs[v]).save(os.path.join(root, "images/{:0>8}.jpg".format(v)))
        eval_io.save_pfm(os.path.join(root, "depth_est/{:0>8}.pfm".format(v)), depths[v])
        eval_io.save_pfm(os.path.join(root, "confidence/{:0>8}.pfm".format(v)), confs[v][2])
    res = dict(method=method, size=[H, W], views=n, sources=len(pairs[0][1]), scene_write_s=round(time.perf_counter() - t0, 2))
    conf = (0.1, 0.15, 0.3)
    kw = dict(conf=conf, thres_view=2, dynamic=dynamic)
    fusion.fuse_scene(pairs[:2], root, os.path.join(tmp, "warm.ply"), **kw)          # warm-up (code objects, allocator)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats_a = fusion.fuse_scene(pairs, root, os.path.join(tmp, "a.ply"), **kw)
    torch.cuda.synchronize()
    res["fuse_scene_wall_s"] = round(time.perf_counter() - t0, 3)
    # resident: maps already on the device, images decoded from the same JPEG bytes by a pool (as the scan driver does)
    dev = [(torch.from_numpy(depths[v]).cuda(), torch.from_numpy(confs[v][2]).cuda()) for v in range(n)]
    jpeg = [open(os.path.join(root, "images/{:0>8}.jpg".format(v)), "rb").read() for v in range(n)]
    cam = [fusion.read_camera_parameters(os.path.join(root, "cams/{:0>8}_cam.txt".format(v))) for v in range(n)]
    from concurrent.futures import ThreadPoolExecutor
    out_b = os.path.join(tmp, "fz_b_" + method)
    os.makedirs(os.path.join(out_b, "depth_est"))

    def decode(b):
        with Image.open(io.BytesIO(b)) as im:
            return np.asarray(im)

    for warm in (True, False):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with ThreadPoolExecutor(4) as pool:
            fz = fusion.ScanFusion([(0, [1]), (1, [0])] if warm else pairs, **kw)
            for v in (range(2) if warm else range(n)):
                fz.add(v, dev[v][0], dev[v][1], cam[v], pool.submit(decode, jpeg[v]))
            if warm:
                fz.close()
                continue
            t_enq = time.perf_counter() - t0
            stats_b = fz.write(out_b, os.path.join(tmp, "b.ply"))
        torch.cuda.synchronize()
        res["scan_fusion_wall_s"] = round(time.perf_counter() - t0, 3)
        res["scan_fusion_enqueue_s"] = round(t_enq, 3)
    res["wall_speedup"] = round(res["fuse_scene_wall_s"] / res["scan_fusion_wall_s"], 3)
    res["gpu_ms_per_view_fused"] = round(fz.device_seconds() * 1e3 / n, 4)
    res["stats_equal"] = stats_a == stats_b
    res["final_fraction_last_view"] = round(stats_b["final"], 4)
    # per-pair launches + finish for one view, events (finish synchronises: its host round trips count)
    r, srcs = pairs[n // 2]
    cam_t = lambda v: (cams[v, 1, :3, :3], cams[v, 0])   # noqa: E731
    ms_pairs, ms_finish = [], []
    for _ in range(4):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        vf = fusion.ViewFilter(dev[r][0], cam_t(r), dev[r][1], conf, dynamic=dynamic)
        for s in srcs:
            vf.add_source(dev[s][0], cam_t(s))
        e1.record()
        fv = vf.finish(imgs[r].astype(np.float32) / 255.0, 2)
        e2.record()
        e2.synchronize()
        ms_pairs.append(e0.elapsed_time(e1))
        ms_finish.append(e1.elapsed_time(e2))
    res["gpu_ms_per_view_pairs"] = round(statistics.median(ms_pairs), 4)
    res["gpu_ms_per_view_finish"] = round(statistics.median(ms_finish), 4)
    # host split per view (one thread): PNG of the three masks (PIL as fuse_scene, zlib as ScanFusion), JPEG decode, D2H
    masks = [fv.photo_mask, fv.geo_mask, fv.final_mask]
    t0 = time.perf_counter()
    for m in masks:
        Image.fromarray(m.astype(np.uint8) * 255).save(io.BytesIO(), format="PNG")
    res["host_ms_png_pil_3_masks"] = round((time.perf_counter() - t0) * 1e3, 2)
    t0 = time.perf_counter()
    for m in masks:
        fusion.png_gray8(m.astype(np.uint8) * 255)
    res["host_ms_png_zlib_3_masks"] = round((time.perf_counter() - t0) * 1e3, 2)
    t0 = time.perf_counter()
    decode(jpeg[r])
    res["host_ms_jpeg_decode"] = round((time.perf_counter() - t0) * 1e3, 2)
    t0 = time.perf_counter()
    fusion.write_ply(os.path.join(tmp, "c.ply"), np.zeros((len(fv.xyz) * n, 3), np.float32), np.zeros((len(fv.xyz) * n, 3), np.uint8))
    res["host_ms_ply_write_scene"] = round((time.perf_counter() - t0) * 1e3, 2)
    out = fusion.fuse_view(dev[r][0], cam_t(r), [dev[s][0] for s in srcs], [cam_t(s) for s in srcs], dev[r][1],
                           thresholds=conf, thres_view=2, dynamic=dynamic)
    torch.cuda.synchronize()
    hm = torch.empty(out["masks"].shape, dtype=torch.uint8, pin_memory=True)
    hx = torch.empty((len(fv.xyz), 3), dtype=torch.float32, pin_memory=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    hm.copy_(out["masks"], non_blocking=True)
    hx.copy_(out["xyz"][:len(fv.xyz)], non_blocking=True)
    e1.record()
    e1.synchronize()
    res["gpu_ms_d2h_per_view"] = round(e0.elapsed_time(e1), 4)
    fm = fv.final_mask
    res["mask_final_fraction"] = round(float(fm.mean()), 4)
    res["mask_row_transitions_per_px"] = round(float((fm[:, 1:] != fm[:, :-1]).mean()), 4)   # 0: solid regions, ~0.4: speckle
    # the outputs: the PLYs (xyz within 1 ulp), the mask pixels
    _, va = fusion_ply(os.path.join(tmp, "a.ply"))
    _, vb = fusion_ply(os.path.join(tmp, "b.ply"))
    same = len(va) == len(vb) and all(np.array_equal(va[c], vb[c]) for c in "rgb")
    for v, _ in pairs:
        for kind in ("photo", "geo", "final"):
            p = "mask/{:0>8}_{}.png".format(v, kind)
            same = same and np.array_equal(np.array(Image.open(os.path.join(root, p))), np.array(Image.open(os.path.join(out_b, p))))
    xa = np.stack([va[c] for c in "xyz"], 1)
    xb = np.stack([vb[c] for c in "xyz"], 1)
    res["points"] = len(va)
    res["xyz_values_differing"] = int((xa != xb).sum()) if same else None
    res["outputs_equal"] = bool(same and res["stats_equal"])
    return res


def fusion_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n")
    return head, np.frombuffer(body, [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])


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
    ap.add_argument("--fusion", choices=("pcd", "dypcd"), help="add the fusion legs (a) and (b) for this filter")
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
        if args.fusion:
            fz = {"a": fusion_alone(args.fusion, args.images, tmp)}
            # (b) end to end on the scan: file fusion vs resident fusion after the same scan-level step 1
            b, walls = {}, {}
            rkw = dict(kw, filter_method=args.fusion)
            eval_io.run_test(net, data, ["warm"], os.path.join(tmp, "rw0"), args.views, *args.max, feature_cache=True, **rkw)
            eval_io.run_test(net, data, ["warm"], os.path.join(tmp, "rw1"), args.views, *args.max, feature_cache=True,
                             resident_fusion=True, **rkw)
            rets, st = {}, {}
            for name, resident in (("file", False), ("resident", True)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st[name] = {}
                rets[name] = eval_io.run_test(net, data, ["scan1"], os.path.join(tmp, "run_" + name), args.views, *args.max,
                                              feature_cache=True, resident_fusion=resident, stats=st[name], **rkw)
                torch.cuda.synchronize()
                walls[name] = time.perf_counter() - t0
                b[f"{name}_wall_s"] = round(walls[name], 3)
                b[f"{name}_maps_per_s"] = round(res["maps"] / walls[name], 3)
            same, nd = _same_run_outputs(os.path.join(tmp, "run_file"), os.path.join(tmp, "run_resident"))
            b["files_equal"] = bool(same and rets["file"] == rets["resident"])
            b["xyz_values_differing"] = nd
            b["wall_speedup"] = round(walls["file"] / walls["resident"], 3)
            b["resident_phases_s"] = {k: round(v, 3) for k, v in st["resident"]["phases_s"].items()}
            b["file_step1_phases_s"] = {k: round(v, 3) for k, v in st["file"]["phases_s"].items()}
            b["fused_views"] = st["resident"]["fused_views"]
            b["fusion_peak_bytes"] = st["resident"]["fusion_peak_bytes"]
            b["final_fraction_last_view"] = rets["resident"]["scan1"]["final"]
            fz["b"] = b
            res["fusion"] = fz
    print(json.dumps(res))
    ok = res["files_equal"] and (not args.fusion or (res["fusion"]["a"]["outputs_equal"] and res["fusion"]["b"]["files_equal"]))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
