"""Deterministic synthetic inputs and weights for the DMVSNet hot path.

No dataset or checkpoint is reachable from the build or GPU boxes, so every
test / bench / golden vector uses the generators below.  Everything is driven
by NumPy ``PCG64`` (version-stable) and plain float32 NumPy arithmetic so the
same seed gives bit-identical tensors in the build container (where the golden
vectors are produced from the reference) and on the GPU box.

Shapes follow the reference's eval loader contract
(/root/reference/datasets/general_eval.py:69,172-198): ``imgs [B,V,3,H,W]`` in
[0,1], ``proj_matrices["stageK"] [B,V,2,4,4]`` with ``[...,0,:,:]`` the
world->camera extrinsic and ``[...,1,:3,:3]`` the intrinsics at that stage's
scale, ``depth_values [B,192]`` ascending.
"""
from __future__ import annotations

import zlib
from typing import Dict, Sequence

import numpy as np
import torch

__all__ = [
    "synth_fusion_scene",
    "synth_cloud_scene",
    "synth_val_scene",
    "synth_images",
    "synth_cameras",
    "synth_depth_values",
    "synth_inputs",
    "synth_state_dict",
    "CONFIGS",
]

# BASELINE.json configs, restated as numbers.
CONFIGS = {
    # plumbing config: image 128x160 -> 32x40 volume, 3 views, single stage D=8
    "c1": dict(H=128, W=160, V=3, ndepths=[8], ratios=[4]),
    # 3-stage variant of c1 used for end-to-end parity fixtures
    "c1s3": dict(H=128, W=160, V=3, ndepths=[16, 8, 8], ratios=[3, 2, 1]),
    # headline: DTU eval 1600x1184, 5 views, 64/32/8
    "c2": dict(H=1184, W=1600, V=5, ndepths=[64, 32, 8], ratios=[3, 2, 1]),
    "c3": dict(H=1184, W=1600, V=11, ndepths=[64, 32, 8], ratios=[3, 2, 1]),
    "c4": dict(H=1024, W=1920, V=11, ndepths=[64, 32, 8], ratios=[3, 2, 1]),
    # BASELINE configs[4] (BlendedMVS 2048x1536, 7 views, 4 stages 96/64/32/8): an EXTENSION -- the reference cannot
    # express a 4th stage; stages 1-2 run at the coarsest FPN level (MVSNet.stage_level)
    "c5": dict(H=1536, W=2048, V=7, ndepths=[96, 64, 32, 8], ratios=[4, 3, 2, 1]),
    # the reference's own eval recipes (not BASELINE lines).  DTU: scripts/dtu_test.sh:10-29 --
    # 48/32/8 planes, ratios 4/2/1, 5 views, --max_h 864 --max_w 1152 (the 1200x1600 frames shrink to 864x1152,
    # general_eval.py:97-110), --inverse_depth.  Tanks&Temples: scripts/tank_test.sh:10-23 -- 64/32/8, 3/2/1, 11 views,
    # filter/tank_test_config.py:10-11 max_h 1080 / max_w 2048: a 1080x2048 frame is only rounded down to base 32
    # (eval_io.ResizePolicy(1080, 2048).target(1080, 2048) == (1056, 2048)), linear depth sampling.
    "dtu": dict(H=864, W=1152, V=5, ndepths=[48, 32, 8], ratios=[4, 2, 1], inverse=True),
    "tnt": dict(H=1056, W=2048, V=11, ndepths=[64, 32, 8], ratios=[3, 2, 1]),
    # c3 at about a quarter of the linear size: what the multi-rank tests (several ranks sharing one GPU over gloo) run
    "c3_small": dict(H=288, W=416, V=11, ndepths=[16, 8, 8], ratios=[3, 2, 1]),
    # ... and config 2's view count at that size: 5 views on 8 ranks = 2 view groups x 4 (the default multi-GPU bench line)
    "c2_small": dict(H=288, W=416, V=5, ndepths=[16, 8, 8], ratios=[3, 2, 1]),
}


def _rng(seed: int, tag: str) -> np.random.Generator:
    return np.random.Generator(np.random.PCG64([int(seed), zlib.crc32(tag.encode())]))


def _upsample_bilinear_np(a: np.ndarray, H: int, W: int) -> np.ndarray:
    """Separable bilinear upsample (half-pixel centres, edge clamp), float32."""
    h, w = a.shape[-2:]

    def axis_weights(n_out, n_in):
        src = (np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5
        src = np.clip(src, 0.0, n_in - 1)
        i0 = np.floor(src).astype(np.int64)
        i1 = np.minimum(i0 + 1, n_in - 1)
        f = (src - i0).astype(np.float32)
        return i0, i1, f

    y0, y1, fy = axis_weights(H, h)
    x0, x1, fx = axis_weights(W, w)
    rows = a[..., y0, :] * (1 - fy)[:, None] + a[..., y1, :] * fy[:, None]
    out = rows[..., :, x0] * (1 - fx) + rows[..., :, x1] * fx
    return out.astype(np.float32)


def synth_images(H: int, W: int, V: int, seed: int = 0) -> torch.Tensor:
    """[1,V,3,H,W] float32 in [0,1]: shared low-frequency texture + per-view noise."""
    g = _rng(seed, "imgs.base")
    base = g.random((3, max(H // 8, 2), max(W // 8, 2)), dtype=np.float32)
    base = _upsample_bilinear_np(base, H, W)
    imgs = np.empty((1, V, 3, H, W), dtype=np.float32)
    for v in range(V):
        noise = _rng(seed, f"imgs.noise.{v}").random((3, H, W), dtype=np.float32)
        imgs[0, v] = np.clip(base + np.float32(0.1) * noise, 0.0, 1.0)
    return torch.from_numpy(imgs)


def synth_cameras(H: int, W: int, V: int, num_stage: int = 3) -> Dict[str, torch.Tensor]:
    """DTU-like cameras.  Stage k (1-based) intrinsics = K_full / 2**(3-k) on rows 0,1
    (mirrors general_eval.py:189-198, where stage1 = K/4 ... stage3 = K)."""
    K = np.array(
        [[2892.33 * W / 1600.0, 0.0, W / 2.0], [0.0, 2883.18 * H / 1200.0, H / 2.0], [0.0, 0.0, 1.0]],
        dtype=np.float64,
    )
    out = {}
    for s in range(1, 4):
        scale = 2.0 ** (3 - s)
        P = np.zeros((1, V, 2, 4, 4), dtype=np.float32)
        Ks = K.copy()
        Ks[:2, :] /= scale
        for v in range(V):
            a = 0.03 * v
            R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
            E = np.eye(4)
            E[:3, :3] = R
            E[:3, 3] = [-30.0 * v, 7.0 * v, 5.0 * v]
            P[0, v, 0] = E.astype(np.float32)
            P[0, v, 1, :3, :3] = Ks.astype(np.float32)
        out[f"stage{s}"] = torch.from_numpy(P)
    return out


def synth_depth_values(n: int = 192) -> torch.Tensor:
    """[1,n]: 425 + 2.5*1.06*i  (DTU depth_min, interval * --interval_scale)."""
    d = np.float32(425.0) + np.float32(2.5 * 1.06) * np.arange(n, dtype=np.float32)
    return torch.from_numpy(d[None].astype(np.float32))


def synth_inputs(H: int, W: int, V: int, seed: int = 0):
    return synth_images(H, W, V, seed), synth_cameras(H, W, V), synth_depth_values()


def synth_state_dict(template: Dict[str, torch.Tensor], seed: int = 0) -> Dict[str, torch.Tensor]:
    """Fill a state_dict *template* (keys + shapes) with a non-degenerate recipe.

    PyTorch default init + fresh BN statistics gives uniform softmax / confidence==1
    (SURVEY.md section 8c).  Recipe: conv weights ~ U(-b,b), b = 1/sqrt(fan_in);
    BN weight ~ U(.5,1.5), bias ~ N(0,.1), running_mean ~ N(0,.1), running_var ~ U(.5,1.5);
    every ``*.prob.weight`` multiplied by 20.  Each tensor is drawn from its own
    PCG64 stream keyed by (seed, crc32(key)) so the result is independent of key order.
    """
    out = {}
    for key, ref in template.items():
        shape = tuple(ref.shape)
        g = _rng(seed, key)
        if key.endswith("num_batches_tracked"):
            val = np.zeros(shape, dtype=np.int64)
        elif key.endswith("bn.weight") or key.endswith("running_var"):
            val = (0.5 + g.random(shape, dtype=np.float32)).astype(np.float32)
        elif key.endswith("bn.bias") or key.endswith("running_mean"):
            val = (np.float32(0.1) * g.standard_normal(shape, dtype=np.float32)).astype(np.float32)
        elif key.endswith("weight"):
            fan_in = int(np.prod(shape[1:]))
            b = np.float32(1.0 / np.sqrt(fan_in))
            val = ((g.random(shape, dtype=np.float32) * 2 - 1) * b).astype(np.float32)
            if key.endswith("prob.weight"):
                val = val * np.float32(20.0)
        elif key.endswith("bias"):
            val = ((g.random(shape, dtype=np.float32) * 2 - 1) * np.float32(0.1)).astype(np.float32)
        else:
            raise KeyError(f"synth_state_dict: no recipe for {key}")
        out[key] = torch.from_numpy(np.ascontiguousarray(val))
    return out


def synth_fusion_scene(H: int, W: int, V: int, seed: int = 0, z0: float = 620.0):
    """A scene for the depth-map fusion filter (row N4): the world plane ``0.05 x + 0.03 y + z = z0`` seen by the
    synthetic cameras.  Returns ``(cams [V,2,4,4], depths, confs, imgs)``: per view an exact plane depth map perturbed
    by 0.3 % multiplicative noise (so that part of the pixels sit near the 1 % consistency gate), a block of zero
    depths, a block of gross outliers, three confidence maps (stage 1 / 2 / 3) and an RGB image in [0,1]."""
    cams = synth_cameras(H, W, V)["stage3"][0].numpy()
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    n, depths, confs, imgs = np.array([0.05, 0.03, 1.0]), [], [], []
    for v in range(V):
        K, E = cams[v, 1, :3, :3].astype(np.float64), cams[v, 0].astype(np.float64)
        R, t = E[:3, :3], E[:3, 3]
        rays = np.linalg.inv(K) @ np.stack((xs.ravel(), ys.ravel(), np.ones(H * W)))
        d = (z0 + n @ (R.T @ t)) / (n @ (R.T @ rays))                 # n . R^T (d ray - t) = z0
        g = _rng(seed, f"fusion.{v}")
        d = d.reshape(H, W) * (1.0 + 0.003 * g.standard_normal((H, W)))
        d[H // 3:H // 3 + 6, W // 4:W // 4 + 9] = 0.0                 # holes
        d[H // 2:H // 2 + 5, W // 2:W // 2 + 7] *= 1.2                # gross outliers
        depths.append(d.astype(np.float32))
        confs.append(g.random((3, H, W), dtype=np.float32))
        imgs.append(g.random((H, W, 3), dtype=np.float32))
    return cams, depths, confs, imgs


def _cloud_surface(x, y, L):
    """The smooth height field of synth_cloud_scene (mm); slopes stay below ~0.5."""
    return 0.04 * L * np.sin(3.0 * np.pi * x / L) * np.cos(2.0 * np.pi * y / L) + 0.02 * L * np.cos(5.0 * x / L + 1.0)


def synth_cloud_scene(seed: int, n_data: int, n_stl: int, noise: float = 0.12, outlier_share: float = 0.03,
                      outside_share: float = 0.01, mask_cells: int = 64) -> Dict[str, np.ndarray]:
    """A deterministic DTU-evaluation scene (millimetres) for cloud_eval's tests and benchmark: one smooth surface sampled twice.

    ``stl``  [~n_stl,3] float32: a jittered 0.3 mm lattice on the surface -- no two points closer than 0.2 mm, as the dataset's
             reference clouds are thinned; the surface dips below the plane ``P`` in places.
    ``data`` [n_data,3] float32: random samples with a density that varies in patches (denser than 0.2 mm where it is high),
             discs without data (holes), Gaussian noise along z, a share of far outliers (5 .. 90 mm off the surface, some
             beyond 60 mm of anything), and a share of points outside ``BB``.
    ``ObsMask`` uint8 [nx,ny,nz] / ``BB`` [2,3] / ``Res``: the observability volume (a band around the surface, minus a border
             strip), its bounding box (not a multiple of 60 mm) and voxel size; ``P`` [4]: the ground plane."""
    rng = np.random.Generator(np.random.PCG64(seed))
    side = max(int(round(np.sqrt(max(n_stl, 1)))), 2)
    step = 0.3
    L = side * step
    gx, gy = np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64), indexing="ij")
    sx = (gx.ravel() + 0.5) * step + rng.uniform(-0.04, 0.04, side * side)
    sy = (gy.ravel() + 0.5) * step + rng.uniform(-0.04, 0.04, side * side)
    stl = np.stack([sx, sy, _cloud_surface(sx, sy, L)], 1).astype(np.float32)

    # data: rejection-sample (x, y) against a patchy density, drop the holes, keep the first n_data
    holes = rng.uniform(0.1 * L, 0.9 * L, (6, 2))
    hole_r = rng.uniform(0.03 * L, 0.07 * L, 6)
    parts, have = [], 0
    while have < n_data:
        m = int(1.6 * (n_data - have)) + 64
        x, y = rng.uniform(0, L, m), rng.uniform(0, L, m)
        dens = 0.55 + 0.45 * np.sin(7.0 * x / L + 0.3) * np.sin(5.0 * y / L + 1.1)
        keep = rng.uniform(0, 1, m) < dens
        for (hx, hy), hr in zip(holes, hole_r):
            keep &= (x - hx) ** 2 + (y - hy) ** 2 > hr * hr
        parts.append(np.stack([x[keep], y[keep]], 1))
        have += int(keep.sum())
    xy = np.concatenate(parts)[:n_data]
    z = _cloud_surface(xy[:, 0], xy[:, 1], L) + rng.normal(0.0, noise, n_data)
    kind = rng.uniform(0, 1, n_data)
    out = kind < outlier_share
    z = np.where(out, z + rng.choice([-1.0, 1.0], n_data) * rng.uniform(5.0, 90.0, n_data), z)
    data = np.stack([xy[:, 0], xy[:, 1], z], 1)
    far = (kind >= outlier_share) & (kind < outlier_share + outside_share)
    data[far, 0] += rng.choice([-1.0, 1.0], n_data)[far] * (L + rng.uniform(20.0, 150.0, n_data)[far])
    data = data.astype(np.float32)

    zr = 0.07 * L
    bb = np.array([[-7.0, -11.0, -zr - 35.0], [L + 9.0, L + 5.0, zr + 41.0]], dtype=np.float64)
    res = float((bb[1] - bb[0]).max() / mask_cells)
    dims = np.floor((bb[1] - bb[0]) / res).astype(np.int64) + 1
    cx = bb[0, 0] + np.arange(dims[0]) * res
    cy = bb[0, 1] + np.arange(dims[1]) * res
    cz = bb[0, 2] + np.arange(dims[2]) * res
    X, Y, Z = np.meshgrid(cx, cy, cz, indexing="ij")
    band = np.abs(Z - _cloud_surface(np.clip(X, 0, L), np.clip(Y, 0, L), L)) < 10.0 + res
    inner = (X > 0.05 * L) & (X < L + 2.0) & (Y > -2.0) & (Y < 0.93 * L)
    obs = np.ascontiguousarray(band & inner, dtype=np.uint8)
    plane = np.array([0.02, -0.015, 1.0, 0.012 * L], dtype=np.float64)
    return dict(data=data, stl=stl, ObsMask=obs, BB=bb, Res=res, P=plane)


def synth_val_scene(root: str, seed: int = 0, V: int = 3, lights: int = 2, scan: str = "scan1", raw_hw=(1200, 1600)) -> Dict[str, object]:
    """Write a small tree in the DTU TRAINING layout (what datasets/dtu_yao.py reads) under ``root``: one scan, ``V`` views,
    ``lights`` light conditions.

      Cameras/pair.txt, Cameras/train/%08d_cam.txt   intrinsics at 1/4 scale (synth_cameras' stage 1), depth line "425.0 2.5"
      Rectified/<scan>_train/rect_%03d_<light>_r5000.png   512 x 640 RGB (view id + 1 in the name)
      Depths_raw/<scan>/depth_map_%04d.pfm           raw ground truth ``raw_hw`` (1200 x 1600: the loader halves it and crops
                                                     512 x 640 from the middle): a smooth surface 450..800 mm
      Depths_raw/<scan>/depth_visual_%04d.png        8-bit mask source (valid > 10): ragged holes, a dark band of values <= 10
      val.txt                                        the scan list

    Returns {"listfile", "scan", "views", "lights"}; the loader's metas are views x 7 lights unless told ``lights``."""
    import os

    from PIL import Image

    from . import eval_io

    H, W = 512, 640
    os.makedirs(os.path.join(root, "Cameras", "train"), exist_ok=True)
    os.makedirs(os.path.join(root, "Rectified", scan + "_train"), exist_ok=True)
    os.makedirs(os.path.join(root, "Depths_raw", scan), exist_ok=True)
    cams = synth_cameras(H, W, V)["stage1"][0].numpy()
    with open(os.path.join(root, "Cameras", "pair.txt"), "w") as f:
        f.write("{}\n".format(V))
        for v in range(V):
            others = [(v + k) % V for k in range(1, V)]
            f.write("{}\n{} {}\n".format(v, len(others), " ".join("{} {}".format(o, 100.0 - k) for k, o in enumerate(others))))
    for v in range(V):
        with open(os.path.join(root, "Cameras", "train", "{:0>8}_cam.txt".format(v)), "w") as f:
            f.write("extrinsic\n")
            for i in range(4):
                f.write(" ".join(str(cams[v, 0, i, j]) for j in range(4)) + " \n")
            f.write("\nintrinsic\n")
            for i in range(3):
                f.write(" ".join(str(cams[v, 1, i, j]) for j in range(3)) + " \n")
            f.write("\n425.0 2.5\n")
        g = _rng(seed, f"val.gt.{v}")
        rh, rw = raw_hw
        depth = np.float32(450.0) + np.float32(350.0) * _upsample_bilinear_np(g.random((6, 8), dtype=np.float32), rh, rw)
        vis = (g.random((rh // 8, rw // 8), dtype=np.float32) > 0.12).astype(np.uint8).repeat(8, 0).repeat(8, 1) * 200
        vis[g.random((rh, rw), dtype=np.float32) < 0.02] = 10                     # single-pixel holes, exactly at the threshold
        vis[rh // 2 - 3:rh // 2 + 4, :] = 7                                        # a dark band through the crop
        depth[vis <= 10] = 0.0
        eval_io.save_pfm(os.path.join(root, "Depths_raw", scan, "depth_map_{:0>4}.pfm".format(v)), depth)
        Image.fromarray(vis).save(os.path.join(root, "Depths_raw", scan, "depth_visual_{:0>4}.png".format(v)))
    for light in range(lights):
        imgs = synth_images(H, W, V, seed=seed + 17 * light)[0].numpy()
        for v in range(V):
            a = np.clip(np.transpose(imgs[v], (1, 2, 0)) * 255.0, 0, 255).astype(np.uint8)
            Image.fromarray(a).save(os.path.join(root, "Rectified", scan + "_train", "rect_{:0>3}_{}_r5000.png".format(v + 1, light)),
                                    compress_level=1)
    listfile = os.path.join(root, "val.txt")
    with open(listfile, "w") as f:
        f.write(scan + "\n")
    return {"listfile": listfile, "scan": scan, "views": V, "lights": lights}
