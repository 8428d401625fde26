"""Depth-map fusion after the network: photometric mask, geometric consistency over
the source views, depth averaging and back-projection to a coloured point cloud.

What the reference does per reference view (/root/reference/filter/pcd.py:244-361 ``filter_depth``; the
Tanks&Temples variant with a ladder of thresholds, filter/dypcd_tanks.py:164-326) becomes:

  ``ViewFilter``         the per-view state on the GPU: photometric mask from the three stage confidences, vote /
                         depth accumulators, one fused kernel launch per source view (``dmvs_geo_consistency`` or
                         ``dmvs_geo_consistency_ladder``), then the static (``votes >= thres_view``) or dynamic
                         (``any_i votes_i >= i``) geometric mask, the averaged depth and the world points
  ``fuse_scene``         the file-based driver over a folder written by ``eval_io.save_depth_maps`` (depth_est/,
                         confidence/, cams/, images/): mask PNGs, the averaged depth PFM of the dynamic variant, the PLY

The per-pixel work runs on the GPU (no CPU fallback); file handling stays in Python.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .eval_io import read_pfm, save_pfm

N_LEVELS = 9   # gates i = 2..10 of the dynamic variant (dypcd_tanks.py:178)


def fold_projection(intrinsics_ref, extrinsics_ref, intrinsics_src, extrinsics_src) -> np.ndarray:
    """The 33 floats the consistency kernels take (fp64 products, rounded once); see include/dmvs.h."""
    Kr, Er = np.asarray(intrinsics_ref, np.float64), np.asarray(extrinsics_ref, np.float64)
    Ks, Es = np.asarray(intrinsics_src, np.float64), np.asarray(extrinsics_src, np.float64)
    rel = Es @ np.linalg.inv(Er)      # ref camera -> src camera
    back = Er @ np.linalg.inv(Es)     # src camera -> ref camera
    A1 = Ks @ rel[:3, :3] @ np.linalg.inv(Kr)
    b1 = Ks @ rel[:3, 3]
    A2 = back[:3, :3] @ np.linalg.inv(Ks)
    t2 = back[:3, 3]
    return np.concatenate([A1.ravel(), b1, A2.ravel(), t2, Kr.ravel()]).astype(np.float32)


def _dev_f32(a, device, what):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    t = t.to(device=device, dtype=torch.float32).contiguous()
    if t.dim() != 2:
        raise _lib.DmvsError(f"{what}: expected an [H,W] map, got {tuple(t.shape)}")
    return t


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def check_geometric_consistency(depth_ref: torch.Tensor, intrinsics_ref, extrinsics_ref, depth_src: torch.Tensor,
                                intrinsics_src, extrinsics_src, dist_thresh: float = 1.0, rel_thresh: float = 0.01,
                                vote_sum: Optional[torch.Tensor] = None, depth_sum: Optional[torch.Tensor] = None,
                                level_votes: Optional[torch.Tensor] = None):
    """One (reference, source) pair, pcd.py:151-242 -> (mask uint8 [H,W], depth_reprojected [H,W]).
    ``vote_sum`` (int32 [H,W]) / ``depth_sum`` (float32 [H,W]) are accumulated when given.
    ``level_votes`` (int32 [9,H,W]) selects the dynamic ladder (dypcd_tanks.py:164-184): ``dist_thresh`` /
    ``rel_thresh`` are then the BASES of the nine gates and mask / sums refer to the last one."""
    if not depth_ref.is_cuda:
        raise _lib.DmvsError("fusion kernels need tensors on a HIP device (no CPU fallback)")
    H, W = depth_ref.shape
    for name, t, dt, shape in (("depth_ref", depth_ref, torch.float32, (H, W)), ("depth_src", depth_src, torch.float32, (H, W)),
                               ("vote_sum", vote_sum, torch.int32, (H, W)), ("depth_sum", depth_sum, torch.float32, (H, W)),
                               ("level_votes", level_votes, torch.int32, (N_LEVELS, H, W))):
        if t is None:
            continue
        # the kernel indexes every map with the reference's H, W: a smaller source map would be read out of bounds
        if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != depth_ref.device:
            raise _lib.DmvsError(f"{name}: need a contiguous {dt} tensor of shape {shape} on {depth_ref.device}, got "
                                 f"{t.dtype} {tuple(t.shape)} on {t.device}")
    P = torch.from_numpy(fold_projection(intrinsics_ref, extrinsics_ref, intrinsics_src, extrinsics_src)).to(depth_ref.device)
    mask = torch.empty((H, W), dtype=torch.uint8, device=depth_ref.device)
    rep = torch.empty((H, W), dtype=torch.float32, device=depth_ref.device)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = _lib.load()
    if level_votes is None:
        code = lib.dmvs_geo_consistency(_ptr(depth_ref), _ptr(depth_src), _ptr(P), H, W, float(dist_thresh),
                                        float(rel_thresh), _ptr(mask), _ptr(rep), _ptr(vote_sum), _ptr(depth_sum), st)
    else:
        code = lib.dmvs_geo_consistency_ladder(_ptr(depth_ref), _ptr(depth_src), _ptr(P), H, W, float(dist_thresh),
                                               float(rel_thresh), _ptr(level_votes), _ptr(mask), _ptr(rep),
                                               _ptr(vote_sum), _ptr(depth_sum), st)
    _lib.check(code, "dmvs_geo_consistency")
    return mask, rep


@dataclass
class FusedView:
    xyz: np.ndarray            # [N,3] float32 world points
    rgb: np.ndarray            # [N,3] uint8
    photo_mask: np.ndarray     # [H,W] bool
    geo_mask: np.ndarray
    final_mask: np.ndarray
    depth_averaged: np.ndarray  # [H,W] float32
    stats: Dict[str, float]


class ViewFilter:
    """Fusion state of ONE reference view on the GPU.  ``conf`` thresholds are per stage ``(c1, c2, c3)`` like
    ``args.conf`` (pcd.py:268-274): the mask is ``conf3 > c3 & conf2 > c2 & conf1 > c1``; a scalar applies one
    threshold to the final confidence only; missing stage maps default to the final one, as in the reference."""

    def __init__(self, depth, cam, confidence, conf=(0.1, 0.1, 0.1), confidence2=None, confidence1=None,
                 dynamic: bool = False, device="cuda"):
        self.device = torch.device(device)
        self.K, self.E = np.asarray(cam[0]), np.asarray(cam[1])
        self.depth = _dev_f32(depth, self.device, "depth")
        c3 = _dev_f32(confidence, self.device, "confidence")
        c2 = c3 if confidence2 is None else _dev_f32(confidence2, self.device, "confidence2")
        c1 = c3 if confidence1 is None else _dev_f32(confidence1, self.device, "confidence1")
        if np.isscalar(conf):
            self.photo_mask = c3 > float(conf)
        else:
            t1, t2, t3 = (float(v) for v in conf)
            self.photo_mask = (c3 > t3) & (c2 > t2) & (c1 > t1)
        self.dynamic = dynamic
        self.votes = torch.zeros(self.depth.shape, dtype=torch.int32, device=self.device)
        self.depth_sum = torch.zeros_like(self.depth)
        self.level_votes = torch.zeros((N_LEVELS,) + tuple(self.depth.shape), dtype=torch.int32, device=self.device) if dynamic else None
        self.nsrc = 0

    def add_source(self, depth_src, cam_src, dist=None, rel=None):
        """Accumulate one source view.  Static: gates ``dist`` px / ``rel`` (default 1 / 0.01, pcd.py:236);
        dynamic: bases of the ladder (default 1/4 px, 1/1300; the tank scripts' ``--dist_base`` / ``--rel_diff_base``)."""
        d_src = _dev_f32(depth_src, self.device, "depth_src")
        if self.dynamic:
            dist, rel = (0.25 if dist is None else dist), (1.0 / 1300 if rel is None else rel)
        else:
            dist, rel = (1.0 if dist is None else dist), (0.01 if rel is None else rel)
        check_geometric_consistency(self.depth, self.K, self.E, d_src, cam_src[0], cam_src[1], dist, rel,
                                    vote_sum=self.votes, depth_sum=self.depth_sum, level_votes=self.level_votes)
        self.nsrc += 1

    def finish(self, image, thres_view: int = 2) -> FusedView:
        """Masks, averaged depth and the world points of the view (pcd.py:299-344 / dypcd_tanks.py:258-304).
        ``image`` [H,W,3] float in [0,1] supplies the colours."""
        d_ref = self.depth
        if self.dynamic:
            # at least i views under gate i, for any i in [2, nsrc]; the all-views test on the last gate is
            # `votes >= nsrc + 1` in the reference and can never hold (dypcd_tanks.py:233,258-260)
            geo = self.votes >= self.nsrc + 1
            for i in range(2, self.nsrc + 1):
                geo |= self.level_votes[i - 2] >= i
            d_base = d_ref
        else:
            geo = self.votes >= thres_view
            # the reference's check overwrites zero reference depths with 1e-4 IN PLACE before averaging (pcd.py:235)
            d_base = torch.where(d_ref == 0, torch.full_like(d_ref, 1e-4), d_ref) if self.nsrc else d_ref
        # float32 sum, promoted to float64 only by the division with the int32 count (NumPy: pcd.py:299, dypcd_tanks.py:248)
        d_avg = (self.depth_sum + d_base).double() / (self.votes + 1).double()
        final = self.photo_mask & geo
        ys, xs = torch.nonzero(final, as_tuple=True)
        depth = d_avg[final]
        Kinv = torch.from_numpy(np.linalg.inv(np.asarray(self.K, np.float32)).astype(np.float64)).to(self.device)
        Einv = torch.from_numpy(np.linalg.inv(np.asarray(self.E, np.float32)).astype(np.float64)).to(self.device)
        pts = Kinv @ (torch.stack((xs.double(), ys.double(), torch.ones_like(depth))) * depth)
        pts = (Einv @ torch.cat((pts, torch.ones_like(depth)[None])))[:3]
        fm = final.cpu().numpy()
        rgb = (np.asarray(image)[fm] * 255).astype(np.uint8)
        stats = {"photo": self.photo_mask.float().mean().item(), "geo": geo.float().mean().item(),
                 "final": final.float().mean().item()}
        return FusedView(pts.T.float().cpu().numpy(), rgb, self.photo_mask.cpu().numpy(), geo.cpu().numpy(), fm,
                         d_avg.float().cpu().numpy(), stats)


def filter_depth(ref_depth, ref_conf, ref_cam, ref_img, src_depths: Sequence, src_cams: Sequence, conf_thresh=0.1,
                 thres_view: int = 2, device="cuda", confidence2=None, confidence1=None, dynamic: bool = False
                 ) -> Tuple[np.ndarray, np.ndarray, Dict[str, float]]:
    """One reference view (pcd.py:256-344): (xyz_world [N,3] float32, rgb [N,3] uint8, mask statistics).
    ``conf_thresh``: scalar or the per-stage triple of ``args.conf``."""
    vf = ViewFilter(ref_depth, ref_cam, ref_conf, conf_thresh, confidence2, confidence1, dynamic, device)
    for d_src, cam in zip(src_depths, src_cams):
        vf.add_source(d_src, cam)
    out = vf.finish(ref_img, thres_view)
    return out.xyz, out.rgb, out.stats


def write_ply(filename: str, xyz: np.ndarray, rgb: np.ndarray) -> None:
    """Binary little-endian PLY with x,y,z float32 + red,green,blue uint8 vertices (what PlyData writes, pcd.py:346-360)."""
    v = np.empty(len(xyz), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    with open(filename, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
                 "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(v)).encode())
        f.write(v.tobytes())


def read_camera_parameters(filename):
    """(intrinsics [3,3], extrinsics [4,4]) from a *_cam.txt as written by eval_io.write_cam (pcd.py:68-78)."""
    with open(filename) as f:
        lines = [line.rstrip() for line in f.readlines()]
    extrinsics = np.array(" ".join(lines[1:5]).split(), dtype=np.float32).reshape(4, 4)
    intrinsics = np.array(" ".join(lines[7:10]).split(), dtype=np.float32).reshape(3, 3)
    return intrinsics, extrinsics


def read_pair_file(filename) -> List[Tuple[int, List[int]]]:
    """pair.txt -> [(ref_view, [src_view, ...]), ...]; views without sources are skipped (pcd.py:82-93)."""
    data = []
    with open(filename) as f:
        for _ in range(int(f.readline())):
            ref_view = int(f.readline().rstrip())
            src_views = [int(x) for x in f.readline().rstrip().split()[1::2]]
            if src_views:
                data.append((ref_view, src_views))
    return data


def fuse_scene(pair_data: Sequence[Tuple[int, List[int]]], out_folder: str, plyfilename: str, conf=(0.1, 0.15, 0.7),
               thres_view: int = 5, dynamic: bool = False, num_stage: int = 3, device="cuda",
               write_masks: bool = True, dist_base: Optional[float] = None, rel_diff_base: Optional[float] = None) -> Dict[str, float]:
    """``filter_depth`` over a scene folder written by eval_io.save_depth_maps (depth_est/, confidence/ incl. the
    optional ``_stage1`` / ``_stage2`` maps, cams/, images/): writes mask/%08d_{photo,geo,final}.png
    (pcd.py:307-310), depth_est/%08d_averaged.pfm for the dynamic variant (dypcd_tanks.py:255) and the PLY.
    Defaults = main.py:60-61 (``--conf 0.1 0.15 0.7``, ``--thres_view 5``); ``dist_base`` / ``rel_diff_base``: the dynamic
    filter's ladder bases (main.py:63-64), ignored by the static one.  Views of one scene must share one size (the
    reference's filters assume it too: they index the source maps with reference-sized grids); a scene with mixed
    image sizes needs ``fix_res`` in step 1."""
    from PIL import Image

    def pfm(sub, v, suffix=""):
        return read_pfm(os.path.join(out_folder, sub, "{:0>8}{}.pfm".format(v, suffix)))[0]

    def cam(v):
        return read_camera_parameters(os.path.join(out_folder, "cams/{:0>8}_cam.txt".format(v)))

    pts, cols, stats = [], [], {}
    for ref_view, src_views in pair_data:
        has_stages = os.path.exists(os.path.join(out_folder, "confidence/{:0>8}_stage2.pfm".format(ref_view)))
        vf = ViewFilter(pfm("depth_est", ref_view), cam(ref_view), pfm("confidence", ref_view), conf,
                        pfm("confidence", ref_view, "_stage2") if has_stages else None,
                        pfm("confidence", ref_view, "_stage1") if has_stages else None, dynamic, device)
        for v in src_views:
            if dynamic:
                vf.add_source(pfm("depth_est", v), cam(v), dist_base, rel_diff_base)
            else:
                vf.add_source(pfm("depth_est", v), cam(v))
        img = np.array(Image.open(os.path.join(out_folder, "images/{:0>8}.jpg".format(ref_view))), dtype=np.float32) / 255.0
        step = 2 ** (3 - num_stage)     # 1- / 2-stage nets stop at 1/4 / 1/2 resolution (pcd.py:332-337)
        out = vf.finish(img[1::step, 1::step] if step > 1 else img, thres_view)
        if write_masks:
            os.makedirs(os.path.join(out_folder, "mask"), exist_ok=True)
            for kind, m in (("photo", out.photo_mask), ("geo", out.geo_mask), ("final", out.final_mask)):
                Image.fromarray(m.astype(np.uint8) * 255).save(os.path.join(out_folder, "mask/{:0>8}_{}.png".format(ref_view, kind)))
        if dynamic:
            save_pfm(os.path.join(out_folder, "depth_est/{:0>8}_averaged.pfm".format(ref_view)), out.depth_averaged)
        pts.append(out.xyz)
        cols.append(out.rgb)
        stats = out.stats
    write_ply(plyfilename, np.concatenate(pts), np.concatenate(cols))
    return stats


# ------------------------------------------------------------------------------------------ scan-level fusion
MAX_SOURCES = 16            # include/dmvs.h DMVS_FUSE_MAX_SRC
MAX_SOURCES_DYNAMIC = 10    # nine gates: the dynamic geo mask reads level i - 2 for i <= nsrc
FUSION_WORKERS = 4          # host threads of ScanFusion (D2H wait, colour gather, PNG encode); a fixed number


class FusionSchedule:
    """When each reference view of ``pair_data`` can be fused and when each map can be released, as maps arrive in any
    order.  A view is ready once its own maps and the depth map of every one of its sources have arrived; its confidence
    maps are released when it is fused, a depth map after the last view that reads it is fused.  Host bookkeeping only."""

    def __init__(self, pair_data: Sequence[Tuple[int, List[int]]]):
        self.pairs = [(int(r), [int(s) for s in srcs]) for r, srcs in pair_data]
        refs = [r for r, _ in self.pairs]
        if len(set(refs)) != len(refs):
            raise _lib.DmvsError("pair list names a reference view twice")
        self.sources = dict(self.pairs)
        self.views = set(refs) | {s for _, srcs in self.pairs for s in srcs}
        self.depth_uses = {v: 0 for v in self.views}          # fusions that still read the depth map of v
        for r, srcs in self.pairs:
            for v in set([r] + srcs):
                self.depth_uses[v] += 1
        self.arrived, self.fused = set(), set()

    def arrive(self, view: int) -> List[int]:
        """Record the maps of ``view``; -> the reference views that became ready (pair order)."""
        view = int(view)
        if view not in self.views:
            raise _lib.DmvsError(f"view {view} is neither a reference nor a source in the pair list")
        if view in self.arrived:
            raise _lib.DmvsError(f"maps of view {view} added twice")
        self.arrived.add(view)
        return [r for r, srcs in self.pairs if r not in self.fused and r in self.arrived
                and all(s in self.arrived for s in srcs) and (view == r or view in srcs)]

    def fuse(self, ref: int) -> List[int]:
        """Mark ``ref`` fused; -> the views whose depth maps are no longer needed."""
        self.fused.add(ref)
        out = []
        for v in set([ref] + self.sources[ref]):
            self.depth_uses[v] -= 1
            if self.depth_uses[v] == 0:
                out.append(v)
        return sorted(out)

    def missing(self) -> List[int]:
        """Views whose maps some unfused reference view still waits for."""
        return sorted({v for r, srcs in self.pairs if r not in self.fused for v in [r] + srcs if v not in self.arrived})

    def done(self) -> bool:
        return len(self.fused) == len(self.pairs)


def png_gray8(a: np.ndarray, level: int = 1) -> bytes:
    """An 8-bit grayscale PNG of ``a`` [H,W] uint8 (filter 0 on every row, one zlib stream).  Written with zlib, which
    releases the GIL while it compresses; decodes to the same pixels as PIL's ``Image.fromarray(a).save(.png)``.  Level 1:
    a speckled 864x1152 mask takes about 7x less time than at PIL's level 6 for a 40 % larger file."""
    import struct
    import zlib
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim != 2:
        raise ValueError(f"png_gray8: expected [H,W], got {a.shape}")
    h, w = a.shape
    raw = np.zeros((h, w + 1), np.uint8)
    raw[:, 1:] = a

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(raw.tobytes(), level)) + chunk(b"IEND", b""))


def fuse_view(depth_ref: torch.Tensor, cam_ref, src_depths: Sequence[torch.Tensor], src_cams, conf3: torch.Tensor,
              conf2: Optional[torch.Tensor] = None, conf1: Optional[torch.Tensor] = None, thresholds=(0.1, 0.15, 0.7),
              thres_view: int = 5, dynamic: bool = False, dist: Optional[float] = None, rel: Optional[float] = None
              ) -> Dict[str, torch.Tensor]:
    """One reference view against all of its sources in one fused pass (``dmvs_fuse_view``) plus the point emission
    (``dmvs_fuse_emit``), enqueued on the current stream; nothing waits.  The maps: contiguous fp32 [H,W] device tensors of
    one size; cams: (K [3,3], E [4,4]) fp32; ``thresholds`` (t1, t2, t3) against (conf1, conf2, conf3) -- missing stage maps
    are ``conf3``; ``dist`` / ``rel``: the gates (static, default 1 / 0.01) or the ladder's bases (dynamic, default
    1/4 / 1/1300).  -> device tensors: masks [3,H,W] uint8 (photo, geo, final as 0 / 255), depth_avg [H,W] fp32, count [1]
    int32, xyz [H*W,3] fp32 of which the first ``count`` rows are the world points of the final pixels in row-major order
    -- what ``ViewFilter.finish`` computes from the same inputs."""
    lib = _lib.load()
    nsrc = len(src_depths)
    limit = MAX_SOURCES_DYNAMIC if dynamic else MAX_SOURCES
    if not 1 <= nsrc <= limit or len(src_cams) != nsrc:
        raise _lib.DmvsError(f"fuse_view: {nsrc} sources ({len(src_cams)} cams); the fused pass takes 1..{limit}")
    if not depth_ref.is_cuda:
        raise _lib.DmvsError("fusion kernels need tensors on a HIP device (no CPU fallback)")
    H, W = depth_ref.shape
    conf2 = conf3 if conf2 is None else conf2
    conf1 = conf3 if conf1 is None else conf1
    for name, t in [("depth_ref", depth_ref), ("conf3", conf3), ("conf2", conf2), ("conf1", conf1)] + \
                   [(f"src_depths[{i}]", t) for i, t in enumerate(src_depths)]:
        # the kernel indexes every map with the reference's H, W: a smaller map would be read out of bounds
        if tuple(t.shape) != (H, W) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != depth_ref.device:
            raise _lib.DmvsError(f"{name}: need a contiguous float32 tensor of shape {(H, W)} on {depth_ref.device}, got "
                                 f"{t.dtype} {tuple(t.shape)} on {t.device}")
    if dynamic:
        dist, rel = (0.25 if dist is None else dist), (1.0 / 1300 if rel is None else rel)
    else:
        dist, rel = (1.0 if dist is None else dist), (0.01 if rel is None else rel)
    K, E = np.asarray(cam_ref[0], np.float32), np.asarray(cam_ref[1], np.float32)
    P = np.ascontiguousarray(np.stack([fold_projection(K, E, *c) for c in src_cams]), dtype=np.float32)
    ptrs = (ctypes.c_void_p * nsrc)(*[t.data_ptr() for t in src_depths])
    kinv = np.ascontiguousarray(np.linalg.inv(K).astype(np.float64))       # as ViewFilter.finish forms them
    einv = np.ascontiguousarray(np.linalg.inv(E).astype(np.float64))
    nblk = int(lib.dmvs_fuse_workgroups(H, W))
    dev = depth_ref.device
    masks = torch.empty((3, H, W), dtype=torch.uint8, device=dev)
    avg = torch.empty((H, W), dtype=torch.float32, device=dev)
    avg64 = torch.empty((H, W), dtype=torch.float64, device=dev)
    counts = torch.empty(nblk, dtype=torch.int32, device=dev)
    offsets = torch.empty(nblk + 1, dtype=torch.int32, device=dev)
    xyz = torch.empty((H * W, 3), dtype=torch.float32, device=dev)
    t1, t2, t3 = (float(v) for v in thresholds)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.dmvs_fuse_view(_ptr(depth_ref), _ptr(conf3), _ptr(conf2), _ptr(conf1), H, W, nsrc, ptrs,
                                  P.ctypes.data_as(ctypes.c_void_p), t1, t2, t3, int(dynamic), int(thres_view), float(dist),
                                  float(rel), _ptr(masks), _ptr(avg), _ptr(avg64), _ptr(counts), st), "dmvs_fuse_view")
    _lib.check(lib.dmvs_fuse_emit(_ptr(masks), _ptr(avg64), _ptr(counts), H, W, kinv.ctypes.data_as(ctypes.c_void_p),
                                  einv.ctypes.data_as(ctypes.c_void_p), _ptr(offsets), _ptr(xyz), st), "dmvs_fuse_emit")
    return {"masks": masks, "depth_avg": avg, "count": offsets[nblk:], "xyz": xyz}


@dataclass
class _ViewResult:
    xyz: np.ndarray
    rgb: np.ndarray
    pngs: Optional[Dict[str, bytes]]
    depth_averaged: Optional[np.ndarray]


class ScanFusion:
    """``fuse_scene`` on device-resident maps, one fused kernel pass per reference view (``dmvs_fuse_view`` +
    ``dmvs_fuse_emit``).  Feed it the maps of every view with ``add`` in any order; each reference view is fused as soon as
    its own maps and the depth map of every source have arrived, and maps are released after their last use
    (``FusionSchedule``).  ``write`` writes what ``fuse_scene`` writes -- mask PNGs (zlib-encoded: same pixels, the bytes may
    differ from PIL's), ``depth_est/%08d_averaged.pfm`` of the dynamic filter, the PLY -- and returns its value.  Same
    arguments and defaults as ``fuse_scene``; ``conf``: the per-stage triple or a scalar.

    Host work (waiting for the copies, the colour gather, PNG encoding) runs on ``workers`` threads; the calling thread
    never waits for the GPU per view.  Results are held on the host until ``write``."""

    def __init__(self, pair_data, conf=(0.1, 0.15, 0.7), thres_view: int = 5, dynamic: bool = False, num_stage: int = 3,
                 dist_base: Optional[float] = None, rel_diff_base: Optional[float] = None, device="cuda",
                 workers: int = FUSION_WORKERS):
        from concurrent.futures import ThreadPoolExecutor
        self.schedule = FusionSchedule(pair_data)
        limit = MAX_SOURCES_DYNAMIC if dynamic else MAX_SOURCES
        for r, srcs in self.schedule.pairs:
            if not 1 <= len(srcs) <= limit:
                raise _lib.DmvsError(f"view {r}: {len(srcs)} sources; the fused pass takes 1..{limit}"
                                     f"{' (dynamic filter: nine gates)' if dynamic else ''}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.DmvsError("fusion kernels need a HIP device (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.scalar_conf = bool(np.isscalar(conf))
        if self.scalar_conf:
            self.thresholds = (float(conf),) * 3
        else:
            self.thresholds = tuple(float(v) for v in conf)
        self.thres_view, self.dynamic, self.num_stage = int(thres_view), bool(dynamic), int(num_stage)
        if dynamic:
            self.dist, self.rel = (0.25 if dist_base is None else dist_base), (1.0 / 1300 if rel_diff_base is None else rel_diff_base)
        else:
            self.dist, self.rel = 1.0, 0.01          # fuse_scene's static filter: ViewFilter.add_source defaults
        self.size = None
        self.depth: Dict[int, torch.Tensor] = {}
        self.conf: Dict[int, tuple] = {}
        self.cams: Dict[int, Tuple[np.ndarray, np.ndarray]] = {}
        self.images: Dict[int, object] = {}
        self.results: Dict[int, object] = {}      # ref -> Future[_ViewResult]
        self.last_masks = None                     # device masks of the last view in pair order (its stats)
        self.bytes = self.peak_bytes = 0
        self.events: List[Tuple[torch.cuda.Event, torch.cuda.Event]] = []
        self.pool = ThreadPoolExecutor(max_workers=max(1, int(workers)), thread_name_prefix="dmvs-fusion")
        self._closed = False

    # -- input -------------------------------------------------------------------------------------------------------
    def add(self, view_id: int, depth, confidence, cam, image, confidence2=None, confidence1=None) -> List[int]:
        """Maps of one view: ``depth`` / ``confidence`` (and the optional stage maps) [H,W] fp32 (device tensors stay where
        they are), ``cam`` = (K [3,3], E [4,4]), ``image`` [h,w,3] uint8 -- or a future of one -- for the colours (h, w: the
        maps' size times 2 ** (3 - num_stage), subsampled ``[1::step, 1::step]`` as fuse_scene does).  -> the reference
        views fused by this call."""
        view_id = int(view_id)
        given = {k: _dev_f32(m, self.device, k) for k, m in (("depth", depth), ("confidence", confidence),
                 ("confidence2", confidence2), ("confidence1", confidence1)) if m is not None}
        for k, m in given.items():
            if self.size is None:
                self.size = tuple(m.shape)
            if tuple(m.shape) != self.size:
                raise _lib.DmvsError(f"view {view_id}: {k} map of size {tuple(m.shape)} in a scene of {self.size} maps "
                                     "(views of one scene must share one size; fix_res in step 1)")
        ready = self.schedule.arrive(view_id)
        stream = torch.cuda.current_stream(self.device)
        for m in given.values():       # the fused launches run on this stream, whichever stream produced the map
            m.record_stream(stream)
        self.depth[view_id] = given["depth"]
        self.bytes += given["depth"].numel() * 4
        if view_id in self.schedule.sources:         # a reference view: its confidences and image until it is fused
            c3 = given["confidence"]
            # a scalar conf gates the final confidence only (ViewFilter); missing stage maps are the final one
            c2 = c3 if self.scalar_conf else given.get("confidence2", c3)
            c1 = c3 if self.scalar_conf else given.get("confidence1", c3)
            self.conf[view_id] = (c3, c2, c1)
            self.bytes += sum(t.numel() * 4 for t in {id(t): t for t in (c3, c2, c1)}.values())
            self.images[view_id] = image
        self.peak_bytes = max(self.peak_bytes, self.bytes)
        self.cams[view_id] = (np.asarray(cam[0], np.float32), np.asarray(cam[1], np.float32))
        for r in ready:
            self._fuse(r)
        return ready

    def _release_depth(self, v):
        t = self.depth.pop(v, None)
        if t is not None:
            self.bytes -= int(t.numel()) * 4

    # -- one reference view --------------------------------------------------------------------------------------------
    def _fuse(self, ref: int):
        H, W = self.size
        srcs = self.schedule.sources[ref]
        c3, c2, c1 = self.conf.pop(ref)
        stream = torch.cuda.current_stream(self.device)
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = fuse_view(self.depth[ref], self.cams[ref], [self.depth[s] for s in srcs], [self.cams[s] for s in srcs],
                        c3, c2, c1, self.thresholds, self.thres_view, self.dynamic, self.dist, self.rel)
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record(stream)
        self.events.append((e0, e1))
        # fixed-size results back through pinned buffers on this stream; the point count decides the last copy
        h_masks = torch.empty((3, H, W), dtype=torch.uint8, pin_memory=True)
        h_masks.copy_(out["masks"], non_blocking=True)
        h_n = torch.empty(1, dtype=torch.int32, pin_memory=True)
        h_n.copy_(out["count"], non_blocking=True)
        h_avg = None
        if self.dynamic:
            h_avg = torch.empty((H, W), dtype=torch.float32, pin_memory=True)
            h_avg.copy_(out["depth_avg"], non_blocking=True)
        done = torch.cuda.Event()
        done.record(stream)
        if ref == self.schedule.pairs[-1][0]:
            self.last_masks = out["masks"]
        self.results[ref] = self.pool.submit(self._host, ref, done, out["xyz"], h_masks, h_n, h_avg, self.images.pop(ref))
        for v in self.schedule.fuse(ref):
            self._release_depth(v)
        self.bytes -= sum(int(t.numel()) * 4 for t in {id(t): t for t in (c3, c2, c1)}.values())

    def _host(self, ref, done, xyz, h_masks, h_n, h_avg, image) -> _ViewResult:
        done.synchronize()
        n = int(h_n[0])
        h_xyz = torch.empty((n, 3), dtype=torch.float32, pin_memory=True)
        if n:
            s = torch.cuda.Stream(device=self.device)
            with torch.cuda.stream(s):
                h_xyz.copy_(xyz[:n], non_blocking=True)
            s.synchronize()
        img = image.result() if hasattr(image, "result") else image
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 3:
            raise _lib.DmvsError(f"view {ref}: image must be [h,w,3] uint8, got {img.dtype} {img.shape}")
        step = 2 ** (3 - self.num_stage)
        m = h_masks.numpy()
        fm = m[2] != 0
        rgb = (img[1::step, 1::step] if step > 1 else img)[fm]     # == (float32(u8) / 255.0 * 255).astype(uint8)[fm]
        pngs = {kind: png_gray8(m[k]) for k, kind in enumerate(("photo", "geo", "final"))}
        return _ViewResult(h_xyz.numpy(), rgb, pngs, None if h_avg is None else h_avg.numpy())

    # -- output -------------------------------------------------------------------------------------------------------
    def fused_views(self) -> int:
        return len(self.schedule.fused)

    def device_seconds(self) -> float:
        """GPU time of the fused launches so far (events; synchronises)."""
        return sum(a.elapsed_time(b) for a, b in self.events) / 1e3

    def write(self, out_folder: str, plyfilename: str, write_masks: bool = True) -> Dict[str, float]:
        """The files fuse_scene writes and its return value: the mask statistics of the last view in pair order."""
        if not self.schedule.done():
            raise _lib.DmvsError(f"write() before every view is fused: {len(self.schedule.pairs) - self.fused_views()} "
                                 f"view(s) still wait for the maps of view(s) {self.schedule.missing()}")
        try:
            res = [(r, self.results[r].result()) for r, _ in self.schedule.pairs]
            if write_masks:
                os.makedirs(os.path.join(out_folder, "mask"), exist_ok=True)
            for r, out in res:
                if write_masks:
                    for kind, b in out.pngs.items():
                        with open(os.path.join(out_folder, "mask/{:0>8}_{}.png".format(r, kind)), "wb") as f:
                            f.write(b)
                if self.dynamic:
                    save_pfm(os.path.join(out_folder, "depth_est/{:0>8}_averaged.pfm".format(r)), out.depth_averaged)
            write_ply(plyfilename, np.concatenate([o.xyz for _, o in res]), np.concatenate([o.rgb for _, o in res]))
            m = self.last_masks
            # ViewFilter.finish's reductions on the same device: photo / geo / final = count / (H*W) in fp32
            return {"photo": (m[0] != 0).float().mean().item(), "geo": (m[1] != 0).float().mean().item(),
                    "final": (m[2] != 0).float().mean().item()}
        finally:
            self.close()

    def close(self):
        if not self._closed:
            self._closed = True
            self.pool.shutdown(wait=True)
            self.depth.clear()
            self.conf.clear()
            self.images.clear()
