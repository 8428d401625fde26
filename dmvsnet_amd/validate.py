"""Validation mode: the dual-depth regression loss and the depth metrics on ground truth (kernels: csrc/validate.h, "N6").

The counterpart of the reference's other inference-only path, ``Model.validate`` (model.py:215-299): the network runs on the
DTU training-format split (datasets/dtu_yao.py: ground-truth depth and mask per reference view) and five scalars come out:

* ``mvs_loss``                -- drop-in for loss.py:5 in mode "regression": per stage ONE fused pass over depth_sub_plus,
  depth_sub_plus_refine, the ground truth and the mask plus a one-workgroup finishing kernel, added into a device scalar.
* ``AbsDepthError_metrics`` / ``Thres_metrics`` -- tools.py:159-201 on the same kernel (metrics-only call).
* ``DTUValDataset``           -- the sample dict of dtu_yao.MVSDataset.__getitem__.
* ``run_validate``            -- the loop of Model.validate; the per-batch scalars stay on the device until the end.

Not training: no backward, no optimiser.  There is no CPU fallback: CPU tensors raise ``DmvsError``.

Unpinned details (no ``cv2`` and no DTU training data are available to the project):
* ``cv2.resize(..., INTER_NEAREST)`` is restated, not executed: source index ``floor(dst * ratio)``, which for the exact integer
  ratios the format has (2, 4) is a strided slice ``a[::r, ::r]``; every other ratio is refused.
* the cell-centre weights are exactly 1/4 here; the reference's ``grid_sample`` computes them in fp32 from a normalised grid, and
  its cell mask ``grid_sample(mask) >= 1`` equals "all four corners valid" only where those weights sum to >= 1 (checked on the
  CPU reference for the sizes the tests use, tests/golden/make_golden_validate.py).
* ``lights`` (an extension): the reference hard-wires 7 light conditions per view; a tree with fewer can say so.
"""
from __future__ import annotations

import ctypes
import os
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, eval_io
from ._lib import DmvsError

__all__ = ["mvs_loss", "AbsDepthError_metrics", "Thres_metrics", "dual_depth_loss_stage", "DTUValDataset", "run_validate",
           "nearest_resize", "average_scalars", "SCALARS", "DECODE_WORKERS"]

SCALARS = ("loss", "abs_depth_error", "thres2mm_error", "thres4mm_error", "thres8mm_error")   # model.py:253-258
THRES_MM = (2.0, 4.0, 8.0)                                                                   # model.py:246-248
DECODE_WORKERS = 4   # PNG / PFM decode threads; a fixed number, as scan.DECODE_WORKERS

_workspaces: Dict[torch.device, torch.Tensor] = {}


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _plane(t, what, shape=None) -> torch.Tensor:
    """fp32, contiguous, on a HIP device (bool masks become 0 / 1)."""
    if not isinstance(t, torch.Tensor):
        raise DmvsError(f"{what}: expected a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise DmvsError(f"{what} is a CPU tensor: the validation kernels run on a HIP device only (no CPU fallback)")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise DmvsError(f"{what}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t.to(torch.float32).contiguous()


def _workspace(device, B, h, w) -> torch.Tensor:
    n = _lib.load().dmvs_dual_depth_loss_workspace(B, h, w)
    if n < 0:
        _lib.check(int(n), f"dmvs_dual_depth_loss_workspace({B}, {h}, {w})")
    ws = _workspaces.get(device)
    if ws is None or ws.numel() < n:   # grows to the largest stage met; calls on one stream reuse it in order
        ws = _workspaces[device] = torch.empty(int(n), dtype=torch.float64, device=device)
    return ws


def _launch(dsp_main, dsp_refine, gt, mask, depth, weight, thres, total, terms, counts, image_sums, metrics4):
    B, h, w = gt.shape
    dev = gt.device
    th = (ctypes.c_float * 3)(*[float(t) for t in thres]) if depth is not None else None
    with torch.cuda.device(dev):
        ws = _workspace(dev, B, h, w)
        code = _lib.load().dmvs_dual_depth_loss(_ptr(dsp_main), _ptr(dsp_refine), _ptr(gt), _ptr(mask), _ptr(depth), B, h, w,
                                                float(weight), th, _ptr(ws), _ptr(total), _ptr(terms), _ptr(counts),
                                                _ptr(image_sums), _ptr(metrics4),
                                                ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    _lib.check(code, "dmvs_dual_depth_loss")


def dual_depth_loss_stage(dsp_main, dsp_refine, depth_gt, mask, weight=1.0, depth=None, thres=THRES_MM, total=None):
    """One stage with every optional output of the kernel, as device tensors: ``total`` [1] fp32 (``total`` given: added into it),
    ``terms`` [2,8] fp32 (main / refine: the two depth means, var small / huge, the four centre terms), ``counts`` [2] int64
    (n, n_cells), and with ``depth``: ``image_sums`` [B,5] fp64 (sum |depth - gt|, n_valid, n above each threshold) and
    ``metrics`` [4] fp32 (batch means of abs error and the three rates).  ``dsp_main`` = None: metrics only."""
    gt = _plane(depth_gt, "depth_gt")
    if gt.dim() != 3:
        raise DmvsError(f"depth_gt: expected [B,h,w], got {tuple(gt.shape)}")
    B, h, w = gt.shape
    mask = _plane(mask, "mask", gt.shape)
    out = {}
    if dsp_main is not None:
        dsp_main = _plane(dsp_main, "depth_sub_plus", (B, 4, h, w))
        dsp_refine = _plane(dsp_refine, "depth_sub_plus_refine", (B, 4, h, w))
        out["total"] = total if total is not None else torch.zeros(1, dtype=torch.float32, device=gt.device)
        out["terms"] = torch.empty((2, 8), dtype=torch.float32, device=gt.device)
        out["counts"] = torch.empty(2, dtype=torch.int64, device=gt.device)
    if depth is not None:
        depth = _plane(depth, "depth", gt.shape)
        out["image_sums"] = torch.empty((B, 5), dtype=torch.float64, device=gt.device)
        out["metrics"] = torch.empty(4, dtype=torch.float32, device=gt.device)
    _launch(dsp_main, dsp_refine, gt, mask, depth, weight, thres, out.get("total"), out.get("terms"), out.get("counts"),
            out.get("image_sums"), out.get("metrics"))
    return out


def _loss_into(total, inputs, depth_gt_ms, mask_ms, kwargs, depth=None, depth_key=None, metrics4=None):
    """loss.py:6-80, mode "regression": every stage's contribution added into ``total`` [1]; the stage ``depth_key`` also
    computes the metrics of ``depth`` into ``metrics4`` in the same pass."""
    keys = [k for k in inputs.keys() if "stage" in k]
    weights = kwargs.get("dlossw", [1.0 for _ in keys])
    if depth is not None and depth_key not in keys:
        raise DmvsError(f"no {depth_key!r} among the stages {keys}")
    for k in keys:
        stage = inputs[k]
        gt = _plane(depth_gt_ms[k], f"depth_gt_ms[{k!r}]")
        if gt.dim() != 3:
            raise DmvsError(f"depth_gt_ms[{k!r}]: expected [B,h,w], got {tuple(gt.shape)}")
        B, h, w = gt.shape
        mask = _plane(mask_ms[k], f"mask_ms[{k!r}]", gt.shape)
        main = _plane(stage["depth_sub_plus"], f"{k}.depth_sub_plus", (B, 4, h, w))
        refine = _plane(stage["depth_sub_plus_refine"], f"{k}.depth_sub_plus_refine", (B, 4, h, w))
        weight = weights[int(k.replace("stage", "")) - 1]
        with_metrics = depth is not None and k == depth_key
        _launch(main, refine, gt, mask, _plane(depth, "depth", gt.shape) if with_metrics else None, weight, THRES_MM, total,
                None, None, None, metrics4 if with_metrics else None)


def mvs_loss(inputs, depth_gt_ms, mask_ms, mode, **kwargs):
    """Drop-in for the reference's ``mvs_loss`` (loss.py:5) in mode "regression": ``inputs`` the network's output dict (the
    stages are its keys containing "stage", in dict order; each needs ``depth_sub_plus`` and ``depth_sub_plus_refine``
    [B,4,h,w]), ``depth_gt_ms`` / ``mask_ms`` {"stageK": [B,h,w]} (valid where mask > 0.5), ``dlossw`` the stage weights
    (default 1.0 per stage present).  Returns a 0-dim fp32 tensor on the device; nothing is read back.  An empty mask gives
    NaN, as in the reference."""
    if mode != "regression":
        raise NotImplementedError(f"mvs_loss: mode {mode!r} is not implemented (only 'regression', the mode the reference's "
                                  "scripts use)")
    ref = mask_ms["stage1"] if "stage1" in mask_ms else next(iter(mask_ms.values()))
    if not isinstance(ref, torch.Tensor) or not ref.is_cuda:
        raise DmvsError("mvs_loss: CPU tensors; the validation kernels run on a HIP device only (no CPU fallback)")
    total = torch.zeros(1, dtype=torch.float32, device=ref.device)
    _loss_into(total, inputs, depth_gt_ms, mask_ms, kwargs)
    return total[0]


def _metrics(depth_est, depth_gt, mask, thres):
    out = dual_depth_loss_stage(None, None, depth_gt, mask, depth=depth_est, thres=thres)
    return out["metrics"]


@torch.no_grad()
def AbsDepthError_metrics(depth_est, depth_gt, mask):
    """tools.py:176-185 (without its unused ``thres`` band): mean |depth_est - depth_gt| over the valid pixels of each image (an
    empty image counts 0), then the mean over the batch.  ``mask``: bool, or float with valid > 0.5.  0-dim fp32, on the device."""
    return _metrics(depth_est, depth_gt, mask, THRES_MM)[0]


@torch.no_grad()
def Thres_metrics(depth_est, depth_gt, mask, thres):
    """tools.py:188-201: the share of valid pixels with |depth_est - depth_gt| > thres per image (empty: 0), mean over the batch."""
    assert isinstance(thres, (int, float))
    return _metrics(depth_est, depth_gt, mask, (thres, thres, thres))[1]


# ------------------------------------------------------------------------------------------ loader
def nearest_resize(a: np.ndarray, new_w: int, new_h: int) -> np.ndarray:
    """``cv2.resize(a, (new_w, new_h), interpolation=cv2.INTER_NEAREST)`` for the exact integer shrink ratios the DTU training
    format has: source index floor(dst * ratio), i.e. ``a[::ry, ::rx]``.  Any other ratio is refused."""
    h, w = a.shape[:2]
    if new_h < 1 or new_w < 1 or h % new_h or w % new_w:
        raise DmvsError(f"nearest resize {h}x{w} -> {new_h}x{new_w}: not an exact integer ratio (cv2's rule is not guessed)")
    return np.ascontiguousarray(a[::h // new_h, ::w // new_w])


class DTUValDataset(torch.utils.data.Dataset):
    """The reference's DTU training-format loader (datasets/dtu_yao.py:11-193) for validation: same constructor arguments, same
    sample dict -- ``imgs`` [V,3,H,W] fp32 in [0,1], ``proj_matrices`` {"stage1|2|3": [V,2,4,4]} (intrinsics x1 / x2 / x4),
    ``depth`` / ``mask`` {"stage1|2|3": [h,w]} of the reference view at 1/4, 1/2 and full size (raw ground truth / 2 nearest,
    centre crop 512x640, then / 4, / 2, x 1 nearest; mask = depth_visual > 10), ``depth_values`` [ndepths].  Metas: every
    viewpoint of Cameras/pair.txt x ``lights`` light conditions per scan (7 in the dataset).  ``mode``: "val" or "test"."""

    CROP = (512, 640)   # dtu_yao.py:87, hard-wired

    def __init__(self, datapath, listfile, mode, nviews, img_size=None, ndepths=192, interval_scale=1.06, lights=7, **kwargs):
        super().__init__()
        self.img_size = img_size if img_size is not None else [512, 640]
        assert self.img_size[0] % 32 == 0 and self.img_size[1] % 32 == 0, "img_wh must both be multiples of 32!"
        if mode not in ("val", "test"):
            raise DmvsError(f"DTUValDataset: mode {mode!r}; training is out of scope (modes 'val' and 'test')")
        self.datapath, self.listfile, self.mode, self.nviews = datapath, listfile, mode, nviews
        self.ndepths, self.interval_scale, self.lights, self.kwargs = ndepths, interval_scale, int(lights), kwargs
        with open(listfile) as f:
            scans = [line.rstrip() for line in f.readlines()]
        self.metas = []
        for scan in scans:
            with open(os.path.join(datapath, "Cameras/pair.txt")) as f:
                for _ in range(int(f.readline())):
                    ref_view = int(f.readline().rstrip())
                    src_views = [int(x) for x in f.readline().rstrip().split()[1::2]]
                    for light_idx in range(self.lights):
                        self.metas.append((scan, light_idx, ref_view, src_views))

    def __len__(self):
        return len(self.metas)

    def view_ids(self, idx):
        _, _, ref_view, src_views = self.metas[idx]
        return [ref_view] + src_views[:self.nviews - 1]

    def image_path(self, scan, light_idx, vid):
        return os.path.join(self.datapath, "Rectified/{}_train/rect_{:0>3}_{}_r5000.png".format(scan, vid + 1, light_idx))

    def _prepare(self, hr: np.ndarray) -> np.ndarray:
        if hr.ndim != 2:
            raise DmvsError(f"ground-truth plane of shape {hr.shape}: expected [H,W]")
        h, w = hr.shape
        ds = nearest_resize(hr, w // 2, h // 2)
        h, w = ds.shape
        th, tw = self.CROP
        if h < th or w < tw:
            raise DmvsError(f"ground truth {hr.shape[0]}x{hr.shape[1]}: half of it is smaller than the {th}x{tw} crop")
        y0, x0 = (h - th) // 2, (w - tw) // 2
        return ds[y0:y0 + th, x0:x0 + tw]

    @staticmethod
    def _pyramid(a: np.ndarray) -> Dict[str, np.ndarray]:
        h, w = a.shape
        return {"stage1": nearest_resize(a, w // 4, h // 4), "stage2": nearest_resize(a, w // 2, h // 2), "stage3": a}

    def ground_truth(self, scan, vid):
        """({"stageK": depth}, {"stageK": mask}) of one view (dtu_yao.py:97-127)."""
        from PIL import Image
        with Image.open(os.path.join(self.datapath, "Depths_raw/{}/depth_visual_{:0>4}.png".format(scan, vid))) as im:
            m = (np.array(im, dtype=np.float32) > 10).astype(np.float32)
        d = np.array(eval_io.read_pfm(os.path.join(self.datapath, "Depths_raw/{}/depth_map_{:0>4}.pfm".format(scan, vid)))[0],
                     dtype=np.float32)
        return self._pyramid(self._prepare(d)), self._pyramid(self._prepare(m))

    def cameras(self, idx):
        """(proj_matrices {"stageK": [V,2,4,4]}, depth_values [ndepths]) of a sample: no pixels are read."""
        scan, _, _, _ = self.metas[idx]
        projs, depth_values = [], None
        for i, vid in enumerate(self.view_ids(idx)):
            cam = eval_io.CamFile.parse(os.path.join(self.datapath, "Cameras/train/{:0>8}_cam.txt".format(vid)))
            proj_mat = np.zeros((2, 4, 4), dtype=np.float32)
            proj_mat[0, :4, :4] = cam.extrinsics
            proj_mat[1, :3, :3] = cam.intrinsics
            projs.append(proj_mat)
            if i == 0:
                depth_interval = cam.depth_interval * self.interval_scale
                depth_max = depth_interval * self.ndepths + cam.depth_min
                depth_values = np.arange(cam.depth_min, depth_max, depth_interval, dtype=np.float32)
        return eval_io.stage_proj_matrices(np.stack(projs)), depth_values

    def __getitem__(self, idx, with_images=True):
        from PIL import Image
        scan, light_idx, _, _ = self.metas[idx]
        view_ids = self.view_ids(idx)
        proj, depth_values = self.cameras(idx)
        depth_ms, mask_ms = self.ground_truth(scan, view_ids[0])
        sample = {"proj_matrices": proj, "depth": depth_ms, "depth_values": depth_values, "mask": mask_ms}
        if with_images:
            imgs = []
            for vid in view_ids:
                with Image.open(self.image_path(scan, light_idx, vid)) as im:
                    imgs.append(np.array(im, dtype=np.float32) / 255.0)
            sample = {"imgs": np.stack(imgs).transpose([0, 3, 1, 2]), **sample}
        return sample


# ------------------------------------------------------------------------------------------ driver
def average_scalars(rows) -> Dict[str, float]:
    """DictAverageMeter (tools.py:18-37) over per-batch scalar rows: Python floats, added in batch order, divided by the count."""
    acc = [0.0] * len(SCALARS)
    for i, r in enumerate(rows):
        for k, v in enumerate(r):
            acc[k] = float(v) if i == 0 else acc[k] + float(v)
    return {name: acc[k] / len(rows) for k, name in enumerate(SCALARS)}


def _collate(samples, device):
    def up(arrs):
        return torch.from_numpy(np.stack(arrs)).to(device, non_blocking=True)
    out = {"proj_matrices": {k: up([s["proj_matrices"][k] for s in samples]) for k in samples[0]["proj_matrices"]},
           "depth": {k: up([s["depth"][k] for s in samples]) for k in samples[0]["depth"]},
           "mask": {k: up([s["mask"][k] for s in samples]) for k in samples[0]["mask"]},
           "depth_values": up([s["depth_values"] for s in samples])}
    if "imgs" in samples[0]:
        out["imgs"] = up([s["imgs"] for s in samples])
    return out


@torch.no_grad()
def run_validate(network, datapath, listfile, nviews=5, numdepth=192, interval_scale=1.06, dlossw=(0.5, 1.0, 2.0), batch_size=1,
                 device="cuda", feature_cache=False, stats: Optional[dict] = None, lights=7, max_batches: Optional[int] = None,
                 batch_scalars: Optional[list] = None, workers: int = DECODE_WORKERS) -> Dict[str, float]:
    """``Model.validate`` (model.py:215-299) without the logging: the network on every sample of the DTU training-format split
    (``DTUValDataset(datapath, listfile, "val", nviews, ndepths=numdepth, interval_scale=...)``, in order, ``batch_size``
    samples per batch, the last one short), the regression loss with ``dlossw`` and the metrics of ``outputs["depth"]`` against
    the last stage's ground truth.  Returns the ``test_avg`` scalars {"loss", "abs_depth_error", "thres2mm_error",
    "thres4mm_error", "thres8mm_error"}.

    The scalars of a batch are written by the kernels into one device buffer [n_batches][5], copied back once at the end and
    averaged on the host as DictAverageMeter does.  ``batch_size > 1`` pools the loss over the batch's pixels and averages the
    metrics per image, as the reference does.  ``feature_cache`` (True, or a byte budget): every (scan, light, view) image is
    decoded, ingested and run through FeatureNet once (``scan.FeatureCache`` / ``MVSNet.encode_views`` /
    ``forward_features``) instead of once per sample that uses it; the scalars are bit-identical to the default path.
    ``stats`` (a dict, filled in): maps, batches, phases_s (decode: host seconds summed over the pool's threads; h2d, forward
    -- h2d_ingest, encode, forward with the cache -- and loss: device seconds from events) and wall_s; with the cache also
    images, encodes / hits / misses / evictions / peak_bytes, budget.  ``lights`` as in ``DTUValDataset``; ``max_batches``
    stops early (benchmarks); ``batch_scalars`` (a list) receives the per-batch rows [loss, abs, thres2, thres4, thres8]."""
    from . import scan as scan_mod
    device = torch.device(device)
    if device.type != "cuda":
        raise DmvsError("run_validate runs on a HIP device only (no CPU fallback)")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if batch_size < 1:
        raise DmvsError(f"batch_size {batch_size}")
    network.eval()
    num_stage = len(network.ndepths)
    last = "stage{}".format(num_stage)
    ds = DTUValDataset(datapath, listfile, "val", nviews, ndepths=numdepth, interval_scale=interval_scale, lights=lights)
    batches = [list(range(i, min(i + batch_size, len(ds)))) for i in range(0, len(ds), batch_size)]
    if max_batches is not None:
        batches = batches[:max_batches]
    t_start = time.perf_counter()
    phases = scan_mod._Phases(stats is not None)
    cached = feature_cache is not False and feature_cache is not None

    def load(idx):
        t0 = time.perf_counter()
        s = ds.__getitem__(idx, with_images=not cached)
        phases.add("decode", time.perf_counter() - t0)
        return s

    def decode_image(path):
        t0 = time.perf_counter()
        t = scan_mod._decode(path)
        phases.add("decode", time.perf_counter() - t0)
        return t

    with torch.cuda.device(device):
        buf = torch.zeros((max(len(batches), 1), len(SCALARS)), dtype=torch.float32, device=device)
        pool = ThreadPoolExecutor(max_workers=max(1, int(workers)), thread_name_prefix="dmvs-val-decode")
        cache, n_images = None, 0
        try:
            order = [i for b in batches for i in b]
            ahead = 2 * max(1, int(workers))
            pending = {}

            def top_up(pos):
                for i in order[pos:pos + ahead]:
                    if i not in pending:
                        pending[i] = pool.submit(load, i)

            if cached:
                network.prepare(device)
                fp, fdt = hash(network._fingerprint(device)), network.feature_dtype
                tables = scan_mod._Tables(device)
                keys = {i: [(ds.metas[i][0], ds.metas[i][1], v, fp, fdt) for v in ds.view_ids(i)] for i in order}
                n_images = len({k for i in order for k in keys[i]})
                decoded = {}

                def encoder(todo):
                    for k in todo:
                        if k not in decoded:
                            decoded[k] = pool.submit(decode_image, ds.image_path(k[0], k[1], k[2]))
                    hosts = [decoded.pop(k).result() for k in todo]
                    H, W = hosts[0].shape[:2]
                    stack = torch.empty((len(todo), 3, H, W), dtype=torch.float32, device=device)
                    e0 = phases.begin()
                    for j, host in enumerate(hosts):
                        if tuple(host.shape[:2]) != (H, W):
                            raise DmvsError(f"images of different sizes in one scan: {tuple(host.shape[:2])} and {(H, W)}")
                        scan_mod.ingest_chain(host.to(device, non_blocking=True), ((H, W),) * 3, tables, stack[j])
                    phases.end("h2d_ingest", e0)
                    e0 = phases.begin()
                    vals = network.encode_views(stack)
                    phases.end("encode", e0)
                    return vals

                budget = scan_mod.default_budget(device) if feature_cache is True else int(feature_cache)
                cache = scan_mod.FeatureCache(encoder, budget)

            pos = 0
            for bi, idxs in enumerate(batches):
                top_up(pos)
                samples = [pending.pop(i).result() for i in idxs]
                pos += len(idxs)
                top_up(pos)
                e0 = phases.begin()
                data = _collate(samples, device)
                phases.end("h2d", e0)
                if cached:
                    outs = []
                    for j, i in enumerate(idxs):
                        views = cache.fetch(keys[i])
                        e0 = phases.begin()
                        outs.append(network.forward_features(views, {k: v[j:j + 1] for k, v in data["proj_matrices"].items()},
                                                             data["depth_values"][j:j + 1]))
                        phases.end("forward", e0)
                    if len(outs) == 1:
                        outputs = outs[0]
                    else:
                        from .mvsnet import _stack_outputs
                        outputs = _stack_outputs(outs)
                else:
                    e0 = phases.begin()
                    outputs = network(data["imgs"], data["proj_matrices"], data["depth_values"])
                    phases.end("forward", e0)
                e0 = phases.begin()
                _loss_into(buf[bi, 0:1], outputs, data["depth"], data["mask"], {"dlossw": list(dlossw)},
                           depth=outputs["depth"], depth_key=last, metrics4=buf[bi, 1:5])
                phases.end("loss", e0)
        finally:
            pool.shutdown(wait=True)
        rows = buf.cpu().tolist()[:len(batches)]   # the one copy back
    if batch_scalars is not None:
        batch_scalars.extend(rows)
    if stats is not None:
        torch.cuda.synchronize(device)
        stats.update(maps=sum(len(b) for b in batches), batches=len(batches), phases_s=phases.result(),
                     wall_s=time.perf_counter() - t_start)
        if cache is not None:
            stats.update(images=n_images, budget=cache.max_bytes, **cache.stats)
    if not rows:
        raise DmvsError(f"{listfile}: no samples")
    return average_scalars(rows)
