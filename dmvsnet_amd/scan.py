"""Scan-level eval path: every image of a scan is decoded, ingested and run through FeatureNet ONCE, and each depth map runs
``MVSNet.forward_features`` on cached features (opt-in: ``eval_io.save_depth_maps(..., feature_cache=True | bytes)``).

  ScanPlan      what ``eval_io.MVSDataset`` hands the network for every sample of one scan -- view ids, each view's resize
                chain, proj_matrices, depth_values, filename -- computed from the cams and the image headers, no pixels
  FeatureCache  key -> ViewFeatures under a byte budget, least recently used out first; the encoder is injected
  save_depth_maps_cached
                decode (thread pool) -> pinned uint8 -> H2D on a copy stream -> dmvs_image_ingest into a FeatureNet input
                stack -> MVSNet.encode_views -> cache; forward_features per depth map; depth / confidence back through
                pinned buffers; a writer thread writes the PFM / cam / JPEG files.  Same files, same bytes as the default path.
"""
from __future__ import annotations

import io
import os
import queue
import threading
import time
from collections import OrderedDict
from concurrent.futures import Future, ThreadPoolExecutor
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import eval_io, ops
from ._lib import DmvsError

DECODE_WORKERS = 4   # PIL decode threads; a fixed number (the GPU boxes give a command 16 CPUs, whatever the machine has)


# ------------------------------------------------------------------------------------------ plan
@dataclass
class PlanSample:
    view_ids: List[int]
    chains: List[Tuple[Tuple[int, int], Tuple[int, int], Tuple[int, int]]]   # per view: source -> policy -> sample size
    proj_matrices: Dict[str, np.ndarray]     # {"stage1|2|3": [V,2,4,4]}
    depth_values: np.ndarray                 # [ndepths] fp32
    filename: str                            # "<scan>/{}/<ref id>{}"

    @property
    def size(self):
        return self.chains[0][2]


class ScanPlan:
    """``MVSDataset(datapath, [scan], "test", nviews, ndepths, interval_scale, inverse_depth, max_h=, max_w=, fix_res=)``
    without pixels: ``samples[i]`` carries what ``MVSDataset[i]`` returns except the images, plus the resize chain of every
    view.  Each cam file is parsed and each image header read once."""

    def __init__(self, datapath, scan, nviews, ndepths=192, interval_scale=1.06, inverse_depth=False, max_h=1200,
                 max_w=1600, fix_res=False):
        self.datapath, self.scan = datapath, scan
        policy = eval_io.ResizePolicy(max_h, max_w, eval_io.GLOBAL_BASE)
        itv_scale = interval_scale if isinstance(interval_scale, float) else interval_scale[scan]
        cams, self.sizes = {}, {}
        scene_size = "first" if fix_res else None
        self.samples: List[PlanSample] = []
        for ref, srcs in eval_io.read_pairs(os.path.join(datapath, scan, "pair.txt"), nviews):
            view_ids = [ref] + srcs[: nviews - 1]
            chains, projs, depth_values, size = [], [], None, None
            for i, vid in enumerate(view_ids):
                if vid not in cams:
                    cams[vid] = eval_io.CamFile.parse(os.path.join(datapath, "{}/cams/{:0>8}_cam.txt".format(scan, vid)))
                K, E, depth_min, depth_interval = cams[vid].for_network(ndepths, itv_scale)
                src = self.image_size(vid)
                tgt = policy.target(*src)
                K = eval_io.scale_intrinsics(K, src, tgt)
                if scene_size == "first":
                    scene_size = tgt
                if i == 0:
                    size = scene_size if isinstance(scene_size, tuple) else tgt
                    depth_values = eval_io.depth_hypothesis_values(depth_min, depth_interval, ndepths, inverse_depth)
                if tgt != tuple(size):
                    K = eval_io.scale_intrinsics(K, tgt, size)
                chains.append((src, tgt, tuple(size)))
                proj_mat = np.zeros((2, 4, 4), dtype=np.float32)
                proj_mat[0], proj_mat[1, :3, :3] = E, K
                projs.append(proj_mat)
            self.samples.append(PlanSample(view_ids, chains, eval_io.stage_proj_matrices(np.stack(projs)), depth_values,
                                           scan + "/{}/" + "{:0>8}".format(view_ids[0]) + "{}"))

    def image_path(self, vid):
        p = os.path.join(self.datapath, "{}/images_post/{:0>8}.jpg".format(self.scan, vid))
        return p if os.path.exists(p) else os.path.join(self.datapath, "{}/images/{:0>8}.jpg".format(self.scan, vid))

    def image_size(self, vid):
        if vid not in self.sizes:
            from PIL import Image
            with Image.open(self.image_path(vid)) as im:   # header only
                self.sizes[vid] = (im.size[1], im.size[0])
        return self.sizes[vid]


# ------------------------------------------------------------------------------------------ cache
def default_budget(device=None) -> int:
    """min(64 GB, half of the device's free memory)."""
    free, _ = torch.cuda.mem_get_info(device)
    return int(min(64 << 30, free // 2))


class FeatureCache:
    """key -> value (anything with ``nbytes``, e.g. ViewFeatures) under ``max_bytes``, least recently used evicted first.
    ``encoder(keys) -> values`` makes the missing entries; keys are (scan, view id, resize chain, weight fingerprint,
    feature_dtype) in the scan driver.  A value handed out stays valid after its eviction (the caller holds a reference);
    the budget bounds what the cache itself keeps."""

    def __init__(self, encoder: Callable[[list], list], max_bytes: Optional[int] = None):
        self.encoder = encoder
        self.max_bytes = default_budget() if max_bytes is None else int(max_bytes)
        self.entries: "OrderedDict[object, object]" = OrderedDict()
        self.bytes = 0
        self.stats = dict(encodes=0, hits=0, misses=0, evictions=0, peak_bytes=0)
        self._entry_bytes = 0   # size of the last entry encoded: the estimate that bounds look-ahead

    def __contains__(self, key):
        return key in self.entries

    def __len__(self):
        return len(self.entries)

    def fetch(self, keys: Sequence, prefetch: Sequence = ()) -> list:
        """Values of ``keys`` (encoded if absent).  ``prefetch``: keys encoded in the same encoder call while the budget has
        room for them, so that FeatureNet batches stay full.  Counters: ``hits`` / ``misses`` per requested key found / not
        found (a prefetched key counts when it is requested), ``encodes`` per value made (prefetch included)."""
        got = {}
        for k in keys:
            if k in self.entries and k not in got:
                self.entries.move_to_end(k)
                got[k] = self.entries[k]
                self.stats["hits"] += 1
        missing = list(dict.fromkeys(k for k in keys if k not in got))
        extra = []
        for k in dict.fromkeys(prefetch):
            if k in self.entries or k in got or k in missing:
                continue
            if self._entry_bytes and (len(missing) + len(extra) + 1) * self._entry_bytes > self.max_bytes - self._pinned_bytes(got):
                break
            extra.append(k)
        todo = missing + extra
        if todo:
            vals = self.encoder(todo)
            assert len(vals) == len(todo)
            self.stats["encodes"] += len(todo)
            self.stats["misses"] += len(missing)
            for k, v in zip(todo, vals):
                self._entry_bytes = int(v.nbytes)
                if k in missing:
                    got[k] = v
                self._insert(k, v)
        return [got[k] for k in keys]

    def _pinned_bytes(self, got):
        return sum(int(v.nbytes) for v in got.values())

    def _insert(self, key, value):
        self.entries[key] = value
        self.bytes += int(value.nbytes)
        while self.bytes > self.max_bytes and self.entries:
            _, old = self.entries.popitem(last=False)
            self.bytes -= int(old.nbytes)
            self.stats["evictions"] += 1
        self.stats["peak_bytes"] = max(self.stats["peak_bytes"], self.bytes)

    def clear(self):
        self.entries.clear()
        self.bytes = 0


# ------------------------------------------------------------------------------------------ device tables
class _Tables:
    """Per device: the uint8 -> float table and the tap tables of every (n_out, n_in) axis resize met."""

    def __init__(self, device):
        self.device = device
        self.lut = torch.from_numpy(eval_io.u8_to_float_table()).to(device)
        self._taps = {}

    def axis(self, n_out, n_in):
        key = (n_out, n_in)
        if key not in self._taps:
            i0, i1, f = eval_io.resize_taps(n_out, n_in)
            idx = torch.from_numpy(np.stack((i0, i1)).astype(np.int32)).to(self.device)
            wt = torch.from_numpy(np.stack((np.float32(1.0) - f, f))).to(self.device)   # (1.0 - fx) of resize_linear, fp32
            self._taps[key] = (idx, wt)
        return self._taps[key]

    def taps(self, src, dst):
        (h, w), (H, W) = src, dst
        return self.axis(W, w) + self.axis(H, h)


def ingest_chain(img_u8: torch.Tensor, chain, tables: _Tables, out: torch.Tensor) -> torch.Tensor:
    """Decoded image [h,w,3] uint8 (device) -> ``out`` [3,H,W]: MVSDataset's resize chain source -> policy size -> sample
    size (an identity step is skipped, as resize_linear does: two launches at most)."""
    sizes = [chain[0]] + [s for a, s in zip(chain, chain[1:]) if s != a]
    if len(sizes) <= 2:
        return ops.image_ingest(img_u8, *sizes[-1], tables.lut, tables.taps(sizes[0], sizes[-1]), out=out)
    mid = ops.image_ingest(img_u8, *sizes[1], tables.lut, tables.taps(sizes[0], sizes[1]), hwc=True)
    return ops.image_ingest(mid, *sizes[2], None, tables.taps(sizes[1], sizes[2]), out=out)


def _decode(path) -> torch.Tensor:
    from PIL import Image
    with Image.open(path) as im:
        a = np.asarray(im)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise DmvsError(f"{path}: expected an 8-bit RGB image, got {a.dtype} {a.shape}")
    t = torch.empty(a.shape, dtype=torch.uint8, pin_memory=True)
    t.numpy()[...] = a
    return t


class _Phases:
    """Per-phase seconds: host phases summed directly, device phases from event pairs read at the end."""

    def __init__(self, on):
        self.on, self.host, self.dev = on, {}, []
        self.lock = threading.Lock()

    def add(self, name, sec):
        if self.on:
            with self.lock:
                self.host[name] = self.host.get(name, 0.0) + sec

    def begin(self):
        if not self.on:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def end(self, name, e0):
        if e0 is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            self.dev.append((name, e0, e1))

    def result(self):
        out = dict(self.host)
        for name, e0, e1 in self.dev:
            out[name] = out.get(name, 0.0) + e0.elapsed_time(e1) / 1e3
        return out


# ------------------------------------------------------------------------------------------ scan driver
@torch.no_grad()
def save_depth_maps_cached(network, datapath: str, testlist: Sequence[str], outdir: str, num_view: int, max_h: int,
                           max_w: int, numdepth: int = 192, interval_scale: float = 1.06, inverse_depth: bool = False,
                           device="cuda", write_images: bool = True, fix_res: bool = False,
                           scene_cfg: Optional[Dict[str, dict]] = None, max_bytes: Optional[int] = None,
                           stats: Optional[dict] = None, workers: int = DECODE_WORKERS, fusion=None) -> List[str]:
    """``eval_io.save_depth_maps`` on the scan-level path: same arguments, same files with the same bytes, same return value.
    ``max_bytes``: feature-cache budget (None: ``default_budget()``).  ``stats`` (a dict, filled in): maps, images (distinct
    (view, resize chain) pairs), encodes / hits / misses / evictions / peak_bytes of the cache, budget, and with it the
    seconds of each phase (decode, h2d_ingest, encode, forward, d2h, write; device phases from events) and wall.
    ``fusion`` (eval_io.run_test's resident path): ``(begin, end)``; ``begin(scene)`` -> a ``fusion.ScanFusion`` that gets
    every depth / confidence map right after ``forward_features``, still on the device, with the camera as ``write_cam``
    writes it and, as the image, the decoded bytes of the JPEG written; ``end(scene, fz)`` after the scene's last map.
    ``stats`` then also gets fused_views, fusion_peak_bytes and the phases fuse (device) and fuse_write (host)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise DmvsError("the scan-level path runs on a HIP device only")
    if device.index is None:   # "cuda": the current device, where the default path's .to(device) puts its tensors
        device = torch.device("cuda", torch.cuda.current_device())
    if fusion is not None and not write_images:
        raise DmvsError("resident fusion takes its colours from the reference images step 1 writes (write_images=True)")
    network.eval()
    num_stage = len(network.ndepths)
    t_start = time.perf_counter()
    phases = _Phases(stats is not None)
    tables = _Tables(device)
    copy_stream = torch.cuda.Stream(device=device)
    main = torch.cuda.current_stream(device)
    written, n_maps, n_images = [], 0, 0
    errors: list = []
    write_q: "queue.Queue" = queue.Queue(maxsize=8)
    pending: list = []              # image futures handed to fusion, failed on the way out if never filled
    fused_views, fusion_peak = 0, 0

    def writer():
        while True:
            job = write_q.get()
            if job is None:
                return
            if errors:
                if job[-1] is not None:
                    job[-1].set_exception(DmvsError("scan writer stopped after an earlier error"))
                continue
            try:
                t0 = time.perf_counter()
                paths, ev, depth, conf, cam, img, fut = job
                ev.synchronize()
                for p in paths.values():
                    os.makedirs(os.path.dirname(p), exist_ok=True)
                eval_io.save_pfm(paths["depth_est"], depth.numpy())
                eval_io.save_pfm(paths["confidence"], conf.numpy())
                eval_io.write_cam(paths["cams"], cam)
                if img is not None:
                    from PIL import Image
                    a = np.clip(np.transpose(img.numpy(), (1, 2, 0)) * 255, 0, 255).astype(np.uint8)
                    if fut is None:
                        Image.fromarray(a).save(paths["images"])
                    else:   # the same encoder call into memory; fusion gets the pixels fuse_scene would decode
                        buf = io.BytesIO()
                        Image.fromarray(a).save(buf, format="JPEG")
                        with open(paths["images"], "wb") as f:
                            f.write(buf.getvalue())
                        with Image.open(io.BytesIO(buf.getvalue())) as im:
                            fut.set_result(np.asarray(im))
                phases.add("write", time.perf_counter() - t0)
            except BaseException as e:   # re-raised on the main thread
                errors.append(e)
                if fut is not None and not fut.done():
                    fut.set_exception(e)

    def timed_decode(path):
        t0 = time.perf_counter()
        t = _decode(path)
        phases.add("decode", time.perf_counter() - t0)
        return t

    wthread = threading.Thread(target=writer, name="dmvs-scan-writer", daemon=True)
    wthread.start()
    pool = ThreadPoolExecutor(max_workers=max(1, int(workers)), thread_name_prefix="dmvs-scan-decode")
    cache = None
    fz = None
    try:
        for scene in testlist:
            sc = (scene_cfg or {}).get(scene, {})
            plan = ScanPlan(datapath, scene, num_view, numdepth, interval_scale, inverse_depth,
                            sc.get("max_h", max_h), sc.get("max_w", max_w), fix_res)
            fz = fusion[0](scene) if fusion is not None else None
            network.prepare(device)
            fp = hash(network._fingerprint(device))
            fdt = network.feature_dtype
            keyof = lambda vid, chain: (scene, vid, chain, fp, fdt)   # noqa: E731
            skeys = [[keyof(v, c) for v, c in zip(s.view_ids, s.chains)] for s in plan.samples]
            distinct = list(dict.fromkeys(k for ks in skeys for k in ks))
            n_images += len(distinct)
            ref_uses = {}
            for ks in (skeys if write_images else ()):
                ref_uses[ks[0]] = ref_uses.get(ks[0], 0) + 1
            # decode ahead in first-need order; a decoded image is dropped once every key of its view has been ingested
            order = list(dict.fromkeys(k[1] for k in distinct))
            uses = {}
            for k in distinct:
                uses[k[1]] = uses.get(k[1], 0) + 1
            decoded, next_dec, ingested, ref_imgs = {}, [0], set(), {}
            ahead = 2 * max(1, int(workers)) + 8

            def top_up():
                while next_dec[0] < len(order) and sum(1 for v in decoded if uses.get(v, 0) > 0) < ahead:
                    vid = order[next_dec[0]]
                    next_dec[0] += 1
                    if vid not in decoded:
                        decoded[vid] = pool.submit(timed_decode, plan.image_path(vid))

            def encoder(keys):
                top_up()
                H, W = keys[0][2][2]
                if any(k[2][2] != (H, W) for k in keys):   # one input stack per size (fix_res-less mixed scenes)
                    out = {}
                    for sz in dict.fromkeys(k[2][2] for k in keys):
                        part = [k for k in keys if k[2][2] == sz]
                        out.update(zip(part, encoder(part)))
                    return [out[k] for k in keys]
                stack = torch.empty((len(keys), 3, H, W), dtype=torch.float32, device=device)
                e0 = phases.begin()
                for i, k in enumerate(keys):
                    vid = k[1]
                    if vid not in decoded:
                        decoded[vid] = pool.submit(timed_decode, plan.image_path(vid))
                    host = decoded[vid].result()
                    with torch.cuda.stream(copy_stream):
                        dev = host.to(device, non_blocking=True)
                        done = torch.cuda.Event()
                        done.record(copy_stream)
                    main.wait_event(done)
                    dev.record_stream(main)
                    ingest_chain(dev, k[2], tables, stack[i])
                    if k not in ingested:
                        ingested.add(k)
                        uses[vid] -= 1
                        if uses[vid] == 0:
                            decoded.pop(vid, None)
                    if ref_uses.get(k, 0) > 0 and k not in ref_imgs:   # (not again after its last use: re-encodes)
                        ref_imgs[k] = _to_pinned(stack[i])
                phases.end("h2d_ingest", e0)
                top_up()
                e0 = phases.begin()
                vals = network.encode_views(stack)
                phases.end("encode", e0)
                return vals

            if cache is None:
                cache = FeatureCache(encoder, default_budget(device) if max_bytes is None else max_bytes)
            cache.encoder = encoder
            gmax = network._feature_group_max(*plan.samples[0].size) if plan.samples else 1
            for i, s in enumerate(plan.samples):
                # look ahead along the pair order so that FeatureNet batches stay full
                need = [k for k in skeys[i] if k not in cache]
                look = []
                if need:
                    for ks in skeys[i + 1:]:
                        look += [k for k in ks if k not in cache and k not in need and k not in look]
                        if len(need) + len(look) >= gmax:
                            break
                    look = look[:max(0, gmax - len(dict.fromkeys(need)))]
                views = cache.fetch(skeys[i], look)
                proj = {k: torch.from_numpy(v)[None].to(device) for k, v in s.proj_matrices.items()}
                dv = torch.from_numpy(s.depth_values)[None].to(device)
                e0 = phases.begin()
                out = network.forward_features(views, proj, dv)
                phases.end("forward", e0)
                e0 = phases.begin()
                depth = _to_pinned(out["depth"][0])
                conf = _to_pinned(out["photometric_confidence"][0])
                img = None
                if write_images:
                    rk = skeys[i][0]
                    img = ref_imgs.get(rk)
                    ref_uses[rk] -= 1
                    if ref_uses[rk] == 0:
                        ref_imgs.pop(rk, None)
                ev = torch.cuda.Event()
                ev.record(main)
                phases.end("d2h", e0)
                paths = {k: os.path.join(outdir, s.filename.format(k, ext)) for k, ext in
                         (("depth_est", ".pfm"), ("confidence", ".pfm"), ("cams", "_cam.txt"), ("images", ".jpg"))}
                if write_images and img is None:
                    raise DmvsError(f"reference image of {s.filename} was not kept")   # (every reference key is ingested first)
                cam = s.proj_matrices["stage{}".format(num_stage)][0]
                fut = None
                if fz is not None:
                    fut = Future()
                    pending.append(fut)
                    fz.add(s.view_ids[0], out["depth"][0], out["photometric_confidence"][0], as_written_cam(cam), fut)
                write_q.put((paths, ev, depth, conf, cam, img, fut))
                written.append(paths["depth_est"])
                n_maps += 1
                if errors:
                    break
            cache.clear()
            if errors:
                break
            if fz is not None:
                t0 = time.perf_counter()
                fusion[1](scene, fz)
                phases.add("fuse_write", time.perf_counter() - t0)
                fused_views += fz.fused_views()
                fusion_peak = max(fusion_peak, fz.peak_bytes)
                if stats is not None:
                    phases.add("fuse", fz.device_seconds())
                fz = None
    finally:
        write_q.put(None)
        wthread.join()
        pool.shutdown(wait=True)
        for fut in pending:
            if not fut.done():
                fut.set_exception(DmvsError("scan driver stopped before this image was written"))
        if fz is not None:
            fz.close()
    if errors:
        raise errors[0]
    if stats is not None:
        torch.cuda.synchronize(device)
        cs = dict(cache.stats) if cache is not None else dict(encodes=0, hits=0, misses=0, evictions=0, peak_bytes=0)
        stats.update(maps=n_maps, images=n_images, budget=cache.max_bytes if cache is not None else max_bytes, **cs,
                     phases_s=phases.result(), wall_s=time.perf_counter() - t_start)
        if fusion is not None:
            stats.update(fused_views=fused_views, fusion_peak_bytes=fusion_peak)
    return written


def as_written_cam(cam: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """(K [3,3], E [4,4]) of a [2,4,4] cam exactly as fusion.read_camera_parameters reads back what eval_io.write_cam writes
    (``str()`` of each fp32 value, parsed as fp32: the same text, the same parse)."""
    def parse(a):
        return np.array(" ".join(str(v) for v in a.ravel()).split(), dtype=np.float32).reshape(a.shape)
    return parse(cam[1][:3, :3]), parse(cam[0])


def _to_pinned(t: torch.Tensor) -> torch.Tensor:
    """Device tensor -> a pinned host copy, enqueued on the current stream (complete once an event recorded after it is)."""
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t, non_blocking=True)
    return h
