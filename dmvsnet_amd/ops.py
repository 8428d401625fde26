"""Thin Python wrappers over the C ABI (include/dmvs.h): tensors in, kernels enqueued on torch's
current HIP stream, tensors out.  PyTorch is used for device memory and streams only.

Every function requires CUDA(HIP) fp32 contiguous tensors and raises otherwise: there is no CPU path
in the product (the CPU restatement lives in oracle/ and is test infrastructure).

Every launch that is logged and timed goes through ``_launch``: it checks the devices of the weights, hands the timer's start event
back when the launch fails, and writes the launch log and the timer record.  The training wrappers share one workspace cache
(``_workspace``) and one gather-index cache (``_pack_index``); the five ``pack_index_*`` functions share one derivation
(``_derive_index``) and the layers one gather (``gather_packed``).  The five weight-gradient wrappers keep a body each -- its shape
rule, output shape, argument tuple, cost and launch -- around one frame: ``_wgrad_out`` (the buffer) and ``_wgrad_workspace`` (which
the five public getters call too).
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence

import torch

from . import _lib

CONV_S1, CONV_S2, DECONV_S2, CONV2D_K5S2, CONV2D_K1 = 0, 1, 2, 3, 4
RELU, SKIP_UP2, OUT_Q4, IN_VIEWS = 1, 2, 8, 16   # include/dmvs.h (bit value 4 is retired)


class KernelTimer:
    """HIP-event timing of individual kernel launches on torch's current stream (the stream every dmvs
    kernel is enqueued on).  Used by bench.py for the live roofline numbers; off (None) by default."""

    def __init__(self):
        self.records = []   # (family, start_event, end_event, flops, bytes, executed flops)
        self.labels = []    # per record: layer name (or the family)
        self.marks = []     # (label, event)
        self._pool = []

    def _event(self):
        return self._pool.pop() if self._pool else torch.cuda.Event(enable_timing=True)

    def reserve(self, n):
        self._pool.extend(torch.cuda.Event(enable_timing=True) for _ in range(n))

    def begin(self):
        e = self._event()
        e.record()
        return e

    def cancel(self, start):
        """Give back the start event of a launch the kernel declined (it never ran)."""
        self._pool.append(start)

    def end(self, family, start, flops, nbytes, exec_flops=None, label=None):
        """``flops`` = algorithmic (direct-form) FLOPs of the launch; ``exec_flops`` = what its MFMAs actually execute when
        that differs (Winograd layers: 16 products per 2x2 output patch instead of 36); ``label`` = the layer / kernel the launch
        belongs to (bench.py: `roofline.largest_kernel`)."""
        e = self._event()
        e.record()
        self.records.append((family, start, e, flops, nbytes, flops if exec_flops is None else exec_flops))
        self.labels.append(label or family)

    def mark(self, label):
        e = self._event()
        e.record()
        self.marks.append((label, e))

    def summary(self):
        """family -> dict(launches, ms, sum_ms, flops, bytes); call after torch.cuda.synchronize().
        ``ms`` is the family's BUSY time: the union of its launches' [start, end] intervals on the device timeline
        (kernels of the two regularisation branches run concurrently on two streams, so summing durations would
        count the overlap twice); ``sum_ms`` is the plain sum of the launch durations."""
        if not self.records:
            return {}
        base = self.records[0][1]
        per = {}
        for fam, s, e, fl, nb, xf in self.records:
            d = per.setdefault(fam, dict(launches=0, sum_ms=0.0, flops=0.0, bytes=0.0, exec_flops=0.0, iv=[]))
            d["exec_flops"] += xf
            t0, t1 = base.elapsed_time(s), base.elapsed_time(e)
            d["launches"] += 1
            d["sum_ms"] += t1 - t0
            d["flops"] += fl
            d["bytes"] += nb
            d["iv"].append((t0, t1))
        for d in per.values():
            busy, cur0, cur1 = 0.0, None, None
            for t0, t1 in sorted(d.pop("iv")):
                if cur1 is None or t0 > cur1:
                    if cur1 is not None:
                        busy += cur1 - cur0
                    cur0, cur1 = t0, t1
                else:
                    cur1 = max(cur1, t1)
            d["ms"] = busy + (cur1 - cur0 if cur1 is not None else 0.0)
        return per

    def by_label(self):
        """label -> dict(launches, sum_ms, flops, exec_flops, bytes): plain sums of the launch durations per layer name."""
        out = {}
        for (fam, s, e, fl, nb, xf), lab in zip(self.records, self.labels):
            d = out.setdefault(lab, dict(family=fam, launches=0, sum_ms=0.0, flops=0.0, exec_flops=0.0, bytes=0.0))
            d["launches"] += 1
            d["sum_ms"] += s.elapsed_time(e)
            d["flops"] += fl
            d["exec_flops"] += xf
            d["bytes"] += nb
        return out

    def spans(self):
        """Elapsed ms between consecutive marks, summed per label of the span's START mark."""
        out = {}
        for (la, ea), (_, eb) in zip(self.marks[:-1], self.marks[1:]):
            out[la] = out.get(la, 0.0) + ea.elapsed_time(eb)
        return out


timer: Optional[KernelTimer] = None
# Optional launch log (profiling tooling): the family name of every K1..K4 launch, in host order, since it was set to
# a list.  scripts/pmc_summary.py joins it with rocprofv3's dispatch order to attribute PMC counters per family
# (kernel names alone cannot tell a FeatureNet launch of the MFMA conv kernel from a regularisation launch).
launch_log: Optional[list] = None


def _log(family: str) -> None:
    if launch_log is not None:
        launch_log.append(family)


def mark(label: str) -> None:
    if timer is not None:
        timer.mark(label)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _req(*ts: torch.Tensor) -> None:
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.DmvsError("dmvsnet_amd kernels need tensors on a HIP device (no CPU fallback); got "
                                 f"{t.device}")
        if t.dtype != torch.float32:
            raise RuntimeError(f"expected float32 tensor, got {t.dtype}")  # same class the reference raises
        if not t.is_contiguous():
            raise _lib.DmvsError("non-contiguous tensor passed to a dmvs kernel")


def _launch(fn, args, name: str, kernel: str, x: torch.Tensor, weights, decline: bool, family: str, cost, label=None) -> bool:
    """Launch ``fn(*args, stream)``, logged and timed.  ``weights``: tensors the kernel reads by raw pointer besides the activations
    ``x`` (one left on the CPU / another GPU would fault): they must be on x's device.  ``cost`` = (flops, bytes, executed flops) of
    the timer record, None while no timer is set.  With ``decline``, DMVS_EUNSUPPORTED (the kernel does not cover the call) returns
    False: nothing ran, nothing is logged or timed.  Every other failure raises."""
    dev = x.get_device()   # (cheaper than comparing torch.device objects: this runs for every conv launch)
    for t in weights:
        if t is not None and t.get_device() != dev:
            raise _lib.DmvsError(f"layer {name}: weights on {t.device}, activations on {x.device}")
    t0 = timer.begin() if timer is not None else None
    code = fn(*args, _stream())
    if code:
        if t0 is not None:
            timer.cancel(t0)
        if decline and code == _lib.EUNSUPPORTED:
            return False
        _lib.check(code, f"{kernel}[{name}]")
    if launch_log is not None:   # (_log, inline: this runs for every launch)
        launch_log.append(family)
    if t0 is not None:
        timer.end(family, t0, *cost, label=label or name)
    return True


# ------------------------------------------------------------------------------------------ layout
def nchw_to_hwc(src: torch.Tensor, c0: int, C: int) -> torch.Tensor:
    """src [1,Ct,H,W] or [Ct,H,W] -> [H,W,C] of channels c0..c0+C."""
    _req(src)
    Ct, H, W = src.shape[-3:]
    assert 0 <= c0 and c0 + C <= Ct
    dst = torch.empty((H, W, C), dtype=torch.float32, device=src.device)
    _lib.check(_lib.load().dmvs_nchw_to_hwc(_ptr(src), c0, C, H, W, _ptr(dst), _stream()), "dmvs_nchw_to_hwc")
    return dst


def planar_to_hwc(stack: torch.Tensor, view: int, c0: int, C: int) -> torch.Tensor:
    """stack [Ct,V,H,W] (views as depth slices) -> [H,W,C] of channels c0..c0+C of one view."""
    _req(stack)
    Ct, V, H, W = stack.shape
    assert 0 <= c0 and c0 + C <= Ct and 0 <= view < V
    dst = torch.empty((H, W, C), dtype=torch.float32, device=stack.device)
    src = ctypes.c_void_p(stack.data_ptr() + view * H * W * 4)
    _lib.check(_lib.load().dmvs_planar_to_hwc(src, V * H * W, c0, C, H, W, _ptr(dst), _stream()), "dmvs_planar_to_hwc")
    return dst


def image_ingest(src: torch.Tensor, H: int, W: int, lut: Optional[torch.Tensor] = None, taps=None,
                 out: Optional[torch.Tensor] = None, hwc: bool = False) -> torch.Tensor:
    """Decoded image src [h,w,3] (uint8 with ``lut`` [256] fp32, or fp32) -> [3,H,W] planes (``hwc``: [H,W,3]) in ``out``
    (e.g. one slot of a [n,3,H,W] FeatureNet input stack; allocated if None).  ``taps`` = (tx_idx [2,W] int32, tx_wt [2,W],
    ty_idx [2,H] int32, ty_wt [2,H]) device tables of eval_io.resize_taps; unused when (h, w) == (H, W).  Layout glue: the
    launch is not logged."""
    if not src.is_cuda or not src.is_contiguous() or src.dim() != 3 or src.shape[2] != 3:
        raise _lib.DmvsError(f"image_ingest: src must be a contiguous [h,w,3] HIP tensor, got {tuple(src.shape)} on {src.device}")
    u8 = src.dtype == torch.uint8
    if not u8 and src.dtype != torch.float32:
        raise _lib.DmvsError(f"image_ingest: src must be uint8 or float32, not {src.dtype}")
    if u8:
        _req(lut)
        assert lut.numel() == 256
    h, w = src.shape[:2]
    shape = (H, W, 3) if hwc else (3, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=src.device)
    _req(out)
    assert tuple(out.shape) == shape, (tuple(out.shape), shape)
    tx_i = tx_w = ty_i = ty_w = None
    if (h, w) != (H, W):
        tx_i, tx_w, ty_i, ty_w = taps
        _req(tx_w, ty_w)
        for t, n in ((tx_i, W), (ty_i, H)):
            if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (2, n)):
                raise _lib.DmvsError("image_ingest: tap indices must be contiguous [2,n] int32 HIP tensors")
        assert tuple(tx_w.shape) == (2, W) and tuple(ty_w.shape) == (2, H)
    _lib.check(_lib.load().dmvs_image_ingest(_ptr(src), int(u8), h, w, _ptr(lut) if u8 else None, _ptr(tx_i), _ptr(tx_w),
                                             _ptr(ty_i), _ptr(ty_w), H, W, _ptr(out), int(hwc), _stream()),
               "dmvs_image_ingest")
    return out


def relative_proj(proj_pairs: torch.Tensor) -> torch.Tensor:
    """proj_pairs [V,2,4,4] -> [V-1,12] (rot 9 + trans 3 of src @ inv(ref))."""
    _req(proj_pairs)
    V = proj_pairs.shape[0]
    out = torch.empty((V - 1, 12), dtype=torch.float32, device=proj_pairs.device)
    _lib.check(_lib.load().dmvs_relative_proj(_ptr(proj_pairs), V, _ptr(out), _stream()), "dmvs_relative_proj")
    return out


# ------------------------------------------------------------------------------------------ hypotheses
@dataclass
class AffinePlanes:
    """Linear-depth hypothesis planes in affine form: plane d = base + d * step, d < D.
    ``base`` [H,W]; ``step`` 0-dim device tensor (the stage's interval).  K1 / K4 take it instead of a [D,H,W] volume."""
    base: torch.Tensor
    step: torch.Tensor
    D: int

    @property
    def shape(self):
        return (self.D,) + tuple(self.base.shape)

    @property
    def device(self):
        return self.base.device

    def rows(self, r0: int, r1: int) -> "AffinePlanes":
        return AffinePlanes(self.base[r0:r1].contiguous(), self.step, self.D)

    def volume(self) -> torch.Tensor:
        """The [D,H,W] tensor the reference materialises (same rounding as the kernels: d * step, then + base)."""
        d = torch.arange(self.D, dtype=torch.float32, device=self.base.device).view(-1, 1, 1)
        return self.base[None] + d * self.step


def planes_rows(planes, r0: int, r1: int):
    return planes.rows(r0, r1) if isinstance(planes, AffinePlanes) else planes[:, r0:r1].contiguous()


def hypotheses_first(depth_values: torch.Tensor, D: int, H: int, W: int, inverse: bool, affine: bool = False):
    """-> (planes [D,H,W] or, with ``affine`` (linear sampling only), AffinePlanes; interval)."""
    _req(depth_values)
    n = depth_values.shape[-1]
    itv = torch.empty((), dtype=torch.float32, device=depth_values.device)
    if affine and not inverse:
        base = torch.empty((H, W), dtype=torch.float32, device=depth_values.device)
        _lib.check(_lib.load().dmvs_hypothesis_base_first(_ptr(depth_values), n, D, H, W, _ptr(base), _ptr(itv), _stream()),
                   "dmvs_hypothesis_base_first")
        return AffinePlanes(base, itv, D), itv
    out = torch.empty((D, H, W), dtype=torch.float32, device=depth_values.device)
    _lib.check(_lib.load().dmvs_hypotheses_first(_ptr(depth_values), n, D, H, W, int(inverse), _ptr(out), _ptr(itv),
                                                 _stream()), "dmvs_hypotheses_first")
    return out, itv


def hypotheses_next(last_depth: torch.Tensor, depth_values: torch.Tensor, ratio: float, D: int, inverse: bool,
                    affine: bool = False, up: int = 2):
    """last_depth [h,w] -> planes [D,up*h,up*w] (or AffinePlanes) + interval.  ``up`` = 2: the reference's x2 resize
    between stages; 1: a same-resolution transition (pyramids deeper than three stages, an extension)."""
    _req(last_depth, depth_values)
    h, w = last_depth.shape[-2:]
    n = depth_values.shape[-1]
    itv = torch.empty((), dtype=torch.float32, device=last_depth.device)
    base_only = affine and not inverse
    out = torch.empty(((up * h, up * w) if base_only else (D, up * h, up * w)), dtype=torch.float32, device=last_depth.device)
    _lib.check(_lib.load().dmvs_hypotheses_next_up(_ptr(last_depth), h, w, int(up), _ptr(depth_values), n, float(ratio), D,
                                                   int(inverse), int(base_only), _ptr(out), _ptr(itv), _stream()),
               "dmvs_hypotheses_next_up")
    return (AffinePlanes(out, itv, D) if base_only else out), itv


# ------------------------------------------------------------------------------------------ K1
def hwc_to_q4(f_hwc: torch.Tensor) -> torch.Tensor:
    """[H,W,C] pixel-major -> [C/4,H,W,4] quad-planar (the layout K1's product kernel samples; layout glue for tests and
    tools -- FeatureNet's output epilogue writes quad-planar directly)."""
    H, W, C = f_hwc.shape
    return f_hwc.view(H, W, C // 4, 4).permute(2, 0, 1, 3).contiguous()


def nchw_to_q4(src: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src [C,H,W] planar (one sample of a torch feature map; may be a channel slice of a wider map, e.g. a ``split`` half:
    rows contiguous, any channel stride) -> [C/4,H,W,4] quad-planar.  Layout glue: the launch is not logged."""
    if not src.is_cuda:
        raise _lib.DmvsError(f"dmvsnet_amd kernels need tensors on a HIP device (no CPU fallback); got {src.device}")
    if src.dtype != torch.float32 or src.dim() != 3:
        raise _lib.DmvsError(f"nchw_to_q4: expected a float32 [C,H,W] map, got {src.dtype} {tuple(src.shape)}")
    C, H, W = src.shape
    if src.stride(2) != 1 or src.stride(1) != W or src.stride(0) < H * W:
        src = src.contiguous()
    dst = torch.empty((C // 4, H, W, 4), dtype=torch.float32, device=src.device) if out is None else out
    _req(dst)
    assert tuple(dst.shape) == (C // 4, H, W, 4), tuple(dst.shape)
    _lib.check(_lib.load().dmvs_nchw_to_q4(_ptr(src), src.stride(0), 0, C, H, W, _ptr(dst), _stream()), "dmvs_nchw_to_q4")
    return dst


def _warp_corr_backward(what: str, ref_q4, src_q4, proj12, depth_dhw, gsim, gref, gsrc, workspace, variant: int, det: bool,
                        presum: Optional[tuple] = None) -> None:
    """Both modes of K1b: validation (errors name the public function ``what``), the two pointer arrays and the call.  ``presum``:
    None, or ``(path_counts,)`` for the pre-summed scatter's entry, which takes the mode as an argument."""
    src_q4, gsrc = list(src_q4), list(gsrc)
    live = [g for g in gsrc if g is not None]
    if depth_dhw.dim() != 3 or ref_q4.dim() != 4 or ref_q4.shape[-1] != 4:
        raise _lib.DmvsError(f"{what}: depth must be [D,H,W] and the features quad-planar [C/4,H,W,4]")
    D, H, W = depth_dhw.shape
    C = 4 * ref_q4.shape[0]
    nsrc = len(src_q4)
    if len(gsrc) != nsrc or proj12.dim() != 2 or tuple(proj12.shape) != (nsrc, 12) or tuple(gsim.shape) != (2, D, H, W):
        raise _lib.DmvsError(f"{what}: {nsrc} source views need {nsrc} gsrc entries, proj12 [{nsrc},12] and gsim "
                             f"{(2, D, H, W)}; got {len(gsrc)}, {tuple(proj12.shape)}, {tuple(gsim.shape)}")
    for s in (ref_q4, *src_q4):
        if tuple(s.shape) != (C // 4, H, W, 4):
            raise _lib.DmvsError(f"{what}: feature map {tuple(s.shape)}, expected {(C // 4, H, W, 4)}")
    for g in (gref, *live):
        if g is not None and tuple(g.shape) != (C, H, W):
            raise _lib.DmvsError(f"{what}: gradient {tuple(g.shape)}, expected {(C, H, W)}")
    counts = None
    if presum is not None:   # what needs no device is refused before a device is asked for
        counts, = presum
        if int(variant) not in (0, 1, 2, 3):
            raise _lib.DmvsError(f"{what}: variant must be 0..3 (bit 0: decomposition, bit 1: test capacity), got {variant}")
        if det and live and workspace is not None and workspace.numel() * 8 < warp_corr_backward_det_workspace(C, H, W, len(live)):
            raise _lib.DmvsError(f"{what}: a workspace of {workspace.numel() * 8} bytes, {len(live)} wanted views need "
                                 f"{warp_corr_backward_det_workspace(C, H, W, len(live))}")
        if counts is not None and not (counts.dtype == torch.int32 and counts.numel() == 3 and counts.is_contiguous()):
            raise _lib.DmvsError(f"{what}: path_counts must be three contiguous int32 words (windowed, direct, empty)")
    _req(ref_q4, proj12, depth_dhw, gsim, gref, *src_q4, *live)
    if counts is not None and not counts.is_cuda:
        raise _lib.DmvsError(f"{what}: path_counts must be on the HIP device")
    if gref is None and not live:
        return
    args = [_ptr(ref_q4), (ctypes.c_void_p * nsrc)(*[s.data_ptr() for s in src_q4]), nsrc, _ptr(proj12), _ptr(depth_dhw), _ptr(gsim),
            _ptr(gref), (ctypes.c_void_p * nsrc)(*[None if g is None else g.data_ptr() for g in gsrc]), C, D, H, W]
    if presum is not None:
        args.append(int(det))
    if det:
        if live and workspace is None:
            need = warp_corr_backward_det_workspace(C, H, W, len(live))
            workspace = torch.empty((need // 8,), dtype=torch.int64, device=ref_q4.device)
        nbytes = 0
        if workspace is not None:
            if not (workspace.is_cuda and workspace.dtype == torch.int64 and workspace.is_contiguous()):
                raise _lib.DmvsError(f"{what}: the workspace must be a contiguous int64 HIP tensor")
            nbytes = workspace.numel() * 8
        args += [_ptr(workspace), nbytes, int(variant)]
    elif presum is not None:
        args += [None, 0, int(variant)]
    if presum is not None:
        args.append(_ptr(counts))
    _lib.check(getattr(_lib.load(), "dmvs_" + what)(*args, _stream()), "dmvs_" + what)


def warp_corr_backward(ref_q4: torch.Tensor, src_q4: Sequence[torch.Tensor], proj12: torch.Tensor, depth_dhw: torch.Tensor,
                       gsim: torch.Tensor, gref: Optional[torch.Tensor], gsrc: Sequence[Optional[torch.Tensor]]) -> None:
    """K1b.  Quad-planar features, gsim [2,D,H,W]; writes gref [C,H,W] (or None: skipped) and ADDS into the gsrc[v] [C,H,W]
    (zero-initialised by the caller; None: that view is skipped).  Not logged as a launch family."""
    _warp_corr_backward("warp_corr_backward", ref_q4, src_q4, proj12, depth_dhw, gsim, gref, gsrc, None, 0, False)


def warp_corr_backward_det_workspace(C: int, H: int, W: int, nact: int) -> int:
    """Bytes of the int64 workspace of ``warp_corr_backward_det`` for ``nact`` wanted source views."""
    return int(_lib.load().dmvs_warp_corr_backward_det_workspace(C, H, W, nact))


def warp_corr_backward_det(ref_q4: torch.Tensor, src_q4: Sequence[torch.Tensor], proj12: torch.Tensor, depth_dhw: torch.Tensor,
                           gsim: torch.Tensor, gref: Optional[torch.Tensor], gsrc: Sequence[Optional[torch.Tensor]],
                           workspace: Optional[torch.Tensor] = None, variant: int = 0) -> None:
    """K1b in deterministic mode: as ``warp_corr_backward``, but the source gradients are accumulated in fixed point (order-free:
    a pure function of the inputs) and every wanted gsrc[v] is WRITTEN, so it needs no zero fill.  ``workspace``: a contiguous
    int64 HIP tensor of at least ``warp_corr_backward_det_workspace(C, H, W, nact) / 8`` elements (allocated when None; the
    kernels clear it).  ``variant``: launch-configuration knob (0 default, 1 another decomposition, the same bits).  Not logged as
    a launch family."""
    _warp_corr_backward("warp_corr_backward_det", ref_q4, src_q4, proj12, depth_dhw, gsim, gref, gsrc, workspace, variant, True)


def warp_corr_backward_presum_cap(C: int, deterministic: bool, variant: int = 0) -> int:
    """Texels an LDS window of ``warp_corr_backward_presum`` holds: a workgroup whose taps span more falls back to global adds."""
    return int(_lib.load().dmvs_warp_corr_backward_presum_cap(C, int(bool(deterministic)), int(variant)))


def warp_corr_backward_presum(ref_q4: torch.Tensor, src_q4: Sequence[torch.Tensor], proj12: torch.Tensor, depth_dhw: torch.Tensor,
                              gsim: torch.Tensor, gref: Optional[torch.Tensor], gsrc: Sequence[Optional[torch.Tensor]],
                              deterministic: bool = False, workspace: Optional[torch.Tensor] = None, variant: int = 0,
                              path_counts: Optional[torch.Tensor] = None) -> None:
    """K1b with the pre-summed source scatter: a workgroup sums its addends in an LDS window over the bounding box of its taps and
    issues one global add per window element (a box above ``warp_corr_backward_presum_cap`` texels falls back to the plain
    scatter's adds).  ``deterministic=False``: as ``warp_corr_backward`` (ADDS into zeroed gsrc; the same addends, another order of
    the fp32 sum); True: as ``warp_corr_backward_det`` (``workspace``; every wanted gsrc WRITTEN; the same bits).  ``variant``: bit 0
    the other decomposition, bit 1 a test capacity of 256 texels.  ``path_counts``: three zeroed int32 words on the device, to which
    the workgroups add how many took the window, fell back, had no tap inside.  Not logged as a launch family."""
    _warp_corr_backward("warp_corr_backward_presum", ref_q4, src_q4, proj12, depth_dhw, gsim, gref, gsrc,
                        workspace if deterministic else None, variant, bool(deterministic), presum=(path_counts,))


def warp_corr(ref: torch.Tensor, src: Sequence[torch.Tensor], proj12: torch.Tensor, depth_dhw: torch.Tensor,
              out: Optional[torch.Tensor] = None, accumulate: bool = False, C: Optional[int] = None,
              pix_stride: Optional[int] = None, variant: int = 0, family: str = "warp_corr",
              layout: Optional[str] = None) -> torch.Tensor:
    """K1.  Features quad-planar [C/4,H,W,4] (``layout="q4"``: the product kernel) or pixel-major [H,W,pix_stride]
    (``"hwc"``: the generic kernel); by default told apart by the trailing dimension (4 = quad-planar; a 4-channel
    pixel-major map does not exist in this network).  proj12 [nsrc,12], depth [D,H,W] (or AffinePlanes) -> sim [2,D,H,W].
    ``variant``: launch-configuration knob of the q4 kernel (0 = default; see dmvs_warp_corr_q4), an explicit argument
    of the C entry point -- no process-wide state."""
    affine = isinstance(depth_dhw, AffinePlanes)
    f16 = ref.dtype == torch.float16      # fp16 FEATURES (extension, q4 layout only); everything else stays fp32
    if f16:
        for t in (ref, *src):
            if not (t.is_cuda and t.dtype == torch.float16 and t.is_contiguous()):
                raise _lib.DmvsError("fp16 features: every view must be a contiguous float16 HIP tensor")
    if affine:
        _req(proj12, depth_dhw.base, depth_dhw.step, *(() if f16 else (ref, *src)))
    else:
        _req(proj12, depth_dhw, *(() if f16 else (ref, *src)))
    D, H, W = depth_dhw.shape
    if layout is None:
        layout = "q4" if (ref.dim() == 4 and ref.shape[-1] == 4) else "hwc"
    if f16 and layout != "q4":
        raise _lib.DmvsError("fp16 features are a quad-planar (q4) extension; the pixel-major kernel is fp32 only")
    if layout == "q4":
        assert ref.dim() == 4 and tuple(ref.shape[1:]) == (H, W, 4), (tuple(ref.shape), (H, W))
        C = 4 * ref.shape[0]
    else:
        pix_stride = ref.shape[-1] if pix_stride is None else pix_stride
        C = pix_stride if C is None else C
    nsrc = len(src)
    if out is None:
        out = torch.empty((2, D, H, W), dtype=torch.float32, device=ref.device)
        assert not accumulate
    if nsrc == 0:  # a view shard with no local source view contributes zeros
        if not accumulate:
            out.zero_()
        return out
    assert proj12.shape[0] == nsrc
    arr = (ctypes.c_void_p * nsrc)(*[s.data_ptr() for s in src])
    lib = _lib.load()
    if layout == "q4":
        fn, kernel = (lib.dmvs_warp_corr_q4_f16 if f16 else lib.dmvs_warp_corr_q4), "dmvs_warp_corr_q4"
        args = (_ptr(ref), arr, nsrc, _ptr(proj12), None if affine else _ptr(depth_dhw), _ptr(depth_dhw.base) if affine else None,
                _ptr(depth_dhw.step) if affine else None, _ptr(out), C, D, H, W, int(accumulate), int(variant))
    elif affine:
        fn, kernel = lib.dmvs_warp_corr_affine, "dmvs_warp_corr_affine"
        args = (_ptr(ref), arr, nsrc, pix_stride, _ptr(proj12), _ptr(depth_dhw.base), _ptr(depth_dhw.step), _ptr(out), C, D, H, W,
                int(accumulate))
    else:
        fn, kernel = lib.dmvs_warp_corr, "dmvs_warp_corr"
        args = (_ptr(ref), arr, nsrc, pix_stride, _ptr(proj12), _ptr(depth_dhw), _ptr(out), C, D, H, W, int(accumulate))
    cost = None
    if timer is not None:
        # algorithmic bytes: features once, similarity volume written once, hypotheses once -- the [D,H,W] volume, or
        # only the [H,W] base plane when the affine form is used (count what is actually read)
        hyp = H * W if affine else D * H * W
        cost = (nsrc * D * H * W * (10.0 * C + 25), (2.0 if f16 else 4.0) * (nsrc + 1) * C * H * W + 4.0 * (2 * D * H * W + hyp), None)
    _launch(fn, args, family, kernel, ref, (), False, family, cost)
    return out


# ------------------------------------------------------------------------------------------ K2 / K3
@dataclass
class ConvLayer:
    """One packed conv layer of the regularisation net (weights already on the device)."""
    name: str
    mode: int            # CONV_S1 / CONV_S2 / DECONV_S2
    kdepth: int          # 3, or 1 for the 2D bottleneck layers of the refine net
    cin: int
    cout: int
    w_direct: Optional[torch.Tensor]    # [taps][Cin][Cout] (None: K3-only layer)
    w_mfma: Optional[torch.Tensor]      # MFMA A-fragment order, or None if the shape is not supported by K3
    scale: Optional[torch.Tensor]       # BN folded: gamma / sqrt(var + eps)
    shift: Optional[torch.Tensor]       # beta - mean * scale
    relu: bool
    w_wino: Optional[torch.Tensor] = None   # Winograd F(2x2,3x3) weights (stride-1 3x3 layers K3w is compiled for)
    w_wino_fpn: Optional[torch.Tensor] = None   # out3 only: composite filters of the fused level-3 merge (pack_wino_fpn)
    ones: dict = field(default_factory=dict)    # out3 only: device -> [constant-one buffers, the last one the largest] (see _ones_hw)
    w_c8: Optional[torch.Tensor] = None     # FeatureNet conv0.0 / conv0.1 only: K3s weights (pack_c8; Cin 3 or 8 -> 8)
    w_coarse: Optional[torch.Tensor] = None  # conv4 / conv6 (3D and 2D forms): K3r register-stationary Winograd weights (pack_coarse)
    w_split: Optional[torch.Tensor] = None   # conv1 only: bf16 terms for the split PROBE (pack_split); never used by `auto`
    w_zmarch: Optional[torch.Tensor] = None  # conv2 (16 -> 16, 3x3x3): K3z z-marching register-stationary Winograd weights (pack_zmarch)

    def out_shape(self, D, H, W):
        if self.mode in (CONV_S1, CONV2D_K1):
            return D, H, W
        if self.mode == CONV2D_K5S2:
            return D, (H + 1) // 2, (W + 1) // 2
        if self.mode == CONV_S2:
            return ((D + 1) // 2 if self.kdepth == 3 else D), (H + 1) // 2, (W + 1) // 2
        return (2 * D if self.kdepth == 3 else D), 2 * H, 2 * W


def pack_direct(w: torch.Tensor, transposed: bool) -> torch.Tensor:
    """PyTorch conv weight -> [kd][kh][kw][Cin][Cout] (2D weights are treated as kd=1)."""
    if w.dim() == 4:
        w = w.unsqueeze(2)
    if transposed:  # [Cin][Cout][k..] -> taps, Cin, Cout
        return w.permute(2, 3, 4, 0, 1).contiguous()
    return w.permute(2, 3, 4, 1, 0).contiguous()


def _pack(floats: str, pack: str, ws: Sequence[torch.Tensor], *shape: int) -> Optional[torch.Tensor]:
    """Host-side packing through the library: ``floats(*shape)`` is the packed length (<= 0: the kernel does not compile the
    shape -> None), ``pack(*ws, out, *shape)`` writes it."""
    lib = _lib.load()
    n = getattr(lib, floats)(*shape)
    if n <= 0:
        return None
    wc = [w.detach().to("cpu", torch.float32).contiguous() for w in ws]
    out = torch.empty(n, dtype=torch.float32)
    _lib.check(getattr(lib, pack)(*(ctypes.c_void_p(w.data_ptr()) for w in wc), ctypes.c_void_p(out.data_ptr()), *shape), pack)
    return out


def pack_mfma(w: torch.Tensor, cin: int, cout: int, mode: int, kdepth: int) -> Optional[torch.Tensor]:
    """Host-side packing into K3's fragment order via the library; None if K3 does not cover the shape."""
    return _pack("dmvs_conv3d_mfma_weight_floats", "dmvs_pack_conv_weights_mfma", (w,), cin, cout, mode, kdepth)


def pack_wino(w: torch.Tensor, cin: int, cout: int, kdepth: int) -> Optional[torch.Tensor]:
    """Host-side G g G^T transform + packing for K3w (csrc/conv3d_wino.hip); None if the layer shape is not compiled."""
    return _pack("dmvs_conv3d_wino_weight_floats", "dmvs_pack_conv_weights_wino", (w,), cin, cout, kdepth)


def pack_coarse(w: torch.Tensor, cin: int, cout: int, kdepth: int) -> Optional[torch.Tensor]:
    """Host-side G g G^T transform + packing for K3r (csrc/conv3d_coarse.hip: the coarse-level conv4 / conv6 with the
    filters held in registers); None if the layer shape is not compiled."""
    return _pack("dmvs_conv3d_coarse_weight_floats", "dmvs_pack_conv_weights_coarse", (w,), cin, cout, kdepth)


def pack_zmarch(w: torch.Tensor, cin: int, cout: int, kdepth: int) -> Optional[torch.Tensor]:
    """Host-side G g G^T transform + packing for K3z (csrc/conv3d_zmarch.hip: conv2 marching along z with the filters held in
    registers); None if the layer shape is not compiled."""
    return _pack("dmvs_conv3d_zmarch_weight_floats", "dmvs_pack_conv_weights_zmarch", (w,), cin, cout, kdepth)


def pack_split(w: torch.Tensor) -> Optional[torch.Tensor]:
    """conv1 weight [16, 8, 3, 3, 3] -> three bf16 terms in MFMA B-operand order for the bf16-split PROBE
    (csrc/conv3d_split.hip; never part of the product's dispatch); None for any other shape."""
    if tuple(w.shape) != (16, 8, 3, 3, 3):
        return None
    return _pack("dmvs_conv3d_split_weight_floats", "dmvs_pack_conv_weights_split", (w,), 8, 16)


def pack_c8(w: torch.Tensor) -> Optional[torch.Tensor]:
    """nn.Conv2d weight [8, Cin, 3, 3] -> K3s operand order (csrc/conv2d_c8.hip); None for any other shape."""
    if w.dim() != 4 or w.shape[0] != 8 or tuple(w.shape[2:]) != (3, 3):
        return None
    return _pack("dmvs_conv2d_c8_weight_floats", "dmvs_pack_conv_weights_c8", (w,), int(w.shape[1]))


def pack_wino_fpn(w3: torch.Tensor, w_lat: torch.Tensor, b_lat: torch.Tensor) -> Optional[torch.Tensor]:
    """Composite Winograd filters of FeatureNet's level-3 merge (inner2 folded into out3, module.py:333-336) for
    dmvs_conv3d_wino_fpn2; w3 [16,32,3,3], w_lat [32,8], b_lat [32].  None for any other shape."""
    if tuple(w3.shape) != (16, 32, 3, 3) or tuple(w_lat.shape) != (32, 8) or tuple(b_lat.shape) != (32,):
        return None
    return _pack("dmvs_conv3d_wino_fpn_weight_floats", "dmvs_pack_conv_weights_wino_fpn", (w3, w_lat, b_lat))


def make_layer(name: str, mode: int, w: torch.Tensor, scale: Optional[torch.Tensor], shift: Optional[torch.Tensor], relu: bool,
               direct: bool = True, coarse: bool = True) -> ConvLayer:
    """PyTorch conv weight (``mode`` DECONV_S2: transposed, [Cin][Cout][k..]; 4-D: a 2D layer, kdepth 1) + folded BatchNorm ->
    ConvLayer with every kernel form that compiles the shape, each moved to the weight's device.  The Winograd family (K3w,
    K3r, K3z) and K3s are packed for stride-1 3x3 layers only, the split probe for stride-2 ones; ``direct``: also the K2 form;
    ``coarse``: also K3r.  A 3-channel (RGB) weight gets a zero fourth channel for K3 (4-channel k-groups); K3s reads the three."""
    w = w.detach()
    kd = 3 if w.dim() == 5 else 1
    tr = mode == DECONV_S2
    cin, cout = (w.shape[0], w.shape[1]) if tr else (w.shape[1], w.shape[0])
    wk = w
    if cin == 3:
        wk, cin = torch.cat((w, torch.zeros_like(w[:, :1])), 1).contiguous(), 4
    s3 = mode == CONV_S1 and w.shape[-1] == 3
    dev = lambda t: None if t is None else t.to(w.device)
    return ConvLayer(name, mode, kd, cin, cout, pack_direct(w, tr) if direct else None, dev(pack_mfma(wk, cin, cout, mode, kd)),
                     None if scale is None else scale.detach().contiguous(), None if shift is None else shift.detach().contiguous(),
                     relu, w_wino=dev(pack_wino(wk, cin, cout, kd)) if s3 else None,
                     w_c8=dev(pack_c8(w)) if s3 else None, w_coarse=dev(pack_coarse(wk, cin, cout, kd)) if s3 and coarse else None,
                     w_split=dev(pack_split(w)) if mode == CONV_S2 else None,
                     w_zmarch=dev(pack_zmarch(wk, cin, cout, kd)) if s3 else None)


# PROBE switch, never on in the product: 3 or 6 = run every conv1 (8 -> 16, stride 2) of the regularisation nets
# through the bf16-split kernel with that many term products; bench.py reports such a run only as `value_split`
split_probe = 0


def conv3d_split(x: torch.Tensor, layer: "ConvLayer", terms: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [8,D,H,W] -> relu(bn(conv3d stride 2)) [16,(D+1)/2,(H+1)/2,(W+1)/2] through the bf16-split probe kernel."""
    _req(x, out)
    if layer.w_split is None or layer.mode != CONV_S2 or layer.kdepth != 3:
        raise _lib.DmvsError(f"layer {layer.name}: the bf16-split probe covers conv1 (8 -> 16, stride 2, 3x3x3) only")
    Cin, D, H, W = x.shape
    Do, Ho, Wo = layer.out_shape(D, H, W)
    if out is None:
        out = torch.empty((16, Do, Ho, Wo), dtype=torch.float32, device=x.device)
    fl = 2.0 * 27 * 8 * 16 * Do * Ho * Wo
    _launch(_lib.load().dmvs_conv3d_split_probe, (_ptr(x), _ptr(out), _ptr(layer.w_split), _ptr(layer.scale), _ptr(layer.shift),
                                                   D, H, W, int(terms), RELU if layer.relu else 0),
            layer.name, "conv3d_split", x, (layer.w_split, layer.scale, layer.shift), False, "conv3d_mfma",
            (fl, 4.0 * (8 * D * H * W + 16 * Do * Ho * Wo), fl))
    return out


# FeatureNet conv0.0 -> conv0.1 as ONE kernel (dmvs_featurenet_conv0); False = two K3s launches (A/B, parity tests)
use_c8_fused = True


def featurenet_conv0(imgs: torch.Tensor, l0: "ConvLayer", l1: "ConvLayer", family: Optional[str] = None) -> Optional[torch.Tensor]:
    """imgs [V,3,H,W] -> conv0.1(conv0.0(imgs)) [8,V,H,W] (module.py:283-286) in one row sweep, the intermediate in registers.
    None when the layers do not carry K3s weights + folded BN + ReLU, or beyond the kernel's offset range (the caller then
    runs the layers one by one)."""
    _req(imgs)
    if not (use_c8 and use_c8_fused) or l0.w_c8 is None or l1.w_c8 is None or not (l0.relu and l1.relu):
        return None
    ts = (l0.w_c8, l0.scale, l0.shift, l1.w_c8, l1.scale, l1.shift)
    if any(t is None for t in ts):
        return None
    V, c3, H, W = imgs.shape
    assert c3 == 3, imgs.shape
    out = torch.empty((8, V, H, W), dtype=torch.float32, device=imgs.device)
    cost = (2.0 * 9 * (3 + 8) * 8 * V * H * W, 4.0 * (3 + 8) * V * H * W, 2.0 * 9 * (3 + 8) * 8 * V * H * W)
    if not _launch(_lib.load().dmvs_featurenet_conv0, (_ptr(imgs), _ptr(out), *(_ptr(t) for t in ts), V, H, W), l0.name,
                   "featurenet_conv0", imgs, ts, True, family or "conv3d_mfma", cost, label="feature.conv0.fused"):
        return None
    return out


def _ones_hw(layer: "ConvLayer", H: int, W: int, device) -> torch.Tensor:
    """The constant-one image the folded bias term of out3 convolves (dmvs_conv3d_wino_fpn2); the kernel only needs H * W
    contiguous ones, so ONE buffer per device serves every image size by prefix.  It is owned by the LAYER and only ever
    replaced by a larger one, the old ones staying referenced: the kernel gets a raw pointer, and a captured HIP graph
    (MVSNet.use_graph) keeps replaying with it -- growth is monotone, so an eval over many image sizes holds at most
    ~2x the largest image, not one tensor per size."""
    key = str(device)
    cur = layer.ones.get(key)
    if cur is None or cur[-1].numel() < H * W:
        n = H * W if cur is None else max(H * W, 2 * cur[-1].numel())
        layer.ones.setdefault(key, []).append(torch.ones(n, dtype=torch.float32, device=device))
        cur = layer.ones[key]
    return cur[-1]


# K3s (the 4x4x1-MFMA row sweep of FeatureNet's 8-channel full-resolution layers) wherever a layer carries w_c8; False
# leaves them to the direct-form K3 kernel (A/B, parity tests)
use_c8 = True
# K3w (Winograd form of the stride-1 3x3 layers) is used wherever a layer carries w_wino and the call has no residual /
# image-stack input; False forces the direct-form K3 kernel everywhere (A/B, parity tests).
use_wino = True
# ... for `auto` only on volumes of at least this many workgroups.  0 = always: the 1/8-scale layers of a few dozen workgroups
# are 10-20 % slower in K3w than in the direct form (together ~0.02 ms per depth map), but a kernel choice that depends on
# the volume size would make the view-group / row-slab / view-shard modes differ from the plain forward in the last bits
WINO_MIN_BLOCKS = 0
# K3r (register-stationary Winograd, persistent) wherever a layer carries w_coarse (conv4 / conv6 of the regularisation nets) and
# the call has no residual; False leaves them to K3w / K3 (A/B, parity tests).  Like K3w the choice does not depend on the volume.
use_coarse = True
# K3z (z-marching register-stationary Winograd) wherever a layer carries w_zmarch (conv2 of the regularisation nets), no residual,
# planar output, W % 4 == 0; False leaves it to K3w / K3 (A/B, parity tests).  The choice does not depend on the volume.
use_zmarch = True
# ... for `auto` only on volumes at least this deep: a z segment of zs planes costs zs + 2 pipeline stages (two halo planes), so at
# D = 4 / 2 (stage 3, the refine passes) half of the patch transforms are halo work and K3w's two-plane tiles are as fast
# (profiles/r06_h_conv2_layers.txt: 0.157 vs 0.153 ms at D = 4; 0.084 vs 0.099 at D = 32, 0.144 vs 0.170 at D = 16).  A rule on D
# only: view groups, row slabs and view shards (which cut H, never D) pick the same kernel as the plain forward.
ZMARCH_MIN_DEPTH = 8
# ... and for FeatureNet's stride-1 3x3 layers of a shape K3r compiles (conv2.1 / conv2.2: 32 -> 32 on the [C][V][H][W] stack), read at
# pack time (MVSNet.prepare).  Off: measured SLOWER than K3w there (0.097 vs 0.082 ms per layer at config 2,
# profiles/r06_a_layers_quick_experiments.txt -- 9250 units of 48 MFMAs per wave between barriers, one whole-CU workgroup)
use_coarse_feature = False


@dataclass(frozen=True)
class _Form:
    """A specialised kernel form of a conv layer.  ``auto`` tries them in the order of _FORMS, before K3 / K2."""
    backend: str      # its forced-backend name
    weight: str       # ConvLayer attribute of its packed weights (None: the layer has no such form)
    skip: bool        # covers a residual
    q4: bool          # covers the quad-planar output
    views: bool       # covers the image-stack input (DMVS_IN_VIEWS)
    auto: Callable    # (layer, D, H, W) -> `auto` takes the form: module switches, depth / plan rule
    entry: str        # C entry: (in, out, w, scale, shift, Cin, Cout, D, H, W, kdepth, flags, stream); conv2d: no Cout / kdepth
    conv2d: bool
    xdiv: float       # algorithmic / executed FLOPs (Winograd F(2x2, 3x3): 36 / 16 products per output patch)


_FORMS = (
    _Form("c8", "w_c8", False, False, True, lambda L, D, H, W: use_c8, "dmvs_conv2d_c8", True, 1.0),
    _Form("zmarch", "w_zmarch", False, False, False, lambda L, D, H, W: use_zmarch and use_wino and D >= ZMARCH_MIN_DEPTH,
          "dmvs_conv3d_zmarch", False, 2.25),
    _Form("coarse", "w_coarse", False, False, False, lambda L, D, H, W: use_coarse and use_wino, "dmvs_conv3d_coarse", False, 2.25),
    # (the plan is negative for W % 4 != 0: `auto` skips K3w there; no image stack: K3w reads planar [C][D][H][W] only)
    _Form("wino", "w_wino", False, True, False,
          lambda L, D, H, W: use_wino and _lib.load().dmvs_conv3d_wino_plan(L.cin, L.cout, D, H, W, L.kdepth) >= WINO_MIN_BLOCKS,
          "dmvs_conv3d_wino", False, 2.25),
)


def dispatch_key() -> tuple:
    """Every module switch that steers which kernels a forward launches (MVSNet._forward_graph keys its captured graph on it).
    use_coarse_feature is not among them: it is read when the weights are packed, not at dispatch."""
    return (use_c8, use_c8_fused, use_wino, use_coarse, use_zmarch, use_prob_fused, PROB_FUSED_DEPTHS, split_probe,
            WINO_MIN_BLOCKS, ZMARCH_MIN_DEPTH)


def conv3d(x: torch.Tensor, layer: ConvLayer, skip: Optional[torch.Tensor] = None,
           out: Optional[torch.Tensor] = None, backend: str = "auto", skip_up2: bool = False,
           family: Optional[str] = None, out_q4: bool = False, in_views: bool = False) -> torch.Tensor:
    """x [Cin,D,H,W] -> [Cout,Do,Ho,Wo];  y = relu(conv(x)*scale+shift) (+ skip).
    ``out_q4``: the result is written as two quad-planar halves, returned as [2,Do,Cout/8,Ho,Wo,4] (K3 only).
    ``in_views``: x is the loader's image stack [V,3,H,W], read in place by a 4-channel layer (DMVS_IN_VIEWS).
    ``backend``: "auto" (the first form of _FORMS that covers the call and accepts it, else K3), "mfma" (K3), "direct" (K2 where
    the layer has it), a form's name or "split3" / "split6" (the probe): a forced form runs its own kernel or raises."""
    _req(x, skip, out)
    if in_views:
        D, c3, H, W = x.shape
        if c3 != 3 or layer.cin != 4 or layer.w_mfma is None or skip is not None or backend == "direct":
            raise _lib.DmvsError(f"layer {layer.name}: in_views is the K3 form of FeatureNet's first layer ([V,3,H,W] input)")
        Cin = 4
    else:
        Cin, D, H, W = x.shape
    assert Cin == layer.cin, (layer.name, Cin, layer.cin)
    Do, Ho, Wo = layer.out_shape(D, H, W)
    oshape = (2, Do, layer.cout // 8, Ho, Wo, 4) if out_q4 else (layer.cout, Do, Ho, Wo)
    if out is None:
        out = torch.empty(oshape, dtype=torch.float32, device=x.device)
    else:
        assert tuple(out.shape) == oshape
    if out_q4 and (skip is not None or layer.w_mfma is None or backend == "direct"):
        raise _lib.DmvsError(f"layer {layer.name}: quad-planar output is a K3 epilogue without residual")
    if skip is not None:
        want = (layer.cout, Do, Ho // 2, Wo // 2) if skip_up2 else tuple(out.shape)
        assert tuple(skip.shape) == want, (tuple(skip.shape), want)
    if backend in ("split3", "split6") or (split_probe and backend == "auto" and layer.w_split is not None and skip is None
                                           and not out_q4 and not in_views):
        if skip is not None or out_q4 or in_views:
            raise _lib.DmvsError(f"layer {layer.name}: the bf16-split probe has no residual, quad-planar output or image-stack input")
        return conv3d_split(x, layer, 3 if backend == "split3" else 6 if backend == "split6" else split_probe, out=out)
    lib = _lib.load()
    fam = family or "conv3d_mfma"
    cin = 3 if in_views else layer.cin
    flags = (RELU if layer.relu else 0) | (OUT_Q4 if out_q4 else 0) | (IN_VIEWS if in_views else 0)
    # every form is a stride-1 3x3 conv (make_layer packs them for those layers only): `auto` skips the table for the others
    for f in _FORMS if (layer.mode == CONV_S1 or backend != "auto") else ():
        w = getattr(layer, f.weight)
        forced = backend == f.backend
        if w is None or (skip is not None and not f.skip) or (out_q4 and not f.q4) or (in_views and not f.views):
            if forced:
                raise _lib.DmvsError(f"layer {layer.name}: shape / residual / layout not covered by the {f.backend} kernel")
            continue
        if not (forced or (backend == "auto" and f.auto(layer, D, H, W))):
            continue
        cost = None
        if timer is not None:   # FLOPs counted in the direct form (what the layer computes), as for every K3 launch
            fl = 2.0 * 9 * layer.kdepth * cin * layer.cout * D * H * W
            # executed: fl / xdiv; conv0 (Cin = 2, K3w) pads its 6 (channel, depth tap) pairs to two k-groups of 4
            cost = (fl, 4.0 * (cin + layer.cout) * D * H * W, fl / f.xdiv * (8.0 / 6.0 if cin == 2 else 1.0))
        dims = (cin, D, H, W) if f.conv2d else (cin, layer.cout, D, H, W, layer.kdepth)
        if _launch(getattr(lib, f.entry), (_ptr(x), _ptr(out), _ptr(w), _ptr(layer.scale), _ptr(layer.shift), *dims, flags),
                   layer.name, f.backend, x, (w, layer.scale, layer.shift), not forced, fam, cost):
            return out
    use_mfma = layer.w_mfma is not None and (backend in ("auto", "mfma") or layer.w_direct is None)
    if backend == "mfma" and layer.w_mfma is None:
        raise _lib.DmvsError(f"layer {layer.name}: shape not covered by the MFMA kernel")
    w = layer.w_mfma if use_mfma else layer.w_direct
    cost = None
    if timer is not None:
        taps = 25 if layer.mode == CONV2D_K5S2 else (1 if layer.mode == CONV2D_K1 else 9 * layer.kdepth)
        vox = D * H * W if layer.mode == DECONV_S2 else Do * Ho * Wo   # deconv: MACs counted on the input grid
        nbytes = 4.0 * (layer.cin * D * H * W + layer.cout * Do * Ho * Wo * (2 if skip is not None else 1))
        cost = (2.0 * taps * layer.cin * layer.cout * vox, nbytes, None)
    _launch(lib.dmvs_conv3d_mfma if use_mfma else lib.dmvs_conv3d_direct,
            (_ptr(x), _ptr(out), _ptr(w), _ptr(layer.scale), _ptr(layer.shift), _ptr(skip), layer.cin, layer.cout, D, H, W,
             layer.mode, layer.kdepth, flags | (SKIP_UP2 if skip_up2 else 0)),
            layer.name, "mfma" if use_mfma else "direct", x, (w, layer.scale, layer.shift), False,
            family or ("conv3d_mfma" if use_mfma else ("prob_head" if layer.cout == 2 else "conv3d_direct")), cost)
    return out


def conv3d_fpn(lat: torch.Tensor, td: torch.Tensor, layer: ConvLayer, out_q4: bool = False,
               family: Optional[str] = None) -> Optional[torch.Tensor]:
    """out = conv3x3(b_lat + w_lat . lat + up2(td)) as ONE Winograd convolution (FeatureNet's inner2 + upsample-add + out3,
    the lateral conv folded into ``layer.w_wino_fpn`` on the host: pack_wino_fpn).  lat [8,V,H,W], td [32,V,H/2,W/2].
    Returns None when the shape is not covered (the caller then runs the layers separately)."""
    _req(lat, td)
    Cl, V, H, W = lat.shape
    Cin = td.shape[0]
    assert tuple(td.shape) == (Cin, V, H // 2, W // 2) and layer.cin == Cin
    if not use_wino or layer.w_wino_fpn is None or (Cl, Cin, layer.cout) != (8, 32, 16):
        return None
    oshape = (2, V, layer.cout // 8, H, W, 4) if out_q4 else (layer.cout, V, H, W)
    out = torch.empty(oshape, dtype=torch.float32, device=lat.device)
    vox = V * H * W
    # executed: (3 x 16 + 8 x 9) MFMAs of 2048 FLOP per 64 pixels
    cost = (2.0 * vox * (9 * Cin * layer.cout + Cl * Cin), 4.0 * (Cl * vox + Cin * vox / 4 + layer.cout * vox), vox * 120 * 2048 / 64.0)
    if not _launch(_lib.load().dmvs_conv3d_wino_fpn2,
                   (_ptr(lat), _ptr(td), _ptr(_ones_hw(layer, H, W, lat.device)), _ptr(out), _ptr(layer.w_wino_fpn), _ptr(layer.scale),
                    _ptr(layer.shift), V, H, W, (RELU if layer.relu else 0) | (OUT_Q4 if out_q4 else 0)),
                   layer.name, "conv3d_fpn", lat, (layer.w_wino_fpn, layer.scale, layer.shift), True, family or "conv3d_mfma",
                   cost, label="feature.out3.fpn"):
        return None
    return out


# ------------------------------------------------------------------------------------------ K4
# `prob` -> K4 for the passes one workgroup can hold (D = 4 / 8; r06): the `prob` head of a branch regresses its own
# two channels (prob_regress) and K4 shrinks to the selection on [4,H,W] (depth_select).  bench.py --no-prob-fused = the two kernels.
use_prob_fused = True
PROB_FUSED_DEPTHS = (4, 8)


def prob_fusable(D: int, W: int, backend: str) -> bool:
    return use_prob_fused and backend in ("auto", "mfma") and D in PROB_FUSED_DEPTHS and W % 4 == 0


def prob_regress(x: torch.Tensor, layer: ConvLayer, depth_dhw, interval: torch.Tensor, alpha: float, out: torch.Tensor) -> bool:
    """x [Cin,D,H,W] (conv11's output) -> out [2,H,W]: softmax over D of alpha * prob(x) and the depth expectation, the branch's two
    channels of depth_sub_plus (module.py:379,397 + mvsnet.py:19-20,68-69).  ``depth_dhw`` as for depth_regress.  Returns False when
    the shape is not covered (the caller then runs conv3d + depth_regress)."""
    affine = isinstance(depth_dhw, AffinePlanes)
    _req(x, depth_dhw.base if affine else depth_dhw, interval, out)
    if affine and depth_dhw.step.data_ptr() != interval.data_ptr():
        raise _lib.DmvsError("prob_regress: AffinePlanes.step is not the `interval` tensor -- the planes regressed on would differ "
                             "from the planes K1 correlated")
    Cin, D, H, W = x.shape
    assert layer.cout == 2 and Cin == layer.cin and tuple(out.shape) == (2, H, W) and tuple(depth_dhw.shape) == (D, H, W)
    hyp = H * W if affine else D * H * W
    cost = None if timer is None else (2.0 * 27 * Cin * 2 * D * H * W, 4.0 * (Cin * D * H * W + hyp + 2 * H * W), None)
    return _launch(_lib.load().dmvs_prob_regress, (_ptr(x), _ptr(layer.w_direct), Cin, D, H, W, None if affine else _ptr(depth_dhw),
                                                   _ptr(depth_dhw.base) if affine else None, _ptr(interval) if affine else None,
                                                   float(alpha), _ptr(out)),
                   layer.name, "prob_regress", x, (layer.w_direct,), True, "prob_head", cost)


def depth_select(dsp: torch.Tensor, interval: torch.Tensor, mode: int):
    """dsp [4,H,W] (two prob_regress calls) -> (sel ([4,H,W] | [H,W]), conf [H,W]): K4's part behind the expectations."""
    _req(dsp, interval)
    _, H, W = dsp.shape
    sel = torch.empty((4, H, W) if mode == 0 else (H, W), dtype=torch.float32, device=dsp.device)
    conf = torch.empty((H, W), dtype=torch.float32, device=dsp.device)
    cost = None if timer is None else (0.0, 4.0 * (4 + (5 if mode == 0 else 2)) * H * W, None)
    _launch(_lib.load().dmvs_depth_select, (_ptr(dsp), _ptr(interval), mode, H, W, _ptr(sel), _ptr(conf)), "depth_regress",
            "dmvs_depth_select", dsp, (), False, "depth_regress", cost)
    return sel, conf


def depth_regress(logits: torch.Tensor, depth_dhw: torch.Tensor, interval: torch.Tensor, alpha: float, mode: int,
                  want_prob: bool):
    """logits [4,D,H,W], depth [D,H,W] (or AffinePlanes) -> (dsp [4,H,W], sel ([4,H,W] | [H,W]), conf [H,W], prob | None)."""
    affine = isinstance(depth_dhw, AffinePlanes)
    _req(logits, depth_dhw.base if affine else depth_dhw, interval)
    if affine and depth_dhw.step.data_ptr() != interval.data_ptr():
        # the kernel forms the planes as base + d * interval[0]: K1 correlated on base + d * step, they must be one scalar
        raise _lib.DmvsError("depth_regress: AffinePlanes.step is not the `interval` tensor handed to K4 -- the planes "
                             "regressed on would differ from the planes K1 correlated")
    _, D, H, W = logits.shape
    assert tuple(depth_dhw.shape) == (D, H, W)
    dev = logits.device
    dsp = torch.empty((4, H, W), dtype=torch.float32, device=dev)
    sel = torch.empty((4, H, W) if mode == 0 else (H, W), dtype=torch.float32, device=dev)
    conf = torch.empty((H, W), dtype=torch.float32, device=dev)
    prob = torch.empty_like(logits) if want_prob else None
    cost = None
    if timer is not None:
        # algorithmic bytes: the 4 logit planes per hypothesis once + the hypotheses ([D,H,W], or only the [H,W] base plane of the
        # affine form -- VERDICT r05: count what is read) + the outputs (dsp 4, sel 4 | 1, conf 1 planes) (+ the softmax volume)
        hyp = H * W if affine else D * H * W
        cost = (0.0, 4.0 * (4 * D * H * W + hyp + (9 if mode == 0 else 6) * H * W + (4 * D * H * W if want_prob else 0)), None)
    fn = _lib.load().dmvs_depth_regress_affine if affine else _lib.load().dmvs_depth_regress
    _launch(fn, (_ptr(logits), _ptr(depth_dhw.base if affine else depth_dhw), _ptr(interval), float(alpha), mode, D, H, W, _ptr(dsp),
                 _ptr(sel), _ptr(conf), _ptr(prob)), "depth_regress", "dmvs_depth_regress", logits, (), False, "depth_regress", cost)
    return dsp, sel, conf, prob


def depth_regress_backward(logits: torch.Tensor, hyp_dhw: torch.Tensor, alpha: float, mode: int, dsp: torch.Tensor,
                           g_dsp: Optional[torch.Tensor], g_sel: Optional[torch.Tensor], want_hyp: bool,
                           g_logits: Optional[torch.Tensor] = None, g_hyp: Optional[torch.Tensor] = None):
    """K4b.  logits [4,D,H,W], hyp [D,H,W], dsp [4,H,W] (the forward's), g_dsp [4,H,W] | None, g_sel ([4,H,W] mode 0 | [H,W] mode 1)
    | None -> (g_logits [4,D,H,W], g_hyp [D,H,W] | None).  ``g_logits`` / ``g_hyp``: buffers to write into (fully overwritten)."""
    _req(logits, hyp_dhw, dsp, g_dsp, g_sel, g_logits, g_hyp)
    _, D, H, W = logits.shape
    assert logits.shape[0] == 4 and tuple(hyp_dhw.shape) == (D, H, W) and tuple(dsp.shape) == (4, H, W)
    assert g_dsp is None or tuple(g_dsp.shape) == (4, H, W)
    assert g_sel is None or tuple(g_sel.shape) == ((4, H, W) if mode == 0 else (H, W))
    if g_dsp is None and g_sel is None:
        raise _lib.DmvsError("depth_regress_backward: no upstream gradient (g_dsp and g_sel are both None)")
    if g_logits is None:
        g_logits = torch.empty_like(logits)
    if want_hyp and g_hyp is None:
        g_hyp = torch.empty_like(hyp_dhw)
    assert g_logits.shape == logits.shape and (g_hyp is None or g_hyp.shape == hyp_dhw.shape)
    cost = None
    if timer is not None:
        # algorithmic bytes: the logit volume read and its gradient written once (32 N, N = D H W), the hypotheses read (and their
        # gradient written), dsp and the upstream planes
        planes = 4 + (4 if g_dsp is not None else 0) + (0 if g_sel is None else (4 if mode == 0 else 1))
        cost = (0.0, 4.0 * (8 * D * H * W + (2 if want_hyp else 1) * D * H * W + planes * H * W), None)
    _launch(_lib.load().dmvs_depth_regress_backward,
            (_ptr(logits), _ptr(hyp_dhw), float(alpha), mode, D, H, W, _ptr(dsp), _ptr(g_dsp), _ptr(g_sel), _ptr(g_logits),
             _ptr(g_hyp if want_hyp else None)), "depth_regress", "dmvs_depth_regress_backward", logits, (), False, "depth_regress", cost)
    return g_logits, (g_hyp if want_hyp else None)


def dual_depth_loss_backward(dsp_main: torch.Tensor, dsp_refine: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor, weight: float,
                             counts: torch.Tensor, g_total: torch.Tensor, want_main: bool = True, want_refine: bool = True):
    """N6b.  dsp_* [B,4,h,w], gt / mask [B,h,w] fp32, ``counts`` [2] int64 (n, n_cells: the forward's), ``g_total`` [1] fp32 on the
    device -> (g_dsp_main, g_dsp_refine), None where not wanted.  Not logged as a launch family (as the N6 forward)."""
    _req(dsp_main, dsp_refine, gt, mask, g_total)
    B, h, w = gt.shape
    assert tuple(dsp_main.shape) == tuple(dsp_refine.shape) == (B, 4, h, w) and mask.shape == gt.shape
    assert counts.dtype == torch.int64 and counts.is_cuda and counts.numel() == 2 and g_total.numel() == 1
    g_main = torch.empty_like(dsp_main) if want_main else None
    g_refine = torch.empty_like(dsp_refine) if want_refine else None
    if g_main is None and g_refine is None:
        return None, None
    _lib.check(_lib.load().dmvs_dual_depth_loss_backward(_ptr(dsp_main), _ptr(dsp_refine), _ptr(gt), _ptr(mask), B, h, w, float(weight),
                                                         _ptr(counts), _ptr(g_total), _ptr(g_main), _ptr(g_refine), _stream()),
               "dmvs_dual_depth_loss_backward")
    return g_main, g_refine


# ------------------------------------------------------------------------------------------ training: shared by K3g / K3h / K2g / K3k / K3f / K5
_pack_index_cache: dict = {}
_ws_cache: dict = {}


def _pack_index(key: tuple, build: Callable[[], torch.Tensor], device) -> torch.Tensor:
    """The gather index ``key`` of the pack_index_* functions from their one cache: the host LongTensor, derived and validated once by
    ``build()``, or its copy on ``device``, made once per device.  Repeated calls return the same tensor object."""
    if device is not None and torch.device(device).type != "cpu":
        dkey = key + (torch.device(device),)
        idx = _pack_index_cache.get(dkey)
        if idx is None:
            idx = _pack_index_cache[dkey] = _pack_index(key, build, None).to(device)
        return idx
    idx = _pack_index_cache.get(key)
    if idx is None:
        idx = _pack_index_cache[key] = build()
    return idx


def _transposed_flipped(w: torch.Tensor) -> torch.Tensor:
    """``w`` transposed in (co, ci) and flipped in every tap: the weight of a stride-1 layer's data gradient."""
    return w.transpose(0, 1).flip(tuple(range(2, w.dim())))


def _derive_index(what: str, shape, arrange: Optional[Callable], pack: Callable, permutation: bool) -> torch.Tensor:
    """The one derivation behind the five pack_index_* functions (``what``: the one that asks).  For a weight of ``shape`` with n
    elements: ``pack(arrange(iota + 1))`` -- the iota in the weight's layout, re-arranged as the layer's weight is (``arrange`` None: as
    it lies), through the library's packer -- minus 1 is the element every packed slot selects; a zero of the packed form selects the
    slot n, which the gather appends (gather_packed).  Every element must be selected exactly once; with ``permutation`` the slot n must
    not be selected at all, so the index serves ``w.reshape(-1)[index]`` as it is."""
    n = 1
    for k in shape:
        n *= int(k)
    if n < 1 or n + 1 >= (1 << 24):   # iota + 1 travels as fp32
        raise _lib.DmvsError(f"{what}: a weight {tuple(shape)} has no gather index (1 <= elements < 2^24 - 1)")
    iota = (torch.arange(n, dtype=torch.float32) + 1.0).reshape(*shape)
    packed = pack(iota if arrange is None else arrange(iota).contiguous())
    if packed is None:
        raise _lib.DmvsError(f"{what}: the library does not compile the layer of a weight {tuple(shape)}")
    idx = packed.reshape(-1).to(torch.int64) - 1
    idx[idx < 0] = n
    counts = torch.bincount(idx, minlength=n + 1)
    if not torch.equal(counts[:n], torch.ones(n, dtype=torch.int64)):
        raise _lib.DmvsError(f"{what}: the packing of a weight {tuple(shape)} does not select every weight element exactly once")
    if permutation and int(counts[n]):
        raise _lib.DmvsError(f"{what}: the packing of a weight {tuple(shape)} is not a permutation")
    return idx


def gather_packed(weight: torch.Tensor, index: torch.Tensor, zero_slot: bool) -> torch.Tensor:
    """The packed form of ``weight`` by one device gather through its pack_index_* ``index``.  ``zero_slot``: the family's packings
    are selections with zeros, which select the one zero appended here; the permutation families (pack_index_mfma, pack_index_direct)
    gather the weight as it lies."""
    flat = weight.detach().reshape(-1)
    if zero_slot:
        flat = torch.cat((flat, flat.new_zeros(1)))
    return torch.index_select(flat, 0, index)


def _workspace(kind: str, n: int, device) -> torch.Tensor:
    """The cached workspace of ``n`` floats of the kernel family ``kind``, one per (kind, size, device, stream)."""
    dev = torch.device(device)
    if dev.index is None:   # "cuda" and "cuda:<current>" are one device and must be one workspace
        dev = torch.device(dev.type, torch.cuda.current_device())
    key = (kind, n, dev, torch.cuda.current_stream(dev).cuda_stream)
    ws = _ws_cache.get(key)
    if ws is None:
        ws = _ws_cache[key] = torch.empty(n, dtype=torch.float32, device=dev)
    return ws


def _no_buffer(what: str) -> _lib.DmvsError:
    return _lib.DmvsError(f"{what}: accumulate needs the buffer to add to (out)")


def _wgrad_out(what: str, out: Optional[torch.Tensor], accumulate: bool, shape: tuple, x: torch.Tensor) -> torch.Tensor:
    """The buffer the weight-gradient wrapper ``what`` writes a gradient of ``shape`` into: ``out``, or a new one beside ``x``."""
    if out is None:
        if accumulate:
            raise _no_buffer(what)
        return torch.empty(shape, dtype=torch.float32, device=x.device)
    if out.numel() != math.prod(shape):
        raise _lib.DmvsError(f"{what}: out {tuple(out.shape)} is not a [{','.join(map(str, shape))}] weight")
    return out


def _wgrad_workspace(what: str, kind: str, n: int, dims: tuple, device, workspace: Optional[torch.Tensor] = None,
                     kernel: str = "weight-gradient kernel") -> torch.Tensor:
    """The workspace of the weight-gradient wrapper ``what``, ``n`` = the library's size for ``dims`` (the arguments of
    dmvs_<what>_workspace; <= 0: the kernel does not cover them): ``workspace`` if it is large enough, else the cached buffer of the
    family ``kind``, one per (size, device, stream) -- the sizes do not depend on the volume."""
    if workspace is None:
        if n <= 0:
            raise _lib.DmvsError(f"{what}: the shape {tuple(dims)} (as dmvs_{what}_workspace takes it) is not covered by the {kernel}")
        return _workspace(kind, n, device)
    if workspace.numel() < n:
        raise _lib.DmvsError(f"{what}: workspace too small ({workspace.numel()} floats, {n} needed)")
    return workspace


# ------------------------------------------------------------------------------------------ K3g (training: the stride-1 square convs)
WGRAD_TILE = (1, 4, 32)   # voxel tile (z, y, x) of K3g: dmvs_conv3d_wgrad_plan counts these (csrc/conv3d_wgrad.h)


def pack_index_mfma(C: int, kdepth: int, transposed_flipped: bool, device=None) -> torch.Tensor:
    """Gather index (cached LongTensor; on the CPU, or a cached copy on ``device``) of K3's weight packing for a stride-1 square layer
    C -> C: for a weight ``w`` in nn.Conv3d / nn.Conv2d layout ``w.reshape(-1)[index] == pack_mfma(w, C, C, CONV_S1, kdepth)`` bit for
    bit (the packing of these shapes is a pure permutation).  ``transposed_flipped``: the index of
    ``pack_mfma(w.transpose(0, 1).flip(2, 3, 4), ...)`` instead -- the weight of the layer's data gradient.  Derived once on the host
    by packing an iota through the library's packer (_derive_index)."""
    def build():
        if kdepth not in (1, 3):
            raise _lib.DmvsError(f"pack_index_mfma: C = {C}, kdepth = {kdepth}")
        return _derive_index("pack_index_mfma", (C, C, kdepth, 3, 3), _transposed_flipped if transposed_flipped else None,
                             lambda w: pack_mfma(w, C, C, CONV_S1, kdepth), True)
    return _pack_index((int(C), int(kdepth), bool(transposed_flipped)), build, device)


def conv3d_wgrad_workspace(C: int, D: int, H: int, W: int, kdepth: int, device) -> torch.Tensor:
    """K3g's workspace, one per (shape class, device, stream): its size does not depend on the volume."""
    dims = (C, D, H, W, kdepth)
    return _wgrad_workspace("conv3d_wgrad", "k3g", _lib.load().dmvs_conv3d_wgrad_workspace(*dims), dims, device)


def conv3d_wgrad(x: torch.Tensor, gy: torch.Tensor, kdepth: int, out: Optional[torch.Tensor] = None, accumulate: bool = False,
                 workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K3g.  x, gy [C,D,H,W] (input of a stride-1 3x3(x3) pad-1 conv C -> C and the gradient on its output) -> the weight gradient
    [C,C,kdepth,3,3].  ``out``: buffer to write into; with ``accumulate`` the result is ADDED to it (it must then be given).
    ``workspace``: at least dmvs_conv3d_wgrad_workspace floats (default: a cached buffer per device and stream)."""
    _req(x, gy, out, workspace)
    if x.dim() != 4 or x.shape != gy.shape:
        raise _lib.DmvsError(f"conv3d_wgrad: x {tuple(x.shape)} and gy {tuple(gy.shape)} must be the same [C,D,H,W]")
    C, D, H, W = x.shape
    lib, dims = _lib.load(), (C, D, H, W, kdepth)
    out = _wgrad_out("conv3d_wgrad", out, accumulate, (C, C, kdepth, 3, 3), x)
    workspace = _wgrad_workspace("conv3d_wgrad", "k3g", lib.dmvs_conv3d_wgrad_workspace(*dims), dims, x.device, workspace)
    cost = None if timer is None else (2.0 * 9 * kdepth * C * C * D * H * W, 4.0 * (2 * C * D * H * W + 9 * kdepth * C * C), None)
    _launch(lib.dmvs_conv3d_wgrad, (_ptr(x), _ptr(gy), _ptr(out), _ptr(workspace), *dims, 1 if accumulate else 0),
            f"wgrad{C}k{kdepth}", "wgrad", x, (gy, out, workspace), False, "conv3d_wgrad", cost)
    _log("conv3d_wgrad")   # two dispatches per call: the partials and their sum (scripts/pmc_summary.py joins by dispatch order)
    return out


# ------------------------------------------------------------------------------------------ K2g (training: the 2-channel ends conv0 / prob)
WGRAD_C2_TILE = (1, 4, 64)          # voxel tile (z, y, x) of K2g: dmvs_conv3d_wgrad_c2_plan counts these (csrc/conv3d_wgrad_c2.h)
WGRAD_C2_SHAPES = ((2, 8), (8, 2))  # (Cin, Cout): conv0 and prob


def pack_index_direct(cin: int, cout: int, transposed_flipped: bool, device=None) -> torch.Tensor:
    """Gather index (cached LongTensor; on the CPU, or a cached copy on ``device``) of K2's weight packing for a 3x3x3 layer
    cin -> cout: for a weight ``w`` [cout,cin,3,3,3] ``w.reshape(-1)[index] == pack_direct(w, False).reshape(-1)`` bit for bit (the
    packing is a pure permutation).  ``transposed_flipped``: the index of ``pack_direct(w.transpose(0, 1).flip(2, 3, 4), False)``
    instead -- the weight of the layer's data gradient, a cout -> cin layer.  Derived once on the host by packing an iota
    (_derive_index)."""
    def build():
        if cin < 1 or cout < 1:
            raise _lib.DmvsError(f"pack_index_direct: cin = {cin}, cout = {cout}")
        return _derive_index("pack_index_direct", (cout, cin, 3, 3, 3), _transposed_flipped if transposed_flipped else None,
                             lambda w: pack_direct(w, False), True)
    return _pack_index(("direct", int(cin), int(cout), bool(transposed_flipped)), build, device)


def _wgrad_c2_dims(x: torch.Tensor, gy: torch.Tensor):
    if x.dim() != 4 or gy.dim() != 4 or x.shape[1:] != gy.shape[1:] or (int(x.shape[0]), int(gy.shape[0])) not in WGRAD_C2_SHAPES:
        raise _lib.DmvsError(f"conv3d_wgrad_c2: x {tuple(x.shape)} and gy {tuple(gy.shape)} must be [Cin,D,H,W] and [Cout,D,H,W] of one "
                             f"volume with (Cin, Cout) in {WGRAD_C2_SHAPES}")
    return (int(x.shape[0]), int(gy.shape[0]), *(int(n) for n in x.shape[1:]))


def conv3d_wgrad_c2_workspace(Cin: int, Cout: int, D: int, H: int, W: int, device) -> torch.Tensor:
    """K2g's workspace, one per (size, device, stream): its size does not depend on the volume."""
    dims = (Cin, Cout, D, H, W)
    return _wgrad_workspace("conv3d_wgrad_c2", "k2g", _lib.load().dmvs_conv3d_wgrad_c2_workspace(*dims), dims, device)


def conv3d_wgrad_c2(x: torch.Tensor, gy: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False,
                    workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K2g.  x [Cin,D,H,W], gy [Cout,D,H,W] (input of a stride-1 3x3x3 pad-1 conv and the gradient on its output), (Cin, Cout) =
    (2, 8) (conv0) or (8, 2) (prob) -> the weight gradient [Cout,Cin,3,3,3].  ``out``: buffer to write into; with ``accumulate`` the
    result is ADDED to it (it must then be given).  ``workspace``: at least dmvs_conv3d_wgrad_c2_workspace floats (default: a cached
    buffer per device and stream)."""
    _req(x, gy, out, workspace)
    Cin, Cout, D, H, W = dims = _wgrad_c2_dims(x, gy)
    lib = _lib.load()
    out = _wgrad_out("conv3d_wgrad_c2", out, accumulate, (Cout, Cin, 3, 3, 3), x)
    workspace = _wgrad_workspace("conv3d_wgrad_c2", "k2g", lib.dmvs_conv3d_wgrad_c2_workspace(*dims), dims, x.device, workspace)
    cost = None if timer is None else (2.0 * 27 * Cin * Cout * D * H * W, 4.0 * ((Cin + Cout) * D * H * W + 27 * Cin * Cout), None)
    _launch(lib.dmvs_conv3d_wgrad_c2, (_ptr(x), _ptr(gy), _ptr(out), _ptr(workspace), *dims, 1 if accumulate else 0),
            f"wgrad{Cin}to{Cout}", "wgrad_c2", x, (gy, out, workspace), False, "conv3d_wgrad_c2", cost)
    _log("conv3d_wgrad_c2")   # two dispatches per call: the partials and their sum (scripts/pmc_summary.py joins by dispatch order)
    return out


# ------------------------------------------------------------------------------------------ K3h (training: the stride-2 and transposed convs)
# coarse voxel tile (z, y, x) of K3h per (Ca, kdepth): dmvs_conv3d_wgrad_s2_plan counts these (csrc/conv3d_wgrad_s2.h)
WGRAD_S2_TILE = {(16, 3): (1, 4, 32), (32, 3): (1, 4, 32), (64, 3): (1, 2, 32), (64, 1): (1, 4, 32)}


def pack_index_mfma_s2(cin: int, cout: int, mode: int, kdepth: int, device=None) -> torch.Tensor:
    """Gather index (cached LongTensor; on the CPU, or a cached copy on ``device``) of K3's weight packing for a stride-2 layer
    (``mode`` CONV_S2, weight [cout][cin][k..]) or a transposed one (DECONV_S2, weight [cin][cout][k..]) with cout = 2 cin resp.
    cin = 2 cout: ``gather_packed(w, index, True) == pack_mfma(w, cin, cout, mode, kdepth)`` bit for bit.  These packings are
    selections with zeros, not permutations (conv1's packed-K form pads its last k-step, conv11's y-parity-merged form has zero rows):
    a zero of the packed form selects the one appended zero slot, index n = cin * cout * 9 * kdepth.  Derived once on the host by
    packing ``iota + 1`` through the library's packer (_derive_index); every weight element must be selected exactly once."""
    def build():
        ok = (mode == CONV_S2 and cout == 2 * cin) or (mode == DECONV_S2 and cin == 2 * cout)
        if not ok or kdepth not in (1, 3):
            raise _lib.DmvsError(f"pack_index_mfma_s2: {cin} -> {cout}, mode {mode}, kdepth {kdepth} is no stride-2 or transposed layer")
        lead = (cout, cin) if mode == CONV_S2 else (cin, cout)
        return _derive_index("pack_index_mfma_s2", (*lead, kdepth, 3, 3), None, lambda w: pack_mfma(w, cin, cout, mode, kdepth), False)
    return _pack_index(("s2", int(cin), int(cout), int(mode), int(kdepth)), build, device)


def _wgrad_s2_dims(coarse: torch.Tensor, fine: torch.Tensor, kdepth: int):
    if coarse.dim() != 4 or fine.dim() != 4:
        raise _lib.DmvsError(f"conv3d_wgrad_s2: coarse {tuple(coarse.shape)} and fine {tuple(fine.shape)} must be [C,D,H,W]")
    Ca, Dc, Hc, Wc = coarse.shape
    want = (Ca // 2, 2 * Dc if kdepth == 3 else Dc, 2 * Hc, 2 * Wc)
    if Ca % 2 or tuple(fine.shape) != want:
        raise _lib.DmvsError(f"conv3d_wgrad_s2: the fine tensor of coarse {tuple(coarse.shape)}, kdepth {kdepth} is {want}, got "
                             f"{tuple(fine.shape)}")
    return Ca, Dc, Hc, Wc


def conv3d_wgrad_s2_workspace(Ca: int, Dc: int, Hc: int, Wc: int, kdepth: int, device) -> torch.Tensor:
    """K3h's workspace, one per (shape class, device, stream): its size does not depend on the volume."""
    dims = (Ca, Dc, Hc, Wc, kdepth)
    return _wgrad_workspace("conv3d_wgrad_s2", "k3h", _lib.load().dmvs_conv3d_wgrad_s2_workspace(*dims), dims, device,
                            kernel="strided weight-gradient kernel")


def conv3d_wgrad_s2(coarse: torch.Tensor, fine: torch.Tensor, kdepth: int, out: Optional[torch.Tensor] = None, accumulate: bool = False,
                    workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K3h.  coarse [Ca,Dc,Hc,Wc], fine [Ca/2,Df,2Hc,2Wc] (Df = 2 Dc, or Dc for kdepth 1) -> G [Ca,Ca/2,kdepth,3,3],
    G[a,b,kz,ky,kx] = sum coarse[a,z,y,x] * fine[b,2z+kz-1,2y+ky-1,2x+kx-1].  Stride-2 conv (kernel 3, padding 1): coarse = the gradient
    on the output, fine = the input, G = dW.  Transposed conv (output_padding 1): coarse = the input, fine = the gradient on the output,
    G = dWt.  ``out``: buffer to write into; with ``accumulate`` the result is ADDED to it (it must then be given).
    ``workspace``: at least dmvs_conv3d_wgrad_s2_workspace floats (default: a cached buffer per device and stream)."""
    _req(coarse, fine, out, workspace)
    Ca, Dc, Hc, Wc = _wgrad_s2_dims(coarse, fine, kdepth)
    lib, dims = _lib.load(), (Ca, Dc, Hc, Wc, kdepth)
    out = _wgrad_out("conv3d_wgrad_s2", out, accumulate, (Ca, Ca // 2, kdepth, 3, 3), coarse)
    workspace = _wgrad_workspace("conv3d_wgrad_s2", "k3h", lib.dmvs_conv3d_wgrad_s2_workspace(*dims), dims, coarse.device, workspace,
                                 "strided weight-gradient kernel")
    cost = None
    if timer is not None:
        nt = 9 * kdepth * Ca * (Ca // 2)
        cost = (2.0 * nt * Dc * Hc * Wc, 4.0 * (coarse.numel() + fine.numel() + nt), None)
    _launch(lib.dmvs_conv3d_wgrad_s2, (_ptr(coarse), _ptr(fine), _ptr(out), _ptr(workspace), *dims, 1 if accumulate else 0),
            f"wgrad_s2_{Ca}k{kdepth}", "wgrad_s2", coarse, (fine, out, workspace), False, "conv3d_wgrad_s2", cost)
    _log("conv3d_wgrad_s2")   # two dispatches per call: the partials and their sum
    return out


# ------------------------------------------------------------------------------------------ K3k / K3d (training: FeatureNet's 5x5 stride-2 convs)
WGRAD_K5S2_TILE = (1, 4, 32)             # coarse tile (plane, y, x) of K3k: dmvs_conv2d_k5s2_wgrad_plan counts these (csrc/conv2d_k5s2_bwd.h)
WGRAD_K5S2_SHAPES = ((8, 16), (16, 32))  # (Cin, Cout): conv1.0 and conv2.0


def pack_index_mfma_k5s2(cin: int, cout: int, device=None) -> torch.Tensor:
    """Gather index (cached LongTensor; on the CPU, or a cached copy on ``device``) of K3's weight packing for a 5x5 stride-2 layer
    (CONV2D_K5S2, weight [cout][cin][5][5], cout = 2 cin): ``gather_packed(w, index, True) == pack_mfma(w, cin, cout, CONV2D_K5S2, 1)``
    bit for bit.  A zero of the packed form (conv1.0's packed-K form may pad) selects the one appended zero slot, index
    n = cin * cout * 25.  Derived once on the host by packing ``iota + 1`` through the library's packer (_derive_index); every weight
    element must be selected exactly once."""
    def build():
        if (cin, cout) not in WGRAD_K5S2_SHAPES:
            raise _lib.DmvsError(f"pack_index_mfma_k5s2: {cin} -> {cout} is no 5x5 stride-2 layer of FeatureNet {WGRAD_K5S2_SHAPES}")
        return _derive_index("pack_index_mfma_k5s2", (cout, cin, 5, 5), None, lambda w: pack_mfma(w, cin, cout, CONV2D_K5S2, 1), False)
    return _pack_index(("k5s2", int(cin), int(cout)), build, device)


def _k5s2_dims(what: str, gy: torch.Tensor, fine_shape):
    """(Ca, D, Hf, Wf) of a coarse tensor [Ca,D,Hc,Wc] and the shape [Ca/2,D,Hf,Wf] of its fine one."""
    if gy.dim() != 4 or len(fine_shape) != 4:
        raise _lib.DmvsError(f"{what}: gy {tuple(gy.shape)} and the fine tensor {tuple(fine_shape)} must be [C,D,H,W]")
    Ca, D, Hc, Wc = (int(n) for n in gy.shape)
    Cb, Df, Hf, Wf = (int(n) for n in fine_shape)
    if (Cb, Ca) not in WGRAD_K5S2_SHAPES or Df != D or Hf < 1 or Wf < 1 or ((Hf + 1) // 2, (Wf + 1) // 2) != (Hc, Wc):
        raise _lib.DmvsError(f"{what}: gy {tuple(gy.shape)} is not the output of a 5x5 stride-2 layer {WGRAD_K5S2_SHAPES} on "
                             f"{tuple(fine_shape)} ([Ca,D,(Hf+1)//2,(Wf+1)//2] for [Ca/2,D,Hf,Wf])")
    return Ca, D, Hf, Wf


def conv2d_k5s2_wgrad_workspace(Ca: int, D: int, Hf: int, Wf: int, device) -> torch.Tensor:
    """K3k's workspace, one per (shape class, device, stream): its size does not depend on the image."""
    dims = (Ca, D, Hf, Wf)
    return _wgrad_workspace("conv2d_k5s2_wgrad", "k3k", _lib.load().dmvs_conv2d_k5s2_wgrad_workspace(*dims), dims, device,
                            kernel="5x5 stride-2 weight-gradient kernel")


def conv2d_k5s2_wgrad(x: torch.Tensor, gy: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False,
                      workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K3k.  x [Cb,D,Hf,Wf] (input of a 5x5 stride-2 pad-2 conv Cb -> Ca = 2 Cb on D independent planes), gy [Ca,D,Hc,Wc] (the gradient
    on its output; Hc = (Hf + 1) // 2, Wc = (Wf + 1) // 2) -> the weight gradient [Ca,Cb,5,5],
    dW[a,b,ky,kx] = sum gy[a,z,y,x] * x[b,z,2y+ky-2,2x+kx-2].  ``out``: buffer to write into; with ``accumulate`` the result is ADDED
    to it (it must then be given).  ``workspace``: at least dmvs_conv2d_k5s2_wgrad_workspace floats (default: a cached buffer per device
    and stream)."""
    _req(x, gy, out, workspace)
    Ca, D, Hf, Wf = dims = _k5s2_dims("conv2d_k5s2_wgrad", gy, x.shape)
    lib = _lib.load()
    out = _wgrad_out("conv2d_k5s2_wgrad", out, accumulate, (Ca, Ca // 2, 5, 5), x)
    workspace = _wgrad_workspace("conv2d_k5s2_wgrad", "k3k", lib.dmvs_conv2d_k5s2_wgrad_workspace(*dims), dims, x.device, workspace,
                                 "5x5 stride-2 weight-gradient kernel")
    cost = None
    if timer is not None:
        nt = 25 * Ca * (Ca // 2)
        cost = (2.0 * nt * D * gy.shape[2] * gy.shape[3], 4.0 * (gy.numel() + x.numel() + nt), None)
    _launch(lib.dmvs_conv2d_k5s2_wgrad, (_ptr(gy), _ptr(x), _ptr(out), _ptr(workspace), *dims, 1 if accumulate else 0),   # (coarse, fine)
            f"wgrad_k5s2_{Ca}", "wgrad_k5s2", x, (gy, out, workspace), False, "conv2d_k5s2_wgrad", cost)
    _log("conv2d_k5s2_wgrad")   # two dispatches per call: the partials and their sum
    return out


def conv2d_k5s2_dgrad(gy: torch.Tensor, w: torch.Tensor, fine_hw, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K3d.  gy [Ca,D,Hc,Wc] (the gradient on the output of a 5x5 stride-2 pad-2 conv Cb -> Ca = 2 Cb), w the layer's weight in
    nn.Conv2d layout [Ca,Cb,5,5] as it lies, ``fine_hw`` = (Hf, Wf) of the layer's input (Hc = (Hf + 1) // 2: two fine extents give one
    coarse one) -> the data gradient [Cb,D,Hf,Wf], every element written once.  ``out``: buffer to write into."""
    _req(gy, w, out)
    Hf, Wf = (int(n) for n in fine_hw)
    Ca, D, Hf, Wf = _k5s2_dims("conv2d_k5s2_dgrad", gy, (int(gy.shape[0]) // 2, int(gy.shape[1]) if gy.dim() == 4 else 0, Hf, Wf))
    Cb = Ca // 2
    if w.numel() != Ca * Cb * 25 or w.dim() != 4 or tuple(w.shape[:2]) != (Ca, Cb):
        raise _lib.DmvsError(f"conv2d_k5s2_dgrad: w {tuple(w.shape)} is not a [{Ca},{Cb},5,5] weight")
    if out is None:
        out = torch.empty((Cb, D, Hf, Wf), dtype=torch.float32, device=gy.device)
    elif tuple(out.shape) != (Cb, D, Hf, Wf):
        raise _lib.DmvsError(f"conv2d_k5s2_dgrad: out {tuple(out.shape)} is not the fine tensor {(Cb, D, Hf, Wf)}")
    cost = None
    if timer is not None:
        nt = 25 * Ca * Cb
        cost = (2.0 * nt * D * gy.shape[2] * gy.shape[3], 4.0 * (gy.numel() + out.numel() + nt), None)
    _launch(_lib.load().dmvs_conv2d_k5s2_dgrad, (_ptr(gy), _ptr(w), _ptr(out), Ca, D, Hf, Wf),
            f"dgrad_k5s2_{Ca}", "dgrad_k5s2", gy, (w, out), False, "conv2d_k5s2_dgrad", cost)
    return out


# ------------------------------------------------------------------------------------------ K3f (training: FeatureNet's rectangular stride-1 convs)
WGRAD_FPN_TILE = (1, 4, 32)   # tile (plane, y, x) of K3f: dmvs_conv2d_wgrad_fpn_plan counts these (csrc/conv2d_wgrad_fpn.h)
# (Cin, Cout, kernel): conv0.0, conv0.1, out3, out1, inner1, inner2 (networks/module.py:284, :285, :309, :301, :305, :306)
FPN_SHAPES = ((3, 8, 3), (8, 8, 3), (32, 16, 3), (32, 64, 1), (16, 32, 1), (8, 32, 1))
FPN_BIAS_SHAPES = ((16, 32, 1), (8, 32, 1))   # ... of which these two have a bias


def pack_index_mfma_fpn(cin: int, cout: int, ksize: int, transposed_flipped: bool, device=None) -> torch.Tensor:
    """Gather index (cached LongTensor; on the CPU, or a cached copy on ``device``) of K3's weight packing for the layer
    ``(cin, cout, ksize)`` of FPN_SHAPES, weight ``w`` [cout,cin,ksize,ksize]: ``gather_packed(w, index, True)`` equals,
    bit for bit, ``pack_mfma(w, cin, cout, mode, 1)`` with mode CONV_S1 (kernel 3) or CONV2D_K1 (kernel 1) -- for cin = 3 the packing of
    ``w`` with a zero fourth channel, as make_layer packs conv0.0.  ``transposed_flipped``: the index of
    ``pack_mfma(w.transpose(0, 1).flip(2, 3), cout, cin, mode, 1)`` instead -- the weight of the layer's data gradient, a layer
    cout -> cin (conv0.0 has none: the image takes no gradient).  These packings are selections with zeros (the zero channel, the zero
    rows of 8 output channels on the 16-row MFMA): a zero selects the one appended slot, index n = cin * cout * ksize^2.  Derived once
    on the host by packing ``iota + 1`` through the library's packer (_derive_index); every weight element must be selected exactly
    once."""
    def build():
        if (cin, cout, ksize) not in FPN_SHAPES or (transposed_flipped and cin == 3):
            raise _lib.DmvsError(f"pack_index_mfma_fpn: ({cin}, {cout}, {ksize}), transposed_flipped = {transposed_flipped} is no layer "
                                 f"of FeatureNet's head {FPN_SHAPES} (conv0.0 has no data gradient)")
        lin, lout = (cout, cin) if transposed_flipped else (max(cin, 4), cout)   # (conv0.0: K3's 4-channel layer)

        def arrange(iota):
            if transposed_flipped:
                return _transposed_flipped(iota)
            return iota if cin != 3 else torch.cat((iota, torch.zeros_like(iota[:, :1])), 1)   # (the fourth channel selects the zero)
        return _derive_index("pack_index_mfma_fpn", (cout, cin, ksize, ksize), arrange,
                             lambda w: pack_mfma(w, lin, lout, CONV_S1 if ksize == 3 else CONV2D_K1, 1), False)
    return _pack_index(("fpn", int(cin), int(cout), int(ksize), bool(transposed_flipped)), build, device)


def _wgrad_fpn_dims(x: torch.Tensor, gy: torch.Tensor, ksize: int):
    if x.dim() != 4 or gy.dim() != 4 or x.shape[1:] != gy.shape[1:] or (int(x.shape[0]), int(gy.shape[0]), int(ksize)) not in FPN_SHAPES:
        raise _lib.DmvsError(f"conv2d_wgrad_fpn: x {tuple(x.shape)} and gy {tuple(gy.shape)} must be [Cin,D,H,W] and [Cout,D,H,W] of the "
                             f"same planes with (Cin, Cout, kernel = {ksize}) in {FPN_SHAPES}")
    return (int(x.shape[0]), int(gy.shape[0]), *(int(n) for n in x.shape[1:]))


def conv2d_wgrad_fpn_workspace(Cin: int, Cout: int, ksize: int, D: int, H: int, W: int, device) -> torch.Tensor:
    """K3f's workspace, one per (shape class, device, stream): its size does not depend on D, H, W."""
    dims = (Cin, Cout, ksize, D, H, W)
    return _wgrad_workspace("conv2d_wgrad_fpn", "k3f", _lib.load().dmvs_conv2d_wgrad_fpn_workspace(*dims), dims, device)


def conv2d_wgrad_fpn(x: torch.Tensor, gy: torch.Tensor, ksize: int, out: Optional[torch.Tensor] = None,
                     bias_out: Optional[torch.Tensor] = None, accumulate: bool = False,
                     workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K3f.  x [Cin,D,H,W], gy [Cout,D,H,W] (input of a stride-1 conv of kernel ``ksize``, padding ``ksize // 2``, on D independent
    planes and the gradient on its output), (Cin, Cout, ksize) in FPN_SHAPES -> the weight gradient [Cout,Cin,ksize,ksize].
    ``bias_out`` ([Cout], the two layers of FPN_BIAS_SHAPES only): also the bias gradient, written there by the same launch.
    ``out``: buffer to write into; with ``accumulate`` both results are ADDED to their buffers (``out`` must then be given).
    ``workspace``: at least dmvs_conv2d_wgrad_fpn_workspace floats (default: a cached buffer per device and stream)."""
    _req(x, gy, out, bias_out, workspace)
    Cin, Cout, D, H, W = _wgrad_fpn_dims(x, gy, ksize)
    if accumulate and out is None:
        raise _no_buffer("conv2d_wgrad_fpn")
    if bias_out is not None:
        if (Cin, Cout, ksize) not in FPN_BIAS_SHAPES:
            raise _lib.DmvsError(f"conv2d_wgrad_fpn: the layer {(Cin, Cout, ksize)} has no bias (only {FPN_BIAS_SHAPES} have)")
        if bias_out.numel() != Cout:
            raise _lib.DmvsError(f"conv2d_wgrad_fpn: bias_out {tuple(bias_out.shape)} is not a [{Cout}] bias")
    lib, dims = _lib.load(), (Cin, Cout, ksize, D, H, W)
    out = _wgrad_out("conv2d_wgrad_fpn", out, accumulate, (Cout, Cin, ksize, ksize), x)
    workspace = _wgrad_workspace("conv2d_wgrad_fpn", "k3f", lib.dmvs_conv2d_wgrad_fpn_workspace(*dims), dims, x.device, workspace)
    cost = None
    if timer is not None:
        nt = ksize * ksize * Cin * Cout
        cost = (2.0 * nt * D * H * W, 4.0 * ((Cin + Cout) * D * H * W + nt), None)
    _launch(lib.dmvs_conv2d_wgrad_fpn,
            (_ptr(x), _ptr(gy), _ptr(out), _ptr(bias_out), _ptr(workspace), Cin, Cout, D, H, W, ksize, 1 if accumulate else 0),
            f"wgrad_fpn_{Cin}to{Cout}k{ksize}", "wgrad_fpn", x, (gy, out, bias_out, workspace), False, "conv2d_wgrad_fpn", cost)
    _log("conv2d_wgrad_fpn")   # two dispatches per call: the partials and their sum
    return out


# ------------------------------------------------------------------------------------------ K5 (training: BatchNorm + ReLU)
BN_CHANNELS = (8, 16, 32, 64)   # the channel counts K5 takes (csrc/batchnorm.h)
BN_CHUNK = 1024                 # elements of a chunk: 256 lanes x 4 floats; a share is a run of whole chunks
BN_MAX_WG = 2048                # workgroups of a launch at most: Smax = BN_MAX_WG // C shares per channel
BN_TRAIN = 32                   # include/dmvs.h DMVS_BN_TRAIN


def _bn_dims(x: torch.Tensor):
    if x.dim() < 3:
        raise _lib.DmvsError(f"bn_relu: the input must be [B,C,...], got {tuple(x.shape)}")
    B, C = int(x.shape[0]), int(x.shape[1])
    V = 1
    for n in x.shape[2:]:
        V *= int(n)
    return B, C, V


def bn_plan(C: int, B: int, V: int) -> int:
    """Shares S a channel of B * V elements is cut into by every K5 launch (grid: C * S workgroups)."""
    S = _lib.load().dmvs_bn_plan(C, B, V)
    if S <= 0:
        raise _lib.DmvsError(f"bn_relu: C = {C}, B = {B}, V = {V} is not covered by the BatchNorm kernels (C in {BN_CHANNELS})")
    return S


def bn_share_range(C: int, B: int, V: int, s: int):
    """[lo, hi) of the flattened (b, v) index that share s owns: the partition function the kernels call."""
    lo, hi = ctypes.c_long(), ctypes.c_long()
    _lib.check(_lib.load().dmvs_bn_share_range(C, B, V, s, ctypes.byref(lo), ctypes.byref(hi)), "bn_share_range")
    return lo.value, hi.value


def bn_workspace(C: int, B: int, V: int, device) -> torch.Tensor:
    """K5's workspace, one per (size, device, stream): its size does not depend on the volume."""
    n = _lib.load().dmvs_bn_workspace(C, B, V)
    if n <= 0:
        raise _lib.DmvsError(f"bn_relu: C = {C}, B = {B}, V = {V} is not covered by the BatchNorm kernels (C in {BN_CHANNELS})")
    return _workspace("k5", n, device)


def _bn_vectors(what: str, C: int, x: torch.Tensor, *vs: torch.Tensor) -> None:
    for v in vs:
        if v.numel() != C or v.device != x.device:
            raise _lib.DmvsError(f"{what}: a per-channel vector has {v.numel()} elements on {v.device}, the input {C} channels on {x.device}")


def bn_relu_forward(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, running_mean: torch.Tensor, running_var: torch.Tensor,
                    momentum: float, eps: float, relu: bool, training: bool, workspace: Optional[torch.Tensor] = None):
    """K5 forward.  x [B,C,...] -> (y, mean, invstd): y = relu(BatchNorm(x)) (``relu`` False: no ReLU), mean / invstd [C] as the
    backward takes them.  ``training``: batch statistics, and running_mean / running_var are blended in place (momentum, unbiased
    variance); else the running statistics are used and left alone."""
    _req(x, gamma, beta, running_mean, running_var, workspace)
    B, C, V = _bn_dims(x)
    _bn_vectors("bn_relu_forward", C, x, gamma, beta, running_mean, running_var)
    if training and B * V < 2:
        raise _lib.DmvsError(f"bn_relu_forward: train mode needs more than one value per channel, got input {tuple(x.shape)}")
    if workspace is None:
        workspace = bn_workspace(C, B, V, x.device)
    elif workspace.numel() < _lib.load().dmvs_bn_workspace(C, B, V):
        raise _lib.DmvsError("bn_relu_forward: workspace too small")
    y = torch.empty_like(x)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty(C, dtype=torch.float32, device=x.device)
    flags = (RELU if relu else 0) | (BN_TRAIN if training else 0)
    cost = None
    if timer is not None:
        cost = (5.0 * B * C * V, 4.0 * B * C * V * (3 if training else 2), None)
    _launch(_lib.load().dmvs_bn_relu_forward,
            (_ptr(x), _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), _ptr(y), _ptr(mean), _ptr(invstd), _ptr(workspace),
             B, C, V, float(momentum), float(eps), flags),
            f"bn{C}", "bn_relu_forward", x, (gamma, beta, running_mean, running_var, workspace), False, "batchnorm", cost)
    if training:
        _log("batchnorm")   # two dispatches in train mode: the partial statistics, then fold + apply
    return y, mean, invstd


def bn_relu_backward(x: torch.Tensor, gy: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor,
                     relu: bool, training: bool, need_gx: bool = True, workspace: Optional[torch.Tensor] = None):
    """K5 backward.  x (the forward's input), gy, and the forward's gamma / beta / mean / invstd -> (gx | None, g_gamma, g_beta).  The
    ReLU mask is recomputed from x; the forward's output is not needed.  ``need_gx`` False skips the apply launch."""
    _req(x, gy, gamma, beta, mean, invstd, workspace)
    if gy.shape != x.shape:
        raise _lib.DmvsError(f"bn_relu_backward: x {tuple(x.shape)} and gy {tuple(gy.shape)} must have the same shape")
    B, C, V = _bn_dims(x)
    _bn_vectors("bn_relu_backward", C, x, gamma, beta, mean, invstd)
    if workspace is None:
        workspace = bn_workspace(C, B, V, x.device)
    elif workspace.numel() < _lib.load().dmvs_bn_workspace(C, B, V):
        raise _lib.DmvsError("bn_relu_backward: workspace too small")
    gx = torch.empty_like(x) if need_gx else None
    g_gamma = torch.empty(C, dtype=torch.float32, device=x.device)
    g_beta = torch.empty(C, dtype=torch.float32, device=x.device)
    flags = (RELU if relu else 0) | (BN_TRAIN if training else 0)
    cost = None
    if timer is not None:
        cost = (12.0 * B * C * V, 4.0 * B * C * V * (5 if need_gx else 2), None)
    _launch(_lib.load().dmvs_bn_relu_backward,
            (_ptr(x), _ptr(gy), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), _ptr(gx), _ptr(g_gamma), _ptr(g_beta), _ptr(workspace),
             B, C, V, flags),
            f"bn{C}", "bn_relu_backward", x, (gy, gamma, beta, mean, invstd, workspace), False, "batchnorm", cost)
    _log("batchnorm")   # two dispatches: the partial sums, then fold + apply (or the fold alone)
    return gx, g_gamma, g_beta


# ------------------------------------------------------------------------------------------ K5, synchronised statistics
BN_MAX_RANKS = 16   # csrc/batchnorm.h kMaxRanks: ranks whose statistics one launch combines


def _bn_gathered(what: str, t: torch.Tensor, x: torch.Tensor, C: int, K: int) -> int:
    """A gathered [R][C][K] fp64 buffer on x's device -> R."""
    if t.dtype != torch.float64 or not t.is_contiguous() or t.device != x.device or t.dim() != 3 or tuple(t.shape[1:]) != (C, K):
        raise _lib.DmvsError(f"{what}: the gathered buffer must be a contiguous float64 [R,{C},{K}] on {x.device}, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
    R = int(t.shape[0])
    if not 1 <= R <= BN_MAX_RANKS:
        raise _lib.DmvsError(f"{what}: {R} ranks; the kernels combine 1 .. {BN_MAX_RANKS}")
    return R


def _bn_sync_ws(what: str, x: torch.Tensor, B: int, C: int, V: int, workspace):
    if workspace is None:
        return bn_workspace(C, B, V, x.device)
    if workspace.numel() < _lib.load().dmvs_bn_workspace(C, B, V):
        raise _lib.DmvsError(f"{what}: workspace too small")
    return workspace


def bn_sync_moments(x: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """This rank's moments of x [B,C,...]: float64 [C,3] = (n, mean, sum of squared deviations about that mean) per channel -- what
    travels between ranks (an all-gather along a new first axis gives ``bn_sync_forward`` its ``gathered``)."""
    _req(x, workspace)
    B, C, V = _bn_dims(x)
    workspace = _bn_sync_ws("bn_sync_moments", x, B, C, V, workspace)
    moments = torch.empty((C, 3), dtype=torch.float64, device=x.device)
    cost = (3.0 * B * C * V, 4.0 * B * C * V, None) if timer is not None else None
    _launch(_lib.load().dmvs_bn_sync_moments, (_ptr(x), _ptr(moments), _ptr(workspace), B, C, V),
            f"bn{C}", "bn_sync_moments", x, (workspace,), False, "batchnorm", cost)
    _log("batchnorm")   # two dispatches: the partial statistics, then their fold
    return moments


def bn_sync_forward(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, running_mean: torch.Tensor, running_var: torch.Tensor,
                    gathered: torch.Tensor, momentum: float, eps: float, relu: bool):
    """K5 forward on the statistics of all ranks.  ``gathered`` float64 [R,C,3]: the ``bn_sync_moments`` of every rank in rank order.
    -> (y, mean, invstd, N): y = relu(BatchNorm(x)) under the global mean and biased variance, mean / invstd [C] (the same bits on every
    rank), N the global count per channel (a host integer: the call reads the R counts back and synchronises the stream once).  The
    running buffers are blended in place with the global mean and unbiased variance."""
    _req(x, gamma, beta, running_mean, running_var)
    B, C, V = _bn_dims(x)
    _bn_vectors("bn_sync_forward", C, x, gamma, beta, running_mean, running_var)
    R = _bn_gathered("bn_sync_forward", gathered, x, C, 3)
    y = torch.empty_like(x)
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    invstd = torch.empty(C, dtype=torch.float32, device=x.device)
    n_total = ctypes.c_long(0)
    cost = (5.0 * B * C * V, 4.0 * B * C * V * 2, None) if timer is not None else None
    _launch(_lib.load().dmvs_bn_sync_forward,
            (_ptr(x), _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), _ptr(gathered), _ptr(y), _ptr(mean), _ptr(invstd),
             ctypes.byref(n_total), B, C, V, R, float(momentum), float(eps), RELU if relu else 0),
            f"bn{C}", "bn_sync_forward", x, (gamma, beta, running_mean, running_var, gathered), False, "batchnorm", cost)
    return y, mean, invstd, n_total.value


def bn_sync_backward_sums(x: torch.Tensor, gy: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, mean: torch.Tensor,
                          invstd: torch.Tensor, relu: bool, workspace: Optional[torch.Tensor] = None):
    """This rank's backward sums under the global mean / invstd of ``bn_sync_forward``: -> (sums float64 [C,2] = (sum g, sum g * xhat)
    -- what travels --, g_gamma, g_beta): the two fp32 gradients are the LOCAL sums."""
    _req(x, gy, gamma, beta, mean, invstd, workspace)
    if gy.shape != x.shape:
        raise _lib.DmvsError(f"bn_sync_backward_sums: x {tuple(x.shape)} and gy {tuple(gy.shape)} must have the same shape")
    B, C, V = _bn_dims(x)
    _bn_vectors("bn_sync_backward_sums", C, x, gamma, beta, mean, invstd)
    workspace = _bn_sync_ws("bn_sync_backward_sums", x, B, C, V, workspace)
    sums = torch.empty((C, 2), dtype=torch.float64, device=x.device)
    g_gamma = torch.empty(C, dtype=torch.float32, device=x.device)
    g_beta = torch.empty(C, dtype=torch.float32, device=x.device)
    cost = (7.0 * B * C * V, 4.0 * B * C * V * 2, None) if timer is not None else None
    _launch(_lib.load().dmvs_bn_sync_backward_sums,
            (_ptr(x), _ptr(gy), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), _ptr(sums), _ptr(g_gamma), _ptr(g_beta),
             _ptr(workspace), B, C, V, RELU if relu else 0),
            f"bn{C}", "bn_sync_backward_sums", x, (gy, gamma, beta, mean, invstd, workspace), False, "batchnorm", cost)
    _log("batchnorm")   # two dispatches: the partial sums, then their fold
    return sums, g_gamma, g_beta


def bn_sync_backward_apply(x: torch.Tensor, gy: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, mean: torch.Tensor,
                           invstd: torch.Tensor, gathered: torch.Tensor, N: int, relu: bool) -> torch.Tensor:
    """gx of this rank from the sums of all ranks.  ``gathered`` float64 [R,C,2]: the ``bn_sync_backward_sums`` of every rank in rank
    order; ``N`` the global count ``bn_sync_forward`` returned."""
    _req(x, gy, gamma, beta, mean, invstd)
    if gy.shape != x.shape:
        raise _lib.DmvsError(f"bn_sync_backward_apply: x {tuple(x.shape)} and gy {tuple(gy.shape)} must have the same shape")
    B, C, V = _bn_dims(x)
    _bn_vectors("bn_sync_backward_apply", C, x, gamma, beta, mean, invstd)
    R = _bn_gathered("bn_sync_backward_apply", gathered, x, C, 2)
    gx = torch.empty_like(x)
    cost = (8.0 * B * C * V, 4.0 * B * C * V * 3, None) if timer is not None else None
    _launch(_lib.load().dmvs_bn_sync_backward_apply,
            (_ptr(x), _ptr(gy), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(invstd), _ptr(gathered), _ptr(gx), B, C, V, R, int(N),
             RELU if relu else 0),
            f"bn{C}", "bn_sync_backward_apply", x, (gy, gamma, beta, mean, invstd, gathered), False, "batchnorm", cost)
    return gx
