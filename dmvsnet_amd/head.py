"""Differentiable dual-depth head: K4 with its backward K4b, and the dual-depth loss N6 with its backward N6b, behind
torch.autograd.

With ``DiffCostAgg`` these are the DMVSNet-specific operators of a training step; a reference user swaps three lines::

    self.cost_aggregation = dmvsnet_amd.DiffCostAgg(agg_mode, self.feature.out_channels)
    self.DepthNet = dmvsnet_amd.DiffDepthNet(depth_mode)
    loss = dmvsnet_amd.diff_mvs_loss(outputs, depth_gt_ms, mask_ms, "regression", dlossw=dlossw)

and keeps ``nn.Conv3d`` / ``nn.Conv2d`` on ATen (``dmvsnet_amd.MVSNet.train()`` still raises).

``DiffDepthNet`` has the reference's ``DepthNet.forward`` / ``.refine`` (networks/mvsnet.py:15-100).  The forward is the eval path's
kernel (``ops.depth_regress``), bit for bit; autograd keeps only the logits, the hypotheses and ``depth_sub_plus`` -- all three alive
in the graph anyway -- where the reference keeps a softmax volume, ``p * depth`` and some sixty planes per pass.  The backward
recomputes the softmax in the forward's operation order and routes min / max by the forward's ``depth_sub_plus``.

Gradient edges, as in the reference's graph:

* ``depth_sub_plus``, ``depth_values_c``, ``depth_sub_plus_refine``, ``depth`` are differentiable with respect to the logits AND the
  hypotheses.  ``depth_values_c`` is not detached in the reference (only ``last_depth`` between stages is, mvsnet.py:221): it is the
  refine pass's hypothesis volume, so the refine loss reaches the main pass's logits through it.  ``DiffCostAgg`` returns no gradient
  for its hypotheses (the reference builds the grid under ``no_grad``), so this is the only way back.
* ``prob_volume`` (only the classification / focal losses read it; out of scope) and the two confidences (computed under
  ``no_grad`` in the reference) are marked non-differentiable.

``diff_mvs_loss`` has the signature of the reference's ``mvs_loss`` (loss.py:5) and of ``validate.mvs_loss``; its value is
``validate.mvs_loss``'s, bit for bit (the same launches, adding into one device scalar in stage order); its backward is one gather
launch per stage.  It differentiates the PRODUCT's forward, including its two documented deviations from the reference: exact
quarter weights at the cell centres, and every all-valid 2x2 cell kept.  An empty mask gives a NaN loss (as the reference) and an
all-zero gradient.

fp32 on a HIP device only; a batch runs as its samples one after the other.  Both backwards use plain stores with one writer per
element: the gradients are bitwise reproducible.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import ops, validate
from ._lib import DmvsError

__all__ = ["DiffDepthNet", "diff_mvs_loss", "depth_regress", "launch_counts", "MAX_D"]

MAX_D = 64   # K4b keeps the D logits of a channel in registers

# launches of the two backward kernels since import (tests check through them that frozen inputs skip their kernel)
launch_counts = {"regress_bwd": 0, "loss_bwd": 0}


class _RegressFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, hyp, interval, alpha, mode, want_prob):
        lg, hp = logits.detach().contiguous(), hyp.detach().contiguous()
        outs = [ops.depth_regress(lg[b], hp[b], interval, alpha, mode, want_prob) for b in range(lg.shape[0])]
        if len(outs) == 1:
            dsp, sel, conf, prob = [None if t is None else t.unsqueeze(0) for t in outs[0]]
        else:
            dsp, sel, conf, prob = [None if ts[0] is None else torch.stack(ts) for ts in zip(*outs)]
        ctx.save_for_backward(lg, hp, dsp)
        ctx.alpha, ctx.mode = alpha, mode
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*[t for t in (conf, prob) if t is not None])   # one call: a second one replaces the first
        return dsp, sel, conf, prob

    @staticmethod
    @once_differentiable
    def backward(ctx, g_dsp, g_sel, g_conf, g_prob):
        need_logits, need_hyp = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_logits or need_hyp) or (g_dsp is None and g_sel is None):
            return None, None, None, None, None, None
        lg, hp, dsp = ctx.saved_tensors
        g_dsp = None if g_dsp is None else g_dsp.contiguous()
        g_sel = None if g_sel is None else g_sel.contiguous()
        # one kernel writes both gradients; with frozen logits and live hypotheses the logit gradient is scratch
        g_logits = torch.empty_like(lg)
        g_hyp = torch.empty_like(hp) if need_hyp else None
        for b in range(lg.shape[0]):
            ops.depth_regress_backward(lg[b], hp[b], ctx.alpha, ctx.mode, dsp[b], None if g_dsp is None else g_dsp[b],
                                       None if g_sel is None else g_sel[b], need_hyp, g_logits[b], None if g_hyp is None else g_hyp[b])
            launch_counts["regress_bwd"] += 1
        return (g_logits if need_logits else None), g_hyp, None, None, None, None


def _check(what, cost_reg, depth_values):
    for name, t in (("cost_reg", cost_reg), ("depth_values", depth_values)):
        if not torch.is_tensor(t):
            raise DmvsError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise DmvsError(f"{what} runs on the HIP kernels only (no CPU fallback); {name} is on {t.device}")
        if t.dtype != torch.float32:
            raise DmvsError(f"{what} is fp32 only (no fp16 / autocast in the differentiable path); {name} is {t.dtype}")
    if cost_reg.dim() != 5 or cost_reg.shape[1] != 4:
        raise DmvsError(f"{what}: cost_reg must be [B,4,D,H,W], got {tuple(cost_reg.shape)}")
    B, _, D, H, W = cost_reg.shape
    if tuple(depth_values.shape) != (B, D, H, W):
        raise DmvsError(f"{what}: depth_values must be [B,D,H,W] = {(B, D, H, W)}, got {tuple(depth_values.shape)}")
    if D > MAX_D:
        raise DmvsError(f"{what}: D = {D}; the backward kernel is built for D <= {MAX_D}")


def depth_regress(cost_reg: torch.Tensor, depth_values: torch.Tensor, interval, alpha: float = 1.0, mode: int = 0,
                  prob_volume: bool = False):
    """K4 behind autograd: cost_reg [B,4,D,H,W], depth_values [B,D,H,W] -> (depth_sub_plus [B,4,H,W], selection ([B,4,H,W] mode 0:
    depth_values_c | [B,H,W] mode 1: depth), confidence [B,H,W], softmax volume [B,4,D,H,W] | None).  The first two are
    differentiable with respect to both inputs; the confidence and the volume are not."""
    _check("depth_regress", cost_reg, depth_values)
    if mode not in (0, 1):
        raise DmvsError(f"depth_regress: mode {mode}")
    itv = torch.as_tensor(interval, dtype=torch.float32, device=cost_reg.device).detach().reshape(-1)[:1].contiguous()
    return _RegressFn.apply(cost_reg, depth_values, itv, float(alpha), int(mode), bool(prob_volume))


class DiffDepthNet(nn.Module):
    """Drop-in for the reference's ``DepthNet`` (networks/mvsnet.py:11-100) that autograd can differentiate on the product's
    kernels.  Owns no parameters.  ``prob_volume=False`` skips writing the softmax volume (the regression loss never reads it) and
    leaves the key out.  Differentiable outputs: ``depth_sub_plus``, ``depth_values_c``, ``depth_sub_plus_refine``, ``depth``.
    NOT differentiable: ``prob_volume``, ``photometric_confidence``, ``photometric_confidence_refine``."""

    def __init__(self, mode="regression", prob_volume=True):
        super().__init__()
        if mode != "regression":
            raise NotImplementedError(f"DiffDepthNet: mode {mode!r} is not implemented (only 'regression', the mode the "
                                      "reference's scripts use)")
        self.mode = mode
        self.prob_volume = bool(prob_volume)

    def forward(self, cost_reg, depth_values, num_depth=None, interval=None, prob_volume_init=None, stage=0):
        _check("DiffDepthNet.forward", cost_reg, depth_values)
        dsp, hyps, conf, prob = depth_regress(cost_reg, depth_values, interval, 1.0, 0, self.prob_volume)
        out = {"photometric_confidence": conf, "depth_sub_plus": dsp, "depth_values_c": hyps, "depth_values": depth_values,
               "interval": interval}
        if prob is not None:
            out["prob_volume"] = prob
        return out

    def refine(self, cost_reg, depth_values, num_depth=None, interval=None, alpha=5):
        _check("DiffDepthNet.refine", cost_reg, depth_values)
        dsp, depth, conf, _ = depth_regress(cost_reg, depth_values, interval, float(alpha), 1, False)
        return {"depth": depth, "photometric_confidence_refine": conf, "depth_sub_plus_refine": dsp}


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, *tensors):
        # tensors: per stage (depth_sub_plus, depth_sub_plus_refine, gt, mask), already fp32 / contiguous / on one device
        K = len(tensors) // 4
        dev = tensors[0].device
        total = torch.zeros(1, dtype=torch.float32, device=dev)
        counts = torch.empty((K, 2), dtype=torch.int64, device=dev)
        for k in range(K):
            main, refine, gt, mask = [t.detach() for t in tensors[4 * k:4 * k + 4]]
            validate._launch(main, refine, gt, mask, None, weights[k], validate.THRES_MM, total, None, counts[k], None, None)
        ctx.weights = list(weights)
        ctx.save_for_backward(counts, *tensors)
        return total[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        counts, *tensors = ctx.saved_tensors
        grads = [None] * len(tensors)
        g_total = g.detach().to(torch.float32).reshape(1).contiguous()
        for k in range(len(tensors) // 4):
            main, refine, gt, mask = tensors[4 * k:4 * k + 4]
            need_main, need_refine = ctx.needs_input_grad[1 + 4 * k], ctx.needs_input_grad[2 + 4 * k]
            if not (need_main or need_refine):
                continue
            grads[4 * k], grads[4 * k + 1] = ops.dual_depth_loss_backward(main, refine, gt, mask, ctx.weights[k], counts[k], g_total,
                                                                          need_main, need_refine)
            launch_counts["loss_bwd"] += 1
        return (None, *grads)


def diff_mvs_loss(inputs, depth_gt_ms, mask_ms, mode, **kwargs):
    """Drop-in for the reference's ``mvs_loss`` (loss.py:5) in mode "regression" that autograd can differentiate: arguments and value
    as ``validate.mvs_loss`` (bit for bit); gradients flow to every stage's ``depth_sub_plus`` and ``depth_sub_plus_refine``."""
    if mode != "regression":
        raise NotImplementedError(f"diff_mvs_loss: mode {mode!r} is not implemented (only 'regression'; the classification / focal "
                                  "losses and the prob_volume gradient are out of scope)")
    keys = [k for k in inputs.keys() if "stage" in k]
    if not keys:
        raise DmvsError("diff_mvs_loss: no 'stage' entries in the inputs")
    weights = kwargs.get("dlossw", [1.0 for _ in keys])
    tensors, stage_weights = [], []
    for k in keys:
        stage = inputs[k]
        for name in ("depth_sub_plus", "depth_sub_plus_refine"):
            t = stage[name]
            if torch.is_tensor(t) and t.is_cuda and t.dtype != torch.float32:
                raise DmvsError(f"diff_mvs_loss is fp32 only; {k}.{name} is {t.dtype}")
        gt = validate._plane(depth_gt_ms[k], f"depth_gt_ms[{k!r}]")
        if gt.dim() != 3:
            raise DmvsError(f"depth_gt_ms[{k!r}]: expected [B,h,w], got {tuple(gt.shape)}")
        B, h, w = gt.shape
        mask = validate._plane(mask_ms[k], f"mask_ms[{k!r}]", gt.shape)
        main = validate._plane(stage["depth_sub_plus"], f"{k}.depth_sub_plus", (B, 4, h, w))
        refine = validate._plane(stage["depth_sub_plus_refine"], f"{k}.depth_sub_plus_refine", (B, 4, h, w))
        if len({t.device for t in (gt, mask, main, refine)}) != 1:
            raise DmvsError(f"diff_mvs_loss: the tensors of {k} are on different devices")
        tensors += [main, refine, gt, mask]
        stage_weights.append(float(weights[int(k.replace("stage", "")) - 1]))
    with torch.cuda.device(tensors[0].device):
        return _LossFn.apply(stage_weights, *tensors)
