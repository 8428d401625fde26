"""Differentiable cost aggregation: the fused warp + correlation (K1) with its backward (K1b) behind torch.autograd.

The one piece of training that runs on the product's kernels.  ``DiffCostAgg`` has the constructor and the
``forward(features, proj_matrices, depth_values, stage_idx)`` of the reference's ``CostAgg`` (networks/mvsnet.py:102-153), so
a reference user changes one line::

    self.cost_aggregation = dmvsnet_amd.DiffCostAgg(agg_mode, self.feature.out_channels)

and keeps the reference module for everything else (``dmvsnet_amd.MVSNet.train()`` still raises).

Gradients flow to the feature maps only.  The reference builds the sampling grid under ``torch.no_grad()``
(networks/module.py:222-243), so its autograd graph has no edge to the cameras or to the depth hypotheses either: the ``None``
this backward returns for them is the reference's behaviour, not an omission.

The forward is the product kernel (quad-planar features, direct-form coordinates); the backward recomputes the taps with the
generic kernel's routine in the reference's op order.  The two differ by < 1e-4 px in the tap position,
i.e. the gradient is taken at taps that differ from the forward's at the fp32 rounding level.  The reference-view gradient is
bitwise reproducible.  The source-view gradients are accumulated with floating-point atomics by default: equal run to run only to
fp32 rounding.  In DETERMINISTIC mode (``deterministic=True``, or ``None`` under ``torch.use_deterministic_algorithms(True)``)
they are accumulated in fixed point instead (``ops.warp_corr_backward_det``: the same scatter kernel on csrc/warp_corr_bwd_det.h's
``FixedSink``): bitwise reproducible, a pure function of the sample's inputs -- independent of the batch around it and of which
other views want a gradient.  ``presum=True`` takes the source scatter of either mode through ``ops.warp_corr_backward_presum``
(csrc/warp_corr_bwd_presum.h: a workgroup's addends are summed in an LDS window before they reach memory): the same bits in
deterministic mode, the same addends in another order of the fp32 sum otherwise.  Off by default.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, ops

SUPPORTED_C = (8, 16, 32)

# launches of the two backward kernels since import (tests check through them that a frozen input skips its kernel)
launch_counts = {"bwd_ref": 0, "bwd_src_views": 0}
# the same for backwards taken in deterministic mode (which leave ``launch_counts`` alone)
det_launch_counts = {"bwd_ref": 0, "bwd_src_views": 0}
# the same for backwards taken with ``presum=True``, in either mode (which leave both dicts above alone)
presum_launch_counts = {"bwd_ref": 0, "bwd_src_views": 0}


class _CostAggFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mode, proj_matrices, depth_values, *features):
        ctx.deterministic, ctx.presum = (bool(m) for m in mode)
        B, C, H, W = features[0].shape
        D = depth_values.shape[1]
        V = len(features)
        depth = depth_values.detach().contiguous()
        pairs = proj_matrices.detach().contiguous()
        sim = torch.empty((B, 2, D, H, W), dtype=torch.float32, device=depth.device)
        q4 = torch.empty((B, V, C // 4, H, W, 4), dtype=torch.float32, device=depth.device)
        proj12 = torch.empty((B, V - 1, 12), dtype=torch.float32, device=depth.device)
        for b in range(B):   # a batch runs as its samples one after the other
            proj12[b].copy_(ops.relative_proj(pairs[b]))
            for v in range(V):
                ops.nchw_to_q4(features[v].detach()[b], out=q4[b, v])
            ops.warp_corr(q4[b, 0], [q4[b, v] for v in range(1, V)], proj12[b], depth[b], out=sim[b], layout="q4")
        ctx.save_for_backward(q4, proj12, depth)
        return sim

    @staticmethod
    @once_differentiable
    def backward(ctx, gsim):
        q4, proj12, depth = ctx.saved_tensors
        B, V = q4.shape[:2]
        C, H, W = 4 * q4.shape[2], q4.shape[3], q4.shape[4]
        need = ctx.needs_input_grad[3:]
        det = ctx.deterministic
        gsim = gsim.contiguous()
        grads: List = [None] * V
        if need[0]:
            grads[0] = torch.empty((B, C, H, W), dtype=torch.float32, device=q4.device)
        for v in range(1, V):
            if need[v]:   # the fixed-point path writes every element; the atomics add into zeros
                grads[v] = (torch.empty if det else torch.zeros)((B, C, H, W), dtype=torch.float32, device=q4.device)
        if any(need):
            nact = sum(int(n) for n in need[1:])
            counts = presum_launch_counts if ctx.presum else det_launch_counts if det else launch_counts
            run, mode = ops.warp_corr_backward, {}
            if ctx.presum:
                run, mode = ops.warp_corr_backward_presum, {"deterministic": det}
            elif det:
                run = ops.warp_corr_backward_det
            if det:
                if nact:   # one workspace for the batch: the samples run one after the other on one stream
                    nbytes = ops.warp_corr_backward_det_workspace(C, H, W, nact)
                    mode["workspace"] = torch.empty((nbytes // 8,), dtype=torch.int64, device=q4.device)
            for b in range(B):
                run(q4[b, 0], [q4[b, v] for v in range(1, V)], proj12[b], depth[b], gsim[b],
                    None if grads[0] is None else grads[0][b], [None if grads[v] is None else grads[v][b] for v in range(1, V)], **mode)
                counts["bwd_ref"] += int(need[0])
                counts["bwd_src_views"] += nact
        # the mode (deterministic, presum); cameras, hypotheses: the reference's grid is built under no_grad (module.py:222-243) -- no gradient exists
        return (None, None, None, *grads)


def cost_agg(features: Sequence[torch.Tensor], proj_matrices: torch.Tensor, depth_values: torch.Tensor,
             deterministic: Optional[bool] = None, presum: bool = False) -> torch.Tensor:
    """features: V tensors [B,C,H,W] fp32 on a HIP device, reference view first; proj_matrices [B,V,2,4,4]; depth_values
    [B,D,H,W] -> similarity volume [B,2,D,H,W] (group k = mean over g of warped[2g+k] * ref[2g+k], summed over the source
    views), differentiable with respect to the feature maps.  ``deterministic``: True / False force the mode of the backward's
    source-view gradients (fixed-point, bitwise reproducible / fp32 atomics); None follows
    ``torch.are_deterministic_algorithms_enabled()`` at the time of this forward.  ``presum``: True takes the backward's source scatter, in
    whichever mode ``deterministic`` resolves to, through ``ops.warp_corr_backward_presum``.  The forward and dRef are the same either
    way."""
    features = list(features)
    V = len(features)
    for t in (*features, proj_matrices, depth_values):
        if not torch.is_tensor(t):
            raise _lib.DmvsError("cost_agg: features, proj_matrices and depth_values must be tensors")
        if not t.is_cuda:
            raise _lib.DmvsError(f"cost_agg runs on the HIP kernels only (no CPU fallback); got a tensor on {t.device}")
        if t.dtype != torch.float32:
            raise _lib.DmvsError(f"cost_agg is fp32 only (no fp16 / autocast features in the differentiable path); got {t.dtype}")
    if V < 2 or V - 1 > 16:
        raise _lib.DmvsError(f"cost_agg needs a reference and 1..16 source views, got {V} feature maps")
    if features[0].dim() != 4 or any(f.shape != features[0].shape for f in features):
        raise _lib.DmvsError("cost_agg: every feature map must be [B,C,H,W] of one shape")
    B, C, H, W = features[0].shape
    if C not in SUPPORTED_C:
        raise _lib.DmvsError(f"cost_agg: C = {C} is not built (C in {SUPPORTED_C})")
    if tuple(proj_matrices.shape) != (B, V, 2, 4, 4):
        raise _lib.DmvsError(f"cost_agg: proj_matrices must be [B,V,2,4,4] = {(B, V, 2, 4, 4)}, got {tuple(proj_matrices.shape)}")
    if depth_values.dim() != 4 or depth_values.shape[0] != B or tuple(depth_values.shape[2:]) != (H, W):
        raise _lib.DmvsError(f"cost_agg: depth_values must be [B,D,H,W] with the features' B, H, W, got {tuple(depth_values.shape)}")
    if deterministic is None:
        deterministic = torch.are_deterministic_algorithms_enabled()
    return _CostAggFn.apply((bool(deterministic), bool(presum)), proj_matrices, depth_values, *features)


class DiffCostAgg(nn.Module):
    """Drop-in for the reference's ``CostAgg`` (networks/mvsnet.py:102-153, "variance" mode) that autograd can differentiate.
    Owns no parameters; train and eval mode compute the same thing."""

    def __init__(self, mode="variance", in_channels=None, deterministic=None, presum=False):
        super().__init__()
        assert mode in ("variance", "adaptive"), "Don't support {}!".format(mode)
        if mode == "adaptive":
            raise NotImplementedError("agg_mode='adaptive' is unreachable from the reference's scripts "
                                      "(SURVEY.md section 2 row 8) and is not built")
        self.mode = mode
        self.deterministic = deterministic   # as cost_agg's keyword
        self.presum = bool(presum)           # as cost_agg's keyword

    def forward(self, features, proj_matrices, depth_values, stage_idx=None):
        return cost_agg(features, proj_matrices, depth_values, deterministic=self.deterministic, presum=self.presum)
