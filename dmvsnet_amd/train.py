"""The training model: the differentiable parts of this package assembled into the reference's ``MVSNet`` (networks/mvsnet.py:156-260),
and one training step on it.  No kernel of its own: every convolution, BatchNorm + ReLU, the cost aggregation, the dual-depth head and
the loss run on the gfx950 kernels behind ``DiffFeatureNet``, ``DiffCostAgg``, the four ``DiffCostRegNet*``, ``DiffDepthNet`` and
``diff_mvs_loss``.  What stays on ATen is what those modules leave there: the skip additions, the channel ``cat`` / ``split`` and
FeatureNet's two nearest up-samplings (elementwise or views).

``DiffMVSNet`` has the reference's positional arguments, children (``feature``, ``cost_aggregation``, ``cost_regularization``,
``cost_regularization_refine``, ``DepthNet``) and state-dict keys: a reference checkpoint's ``model`` entry loads with ``strict=True``, and
the state dict loads into ``dmvsnet_amd.MVSNet`` (the inference path) and back.  ``forward(imgs, proj_matrices, depth_values)`` returns
the reference's dict: ``stage1`` .. ``stage3`` plus the last stage's entries at top level.  Train and eval mode both run; a reference user
swaps the constructor at model.py:32 and the loss at model.py:47.

The wiring of ``forward`` is ONE plain function, ``wire(parts, ...)``, over a small namespace of callables (``Parts``).
``DiffMVSNet.forward`` calls it with its own children; the tests call the same function with stock ATen parts in float64 on the CPU and
hold it to the reference there, where no ReLU decision can flip ("Testing a whole training step").  What the function keeps of
the reference's graph:

* FeatureNet runs once PER VIEW on [B,3,H,W], not on a B * V batch: in train mode each call normalises with its own batch statistics
  and blends the running buffers, ``num_batches_tracked`` advances by V per step (mvsnet.py:200-202);
* ``last_depth`` is detached between the stages (:221), and the hypothesis planes are built under ``no_grad``;
* ``depth_values_c`` is NOT detached: it is the refine pass's hypothesis volume and reaches the main pass's logits through the head's
  backward (``dmvsnet_amd.head``).  The cost aggregation returns no gradient for its hypotheses, as in the reference.

One deviation: with B > 1 the reference takes ``depth_interval`` and the first stage's planes' interval from sample 0 of
``depth_values`` (mvsnet.py:196, module.py:564); here every sample's planes come from its own row of ``depth_values``.  Batches whose
samples share one depth range (DTU) give the reference's result.  The ``interval`` entry of the outputs, which only the (non
differentiable) confidences read, is sample 0's, as in the reference.

Refused with a ``DmvsError`` that names the rule, in the constructor or at the top of ``forward``: anything but three stages,
``cr_base_chs`` other than 8, an ``ndepths[i]`` that is no multiple of 8 or exceeds ``head.MAX_D``, H or W that is no multiple of 32
(stage-1 volume extents must be multiples of 8), V outside 2 .. 17, inputs that are not fp32 on a HIP device, and the modes the parts do
not build (``fea_mode`` other than "fpn", ``agg_mode`` other than "variance", ``depth_mode`` other than "regression").
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict

import torch
from torch import nn

from . import head, ops, validate
from ._lib import DmvsError
from .costagg import DiffCostAgg
from .featurenet import DiffFeatureNet
from .head import DiffDepthNet, diff_mvs_loss
from .regnet import DiffCostRegNet, DiffCostRegNetRefine

__all__ = ["DiffMVSNet", "Parts", "wire", "train_step", "NUM_STAGE", "MAX_VIEWS", "REFINE_D"]

NUM_STAGE = 3     # the feature pyramid has three levels (mvsnet.py:214-216; a fourth stage raises KeyError in the reference)
MAX_VIEWS = 17    # a reference view and the 16 source views K1 takes
REFINE_D = 4      # planes of the refine pass: depth_values_c


class Parts(SimpleNamespace):
    """What ``wire`` calls, on tensors with a leading batch axis:

    ``feature(img [B,3,H,W])`` -> {"stage1", "stage1_c", ... "stage3_c"};
    ``cost_agg(features, proj [B,V,2,4,4], hyp [B,D,h,w])`` -> [B,2,D,h,w];
    ``regnet[s](vol)`` / ``regnet_refine[s](vol)`` -> [B,4,D,h,w];
    ``head(cost_reg, hyp, interval)`` -> dict with ``depth_sub_plus``, ``depth_values_c``, ...;
    ``head_refine(cost_reg, hyp_c, interval)`` -> dict with ``depth``, ``depth_sub_plus_refine``, ...;
    ``hypotheses_first(depth_values [B,n], D, h, w, inverse)`` -> (planes [B,D,h,w], interval);
    ``hypotheses_next(last_depth [B,h,w], depth_values [B,n], ratio, D, inverse)`` -> (planes [B,D,2h,2w], interval)."""


def wire(parts, imgs, proj_matrices, depth_values, ndepths, depth_interval_ratio, inverse_depth=False):
    """The reference's ``MVSNet.forward`` (networks/mvsnet.py:188-260) over ``parts``."""
    features = [parts.feature(imgs[:, v]) for v in range(imgs.shape[1])]   # once per view (:200-202)
    H, W = (int(n) for n in imgs.shape[-2:])
    outputs = {}
    last_depth = None
    for s, D in enumerate(ndepths):
        key = "stage{}".format(s + 1)
        scale = 2 ** (len(ndepths) - s - 1)                                 # stage1: 1/4, stage2: 1/2, stage3: 1 (:214)
        with torch.no_grad():
            if s == 0:
                hyp, interval = parts.hypotheses_first(depth_values, D, H // scale, W // scale, inverse_depth)
            else:
                hyp, interval = parts.hypotheses_next(last_depth.detach(), depth_values, depth_interval_ratio[s], D, inverse_depth)
        proj = proj_matrices[key]
        cost_reg = parts.regnet[s](parts.cost_agg([f[key] for f in features], proj, hyp))
        out_main = parts.head(cost_reg, hyp, interval)
        hyp_c = out_main["depth_values_c"]                                  # NOT detached (:246)
        cost_reg_c = parts.regnet_refine[s](parts.cost_agg([f[key + "_c"] for f in features], proj, hyp_c))
        out_refine = parts.head_refine(cost_reg_c, hyp_c, interval)
        outputs_stage = {**out_refine, **out_main}                          # :254
        last_depth = outputs_stage["depth"]
        outputs[key] = outputs_stage
        outputs.update(outputs_stage)
    return outputs


def _hypotheses_first(depth_values, D, h, w, inverse):
    per = [ops.hypotheses_first(dv.contiguous(), D, h, w, inverse) for dv in depth_values]   # every sample from its own depth range
    return torch.stack([p for p, _ in per]), per[0][1]


def _hypotheses_next(last_depth, depth_values, ratio, D, inverse):
    per = [ops.hypotheses_next(ld.contiguous(), dv.contiguous(), ratio, D, inverse) for ld, dv in zip(last_depth, depth_values)]
    return torch.stack([p for p, _ in per]), per[0][1]


def _check_config(ndepths, depth_interval_ratio, cr_base_chs, fea_mode, agg_mode, depth_mode):
    what = "DiffMVSNet"
    if len(ndepths) != NUM_STAGE or len(depth_interval_ratio) != NUM_STAGE:
        raise DmvsError(f"{what}: three stages only (the feature pyramid has three levels); got ndepths = {list(ndepths)}, "
                        f"depth_interval_ratio = {list(depth_interval_ratio)}")
    if len(cr_base_chs) != NUM_STAGE or any(c != 8 for c in cr_base_chs):
        raise DmvsError(f"{what}: cr_base_chs must be 8 at every stage (the channel counts the kernels compile); got {list(cr_base_chs)}")
    for i, D in enumerate(ndepths):
        if int(D) != D or D < 8 or D % 8 or D > head.MAX_D:
            raise DmvsError(f"{what}: every ndepths[i] must be a multiple of 8 (three stride-2 levels of the regularisation network) and "
                            f"<= head.MAX_D = {head.MAX_D} (the head's backward kernel); got ndepths[{i}] = {D}")
    if fea_mode != "fpn":
        raise DmvsError(f"{what}: fea_mode must be 'fpn' (the only FeatureNet that is built); got {fea_mode!r}")
    if agg_mode != "variance":
        raise DmvsError(f"{what}: agg_mode must be 'variance' ('adaptive' is unreachable from the reference's scripts and not built); got "
                        f"{agg_mode!r}")
    if depth_mode != "regression":
        raise DmvsError(f"{what}: depth_mode must be 'regression' (the classification / focal losses are not built); got {depth_mode!r}")


def _check_inputs(what, imgs, proj_matrices, depth_values):
    """The refusals of ``forward``: the shape rules first (they hold for tensors on any device), then fp32 on a HIP device."""
    if not torch.is_tensor(imgs) or imgs.dim() != 5 or imgs.shape[2] != 3:
        raise DmvsError(f"{what}: imgs must be a [B,V,3,H,W] tensor, got {tuple(imgs.shape) if torch.is_tensor(imgs) else type(imgs).__name__}")
    B, V, _, H, W = (int(n) for n in imgs.shape)
    if H % 32 or W % 32 or H < 32 or W < 32:
        raise DmvsError(f"{what}: H and W must be multiples of 32 (the stage-1 volume is H / 4 x W / 4, and the regularisation networks "
                        f"take extents that are multiples of 8); got H, W = {(H, W)}")
    if not 2 <= V <= MAX_VIEWS:
        raise DmvsError(f"{what}: 2 <= V <= {MAX_VIEWS} views (a reference view and 1 .. 16 source views); got V = {V}")
    if not torch.is_tensor(depth_values) or depth_values.dim() != 2 or depth_values.shape[0] != B or depth_values.shape[1] < 2:
        raise DmvsError(f"{what}: depth_values must be a [B,n] tensor with the images' B = {B} and n >= 2, got "
                        f"{tuple(depth_values.shape) if torch.is_tensor(depth_values) else type(depth_values).__name__}")
    tensors = [("imgs", imgs), ("depth_values", depth_values)]
    for s in range(NUM_STAGE):
        key = "stage{}".format(s + 1)
        p = proj_matrices.get(key) if isinstance(proj_matrices, dict) else None
        if not torch.is_tensor(p) or tuple(p.shape) != (B, V, 2, 4, 4):
            raise DmvsError(f"{what}: proj_matrices[{key!r}] must be a [B,V,2,4,4] = {(B, V, 2, 4, 4)} tensor, got "
                            f"{tuple(p.shape) if torch.is_tensor(p) else type(p).__name__}")
        tensors.append((f"proj_matrices[{key!r}]", p))
    for name, t in tensors:
        if not t.is_cuda or t.dtype != torch.float32:
            raise DmvsError(f"{what}: fp32 on a HIP device only (no CPU fallback, no fp16 / autocast in the differentiable path); {name} is "
                            f"{t.dtype} on {t.device}")
    if len({t.device for _, t in tensors}) != 1:
        raise DmvsError(f"{what}: the inputs are on different devices: {sorted({str(t.device) for _, t in tensors})}")


class DiffMVSNet(nn.Module):
    """The reference's ``MVSNet`` on the differentiable gfx950 parts; see the module's text.  Beyond the reference's arguments:
    ``deterministic`` goes to ``DiffCostAgg`` (True: bitwise reproducible source-view gradients; None follows
    ``torch.are_deterministic_algorithms_enabled()``); ``presum`` goes there too (True: the backward's source scatter pre-summed in
    LDS windows, in whichever mode ``deterministic`` resolves to; the default False is the plain scatter);
    ``prob_volume=True`` adds the softmax volume to the outputs (the regression loss never reads it); ``verbose=True`` prints the configuration as the reference does on construction."""

    def __init__(self, ndepths, depth_interval_ratio, cr_base_chs=None, fea_mode="fpn", agg_mode="variance", depth_mode="regression",
                 winner_take_all_to_generate_depth=True, inverse_depth=False, deterministic=None, prob_volume=False, verbose=False,
                 presum=False):
        super().__init__()
        if cr_base_chs is None:
            cr_base_chs = [8] * len(ndepths)
        _check_config(ndepths, depth_interval_ratio, cr_base_chs, fea_mode, agg_mode, depth_mode)
        self.ndepths = [int(D) for D in ndepths]
        self.depth_interval_ratio = list(depth_interval_ratio)
        self.fea_mode = fea_mode
        self.cr_base_chs = list(cr_base_chs)
        self.num_stage = len(ndepths)
        self.inverse_depth = bool(inverse_depth)
        if verbose:   # mvsnet.py:169-174
            print("netphs:", ndepths)
            print("depth_intervals_ratio:", depth_interval_ratio)
            print("cr_base_chs:", cr_base_chs)
            print("fea_mode:", fea_mode)
            print("agg_mode:", agg_mode)
            print("depth_mode:", depth_mode)
        self.feature = DiffFeatureNet(base_channels=8, stride=4, num_stage=self.num_stage, mode=fea_mode)
        self.cost_aggregation = DiffCostAgg(agg_mode, self.feature.out_channels, deterministic=deterministic, presum=presum)
        self.cost_regularization = nn.ModuleList([DiffCostRegNet(2, self.cr_base_chs[i], stage=i) for i in range(self.num_stage)])
        self.cost_regularization_refine = nn.ModuleList([DiffCostRegNetRefine(2, self.cr_base_chs[i], stage=i)
                                                         for i in range(self.num_stage)])
        self.DepthNet = DiffDepthNet(depth_mode, prob_volume=prob_volume)

    def load_state_dict(self, state_dict, strict=True, **kw):
        # model.py:65-70 drops the attn_mask keys of a checkpoint before its strict load
        return super().load_state_dict({k: v for k, v in state_dict.items() if "attn_mask" not in k}, strict=strict, **kw)

    def parts(self) -> Parts:
        """This model's children as the namespace ``wire`` takes."""
        return Parts(feature=lambda img: self.feature(img.contiguous()),
                     cost_agg=lambda features, proj, hyp: self.cost_aggregation(features, proj, hyp, None),
                     regnet=self.cost_regularization, regnet_refine=self.cost_regularization_refine,
                     head=lambda cost_reg, hyp, interval: self.DepthNet(cost_reg, hyp, interval=interval),
                     head_refine=lambda cost_reg, hyp, interval: self.DepthNet.refine(cost_reg, hyp, num_depth=REFINE_D, interval=interval),
                     hypotheses_first=_hypotheses_first, hypotheses_next=_hypotheses_next)

    def forward(self, imgs, proj_matrices, depth_values):
        """imgs [B,V,3,H,W]; proj_matrices {"stageK": [B,V,2,4,4]}; depth_values [B,n] (mvsnet.py:188) -> the reference's output dict."""
        _check_inputs(type(self).__name__, imgs, proj_matrices, depth_values)
        with torch.cuda.device(imgs.device):
            return wire(self.parts(), imgs, proj_matrices, depth_values.contiguous(), self.ndepths, self.depth_interval_ratio,
                        self.inverse_depth)


def train_step(model, optimizer, sample, dlossw, depth_mode="regression") -> Dict[str, torch.Tensor]:
    """The body of the reference's ``train_epoch`` loop (model.py:130-160) on ``sample`` = {"imgs", "proj_matrices", "depth_values",
    "depth": {"stageK": [B,h,w]}, "mask": {"stageK": [B,h,w]}} (on the model's device): forward, ``diff_mvs_loss``, ``zero_grad``,
    ``backward``, ``step``.  ``model``: a ``DiffMVSNet`` in train mode, bare or inside ``DistributedDataParallel``.  Returns the
    reference's scalars -- ``loss``, ``abs_depth_error``, ``thres2mm_error``, ``thres4mm_error``, ``thres8mm_error`` of the last stage's
    ``depth`` -- as 0-dim tensors on the device (nothing is read back: ``float(...)`` them where a number is needed)."""
    outputs = model(sample["imgs"], sample["proj_matrices"], sample["depth_values"])
    loss = diff_mvs_loss(outputs, sample["depth"], sample["mask"], depth_mode, dlossw=dlossw)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    last = "stage{}".format(sum(1 for k in outputs if "stage" in k))
    with torch.no_grad():   # validate's metrics: one launch for the four numbers
        m = validate.dual_depth_loss_stage(None, None, sample["depth"][last], sample["mask"][last], depth=outputs["depth"].detach())["metrics"]
    return {"loss": loss.detach(), "abs_depth_error": m[0], "thres2mm_error": m[1], "thres4mm_error": m[2], "thres8mm_error": m[3]}
