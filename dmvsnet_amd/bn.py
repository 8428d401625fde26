"""Differentiable BatchNorm + ReLU behind torch.autograd on the K5 kernels (csrc/batchnorm.h, docs/kernels/K5_batchnorm_relu.md), and
the four blocks of the regularisation U-Nets built from it and the differentiable convolutions of ``dmvsnet_amd.conv``.

``DiffBatchNormReLU3d`` / ``DiffBatchNormReLU2d`` are ``nn.BatchNorm3d`` / ``nn.BatchNorm2d`` with another ``forward`` and one more
keyword, ``relu=True``: parameter and buffer names, the state-dict layout and ``isinstance(m, nn.BatchNorm3d)`` initialisers are the
parent's.  A reference user swaps the constructor inside the reference's blocks (networks/module.py:50, :95, :144, :189)::

    self.bn = dmvsnet_amd.DiffBatchNormReLU3d(out_channels, momentum=bn_momentum) if bn else None

and may leave the block's ``x = F.relu(x, inplace=True)`` (:62, :110, :156, :201) where it is: the module has already applied the
ReLU, the ReLU of a non-negative tensor is that tensor with the same mask, so values and gradients are bit for bit those of the block
without that line -- the line may then be dropped, which saves ATen's pass and the output autograd keeps for it.  For a block with
``relu=False`` pass ``relu=False`` to the module as well.

Accepted: ``num_features`` in {8, 16, 32, 64}, ``affine=True``, ``track_running_stats=True``, a numeric ``momentum``; everything else
raises in the constructor: there is no ATen fallback.  fp32, contiguous, on a HIP device only.

* train mode: two launches forward (partial statistics around a per-channel pivot; fold + normalise + ReLU), two backward (partial sums
  of g and g * xhat; fold + apply).  ``running_mean`` / ``running_var`` are blended by the kernel (momentum, unbiased variance),
  ``num_batches_tracked += 1`` is a device-side add: no host sync anywhere;
* eval mode (``module.eval()``): the running statistics; one launch forward, two backward;
* autograd keeps the input, ``weight``, ``bias`` and the two [C] vectors mean / invstd -- NOT the output: the backward recomputes the
  ReLU mask from the input with the forward's own device function.  When the input needs no gradient the apply launch is skipped;
* no atomics: forward and backward are bitwise reproducible.

``DiffSyncBatchNormReLU3d`` / ``DiffSyncBatchNormReLU2d`` are the same modules with the statistics of ``torch.nn.SyncBatchNorm``: in
train mode, under a process group of more than one rank, mean and variance are those of the batches of ALL ranks (two all-gathers of a
few doubles per channel, one in each direction).  ``convert_sync_batchnorm(module, process_group=None)`` swaps every
``DiffBatchNormReLU*`` of a network for its sync form; the stock ``torch.nn.SyncBatchNorm.convert_sync_batchnorm`` must NOT be used on
these networks (it would replace the modules by ATen's and drop the fused ReLU): a block it went over raises.

``DiffConvBlock3d`` / ``DiffDeconvBlock3d`` / ``DiffConvBlock2d`` / ``DiffDeconvBlock2d`` take the reference blocks' constructor
arguments and have their children (``.conv``, ``.bn``) and state-dict keys; each is a ``DiffConv*`` / ``DiffConvTranspose*`` layer and a
``DiffBatchNormReLU*``.  ``bn=False`` or a layer shape the convolution classes refuse raises.  ``DiffConvBlock3d(2, 8, 3, padding=1)`` is
conv0 as the reference builds it; ``prob`` has no BatchNorm and is a bare ``DiffConv3d(8, 2, ...)`` (``dmvsnet_amd.regnet`` builds the
whole networks).  ``DiffConvBlock2d(8, 16, 5, stride=2, padding=2)`` and ``(16, 32, 5, stride=2, padding=2)`` are FeatureNet's conv1.0 /
conv2.0 (networks/module.py:289, :295) on K3, K3d, K3k and K5.  The block around conv0.0 / conv0.1 is
``dmvsnet_amd.featurenet.DiffFeatureConvBlock2d`` (``_DiffBlock`` on ``DiffFeatureConv2d``): with it no block of a training step is left on
ATen.
"""
from __future__ import annotations

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import ops
from ._lib import DmvsError
from .conv import DiffConv2d, DiffConv3d, DiffConvTranspose2d, DiffConvTranspose3d

__all__ = ["DiffBatchNormReLU3d", "DiffBatchNormReLU2d", "DiffSyncBatchNormReLU3d", "DiffSyncBatchNormReLU2d", "convert_sync_batchnorm",
           "DiffConvBlock3d", "DiffDeconvBlock3d", "DiffConvBlock2d", "DiffDeconvBlock2d",
           "launch_counts", "sync_launch_counts", "CHANNELS"]

CHANNELS = ops.BN_CHANNELS

# backward launches since import (tests check through them that a frozen input skips the apply launch)
launch_counts = {"reduce": 0, "apply": 0}
# the same for the sync path, which counts here alone: "moments" (statistics + fold) and "sums" (reduce + fold) once per forward /
# backward, "apply" the backward's apply launch, "gather" the collectives (two per step when the input needs a gradient, else one)
sync_launch_counts = {"moments": 0, "sums": 0, "apply": 0, "gather": 0}


class _BnReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, relu, training):
        xd = x.detach()
        y, mean, invstd = ops.bn_relu_forward(xd, weight.detach(), bias.detach(), running_mean, running_var, momentum, eps, relu, training)
        ctx.save_for_backward(xd, weight, bias, mean, invstd)
        ctx.relu, ctx.training = relu, training
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, weight, bias, mean, invstd = ctx.saved_tensors   # (raises if weight or bias was changed in place since the forward)
        need_gx = ctx.needs_input_grad[0]
        gx, g_gamma, g_beta = ops.bn_relu_backward(x, gy.contiguous(), weight.detach(), bias.detach(), mean, invstd, ctx.relu,
                                                   ctx.training, need_gx)
        launch_counts["reduce"] += 1
        if need_gx:
            launch_counts["apply"] += 1
        return (gx, g_gamma if ctx.needs_input_grad[1] else None, g_beta if ctx.needs_input_grad[2] else None,
                None, None, None, None, None, None)


def _all_gather(send, world, group):
    """[world, *send.shape] in rank order, on the current stream."""
    import torch.distributed as dist
    recv = torch.empty((world * send.shape[0],) + tuple(send.shape[1:]), dtype=send.dtype, device=send.device)   # rank-major
    dist.all_gather_into_tensor(recv, send, group=group)
    sync_launch_counts["gather"] += 1
    return recv.view((world,) + tuple(send.shape))


class _SyncBnReluFn(torch.autograd.Function):
    """Train mode over the ranks of ``group``: local moments, all-gather, apply on the combined statistics; backward: local sums,
    all-gather, apply.  Both collectives are issued on the current stream, the second one if and only if the input needs a gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum, eps, relu, group, world):
        xd = x.detach()
        gathered = _all_gather(ops.bn_sync_moments(xd), world, group)
        sync_launch_counts["moments"] += 1
        y, mean, invstd, N = ops.bn_sync_forward(xd, weight.detach(), bias.detach(), running_mean, running_var, gathered, momentum, eps,
                                                 relu)
        ctx.save_for_backward(xd, weight, bias, mean, invstd)
        ctx.relu, ctx.group, ctx.world, ctx.N = relu, group, world, N
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, weight, bias, mean, invstd = ctx.saved_tensors
        gy = gy.contiguous()
        sums, g_gamma, g_beta = ops.bn_sync_backward_sums(x, gy, weight.detach(), bias.detach(), mean, invstd, ctx.relu)
        sync_launch_counts["sums"] += 1
        gx = None
        if ctx.needs_input_grad[0]:
            gathered = _all_gather(sums, ctx.world, ctx.group)
            gx = ops.bn_sync_backward_apply(x, gy, weight.detach(), bias.detach(), mean, invstd, gathered, ctx.N, ctx.relu)
            sync_launch_counts["apply"] += 1
        return (gx, g_gamma if ctx.needs_input_grad[1] else None, g_beta if ctx.needs_input_grad[2] else None,
                None, None, None, None, None, None, None)


def _check_ctor(what, m):
    if not m.affine or not m.track_running_stats or m.momentum is None or m.num_features not in CHANNELS:
        raise DmvsError(f"{what}: only affine=True, track_running_stats=True, a numeric momentum and num_features in {CHANNELS} run on "
                        f"the gfx950 kernels (no ATen fallback); got {m}")


def _check_layout(what, is_cuda, device, dtype, shape, contiguous, nd, C, training):
    """The refusals of an input, on its properties alone (so that they can be checked without a device)."""
    if not is_cuda:
        raise DmvsError(f"{what} runs on the HIP kernels only (no CPU fallback); the input is on {device}")
    if dtype != torch.float32:
        raise DmvsError(f"{what} is fp32 only (no fp16 / autocast in the differentiable path); the input is {dtype}")
    if len(shape) != nd + 2 or shape[1] != C:
        raise DmvsError(f"{what}: the input must be [B,{C},{'D,H,W' if nd == 3 else 'H,W'}], got {tuple(shape)}")
    if not contiguous:
        raise DmvsError(f"{what}: the input must be contiguous")
    n = 1
    for s in shape:
        n *= int(s)
    if training and n // C < 2:
        raise DmvsError(f"{what}: train mode needs more than one value per channel, got input {tuple(shape)}")


def _check_input(what, x, nd, C, training):
    if not torch.is_tensor(x):
        raise DmvsError(f"{what}: the input must be a tensor, got {type(x).__name__}")
    _check_layout(what, x.is_cuda, x.device, x.dtype, x.shape, x.is_contiguous(), nd, C, training)


def _sync_world(group):
    """Ranks whose statistics a sync module combines: 1 without an initialised process group."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return 1
    return dist.get_world_size(group)


class _DiffBatchNormReLU:
    """What the 3D and the 2D module share (mixed in front of the nn class)."""
    _nd = 3

    def _init_diff(self, relu):
        self.relu = bool(relu)
        _check_ctor(type(self).__name__, self)

    def _sync(self):
        """(process group, its size) when this forward takes its statistics from other ranks too, else None."""
        return None

    def forward(self, x):
        what = type(self).__name__
        sync = self._sync()
        # (under a group every rank holds at least one value per channel and all of them two: the launch checks the sum)
        _check_input(what, x, self._nd, self.num_features, self.training and sync is None)
        for t in (self.weight, self.bias, self.running_mean, self.running_var):
            if t.device != x.device or t.dtype != torch.float32 or not t.is_contiguous():
                raise DmvsError(f"{what}: parameters and buffers must be contiguous fp32 on the input's device {x.device}; one is "
                                f"{t.dtype} on {t.device}")
        with torch.cuda.device(x.device):
            if sync is not None:
                y = _SyncBnReluFn.apply(x, self.weight, self.bias, self.running_mean, self.running_var, float(self.momentum),
                                        float(self.eps), self.relu, *sync)
            else:
                y = _BnReluFn.apply(x, self.weight, self.bias, self.running_mean, self.running_var, float(self.momentum),
                                    float(self.eps), self.relu, self.training)
            if self.training:
                self.num_batches_tracked.add_(1)   # after the launch went through; on the device: no host sync
            return y

    def extra_repr(self):
        return super().extra_repr() + f", relu={self.relu}"


class DiffBatchNormReLU3d(_DiffBatchNormReLU, nn.BatchNorm3d):
    """``nn.BatchNorm3d(C)`` followed by ReLU (``relu=False``: BatchNorm alone), C in {8, 16, 32, 64}, on K5 in both directions.  Input
    [B,C,D,H,W], fp32, contiguous, on a HIP device."""
    _nd = 3

    def __init__(self, *args, relu=True, **kwargs):
        super().__init__(*args, **kwargs)
        self._init_diff(relu)


class DiffBatchNormReLU2d(_DiffBatchNormReLU, nn.BatchNorm2d):
    """``nn.BatchNorm2d(C)`` followed by ReLU (``relu=False``: BatchNorm alone), C in {8, 16, 32, 64}, on K5 in both directions.  Input
    [B,C,H,W], fp32, contiguous, on a HIP device."""
    _nd = 2

    def __init__(self, *args, relu=True, **kwargs):
        super().__init__(*args, **kwargs)
        self._init_diff(relu)


class _DiffSyncBatchNormReLU(_DiffBatchNormReLU):
    """The sync forms: the plain path in eval mode and under a group of one rank (bit for bit ``DiffBatchNormReLU*``: the same
    launches, no collective), else statistics over all ranks of ``process_group`` (None: the default group), the semantics of
    ``torch.nn.SyncBatchNorm``: mean and biased variance over the values of all ranks, whose batch sizes may differ (every rank at least
    one sample); the running buffers are blended with the global mean and unbiased variance and are the same bits on every rank;
    ``weight.grad`` / ``bias.grad`` are the LOCAL sums (DistributedDataParallel averages them, as with the stock module).  The backward
    issues its collective if and only if the input needs a gradient: as with the stock module, ``requires_grad`` of the input must
    agree across ranks, or the ranks that issue it wait for those that do not."""

    def _sync(self):
        if not self.training:
            return None
        world = _sync_world(self.process_group)
        return (self.process_group, world) if world > 1 else None

    def extra_repr(self):
        return super().extra_repr() + f", process_group={self.process_group}"


class DiffSyncBatchNormReLU3d(_DiffSyncBatchNormReLU, nn.BatchNorm3d):
    """``DiffBatchNormReLU3d`` with statistics over the ranks of ``process_group`` in train mode (``torch.nn.SyncBatchNorm`` + ReLU)."""
    _nd = 3

    def __init__(self, *args, relu=True, process_group=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.process_group = process_group
        self._init_diff(relu)


class DiffSyncBatchNormReLU2d(_DiffSyncBatchNormReLU, nn.BatchNorm2d):
    """``DiffBatchNormReLU2d`` with statistics over the ranks of ``process_group`` in train mode (``torch.nn.SyncBatchNorm`` + ReLU)."""
    _nd = 2

    def __init__(self, *args, relu=True, process_group=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.process_group = process_group
        self._init_diff(relu)


_SYNC_FORM = {DiffBatchNormReLU3d: DiffSyncBatchNormReLU3d, DiffBatchNormReLU2d: DiffSyncBatchNormReLU2d}


def convert_sync_batchnorm(module, process_group=None):
    """``torch.nn.SyncBatchNorm.convert_sync_batchnorm`` for this package's networks: every ``DiffBatchNormReLU3d`` /
    ``DiffBatchNormReLU2d`` in ``module`` (itself included) becomes its sync form on ``process_group``; ``relu``, ``momentum``, ``eps``
    and the ``training`` flag are carried over, and the parameter and buffer OBJECTS are kept (an optimiser built before the conversion
    still holds them).  Everything else is left alone.  Returns the module (a new one only when ``module`` itself is converted)."""
    out = module
    if type(module) in _SYNC_FORM:
        out = _SYNC_FORM[type(module)](module.num_features, module.eps, module.momentum, module.affine, module.track_running_stats,
                                       relu=module.relu, process_group=process_group)
        out.weight, out.bias = module.weight, module.bias
        out.running_mean, out.running_var, out.num_batches_tracked = module.running_mean, module.running_var, module.num_batches_tracked
        out.training = module.training
        if hasattr(module, "qconfig"):
            out.qconfig = module.qconfig
    for name, child in module.named_children():
        out.add_module(name, convert_sync_batchnorm(child, process_group))
    return out


class _DiffBlock(nn.Module):
    """layer + BatchNorm + ReLU with the reference blocks' constructor signature, children and state-dict keys."""
    _conv_cls, _bn_cls = None, None

    def __init__(self, in_channels, out_channels, kernel_size=3, stride=1, relu=True, bn=True, bn_momentum=0.1, init_method="xavier", **kwargs):
        super().__init__()
        if not bn:
            raise DmvsError(f"{type(self).__name__}: bn=False is not a block of the gfx950 training path (no ATen fallback); use the "
                            "convolution class alone")
        self.conv = self._conv_cls(in_channels, out_channels, kernel_size, stride=stride, bias=False, **kwargs)
        self.bn = self._bn_cls(out_channels, momentum=bn_momentum, relu=relu)
        self.kernel_size, self.stride, self.relu, self.out_channels = kernel_size, stride, relu, out_channels

    def forward(self, x):
        if not isinstance(self.bn, _DiffBatchNormReLU):
            raise DmvsError(f"{type(self).__name__}: .bn is a {type(self.bn).__name__}, not one of this package's BatchNorm + ReLU modules "
                            "(torch.nn.SyncBatchNorm.convert_sync_batchnorm leaves that behind: it drops the fused ReLU and takes the "
                            "layer off the gfx950 kernels); convert with dmvsnet_amd.convert_sync_batchnorm instead")
        return self.bn(self.conv(x))

    def init_weights(self, init_method):
        if init_method == "kaiming":
            nn.init.kaiming_uniform_(self.conv.weight)
        elif init_method == "xavier":
            nn.init.xavier_uniform_(self.conv.weight)
        nn.init.ones_(self.bn.weight)
        nn.init.zeros_(self.bn.bias)


class DiffConvBlock3d(_DiffBlock):
    """The reference's ``Conv3d`` block (networks/module.py:120) on ``DiffConv3d`` + ``DiffBatchNormReLU3d``."""
    _conv_cls, _bn_cls = DiffConv3d, DiffBatchNormReLU3d


class DiffDeconvBlock3d(_DiffBlock):
    """The reference's ``Deconv3d`` block (networks/module.py:166) on ``DiffConvTranspose3d`` + ``DiffBatchNormReLU3d``."""
    _conv_cls, _bn_cls = DiffConvTranspose3d, DiffBatchNormReLU3d


class DiffConvBlock2d(_DiffBlock):
    """The reference's ``Conv2d`` block (networks/module.py:28) on ``DiffConv2d`` + ``DiffBatchNormReLU2d``."""
    _conv_cls, _bn_cls = DiffConv2d, DiffBatchNormReLU2d


class DiffDeconvBlock2d(_DiffBlock):
    """The reference's ``Deconv2d`` block (networks/module.py:72) on ``DiffConvTranspose2d`` + ``DiffBatchNormReLU2d`` (its crop to twice
    the input is the identity at output_padding 1, the only form the layer takes)."""
    _conv_cls, _bn_cls = DiffConvTranspose2d, DiffBatchNormReLU2d
