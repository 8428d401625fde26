"""Differentiable stride-1 square convolutions of the regularisation U-Nets and FeatureNet: K3 forward and data gradient, K3g weight
gradient, behind torch.autograd.

``DiffConv3d`` / ``DiffConv2d`` are ``nn.Conv3d`` / ``nn.Conv2d`` with another ``forward``: parameter name, shape, state-dict layout and
``isinstance(m, nn.Conv3d)`` initialisers are the reference's.  A reference user swaps the constructor inside the reference's blocks
(networks/module.py:142 ``Conv3d.__init__``, :46 ``Conv2d.__init__``) for the layers the classes accept::

    self.conv = dmvsnet_amd.DiffConv3d(in_channels, out_channels, kernel_size, stride=stride, bias=(not bn), **kwargs)

Accepted: kernel 3, stride 1, padding 1, dilation 1, groups 1, no bias, in == out in {16, 32, 64} -- conv2 / conv4 / conv6 of
CostRegNet_part, conv2 / conv4 and the 2D conv6 of CostRegNet_part_refine, conv1.1 / 1.2 / 2.1 / 2.2 and out2 of FeatureNet.  Everything
else raises in the constructor: there is no ATen fallback.  BatchNorm, ReLU, the stride-2 and transposed layers, conv0 and ``prob``
stay on ATen (``dmvsnet_amd.MVSNet.train()`` still raises).

* forward: ``ops.conv3d(x[b], layer, backend="mfma")`` per sample, bit for bit, the layer being the bare convolution (no scale / shift /
  ReLU) with the weight packed on the device by one gather (``ops.pack_index_mfma``);
* data gradient: the SAME K3 launch on the weight transposed in (co, ci) and flipped in every tap -- the stride-1 square layers are
  closed under transposition -- packed by the composed gather;
* weight gradient: K3g (``ops.conv3d_wgrad``), accumulated over the samples in batch order.

Autograd keeps the input and the weight only.  Both packed weights are cached per module, keyed on the weight's version counter, data
pointer and device: an in-place optimiser step invalidates them, and after the first call a step makes no host copy and no host sync.
fp32 on a HIP device only.  No atomics anywhere: forward and both gradients are bitwise reproducible.
"""
from __future__ import annotations

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import ops
from ._lib import DmvsError

__all__ = ["DiffConv3d", "DiffConv2d", "launch_counts", "CHANNELS"]

CHANNELS = (16, 32, 64)   # the square shapes K3 and K3g compile

# launches of the two backward paths since import (tests check through them that frozen inputs skip their kernel)
launch_counts = {"dgrad": 0, "wgrad": 0}


def _packed_layer(cache: dict, weight: torch.Tensor, kdepth: int, transposed_flipped: bool) -> ops.ConvLayer:
    """The bare K3 layer of ``weight`` ([C,C,kd,3,3] or [C,C,3,3]) or of its transposed-flipped form, from the module's cache."""
    key = (weight._version, weight.data_ptr(), weight.device)
    hit = cache.get(transposed_flipped)
    if hit is not None and hit[0] == key and hit[2] is weight:   # (the entry holds the tensor: its address cannot be re-used meanwhile)
        return hit[1]
    C = weight.shape[0]
    index = ops.pack_index_mfma(C, kdepth, transposed_flipped, weight.device)
    packed = torch.index_select(weight.detach().reshape(-1), 0, index)   # one device gather: the packing is a permutation
    layer = ops.ConvLayer("diffconv%d%s" % (C, "t" if transposed_flipped else ""), ops.CONV_S1, kdepth, C, C, None, packed, None, None,
                          False)
    cache[transposed_flipped] = (key, layer, weight)
    return layer


class _ConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, kdepth, cache):
        xd = x.detach()
        layer = _packed_layer(cache, weight, kdepth, False)
        out = torch.empty_like(xd)
        for b in range(xd.shape[0]):
            ops.conv3d(xd[b], layer, out=out[b], backend="mfma")
        ctx.save_for_backward(xd, weight)
        ctx.kdepth, ctx.cache = kdepth, cache
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors   # (raises if the weight was changed in place since the forward)
        gy = gy.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            layer = _packed_layer(ctx.cache, weight, ctx.kdepth, True)
            gx = torch.empty_like(x)
            for b in range(x.shape[0]):
                ops.conv3d(gy[b], layer, out=gx[b], backend="mfma")
                launch_counts["dgrad"] += 1
        if ctx.needs_input_grad[1]:
            gw = torch.empty_like(weight, memory_format=torch.contiguous_format)
            for b in range(x.shape[0]):
                ops.conv3d_wgrad(x[b], gy[b], ctx.kdepth, out=gw, accumulate=b > 0)
                launch_counts["wgrad"] += 1
        return gx, gw, None, None


def _check_ctor(what, nd, m):
    one, three = (1,) * nd, (3,) * nd
    if m.kernel_size != three or m.stride != one or m.padding != one or m.dilation != one or m.groups != 1 or m.bias is not None \
            or m.padding_mode != "zeros" or m.in_channels != m.out_channels or m.in_channels not in CHANNELS:
        raise DmvsError(f"{what}: only kernel 3, stride 1, padding 1, dilation 1, groups 1, bias=False and in == out in {CHANNELS} run "
                        f"on the gfx950 kernels (no ATen fallback); got {m}")


def _check_input(what, x, nd, C):
    if not torch.is_tensor(x):
        raise DmvsError(f"{what}: the input must be a tensor, got {type(x).__name__}")
    if not x.is_cuda:
        raise DmvsError(f"{what} runs on the HIP kernels only (no CPU fallback); the input is on {x.device}")
    if x.dtype != torch.float32:
        raise DmvsError(f"{what} is fp32 only (no fp16 / autocast in the differentiable path); the input is {x.dtype}")
    if x.dim() != nd + 2 or x.shape[1] != C:
        raise DmvsError(f"{what}: the input must be [B,{C},{'D,H,W' if nd == 3 else 'H,W'}], got {tuple(x.shape)}")
    if not x.is_contiguous():
        raise DmvsError(f"{what}: the input must be contiguous")


def _check_weight(what, w, x):
    if w.device != x.device or w.dtype != torch.float32 or not w.is_contiguous():
        raise DmvsError(f"{what}: the weight must be contiguous fp32 on the input's device {x.device}; it is {w.dtype} on {w.device}")


class DiffConv3d(nn.Conv3d):
    """``nn.Conv3d(C, C, 3, stride=1, padding=1, bias=False)``, C in {16, 32, 64}, on K3 (forward, data gradient) and K3g (weight
    gradient).  Input [B,C,D,H,W], fp32, contiguous, on a HIP device."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        _check_ctor("DiffConv3d", 3, self)
        self._packed = {}

    def forward(self, x):
        _check_input("DiffConv3d", x, 3, self.in_channels)
        _check_weight("DiffConv3d", self.weight, x)
        with torch.cuda.device(x.device):
            return _ConvFn.apply(x, self.weight, 3, self._packed)


class DiffConv2d(nn.Conv2d):
    """``nn.Conv2d(C, C, 3, stride=1, padding=1, bias=False)``, C in {16, 32, 64}, on the kdepth-1 forms of K3 and K3g.  Input
    [B,C,H,W], fp32, contiguous, on a HIP device; each sample is a D = 1 volume."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        _check_ctor("DiffConv2d", 2, self)
        self._packed = {}

    def forward(self, x):
        _check_input("DiffConv2d", x, 2, self.in_channels)
        _check_weight("DiffConv2d", self.weight, x)
        with torch.cuda.device(x.device):
            return _ConvFn.apply(x.unsqueeze(2), self.weight, 1, self._packed).squeeze(2)
