"""Differentiable convolutions of the regularisation U-Nets and FeatureNet behind torch.autograd: the stride-1 square layers (K3 forward
and data gradient, K3g weight gradient), the stride-2 / transposed layers between them (K3 in both stride-2 modes, K3h weight
gradient; second part of this text), the U-Nets' 2-channel ends conv0 / ``prob`` (K2 forward and data gradient, K2g weight gradient;
third part) and FeatureNet's 5x5 stride-2 layers conv1.0 / conv2.0 (K3 forward, K3d data gradient, K3k weight gradient; fourth part).

``DiffConv3d`` / ``DiffConv2d`` are ``nn.Conv3d`` / ``nn.Conv2d`` with another ``forward``: parameter name, shape, state-dict layout and
``isinstance(m, nn.Conv3d)`` initialisers are the reference's.  A reference user swaps the constructor inside the reference's blocks
(networks/module.py:142 ``Conv3d.__init__``, :46 ``Conv2d.__init__``) for the layers the classes accept::

    self.conv = dmvsnet_amd.DiffConv3d(in_channels, out_channels, kernel_size, stride=stride, bias=(not bn), **kwargs)

Accepted at stride 1: kernel 3, padding 1, dilation 1, groups 1, no bias, in == out in {16, 32, 64} -- conv2 / conv4 / conv6 of
CostRegNet_part, conv2 / conv4 and the 2D conv6 of CostRegNet_part_refine, conv1.1 / 1.2 / 2.1 / 2.2 and out2 of FeatureNet.  Everything
else raises in the constructor: there is no ATen fallback.  FeatureNet's 1x1 layers, conv0.0 / conv0.1 and out3 are refused here and
run on ``dmvsnet_amd.featurenet.DiffFeatureConv2d`` (K3 + K3f): no layer is left on ATen (``dmvsnet_amd.MVSNet.train()`` still raises:
the parts exist, their assembly does not); BatchNorm + ReLU run on K5 (``dmvsnet_amd.bn``: ``DiffBatchNormReLU3d`` / ``2d``, and the
blocks ``DiffConvBlock3d`` ... that pair these layers with it); ``dmvsnet_amd.regnet`` builds the four regularisation networks.

* forward: ``ops.conv3d(x[b], layer, backend="mfma")`` per sample, bit for bit, the layer being the bare convolution (no scale / shift /
  ReLU) with the weight packed on the device by one gather (``ops.pack_index_mfma``);
* data gradient: the SAME K3 launch on the weight transposed in (co, ci) and flipped in every tap -- the stride-1 square layers are
  closed under transposition -- packed by the composed gather;
* weight gradient: K3g (``ops.conv3d_wgrad``), accumulated over the samples in batch order.

Autograd keeps the input and the weight only.  Both packed weights are cached per module, keyed on the weight's version counter, data
pointer and device: an in-place optimiser step invalidates them, and after the first call a step makes no host copy and no host sync.
fp32 on a HIP device only.  No atomics anywhere: forward and both gradients are bitwise reproducible.

The stride-2 and transposed layers (kernel 3, stride 2, padding 1, no bias; transposed: output_padding 1, so fine extent = 2 x coarse):
``DiffConv3d`` also takes stride 2 for (in, out) in {(8, 16), (16, 32), (32, 64)} (conv1 / 3 / 5), ``DiffConv2d`` for (32, 64) (the refine
net's 2D conv5); ``DiffConvTranspose3d`` takes (64, 32), (32, 16), (16, 8) (conv7 / 9 / 11) and ``DiffConvTranspose2d`` (64, 32) (the 2D
conv7).  The reference's ``Deconv3d`` / ``Deconv2d`` blocks swap ``nn.ConvTranspose3d`` / ``nn.ConvTranspose2d`` for them.

* forward: K3's ``CONV_S2`` resp. ``DECONV_S2`` launch on the weight packed by one gather (``ops.pack_index_mfma_s2``);
* data gradient: K3's launch in the OTHER mode, out -> in channels, on the SAME weight tensor -- no flip, no transposition: a
  ConvTranspose weight is laid out [in][out], which is a conv weight's [out][in] read the other way.  For the stride-2 conv this
  needs even input extents (H and W, and D for the 3D layers); odd ones are refused;
* weight gradient: K3h (``ops.conv3d_wgrad_s2``) on (coarse, fine) = (dY, X) for the conv and (X, dY) for the transposed conv,
  accumulated over the samples in batch order.

The 2-channel ends (kernel 3, stride 1, padding 1, no bias): ``DiffConv3d`` also takes (in, out) = (2, 8) -- conv0 -- and (8, 2) --
``prob``.  ``DiffConv2d`` does not: no 2D layer has these shapes.  Each one's data gradient has the other one's shape:

* forward: ``ops.conv3d(x[b], layer, backend="direct")`` per sample, bit for bit: K2's ``cout2`` kernel for 8 -> 2 and its
  ``Cin == 2`` direct form for 2 -> 8, the weight packed on the device by one gather (``ops.pack_index_direct``);
* data gradient: the OTHER of those two launches on the weight transposed in (co, ci) and flipped in every tap;
* weight gradient: K2g (``ops.conv3d_wgrad_c2``), accumulated over the samples in batch order.

The 5x5 stride-2 layers (kernel 5, stride 2, padding 2, no bias; 2D only): ``DiffConv2d`` also takes (in, out) = (8, 16) and (16, 32) --
FeatureNet's conv1.0 / conv2.0 (networks/module.py:289, :295).  Even and odd H, W: the output is (H + 1) // 2 x (W + 1) // 2.

* forward: K3's ``CONV2D_K5S2`` launch on the weight packed by one gather (``ops.pack_index_mfma_k5s2``), bit for bit;
* data gradient: K3d (``ops.conv2d_k5s2_dgrad``), a gather over the four parity classes of the input pixels on the RAW weight -- K3 has
  no transposed 5x5 form, and nothing is packed or cached for this direction;
* weight gradient: K3k (``ops.conv2d_k5s2_wgrad``), accumulated over the samples in batch order.

In the code: one autograd Function (``_ConvFn``) runs every kind of layer, FeatureNet's rectangular ones included
(``dmvsnet_amd.featurenet``: the sixth kind, which brings the optional bias and conv0.0's launch on its 3-channel sample in place).  A
``_Kind`` value per kind (square, stride-2, transposed, ends, 5x5, rectangular) names the builder of its packed layers (the family's
gather index, ``ops.gather_packed`` and the ``ConvLayer``), the forms of the weight the forward and the data gradient launch, the
``ops.conv3d`` backend, the weight-gradient call with its argument order and, for the 5x5 kind, the data-gradient call that stands in
for the ``ops.conv3d`` launch.  Every packed layer comes through one cache lookup (``_cached_layer``; ``_biased_layer`` keys a
lateral's on its bias too; ``_packed_layer*`` name it per kind), and the four classes share their constructor and ``forward``
(``_DiffConv``, mixed in front of the nn class).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Union

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import ops
from ._lib import DmvsError

__all__ = ["DiffConv3d", "DiffConv2d", "DiffConvTranspose3d", "DiffConvTranspose2d", "launch_counts", "CHANNELS", "CHANNELS_S2",
           "CHANNELS_C2", "CHANNELS_K5S2"]

CHANNELS = (16, 32, 64)   # the square shapes K3 and K3g compile
# (fine, coarse) channels of the stride-2 / transposed layers K3 and K3h compile, per number of spatial dimensions
CHANNELS_S2 = {3: ((8, 16), (16, 32), (32, 64)), 2: ((32, 64),)}
CHANNELS_C2 = ops.WGRAD_C2_SHAPES   # (in, out) of the 2-channel ends K2 and K2g run: conv0 and prob (3D only)
CHANNELS_K5S2 = ((8, 16), (16, 32))  # (in, out) of the 5x5 stride-2 layers K3, K3k and K3d run: FeatureNet's conv1.0 and conv2.0 (2D only)

# launches of the two backward paths since import (tests check through them that frozen inputs skip their kernel)
launch_counts = {"dgrad": 0, "wgrad": 0}


def _cached_layer(cache: dict, slot, weight: torch.Tensor, build, kdepth: int) -> ops.ConvLayer:
    """The layer ``build(weight, kdepth, slot)`` packs, from the module's ``cache`` under ``slot`` (the form of the weight: see the
    builders) while the weight's version counter, data pointer and device are those it was built from."""
    key = (weight._version, weight.data_ptr(), weight.device)
    hit = cache.get(slot)
    if hit is not None and hit[0] == key and hit[2] is weight:   # (the entry holds the tensor: its address cannot be re-used meanwhile)
        return hit[1]
    layer = build(weight, kdepth, slot)
    cache[slot] = (key, layer, weight)
    return layer


def _biased_layer(cache: dict, weight: torch.Tensor, bias: torch.Tensor, kind: "_Kind", kdepth: int) -> ops.ConvLayer:
    """The layer of the forward launch of a layer with a ``bias``: its epilogue adds the bias, and the slot also carries the bias's data
    pointer and device."""
    slot = (kind.fwd, bias.data_ptr(), bias.device)
    for old in [k for k in cache if isinstance(k, tuple) and k != slot]:   # (a bias that moved leaves no layer behind)
        del cache[old]
    return _cached_layer(cache, slot, weight, lambda w, kd, s: kind.build(w, kd, kind.fwd, bias), kdepth)


# The builders: (weight, kdepth, the form of the weight) -> the bare layer (no scale / shift / ReLU), packed on the device by one gather
def _build_s1(weight, kdepth, transposed_flipped):
    C = weight.shape[0]
    packed = ops.gather_packed(weight, ops.pack_index_mfma(C, kdepth, transposed_flipped, weight.device), False)
    return ops.ConvLayer("diffconv%d%s" % (C, "t" if transposed_flipped else ""), ops.CONV_S1, kdepth, C, C, None, packed, None, None, False)


def _build_s2(weight, kdepth, mode):
    big, small = weight.shape[0], weight.shape[1]
    cin, cout = (small, big) if mode == ops.CONV_S2 else (big, small)
    packed = ops.gather_packed(weight, ops.pack_index_mfma_s2(cin, cout, mode, kdepth, weight.device), True)
    return ops.ConvLayer("diff%s%dto%d" % ("conv_s2_" if mode == ops.CONV_S2 else "deconv_s2_", cin, cout), mode, kdepth, cin, cout, None,
                         packed, None, None, False)


def _build_c2(weight, kdepth, transposed_flipped):
    cout, cin = weight.shape[0], weight.shape[1]
    packed = ops.gather_packed(weight, ops.pack_index_direct(cin, cout, transposed_flipped, weight.device), False)
    lin, lout = (cout, cin) if transposed_flipped else (cin, cout)
    return ops.ConvLayer("diffconv%dto%d%s" % (cin, cout, "t" if transposed_flipped else ""), ops.CONV_S1, 3, lin, lout, packed, None, None,
                         None, False)


def _build_k5(weight, kdepth, slot):
    cout, cin = weight.shape[0], weight.shape[1]
    packed = ops.gather_packed(weight, ops.pack_index_mfma_k5s2(cin, cout, weight.device), True)
    return ops.ConvLayer("diffconv_k5s2_%dto%d" % (cin, cout), ops.CONV2D_K5S2, 1, cin, cout, None, packed, None, None, False)


def _packed_layer(cache: dict, weight: torch.Tensor, kdepth: int, transposed_flipped: bool) -> ops.ConvLayer:
    """The bare K3 layer of ``weight`` ([C,C,kd,3,3] or [C,C,3,3]) or of its transposed-flipped form, from the module's cache."""
    return _cached_layer(cache, transposed_flipped, weight, _build_s1, kdepth)


def _packed_layer_s2(cache: dict, weight: torch.Tensor, kdepth: int, mode: int) -> ops.ConvLayer:
    """The bare K3 layer that reads ``weight`` in ``mode``: CONV_S2 takes it as [out][in][k..], DECONV_S2 as [in][out][k..] -- the same
    tensor either way, so a layer's forward and its data gradient are the two modes.  From the module's cache, keyed as _packed_layer."""
    return _cached_layer(cache, mode, weight, _build_s2, kdepth)


def _packed_layer_c2(cache: dict, weight: torch.Tensor, transposed_flipped: bool) -> ops.ConvLayer:
    """The bare K2 layer of ``weight`` ([8,2,3,3,3] or [2,8,3,3,3]) or of its transposed-flipped form (a layer out -> in), from the
    module's cache, keyed as _packed_layer."""
    return _cached_layer(cache, transposed_flipped, weight, _build_c2, 3)


# The weight-gradient calls in the Function's argument order (x, gy, kdepth, out=, accumulate=)
def _wgrad_down(x, gy, kdepth, **kw):
    return ops.conv3d_wgrad_s2(gy, x, kdepth, **kw)   # K3h takes (coarse, fine)


def _wgrad_ends(x, gy, kdepth, **kw):
    return ops.conv3d_wgrad_c2(x, gy, **kw)


def _wgrad_k5(x, gy, kdepth, **kw):
    return ops.conv2d_k5s2_wgrad(x, gy, **kw)


def _dgrad_k5(gy, weight, x, out):
    return ops.conv2d_k5s2_dgrad(gy, weight, x.shape[-2:], out=out)   # K3d reads the raw weight: no packed layer


@dataclass(frozen=True)
class _Kind:
    """What tells the kinds of layer apart behind _ConvFn."""
    build: Callable          # the builder of its packed layers (_cached_layer)
    fwd: Union[bool, int]    # the form of the weight the forward launches: the builder's last argument and the cache slot
    bwd: Union[bool, int]    # ... and the data gradient
    backend: str             # of ops.conv3d, forward and data gradient
    wgrad: Callable          # (x, gy, kdepth, out=, accumulate=) -> the weight-gradient launch of one sample
    dgrad: Optional[Callable] = None   # (gy, weight, x, out) -> the data-gradient launch of one sample, in place of ops.conv3d on `bwd`


_SQUARE = _Kind(_build_s1, False, True, "mfma", ops.conv3d_wgrad)
# a stride-2 conv and a transposed conv: the weight is [coarse channels][fine channels][k..] in both, and the forward of the one is the
# data gradient of the other
_DOWN = _Kind(_build_s2, ops.CONV_S2, ops.DECONV_S2, "mfma", _wgrad_down)
_UP = _Kind(_build_s2, ops.DECONV_S2, ops.CONV_S2, "mfma", ops.conv3d_wgrad_s2)
# conv0 (2 -> 8) or prob (8 -> 2) on K2: the forward of the one has the shape of the data gradient of the other
_ENDS = _Kind(_build_c2, False, True, "direct", _wgrad_ends)
# FeatureNet's 5x5 stride-2 layers: K3's CONV2D_K5S2 forward; no K3 launch has the data gradient's shape, K3d has it on the raw weight
_DOWN5 = _Kind(_build_k5, ops.CONV2D_K5S2, None, "mfma", _wgrad_k5, _dgrad_k5)
# (the sixth kind, FeatureNet's rectangular stride-1 layers, is dmvsnet_amd.featurenet._FPN)


class _ConvFn(torch.autograd.Function):
    """x [B,Cin,D,H,W], or [B,Cin,H,W] of a 2D layer (its samples run as D = 1 volumes: the axis is inserted and removed here, on
    detached tensors), weight, the module's cache of packed layers, the kind; ``bias`` [Cout] (the two FeatureNet laterals only: the
    kind's builder and its weight-gradient call take it) -> [B,Cout,D',H',W'] resp. [B,Cout,H',W']."""

    @staticmethod
    def forward(ctx, x, weight, cache, kind, bias=None):
        xd = x.detach()
        flat = xd.dim() == 4
        if flat:
            xd = xd.unsqueeze(2)
        kdepth = 3 if weight.dim() == 5 else 1
        if bias is None:
            layer = _cached_layer(cache, kind.fwd, weight, kind.build, kdepth)
        else:
            layer = _biased_layer(cache, weight, bias, kind, kdepth)
        if layer.mode == ops.CONV_S1 and layer.cout == layer.cin:   # a square layer: the output has the input's shape
            out = torch.empty_like(xd)
        else:
            out = xd.new_empty((xd.shape[0], layer.cout, *layer.out_shape(*xd.shape[2:])))
        for b in range(xd.shape[0]):
            if layer.cin == 4:   # FeatureNet's conv0.0, K3's 4-channel layer: the sample as a stack of one 3-channel view, read in place
                ops.conv3d(xd[b:b + 1].squeeze(2), layer, out=out[b], backend=kind.backend, in_views=True)
            else:
                ops.conv3d(xd[b], layer, out=out[b], backend=kind.backend)
        ctx.save_for_backward(xd, weight, *(() if bias is None else (bias,)))
        ctx.kdepth, ctx.cache, ctx.kind, ctx.flat = kdepth, cache, kind, flat
        return out.squeeze(2) if flat else out

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, weight, *bias = ctx.saved_tensors   # (raises if the weight or the bias was changed in place since the forward)
        gy = gy.contiguous()
        if ctx.flat:
            gy = gy.unsqueeze(2)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            if ctx.kind.dgrad is None:
                layer = _cached_layer(ctx.cache, ctx.kind.bwd, weight, ctx.kind.build, ctx.kdepth)
            for b in range(x.shape[0]):
                if ctx.kind.dgrad is None:
                    ops.conv3d(gy[b], layer, out=gx[b], backend=ctx.kind.backend)
                else:
                    ctx.kind.dgrad(gy[b], weight.detach(), x[b], gx[b])
                launch_counts["dgrad"] += 1
        with_bias = {}
        if bias and ctx.needs_input_grad[4]:   # (the bias alone needs the weight-gradient kernel too: one launch pair gives both)
            gb = torch.empty_like(bias[0])
            with_bias = {"bias_out": gb}
        if ctx.needs_input_grad[1] or gb is not None:
            gw = torch.empty_like(weight, memory_format=torch.contiguous_format)
            for b in range(x.shape[0]):
                ctx.kind.wgrad(x[b], gy[b], ctx.kdepth, out=gw, accumulate=b > 0, **with_bias)
                launch_counts["wgrad"] += 1
            if not ctx.needs_input_grad[1]:
                gw = None
        if gx is not None and ctx.flat:
            gx = gx.squeeze(2)
        return gx, gw, None, None, gb


def _check_even(what, x, nd):
    if any(int(n) % 2 for n in x.shape[2:]):
        raise DmvsError(f"{what}: the stride-2 layer needs even {'D, H, W' if nd == 3 else 'H, W'} (its data gradient is the transposed "
                        f"layer with output_padding 1, and the U-Net's skip additions need them anyway); got {tuple(x.shape)}")


def _ctor_common(nd, m):
    """Holds for every layer the kernels take: kernel 3, padding 1, dilation 1, groups 1, no bias, zero padding."""
    return m.kernel_size == (3,) * nd and m.padding == (1,) * nd and m.dilation == (1,) * nd and m.groups == 1 and m.bias is None \
        and m.padding_mode == "zeros"


def _check_ctor_transposed(what, nd, m):
    pairs = tuple((co, ci) for ci, co in CHANNELS_S2[nd])
    if not _ctor_common(nd, m) or m.stride != (2,) * nd or m.output_padding != (1,) * nd or (m.in_channels, m.out_channels) not in pairs:
        raise DmvsError(f"{what}: only kernel 3, stride 2, padding 1, output_padding 1, dilation 1, groups 1, bias=False and (in, out) in "
                        f"{pairs} run on the gfx950 kernels (no ATen fallback); got {m}")


def _check_ctor(what, nd, m):
    if nd == 2 and m.kernel_size == (5, 5):
        if m.stride != (2, 2) or m.padding != (2, 2) or m.dilation != (1, 1) or m.groups != 1 or m.bias is not None \
                or m.padding_mode != "zeros" or (m.in_channels, m.out_channels) not in CHANNELS_K5S2:
            raise DmvsError(f"{what}: at kernel 5 only stride 2, padding 2, dilation 1, groups 1, bias=False and (in, out) in "
                            f"{CHANNELS_K5S2} run on the gfx950 kernels (no ATen fallback); got {m}")
        return
    if m.stride == (2,) * nd:
        if not _ctor_common(nd, m) or (m.in_channels, m.out_channels) not in CHANNELS_S2[nd]:
            raise DmvsError(f"{what}: at stride 2 only kernel 3, padding 1, dilation 1, groups 1, bias=False and (in, out) in "
                            f"{CHANNELS_S2[nd]} run on the gfx950 kernels (no ATen fallback); got {m}")
        return
    square = m.in_channels == m.out_channels and m.in_channels in CHANNELS
    ends = nd == 3 and (m.in_channels, m.out_channels) in CHANNELS_C2
    if not _ctor_common(nd, m) or m.stride != (1,) * nd or not (square or ends):
        raise DmvsError(f"{what}: only kernel 3, stride 1, padding 1, dilation 1, groups 1, bias=False and in == out in {CHANNELS}"
                        f"{f' or (in, out) in {CHANNELS_C2}' if nd == 3 else ''} run on the gfx950 kernels (no ATen fallback); got {m}")


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


class _DiffConv:
    """What the four layer classes share (mixed in front of the nn class): the constructor's refusals, the per-module cache of packed
    weights and the forward.  A 2D layer runs each sample as a D = 1 volume."""
    _nd, _transposed = 3, False

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        (_check_ctor_transposed if self._transposed else _check_ctor)(type(self).__name__, self._nd, self)
        self._packed = {}

    def forward(self, x):
        what, nd, weight = type(self).__name__, self._nd, self.weight
        # (chosen on every call from what nn.Module copies and pickles, so a copied or reloaded module runs as the one it was made from)
        k5 = self.kernel_size[0] == 5   # (odd extents too: K3d writes the fine tensor the forward read)
        down = self.stride[0] == 2 and not self._transposed and not k5
        if self._transposed:
            kind = _UP
        elif k5:
            kind = _DOWN5
        elif down:
            kind = _DOWN
        else:
            kind = _SQUARE if self.in_channels == self.out_channels else _ENDS
        _check_input(what, x, nd, self.in_channels)
        _check_weight(what, weight, x)
        if down:
            _check_even(what, x, nd)
        with torch.cuda.device(x.device):
            return _ConvFn.apply(x, weight, self._packed, kind)


class _DiffConvTranspose(_DiffConv):
    _transposed = True

    def forward(self, x, output_size=None):
        if output_size is not None:
            raise DmvsError(f"{type(self).__name__}: output_size is not supported (the output is twice the input)")
        return super().forward(x)


class DiffConv3d(_DiffConv, nn.Conv3d):
    """``nn.Conv3d(C, C, 3, stride=1, padding=1, bias=False)``, C in {16, 32, 64}, on K3 (forward, data gradient) and K3g (weight
    gradient); or ``nn.Conv3d(C, 2 * C, 3, stride=2, padding=1, bias=False)``, C in {8, 16, 32}, on K3 and K3h (even D, H, W); or
    ``nn.Conv3d(2, 8, 3, stride=1, padding=1, bias=False)`` / ``nn.Conv3d(8, 2, ...)``, conv0 / ``prob``, on K2 and K2g.  Input
    [B,C,D,H,W], fp32, contiguous, on a HIP device."""


class DiffConv2d(_DiffConv, nn.Conv2d):
    """``nn.Conv2d(C, C, 3, stride=1, padding=1, bias=False)``, C in {16, 32, 64}, on the kdepth-1 forms of K3 and K3g; or
    ``nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=False)`` on those of K3 and K3h (even H, W); or
    ``nn.Conv2d(C, 2 * C, 5, stride=2, padding=2, bias=False)``, C in {8, 16}, on K3, K3d and K3k (any H, W).  Input [B,C,H,W], fp32,
    contiguous, on a HIP device; each sample is a D = 1 volume."""
    _nd = 2


class DiffConvTranspose3d(_DiffConvTranspose, nn.ConvTranspose3d):
    """``nn.ConvTranspose3d(2 * C, C, 3, stride=2, padding=1, output_padding=1, bias=False)``, C in {32, 16, 8}, on K3 (forward: the
    transposed launch; data gradient: the stride-2 launch on the same weight) and K3h (weight gradient).  Input [B,2C,D,H,W], fp32,
    contiguous, on a HIP device; output [B,C,2D,2H,2W]."""


class DiffConvTranspose2d(_DiffConvTranspose, nn.ConvTranspose2d):
    """``nn.ConvTranspose2d(64, 32, 3, stride=2, padding=1, output_padding=1, bias=False)`` on the kdepth-1 forms of K3 and K3h.  Input
    [B,64,H,W], fp32, contiguous, on a HIP device; output [B,32,2H,2W]."""
    _nd = 2
