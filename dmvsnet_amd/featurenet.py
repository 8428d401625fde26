"""The differentiable FeatureNet: the six layers of the reference's ``FeatureNet`` (networks/module.py:274-340) that ``dmvsnet_amd.conv``
does not take, and the whole network built from them and from the layers it does take.  With it every convolution and every
BatchNorm + ReLU of FeatureNet runs on the gfx950 kernels in both directions.

``DiffFeatureConv2d`` is ``nn.Conv2d`` with another ``forward``; parameter names, shapes and the state-dict layout are the parent's.  It
accepts exactly these layers, as the reference constructs them (stride 1, padding ``k // 2``, dilation 1, groups 1, zero padding):

=========  ===================  ====================
conv0.0    3 -> 8, 3x3           no bias  (:284)
conv0.1    8 -> 8, 3x3           no bias  (:285)
out1       32 -> 64, 1x1         no bias  (:301)
inner1     16 -> 32, 1x1         bias     (:305)
inner2     8 -> 32, 1x1          bias     (:306)
out3       32 -> 16, 3x3         no bias  (:309)
=========  ===================  ====================

Everything else raises ``DmvsError`` in the constructor: there is no ATen fallback (``DiffConv2d`` keeps refusing these shapes; the
square layers and the 5x5 stride-2 layers stay there).

* forward: the bare K3 launch per sample (``ops.conv3d(..., backend="mfma")``), the weight packed on the device by one gather
  (``ops.pack_index_mfma_fpn``).  conv0.0 reads its 3-channel sample in place (``in_views``: K3's 4-channel layer with a zero fourth
  channel).  The two laterals run K3's epilogue with ``scale = ones``, ``shift = bias.detach()`` -- a view of the parameter's storage, so
  an in-place optimiser step on the bias is seen without re-packing;
* data gradient: the K3 launch of the layer out -> in on the weight transposed in (co, ci) and flipped in every tap, packed by the
  composed gather.  conv0.0 has none (the image takes no gradient: an input that requires one is refused); a frozen input skips the
  launch;
* weight and bias gradient: K3f (``ops.conv2d_wgrad_fpn``), one launch pair for both, accumulated over the samples in batch order.

Autograd keeps the input, the weight and the bias.  Packed layers are cached per module as in ``dmvsnet_amd.conv`` (``_cached_layer``:
keyed on the weight's version counter, data pointer and device; the laterals' key also carries the bias's data pointer and device).
fp32, contiguous, on a HIP device, any H, W.  No atomics: forward and gradients are bitwise reproducible.  Double backward raises.
In the code the layers are one more ``_Kind`` (``_FPN``) behind ``dmvsnet_amd.conv._ConvFn``, each sample a D = 1 volume: this module
holds the kind's builder and weight-gradient call, the constructor's refusals and the refusals of ``forward``.

``DiffFeatureConvBlock2d`` is the reference's ``Conv2d`` block (:28) on ``DiffFeatureConv2d`` + ``DiffBatchNormReLU2d`` (K5), for
conv0.0 / conv0.1; children and state-dict keys are the reference's.

``DiffFeatureNet(base_channels, num_stage=3, stride=4, mode="fpn", layernorm=False)`` is the reference's constructor with its
children (``conv0``, ``conv1``, ``conv2``, ``out1``, ``inner1``, ``inner2``, ``out2``, ``out3``), ``out_channels == [32, 16, 8]`` and
state-dict keys: a reference checkpoint's ``feature.*`` entries load with ``strict=True``.  Only ``base_channels == 8, num_stage == 3,
mode == "fpn"`` is accepted.  ``forward(x)``, x [B,3,H,W], returns the reference's dict of six tensors (``stage1``, ``stage1_c``, ...
``stage3_c``), split as :326-336.  The two nearest up-samplings, the additions onto the laterals and the splits stay torch ops: they
are elementwise or views, as the U-Nets' skip additions are (the inference path's fused up-sample epilogue and fused level-3 merge are
not used here).  H and W must be multiples of 4, so that the two up-sampled levels add back.  Train and eval mode both run.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from ._lib import DmvsError
from .bn import DiffBatchNormReLU2d, DiffConvBlock2d, _DiffBlock
from .conv import DiffConv2d, _check_input, _check_weight, _ConvFn, _Kind

__all__ = ["DiffFeatureConv2d", "DiffFeatureConvBlock2d", "DiffFeatureNet", "SHAPES", "BIAS_SHAPES"]

SHAPES = ops.FPN_SHAPES             # (in, out, kernel) of the six layers K3 and K3f run
BIAS_SHAPES = ops.FPN_BIAS_SHAPES   # ... of which inner1 and inner2 have a bias


def _build_fpn(weight, kdepth, transposed_flipped, bias=None):
    """The bare K3 layer of ``weight`` [out,in,k,k] (with ``bias``: its epilogue adds the bias) or of its transposed-flipped form, the
    layer out -> in of the data gradient."""
    cout, cin, k = (int(n) for n in weight.shape[:3])
    packed = ops.gather_packed(weight, ops.pack_index_mfma_fpn(cin, cout, k, transposed_flipped, weight.device), True)
    lin, lout = (cout, cin) if transposed_flipped else (max(cin, 4), cout)        # (conv0.0: K3's 4-channel layer)
    scale = shift = None
    if bias is not None:
        scale, shift = torch.ones_like(bias), bias.detach()   # (the shift shares the parameter's storage)
    return ops.ConvLayer("difffpn%dto%dk%d%s" % (cin, cout, k, "t" if transposed_flipped else ""), ops.CONV_S1 if k == 3 else ops.CONV2D_K1,
                         1, lin, lout, None, packed, scale, shift, False)


_KERNEL = {(cin, cout): k for cin, cout, k in SHAPES}   # (the six channel pairs are distinct)


def _wgrad_fpn(x, gy, kdepth, **kw):
    return ops.conv2d_wgrad_fpn(x, gy, _KERNEL[(int(x.shape[0]), int(gy.shape[0]))], **kw)


# FeatureNet's rectangular stride-1 layers behind conv._ConvFn: K3 forward, K3 on the transposed-flipped weight for the data gradient, K3f
_FPN = _Kind(_build_fpn, False, True, "mfma", _wgrad_fpn)


def _check_ctor(what, m):
    shape = (m.in_channels, m.out_channels, m.kernel_size[0])
    k = m.kernel_size[0]
    ok = shape in SHAPES and m.kernel_size == (k, k) and m.stride == (1, 1) and m.padding == (k // 2, k // 2) and m.dilation == (1, 1) \
        and m.groups == 1 and m.padding_mode == "zeros" and (m.bias is not None) == (shape in BIAS_SHAPES)
    if not ok:
        raise DmvsError(f"{what}: only (in, out, kernel) in {SHAPES} with stride 1, padding kernel // 2, dilation 1, groups 1, zero padding "
                        f"and a bias exactly for {BIAS_SHAPES} run on the gfx950 kernels (no ATen fallback); got {m}")


class DiffFeatureConv2d(nn.Conv2d):
    """One of FeatureNet's six rectangular stride-1 layers (see the module's text) on K3 (forward, data gradient) and K3f (weight and
    bias gradient).  Input [B,Cin,H,W], fp32, contiguous, on a HIP device; any H, W."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        _check_ctor(type(self).__name__, self)
        self._packed = {}

    def forward(self, x):
        what, weight, bias = type(self).__name__, self.weight, self.bias
        _check_input(what, x, 2, self.in_channels)
        _check_weight(what, weight, x)
        if bias is not None and (bias.device != x.device or bias.dtype != torch.float32 or not bias.is_contiguous()):
            raise DmvsError(f"{what}: the bias must be contiguous fp32 on the input's device {x.device}; it is {bias.dtype} on {bias.device}")
        if self.in_channels == 3 and x.requires_grad:
            raise DmvsError(f"{what}: conv0.0 has no data gradient (the image takes none); the input must not require one")
        with torch.cuda.device(x.device):   # (each sample a D = 1 volume, as DiffConv2d's)
            return _ConvFn.apply(x, weight, self._packed, _FPN, bias)


class DiffFeatureConvBlock2d(_DiffBlock):
    """The reference's ``Conv2d`` block (networks/module.py:28) on ``DiffFeatureConv2d`` + ``DiffBatchNormReLU2d``: conv0.0 / conv0.1."""
    _conv_cls, _bn_cls = DiffFeatureConv2d, DiffBatchNormReLU2d


class DiffFeatureNet(nn.Module):
    """The reference's ``FeatureNet`` (networks/module.py:274-340) on the differentiable layers; see the module's text."""

    def __init__(self, base_channels, num_stage=3, stride=4, mode="fpn", layernorm=False):
        super().__init__()
        if base_channels != 8 or num_stage != 3 or mode != "fpn":
            raise DmvsError(f"{type(self).__name__}: only base_channels == 8, num_stage == 3, mode == 'fpn' run on the gfx950 kernels (no "
                            f"ATen fallback); got base_channels = {base_channels}, num_stage = {num_stage}, mode = {mode!r}")
        self.mode, self.stride, self.base_channels, self.num_stage, self.layernorm = mode, stride, base_channels, num_stage, layernorm
        b = base_channels
        self.conv0 = nn.Sequential(DiffFeatureConvBlock2d(3, b, 3, 1, padding=1), DiffFeatureConvBlock2d(b, b, 3, 1, padding=1))
        self.conv1 = nn.Sequential(DiffConvBlock2d(b, b * 2, 5, stride=2, padding=2), DiffConvBlock2d(b * 2, b * 2, 3, 1, padding=1),
                                   DiffConvBlock2d(b * 2, b * 2, 3, 1, padding=1))
        self.conv2 = nn.Sequential(DiffConvBlock2d(b * 2, b * 4, 5, stride=2, padding=2), DiffConvBlock2d(b * 4, b * 4, 3, 1, padding=1),
                                   DiffConvBlock2d(b * 4, b * 4, 3, 1, padding=1))
        self.out1 = DiffFeatureConv2d(b * 4, b * 8, 1, bias=False)
        self.out_channels = [4 * b]
        final_chs = b * 4
        self.inner1 = DiffFeatureConv2d(b * 2, final_chs, 1, bias=True)
        self.inner2 = DiffFeatureConv2d(b, final_chs, 1, bias=True)
        self.out2 = DiffConv2d(final_chs, b * 4, 3, padding=1, bias=False)
        self.out3 = DiffFeatureConv2d(final_chs, b * 2, 3, padding=1, bias=False)
        self.out_channels.append(b * 2)
        self.out_channels.append(b)

    def forward(self, x):
        what = type(self).__name__
        _check_input(what, x, 2, 3)
        H, W = (int(n) for n in x.shape[2:])
        if H % 4 or W % 4 or H < 4 or W < 4:
            raise DmvsError(f"{what}: H and W must be multiples of 4 (two stride-2 levels, whose up-sampled maps are added back onto the "
                            f"finer laterals); got H, W = {(H, W)}")
        conv0 = self.conv0(x)
        conv1 = self.conv1(conv0)
        conv2 = self.conv2(conv1)
        outputs = {}
        out = self.out1(conv2)
        outputs["stage1"], outputs["stage1_c"] = out.split([out.shape[1] // 2, out.shape[1] // 2], 1)
        intra = F.interpolate(conv2, scale_factor=2, mode="nearest") + self.inner1(conv1)
        out = self.out2(intra)
        outputs["stage2"], outputs["stage2_c"] = out.split([out.shape[1] // 2, out.shape[1] // 2], 1)
        intra = F.interpolate(intra, scale_factor=2, mode="nearest") + self.inner2(conv0)
        out = self.out3(intra)
        outputs["stage3"], outputs["stage3_c"] = out.split([out.shape[1] // 2, out.shape[1] // 2], 1)
        return outputs
