"""The four regularisation networks of the reference (networks/module.py:342-436) built from this package's differentiable layers:
every convolution and every BatchNorm + ReLU of a training step runs on the gfx950 kernels in both directions.

``DiffCostRegNetPart`` / ``DiffCostRegNetPartRefine`` are ``CostRegNet_part`` / ``CostRegNet_part_refine``; ``DiffCostRegNet`` /
``DiffCostRegNetRefine`` are ``CostRegNet`` / ``CostRegNet_refine`` (two parts, ``cosR_small`` and ``cosR_huge``, on the same input,
concatenated along the channels).  Constructor ``(in_channels, base_channels, stage=0)``, children (``conv0`` .. ``conv11``, ``prob``)
and state-dict keys are the reference's: a reference checkpoint's ``cost_regularization.N.*`` / ``cost_regularization_refine.N.*``
entries load with ``strict=True``.  A reference user swaps the four constructors in ``networks/mvsnet.py``.

Only ``in_channels == 2, base_channels == 8`` is accepted -- the shapes the kernels compile; everything else raises ``DmvsError`` in the
constructor (no ATen fallback).

* conv0   ``DiffConvBlock3d(2, 8, padding=1)``: K2's direct ``Cin == 2`` form forward, K2's ``cout2`` kernel for the data gradient, K2g for
  the weight gradient; K5 for BatchNorm + ReLU;
* conv1 .. conv6   ``DiffConvBlock3d`` / ``DiffConvBlock2d``: K3 forward and data gradient, K3g (stride 1) / K3h (stride 2); K5;
* conv7 .. conv11   ``DiffDeconvBlock3d`` / ``DiffDeconvBlock2d``: K3 forward and data gradient, K3h; K5;
* prob   ``DiffConv3d(8, 2, 3, padding=1, bias=False)``: K2's ``cout2`` kernel forward, its direct ``Cin == 2`` form for the data gradient,
  K2g for the weight gradient.

The three skip additions of a part, the channel ``cat`` of the pair and the refine part's ``squeeze(2)`` / ``unsqueeze(2)`` around its
2D levels stay torch ops: they are elementwise (or views) and at the memory roofline already.  ``dmvsnet_amd.featurenet`` does the same
for FeatureNet; between them no ATen convolution or normalisation is left in a training step.

Extents: the full part halves D, H, W three times and adds the up-sampled levels back, so all three must be multiples of 8.  The refine
part halves D twice down to ONE plane (its conv5 .. conv7 are 2D layers on [B,C,H,W]), so D must be 4, and H, W multiples of 8.
Anything else raises a ``DmvsError`` that names the rule.  Inputs are [B,2,D,H,W], fp32, contiguous, on a HIP device.
"""
from __future__ import annotations

import torch
from torch import nn

from ._lib import DmvsError
from .bn import DiffConvBlock2d, DiffConvBlock3d, DiffDeconvBlock2d, DiffDeconvBlock3d
from .conv import DiffConv3d

__all__ = ["DiffCostRegNetPart", "DiffCostRegNetPartRefine", "DiffCostRegNet", "DiffCostRegNetRefine"]


def _check_channels(what, in_channels, base_channels):
    if in_channels != 2 or base_channels != 8:
        raise DmvsError(f"{what}: only in_channels == 2, base_channels == 8 run on the gfx950 kernels (no ATen fallback); got "
                        f"in_channels = {in_channels}, base_channels = {base_channels}")


def _check_volume(what, x, refine):
    if not torch.is_tensor(x) or x.dim() != 5 or x.shape[1] != 2:
        raise DmvsError(f"{what}: the input must be a [B,2,D,H,W] tensor, got "
                        f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    D, H, W = (int(n) for n in x.shape[2:])
    if refine:
        if D != 4 or H % 8 or W % 8 or H < 8 or W < 8:
            raise DmvsError(f"{what}: D must be 4 (two stride-2 levels leave the one plane the 2D levels conv5 .. conv7 take) and H, W "
                            f"multiples of 8 (three stride-2 levels, added back by the skip connections); got D, H, W = {(D, H, W)}")
    elif D % 8 or H % 8 or W % 8 or min(D, H, W) < 8:
        raise DmvsError(f"{what}: D, H, W must be multiples of 8 (three stride-2 levels, added back by the skip connections); got "
                        f"D, H, W = {(D, H, W)}")


class DiffCostRegNetPart(nn.Module):
    """The reference's ``CostRegNet_part`` (networks/module.py:358-398): a 3D U-Net 2 -> 8 -> 16 -> 32 -> 64 -> ... -> 8 -> 2."""

    def __init__(self, in_channels, base_channels, stage=0):
        super().__init__()
        _check_channels(type(self).__name__, in_channels, base_channels)
        b = base_channels
        self.conv0 = DiffConvBlock3d(in_channels, b, padding=1)
        self.conv1 = DiffConvBlock3d(b, b * 2, stride=2, padding=1)
        self.conv2 = DiffConvBlock3d(b * 2, b * 2, padding=1)
        self.conv3 = DiffConvBlock3d(b * 2, b * 4, stride=2, padding=1)
        self.conv4 = DiffConvBlock3d(b * 4, b * 4, padding=1)
        self.conv5 = DiffConvBlock3d(b * 4, b * 8, stride=2, padding=1)
        self.conv6 = DiffConvBlock3d(b * 8, b * 8, padding=1)
        self.conv7 = DiffDeconvBlock3d(b * 8, b * 4, stride=2, padding=1, output_padding=1)
        self.conv9 = DiffDeconvBlock3d(b * 4, b * 2, stride=2, padding=1, output_padding=1)
        self.conv11 = DiffDeconvBlock3d(b * 2, b, stride=2, padding=1, output_padding=1)
        self.prob = DiffConv3d(b, 2, 3, stride=1, padding=1, bias=False)

    def forward(self, x):
        _check_volume(type(self).__name__, x, False)
        conv0 = self.conv0(x)
        conv2 = self.conv2(self.conv1(conv0))
        conv4 = self.conv4(self.conv3(conv2))
        x = self.conv6(self.conv5(conv4))
        x = conv4 + self.conv7(x)
        x = conv2 + self.conv9(x)
        x = conv0 + self.conv11(x)
        return self.prob(x)


class DiffCostRegNetPartRefine(nn.Module):
    """The reference's ``CostRegNet_part_refine`` (networks/module.py:400-436): as the full part down to quarter resolution, where the
    volume is one plane deep and conv5 / conv6 / conv7 are 2D layers."""

    def __init__(self, in_channels, base_channels, stage=0):
        super().__init__()
        _check_channels(type(self).__name__, in_channels, base_channels)
        b = base_channels
        self.conv0 = DiffConvBlock3d(in_channels, b, padding=1)
        self.conv1 = DiffConvBlock3d(b, b * 2, stride=2, padding=1)
        self.conv2 = DiffConvBlock3d(b * 2, b * 2, padding=1)
        self.conv3 = DiffConvBlock3d(b * 2, b * 4, stride=2, padding=1)
        self.conv4 = DiffConvBlock3d(b * 4, b * 4, padding=1)
        self.conv5 = DiffConvBlock2d(b * 4, b * 8, 3, stride=2, padding=1)
        self.conv6 = DiffConvBlock2d(b * 8, b * 8, 3, padding=1)
        self.conv7 = DiffDeconvBlock2d(b * 8, b * 4, 3, stride=2, padding=1, output_padding=1)
        self.conv9 = DiffDeconvBlock3d(b * 4, b * 2, stride=2, padding=1, output_padding=1)
        self.conv11 = DiffDeconvBlock3d(b * 2, b, stride=2, padding=1, output_padding=1)
        self.prob = DiffConv3d(b, 2, 3, stride=1, padding=1, bias=False)

    def forward(self, x, stage=0):
        _check_volume(type(self).__name__, x, True)
        conv0 = self.conv0(x)
        conv2 = self.conv2(self.conv1(conv0))
        conv4 = self.conv4(self.conv3(conv2)).squeeze(2)
        x = self.conv6(self.conv5(conv4))
        x = conv4 + self.conv7(x)
        x = x.unsqueeze(2)
        x = conv2 + self.conv9(x)
        x = conv0 + self.conv11(x)
        return self.prob(x)


class _Pair(nn.Module):
    """Two parts on the same input, concatenated along the channels (networks/module.py:342-357)."""
    _part = None

    def __init__(self, in_channels, base_channels, stage=0):
        super().__init__()
        _check_channels(type(self).__name__, in_channels, base_channels)
        self.cosR_small = self._part(in_channels, base_channels, stage=0)
        self.cosR_huge = self._part(in_channels, base_channels, stage=0)

    def forward(self, x):
        return torch.cat((self.cosR_small(x), self.cosR_huge(x)), dim=1)


class DiffCostRegNet(_Pair):
    """The reference's ``CostRegNet``: ``cosR_small`` and ``cosR_huge``, two ``DiffCostRegNetPart``; output [B,4,D,H,W]."""
    _part = DiffCostRegNetPart


class DiffCostRegNetRefine(_Pair):
    """The reference's ``CostRegNet_refine``: two ``DiffCostRegNetPartRefine``; output [B,4,4,H,W]."""
    _part = DiffCostRegNetPartRefine
