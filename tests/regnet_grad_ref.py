"""Yardsticks of the differentiable 2-channel ends (conv0 2 -> 8, prob 8 -> 2: K2 forward / data gradient, K2g weight gradient) and of
the four regularisation networks built on them (dmvsnet_amd.regnet).  No product code here.

* ``g_ref`` restates K2g's one formula on a pair of equally sized volumes, P with 8 channels and Q with 2, with no convolution library
  (a zero-padded copy, tap-shifted slices and einsum)::

      G[p][q][tz][ty][tx] = sum_{b,v} P[b][p][v] * Q[b][q][v + (tz - 1, ty - 1, tx - 1)]          (Q is zero outside the volume)

  ``wgrad_ref`` applies the two role maps: conv0 (P = dY, Q = X) ``dW[p][q][t] = G[p][q][t]``; prob (P = X, Q = dY)
  ``dW[q][p][t] = G[p][q][flip(t)]``.  tests/test_regnet_grad_cpu.py checks it against float64 autograd of F.conv3d.
* ``conv_ref`` / ``dgrad_ref``: the forward and the data gradient of a 3x3x3 pad-1 layer with any channel counts, the same way.
* ``PlainPart`` / ``PlainPartRefine``: the reference's CostRegNet_part / CostRegNet_part_refine (networks/module.py:358-436) as a stack
  of stock nn layers with the reference's child names and state-dict keys; run in float64 on the CPU it is the yardstick of the whole
  networks, in float32 the stock-ATen ``e_ref``.  ``run_part`` returns the output, every gradient and every BatchNorm output.

Functions run on whatever device their inputs are on, in ``dtype`` (float64 by default; float32 gives the stock-ATen fp32 run of the
same restatement, the ``e_ref`` of the bare-kernel tests)."""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

SHAPES = ((2, 8), (8, 2))   # (Cin, Cout): conv0 and prob
KINK_MARGIN = 1e-4          # no BatchNorm output of the float64 run of a stored network case lies this close to the ReLU kink
BN_EPS = 1e-5
FACTOR = 8.0                # criterion: e_hip <= FACTOR * e_ref ...
EPS32 = 2.0 ** -23          # ... and where e_ref < 4 * EPS32 the bound is 16 * EPS32

# the stored whole-network cases of tests/golden/op_regnet_grad.npz: batch 2, the smallest volumes the U-Nets take with ragged W / 8
GOLDEN_NETS = {"part": dict(refine=False, B=2, D=8, H=16, W=24), "refine": dict(refine=True, B=2, D=4, H=16, W=24)}
STORED_WEIGHT_GRADS = ("conv0.conv.weight", "conv1.conv.weight", "conv2.conv.weight", "conv11.conv.weight", "prob.weight")
BLOCKS = ("conv0", "conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv9", "conv11")   # in forward order


def bound_of(e_ref):
    return FACTOR * e_ref if e_ref >= 4 * EPS32 else 16 * EPS32


def rel_dist(a, b):
    """max|a - b| / max|b| in float64."""
    a, b = a.detach().to("cpu", torch.float64), b.detach().to("cpu", torch.float64)
    return ((a - b).abs().max() / b.abs().max()).item()


def _taps():
    return [(kz, ky, kx) for kz in range(3) for ky in range(3) for kx in range(3)]


def g_ref(P, Q, dtype=torch.float64):
    """P [B,8,D,H,W], Q [B,2,D,H,W] -> G [8,2,3,3,3]."""
    P, Q = P.to(dtype), Q.to(dtype)
    B, _, D, H, W = P.shape
    qp = F.pad(Q, (1, 1, 1, 1, 1, 1))
    p2 = P.permute(1, 0, 2, 3, 4).reshape(P.shape[1], -1)
    G = torch.zeros(P.shape[1], Q.shape[1], 3, 3, 3, dtype=dtype, device=P.device)
    for tz, ty, tx in _taps():
        qs = qp[:, :, tz:tz + D, ty:ty + H, tx:tx + W].permute(1, 0, 2, 3, 4).reshape(Q.shape[1], -1)
        G[:, :, tz, ty, tx] = torch.einsum("pv,qv->pq", p2, qs)
    return G


def wgrad_ref(x, gy, dtype=torch.float64):
    """x [B,Cin,D,H,W], gy [B,Cout,D,H,W], (Cin, Cout) in SHAPES -> dW [Cout,Cin,3,3,3] through G and the layer's role map."""
    if (x.shape[1], gy.shape[1]) == (2, 8):     # conv0: P = dY, Q = X, dW[co = p][ci = q][t] = G[p][q][t]
        return g_ref(gy, x, dtype)
    assert (x.shape[1], gy.shape[1]) == (8, 2)  # prob: P = X, Q = dY, dW[co = q][ci = p][t] = G[p][q][flip(t)]
    return g_ref(x, gy, dtype).flip(2, 3, 4).transpose(0, 1).contiguous()


def conv_ref(x, w, dtype=torch.float64):
    """y[b,co,v] = sum_{ci,t} w[co,ci,t] * x[b,ci,v + t - 1]."""
    x, w = x.to(dtype), w.to(dtype)
    B, _, D, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    out = torch.zeros(B, w.shape[0], D, H, W, dtype=dtype, device=x.device)
    for kz, ky, kx in _taps():
        out = out + torch.einsum("oi,bidhw->bodhw", w[:, :, kz, ky, kx], xp[:, :, kz:kz + D, ky:ky + H, kx:kx + W])
    return out


def dgrad_ref(gy, w, dtype=torch.float64):
    """dX[b,ci,v] = sum_{co,t} w[co,ci,t] * gy[b,co,v - t + 1]: the transposed form."""
    gy, w = gy.to(dtype), w.to(dtype)
    B, _, D, H, W = gy.shape
    gp = F.pad(gy, (1, 1, 1, 1, 1, 1))
    gx = torch.zeros(B, w.shape[1], D, H, W, dtype=dtype, device=gy.device)
    for kz, ky, kx in _taps():
        gx = gx + torch.einsum("oi,bodhw->bidhw", w[:, :, kz, ky, kx], gp[:, :, 2 - kz:2 - kz + D, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W])
    return gx


def rand_case(cin, cout, D, H, W, B=1, seed=0):
    """fp32 x [B,cin,D,H,W], gy [B,cout,D,H,W] and a He-sized weight [cout,cin,3,3,3] (CPU)."""
    gen = torch.Generator().manual_seed(7919 * seed + 31 * cin + cout + D * H * W)
    x = torch.randn(B, cin, D, H, W, generator=gen)
    gy = torch.randn(B, cout, D, H, W, generator=gen)
    w = torch.randn(cout, cin, 3, 3, 3, generator=gen) * (2.0 / (cin * 27)) ** 0.5
    return x, gy, w


# ------------------------------------------------------------------------------------------------ the whole networks on stock layers
class PlainBlock(nn.Module):
    """The reference's Conv3d / Deconv3d / Conv2d / Deconv2d block: layer + BatchNorm + ReLU, children ``conv`` and ``bn``."""

    def __init__(self, conv):
        super().__init__()
        self.conv = conv
        self.bn = (nn.BatchNorm3d if isinstance(conv, (nn.Conv3d, nn.ConvTranspose3d)) else nn.BatchNorm2d)(conv.out_channels)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


def _c3(ci, co, stride=1):
    return PlainBlock(nn.Conv3d(ci, co, 3, stride=stride, padding=1, bias=False))


def _t3(ci, co):
    return PlainBlock(nn.ConvTranspose3d(ci, co, 3, stride=2, padding=1, output_padding=1, bias=False))


class PlainPart(nn.Module):
    """CostRegNet_part (networks/module.py:358-398) on stock layers."""
    refine = False

    def __init__(self, in_channels=2, b=8):
        super().__init__()
        self.conv0 = _c3(in_channels, b)
        self.conv1, self.conv2 = _c3(b, 2 * b, 2), _c3(2 * b, 2 * b)
        self.conv3, self.conv4 = _c3(2 * b, 4 * b, 2), _c3(4 * b, 4 * b)
        self._bottom(b)
        self.conv9, self.conv11 = _t3(4 * b, 2 * b), _t3(2 * b, b)
        self.prob = nn.Conv3d(b, 2, 3, stride=1, padding=1, bias=False)

    def _bottom(self, b):
        self.conv5, self.conv6 = _c3(4 * b, 8 * b, 2), _c3(8 * b, 8 * b)
        self.conv7 = _t3(8 * b, 4 * b)

    def forward(self, x):
        conv0 = self.conv0(x)
        conv2 = self.conv2(self.conv1(conv0))
        conv4 = self.conv4(self.conv3(conv2))
        if self.refine:
            conv4 = conv4.squeeze(2)
        x = self.conv6(self.conv5(conv4))
        x = conv4 + self.conv7(x)
        if self.refine:
            x = x.unsqueeze(2)
        x = conv2 + self.conv9(x)
        x = conv0 + self.conv11(x)
        return self.prob(x)


class PlainPartRefine(PlainPart):
    """CostRegNet_part_refine (networks/module.py:400-436) on stock layers: conv5 / conv6 / conv7 are 2D."""
    refine = True

    def _bottom(self, b):
        self.conv5 = PlainBlock(nn.Conv2d(4 * b, 8 * b, 3, stride=2, padding=1, bias=False))
        self.conv6 = PlainBlock(nn.Conv2d(8 * b, 8 * b, 3, stride=1, padding=1, bias=False))
        self.conv7 = PlainBlock(nn.ConvTranspose2d(8 * b, 4 * b, 3, stride=2, padding=1, output_padding=1, bias=False))


class PlainPair(nn.Module):
    """CostRegNet / CostRegNet_refine (networks/module.py:342-357) on stock layers."""

    def __init__(self, refine):
        super().__init__()
        part = PlainPartRefine if refine else PlainPart
        self.cosR_small, self.cosR_huge = part(), part()

    def forward(self, x):
        return torch.cat((self.cosR_small(x), self.cosR_huge(x)), dim=1)


def bn_outputs(net):
    """Hooks that record every block's BatchNorm output (before the ReLU) of the next forward, as {block name: tensor}.  ``net`` is any
    module with the reference's child names whose blocks have a ``bn`` child that is a stock BatchNorm (ReLU applied after it)."""
    pre, hooks = {}, []
    for name in BLOCKS:
        hooks.append(getattr(net, name).bn.register_forward_hook(lambda mod, inp, out, name=name: pre.__setitem__(name, out.detach().clone())))
    return pre, hooks


def run_part(net, x, gy):
    """Train-mode forward + backward of a part (stock or reference) on a fresh leaf: output, {name: gradient} (``x`` and every
    parameter) and {block: BatchNorm output}."""
    net.train()
    pre, hooks = bn_outputs(net)
    dt = next(net.parameters()).dtype
    xin = x.detach().to(dt).clone().requires_grad_(True)
    for p in net.parameters():
        p.grad = None
    out = net(xin)
    for h in hooks:
        h.remove()
    out.backward(gy.to(dt))
    return out.detach(), {"x": xin.grad, **{n: p.grad for n, p in net.named_parameters()}}, pre


def net_inputs(name, seed):
    """x, gy (fp32, CPU) of the stored case ``name`` for ``seed``."""
    kw = GOLDEN_NETS[name]
    g = np.random.Generator(np.random.PCG64([seed, 1 + int(kw["refine"])]))
    shape = (kw["B"], 2, kw["D"], kw["H"], kw["W"])
    x = torch.from_numpy(g.standard_normal(shape, dtype=np.float32) * np.float32(0.3))
    gy = torch.from_numpy(g.standard_normal(shape, dtype=np.float32))
    return x, gy


def net_weights(name, seed, beta=None):
    """The case's state dict: dmvsnet_amd.synth's recipe on the part's own keys for ``seed``; ``beta`` {block: [C] array} replaces the
    BatchNorm biases (the stored case carries them: see tests/golden/make_golden_regnet_grad.py)."""
    from dmvsnet_amd import synth
    part = (PlainPartRefine if GOLDEN_NETS[name]["refine"] else PlainPart)()
    sd = synth.synth_state_dict(part.state_dict(), seed)
    for blk, b in (beta or {}).items():
        sd[f"{blk}.bn.bias"] = torch.as_tensor(np.asarray(b), dtype=torch.float32).clone()
    return sd


def plain_net(name, sd, dtype):
    net = (PlainPartRefine if GOLDEN_NETS[name]["refine"] else PlainPart)()
    net.load_state_dict(sd, strict=True)
    return net.to(dtype)


def kink_violations(pre):
    """Number of BatchNorm outputs within KINK_MARGIN of the ReLU kink."""
    return sum(int((p.abs() <= KINK_MARGIN).sum().item()) for p in pre.values())


def same_masks(pre_a, pre_b):
    """The ReLU masks (BatchNorm output > 0) of two runs agree at every block."""
    return set(pre_a) == set(pre_b) and all(torch.equal(pre_a[k].cpu() > 0, pre_b[k].cpu() > 0) for k in pre_a)
