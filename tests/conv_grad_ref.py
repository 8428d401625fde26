"""Yardstick of the differentiable stride-1 square convolutions (K3 forward / data gradient, K3g weight gradient): a float64
restatement that uses no convolution library -- zero-padded copies, tap-shifted slices and einsum -- and the block the reference
builds around such a layer (conv + train-mode BatchNorm + ReLU, networks/module.py:28-70, 120-163), restated in float64 with
autograd over the restatement.  No product code here.

Layouts: activations [B,C,D,H,W] (a 2D layer is D = 1), weights [C,C,kd,3,3] (kd 3, or 1 for the 2D layers: no z taps).
The functions run on whatever device their inputs are on, in ``dtype`` (float64 by default; float32 gives the stock-ATen fp32 run of
the same restatement, the ``e_ref`` of the bare-kernel tests)."""
import torch
import torch.nn.functional as F

SHAPES = ((16, 3), (32, 3), (64, 3), (64, 1), (16, 1), (32, 1))   # (C, kdepth): the six square shapes K3 compiles
KINK_MARGIN = 1e-5
BN_EPS = 1e-5

# [B,C,D,H,W] (kd 3) / [B,C,H,W] (kd 1, D = 1 here).  Seeds: the first for which no BatchNorm output lies within KINK_MARGIN of 0.
GOLDEN_CASES = {
    "c16_3x9x11": dict(C=16, kd=3, D=3, H=9, W=11, B=1, seed=0),
    "c16_b2_1x5x7": dict(C=16, kd=3, D=1, H=5, W=7, B=2, seed=0),
    "c32_2x7x10": dict(C=32, kd=3, D=2, H=7, W=10, B=1, seed=0),
    "c64_2d_b2_6x9": dict(C=64, kd=1, D=1, H=6, W=9, B=2, seed=0),
    "c16_2d_19x35": dict(C=16, kd=1, D=1, H=19, W=35, B=1, seed=0),
}


def rel_dist(a, b):
    """max|a - b| / max|b| in float64."""
    a, b = a.detach().to("cpu", torch.float64), b.detach().to("cpu", torch.float64)
    return ((a - b).abs().max() / b.abs().max()).item()


def _padded(t, kd):
    return F.pad(t, (1, 1, 1, 1, 1 if kd == 3 else 0, 1 if kd == 3 else 0))


def _taps(kd):
    return [(kz, ky, kx) for kz in range(kd) for ky in range(3) for kx in range(3)]


def conv_ref(x, w, kd, dtype=torch.float64):
    """y[b,co,z,y,x] = sum_{ci,taps} w[co,ci,kz,ky,kx] * x[b,ci,z+kz-1,y+ky-1,x+kx-1]  (differentiable)."""
    x, w = x.to(dtype), w.to(dtype)
    B, C, D, H, W = x.shape
    xp = _padded(x, kd)
    out = torch.zeros_like(x)
    for kz, ky, kx in _taps(kd):
        out = out + torch.einsum("oi,bidhw->bodhw", w[:, :, kz, ky, kx], xp[:, :, kz:kz + D, ky:ky + H, kx:kx + W])
    return out


def wgrad_ref(x, gy, kd, dtype=torch.float64):
    """dW[co,ci,kz,ky,kx] = sum_{b,z,y,x} gy[b,co,z,y,x] * x[b,ci,z+kz-1,y+ky-1,x+kx-1]: 27 (9) tap-shifted einsum products."""
    x, gy = x.to(dtype), gy.to(dtype)
    B, C, D, H, W = x.shape
    xp = _padded(x, kd)
    g2 = gy.permute(1, 0, 2, 3, 4).reshape(C, -1)
    gw = torch.zeros(C, C, kd, 3, 3, dtype=dtype, device=x.device)
    for kz, ky, kx in _taps(kd):
        xs = xp[:, :, kz:kz + D, ky:ky + H, kx:kx + W].permute(1, 0, 2, 3, 4).reshape(C, -1)
        gw[:, :, kz, ky, kx] = torch.einsum("ov,iv->oi", g2, xs)
    return gw


def dgrad_ref(gy, w, kd, dtype=torch.float64):
    """dX[b,ci,z,y,x] = sum_{co,taps} w[co,ci,kz,ky,kx] * gy[b,co,z-kz+1,y-ky+1,x-kx+1]: the transposed form."""
    gy, w = gy.to(dtype), w.to(dtype)
    B, C, D, H, W = gy.shape
    gp = _padded(gy, kd)
    gx = torch.zeros_like(gy)
    for kz, ky, kx in _taps(kd):
        z0 = 2 - kz if kd == 3 else 0
        gx = gx + torch.einsum("oi,bodhw->bidhw", w[:, :, kz, ky, kx], gp[:, :, z0:z0 + D, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W])
    return gx


def make_case(C, kd, D, H, W, B, seed):
    """fp32 inputs of one block: x, weight (xavier-sized), BatchNorm gamma / beta, upstream gradient gy."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * C + kd)
    x = torch.randn(B, C, D, H, W, generator=g)
    # the weight sits on a 2^-9 grid (it is the largest stored tensor and compresses that way); still fp32 data like any other
    w = torch.round(torch.randn(C, C, kd, 3, 3, generator=g) * (2.0 / (C * 9 * kd)) ** 0.5 * 512.0) / 512.0
    gamma = 1.0 + 0.2 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    gy = torch.randn(B, C, D, H, W, generator=g)
    return dict(C=C, kd=kd, x=x, w=w, gamma=gamma, beta=beta, gy=gy)


def golden_case(g, name):
    """The stored case ``name`` of op_conv_grad.npz as torch tensors (inputs and the reference's recorded fp32 results)."""
    kw = GOLDEN_CASES[name]
    case = dict(C=kw["C"], kd=kw["kd"])
    for k in ("x", "w", "gamma", "beta", "gy", "out", "g_x", "g_w", "g_gamma", "g_beta"):
        case[k] = torch.from_numpy(g[f"{name}.{k}"])
    return case


def bn_train(y, gamma, beta):
    """Train-mode BatchNorm of [B,C,D,H,W] in y's dtype: batch statistics, biased variance, eps 1e-5."""
    mean = y.mean(dim=(0, 2, 3, 4), keepdim=True)
    var = ((y - mean) ** 2).mean(dim=(0, 2, 3, 4), keepdim=True)
    sh = (1, -1, 1, 1, 1)
    return (y - mean) / torch.sqrt(var + BN_EPS) * gamma.to(y.dtype).reshape(sh) + beta.to(y.dtype).reshape(sh)


def bn_pre_relu_f64(case):
    """The BatchNorm output (before the ReLU) of the block in float64."""
    return bn_train(conv_ref(case["x"], case["w"], case["kd"]), case["gamma"], case["beta"])


def kink_violations(case):
    """Number of BatchNorm outputs within KINK_MARGIN of the ReLU kink (must be 0: a flipped kink dominates every gradient)."""
    return int((bn_pre_relu_f64(case).abs() <= KINK_MARGIN).sum().item())


def block_f64(case):
    """conv + train-mode BatchNorm (biased variance, eps 1e-5) + ReLU in float64 and its gradients for the upstream gradient gy."""
    leaves = {k: case[k].double().clone().requires_grad_(True) for k in ("x", "w", "gamma", "beta")}
    out = torch.relu(bn_pre_relu_f64({**case, **leaves}))
    gx, gw, gg, gb = torch.autograd.grad(out, [leaves[k] for k in ("x", "w", "gamma", "beta")], case["gy"].double())
    return dict(out=out.detach(), g_x=gx, g_w=gw, g_gamma=gg, g_beta=gb)
