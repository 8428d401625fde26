"""Yardstick of the differentiable BatchNorm + ReLU (K5): a float64 restatement that calls no ``batch_norm`` -- per-channel mean, biased
variance, the closed-form backward and the running-statistics update, written out -- plus the seeded case generator of the tests and
the kink count.  No product code here.

Layouts: x, gy [B,C,*spatial]; gamma, beta, mean, invstd, running_* [C].  The functions run on the CPU in ``dtype`` (float64 by
default)."""
import torch

KINK_MARGIN = 1e-5
BN_EPS = 1e-5
CHANNELS = (8, 16, 32, 64)


def rel_dist(a, b):
    """max|a - b| / max|b| in float64."""
    a, b = a.detach().to("cpu", torch.float64), b.detach().to("cpu", torch.float64)
    return ((a - b).abs().max() / b.abs().max()).item()


def _per_channel(t):
    """[B,C,*] -> [C, B * V]"""
    return t.transpose(0, 1).reshape(t.shape[1], -1)


def _bc(v, t):
    """[C] -> broadcastable against [B,C,*]"""
    return v.reshape((1, -1) + (1,) * (t.dim() - 2))


def stats(x, eps=BN_EPS, dtype=torch.float64):
    """(mean, biased variance, invstd) per channel."""
    xc = _per_channel(x.detach().to("cpu", dtype))
    mean = xc.sum(1) / xc.shape[1]
    var = ((xc - mean[:, None]) ** 2).sum(1) / xc.shape[1]
    return mean, var, 1.0 / torch.sqrt(var + eps)


def forward(x, gamma, beta, relu=True, eps=BN_EPS, mean=None, var=None, dtype=torch.float64):
    """(pre, y, mean, invstd): train mode (batch statistics) unless mean / var are given (eval mode: the running statistics)."""
    x, gamma, beta = (t.detach().to("cpu", dtype) for t in (x, gamma, beta))
    if mean is None:
        mean, var, invstd = stats(x, eps, dtype)
    else:
        mean, var = mean.detach().to("cpu", dtype), var.detach().to("cpu", dtype)
        invstd = 1.0 / torch.sqrt(var + eps)
    pre = (x - _bc(mean, x)) * _bc(invstd * gamma, x) + _bc(beta, x)
    y = torch.where(pre > 0, pre, torch.zeros_like(pre)) if relu else pre
    return pre, y, mean, invstd


def backward(x, gy, gamma, beta, relu=True, eps=BN_EPS, mean=None, var=None, dtype=torch.float64):
    """Closed form: g = gy * [pre > 0]; g_beta = sum g; g_gamma = sum g * xhat;
    train: g_x = gamma * invstd * (g - g_beta / N - xhat * g_gamma / N); eval: g_x = gamma * invstd * g."""
    train = mean is None
    pre, _, mean, invstd = forward(x, gamma, beta, relu, eps, mean, var, dtype)
    x, gy, gamma = (t.detach().to("cpu", dtype) for t in (x, gy, gamma))
    g = torch.where(pre > 0, gy, torch.zeros_like(gy)) if relu else gy
    xhat = (x - _bc(mean, x)) * _bc(invstd, x)
    n = x.numel() // x.shape[1]
    g_beta, g_gamma = _per_channel(g).sum(1), _per_channel(g * xhat).sum(1)
    if train:
        g_x = _bc(gamma * invstd, x) * (g - _bc(g_beta, x) / n - xhat * _bc(g_gamma, x) / n)
    else:
        g_x = _bc(gamma * invstd, x) * g
    return dict(g_x=g_x, g_gamma=g_gamma, g_beta=g_beta)


def all_f64(x, gy, gamma, beta, relu=True, eps=BN_EPS, mean=None, var=None):
    """Every tensor the tests compare, in float64."""
    _, y, m, invstd = forward(x, gamma, beta, relu, eps, mean, var)
    return dict(y=y, mean=m, invstd=invstd, **backward(x, gy, gamma, beta, relu, eps, mean, var))


def running_update(running_mean, running_var, x, momentum, eps=BN_EPS, dtype=torch.float64):
    """One train-mode step of the running statistics: momentum blend, UNBIASED variance n / (n - 1)."""
    mean, var, _ = stats(x, eps, dtype)
    n = x.numel() // x.shape[1]
    rm = (1 - momentum) * running_mean.to("cpu", dtype) + momentum * mean
    rv = (1 - momentum) * running_var.to("cpu", dtype) + momentum * var * (n / (n - 1))
    return rm, rv


def aten_fp32(x, gy, gamma, beta, relu=True, eps=BN_EPS, mean=None, var=None):
    """The fp32 run of stock ATen on the CPU (F.batch_norm + relu through autograd): the e_ref of the bare-operator tests."""
    import torch.nn.functional as F
    x, gamma, beta = (t.detach().cpu().float().clone().requires_grad_(True) for t in (x, gamma, beta))
    if mean is None:
        pre = F.batch_norm(x, None, None, gamma, beta, True, 0.1, eps)
        _, m, invstd = torch.native_batch_norm(x.detach(), gamma.detach(), beta.detach(), None, None, True, 0.1, eps)   # ATen's saved ones
    else:
        pre = F.batch_norm(x, mean.detach().cpu().float(), var.detach().cpu().float(), gamma, beta, False, 0.1, eps)
        m, invstd = mean.detach().cpu().float(), 1.0 / torch.sqrt(var.detach().cpu().float() + eps)
    y = torch.relu(pre) if relu else pre
    gx, gg, gb = torch.autograd.grad(y, [x, gamma, beta], gy.detach().cpu().float())
    return dict(y=y.detach(), mean=m, invstd=invstd, g_x=gx, g_gamma=gg, g_beta=gb)


def make_case(C, B, spatial, seed, offset=0.0):
    """fp32 inputs of one bare-operator case: x (``offset`` + N(0, 1)), gamma, beta, upstream gradient gy."""
    V = 1
    for n in spatial:
        V *= n
    g = torch.Generator().manual_seed(1000 * seed + 17 * C + 3 * B + V % 997)
    x = torch.randn((B, C) + tuple(spatial), generator=g) + offset
    gamma = 1.0 + 0.2 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    gy = torch.randn(x.shape, generator=g)
    return dict(x=x, gamma=gamma, beta=beta, gy=gy)


def kink_violations(case, eps=BN_EPS, mean=None, var=None):
    """Number of pre-ReLU values within KINK_MARGIN of the kink in float64 (must be 0 where a ReLU is compared: a flipped mask
    dominates every gradient)."""
    pre = forward(case["x"], case["gamma"], case["beta"], True, eps, mean, var)[0]
    return int((pre.abs() <= KINK_MARGIN).sum().item())


def first_clean_seed(C, B, spatial, offset=0.0, limit=20):
    """The first seed whose case has no kink violation."""
    for seed in range(limit):
        if kink_violations(make_case(C, B, spatial, seed, offset)) == 0:
            return seed
    raise AssertionError(f"no seed below {limit} without a kink violation for C {C}, B {B}, {spatial}")


# ---- the shapes of the GPU tests, derived from the kernels' constants (the CPU tests walk the partition over the same ones)
def bare_volumes(chunk):
    """name -> (B, 3D spatial); the 2D modules take (D * H, W).  V = 90 (V % 4 != 0, under one chunk; with B = 2 the sample boundary
    falls inside the only share), 540 (V % 4 == 0), 670, chunk + 4 (two chunks, the second almost empty) and 3 * chunk + 1 (scalar
    path, ragged last chunk, several shares)."""
    assert chunk % 4 == 0, chunk
    return {"2x5x9": (1, (2, 5, 9)), "2x5x9_b2": (2, (2, 5, 9)), "3x10x18": (1, (3, 10, 18)), "2x5x67": (1, (2, 5, 67)),
            "chunk+4": (1, (1, 4, (chunk + 4) // 4)), "3chunk+1": (1, (1, 1, 3 * chunk + 1))}


def grid_shape(C, chunk, max_wg):
    """(B, spatial) with S == Smax = max_wg / C shares of about 8 chunks each, B = 2, V % 4 == 0 and V no multiple of the chunk: the
    sample boundary falls inside a share.  About 16 M floats."""
    smax = max_wg // C
    V = smax * chunk * 8 // 2 + 148
    return 2, (2, 2, V // 4)


def spatial_2d(spatial):
    return (spatial[0] * spatial[1], spatial[2])


def volume(spatial):
    v = 1
    for n in spatial:
        v *= n
    return v
