"""Yardstick of the differentiable 5x5 stride-2 convolutions of FeatureNet (K3 forward, K3d data gradient, K3k weight gradient): a
float64 restatement that uses no convolution library -- a zero-padded copy, stride-2 slices and einsum -- and the block the reference
builds around such a layer (conv + train-mode BatchNorm + ReLU: networks/module.py Conv2d, :289 and :295), restated in float64 with
autograd over the restatement.  No product code here.

The layer is kernel 5, stride 2, padding 2, no bias.  Activations are [N,C,H,W]: N counts samples or, for the bare kernels (whose
tensors are [C,D,H,W]), the D independent planes.  The FINE tensor has Cb channels and extents Hf x Wf, even or odd; the COARSE one
Ca = 2 Cb channels and Hc x Wc = (Hf + 1) // 2 x (Wf + 1) // 2.  The weight is [Ca,Cb,5,5].  The functions run on whatever device
their inputs are on, in ``dtype`` (float64 by default; float32 gives the stock-ATen fp32 run of the same restatement, the ``e_ref`` of
the bare-kernel tests)."""
import torch
import torch.nn.functional as F

PAIRS = ((8, 16), (16, 32))   # (Cb, Ca): conv1.0 and conv2.0
# (D, Hf, Wf): the forward's own K3_K5S2_SHAPES plus the single pixel -- odd and even extents in both axes, Wc = 34 / 35 / 65 across
# the 32-column tile seam, Hc = 9 / 17 across the row-tile seam, D = 2 across a plane
SHAPES = ((1, 1, 1), (1, 2, 3), (1, 5, 8), (1, 17, 67), (2, 18, 70), (2, 33, 130))
KINK_MARGIN = 1e-5
BN_EPS = 1e-5
TAPS = [(ky, kx) for ky in range(5) for kx in range(5)]

# seeds: the first for which no BatchNorm output lies within KINK_MARGIN of 0 (tests/golden/make_golden_conv_k5s2_grad.py asserts it,
# the tests re-assert it)
GOLDEN_CASES = {
    "conv_8to16_10x13": dict(Cb=8, Hf=10, Wf=13, B=1, seed=0),
    "conv_16to32_b2_7x12": dict(Cb=16, Hf=7, Wf=12, B=2, seed=0),
    "conv_8to16_9x9": dict(Cb=8, Hf=9, Wf=9, B=1, seed=0),
}


def rel_dist(a, b):
    """max|a - b| / max|b| in float64."""
    a, b = a.detach().to("cpu", torch.float64), b.detach().to("cpu", torch.float64)
    return ((a - b).abs().max() / b.abs().max()).item()


def coarse_hw(Hf, Wf):
    return (Hf + 1) // 2, (Wf + 1) // 2


def _padded(x):
    """Zeros around the fine tensor so that index f + 2 holds fine pixel f and every window 2y + ky, y < Hc, ky < 5 exists."""
    Hf, Wf = x.shape[-2:]
    Hc, Wc = coarse_hw(Hf, Wf)
    return F.pad(x, (2, 2 * Wc + 1 - Wf, 2, 2 * Hc + 1 - Hf))


def _window(xp, ky, kx, Hc, Wc):
    """The padded fine tensor at 2y + ky - 2, 2x + kx - 2 for every coarse (y, x): a stride-2 slice."""
    return xp[..., ky:ky + 2 * Hc:2, kx:kx + 2 * Wc:2]


def conv_k5s2_ref(x, w, dtype=torch.float64):
    """Y[n,a,y,x] = sum_{b,ky,kx} w[a,b,ky,kx] * X[n,b,2y+ky-2,2x+kx-2]  (zero outside; differentiable)."""
    x, w = x.to(dtype), w.to(dtype)
    Hc, Wc = coarse_hw(*x.shape[-2:])
    xp = _padded(x)
    out = torch.zeros(x.shape[0], w.shape[0], Hc, Wc, dtype=dtype, device=x.device)
    for ky, kx in TAPS:
        out = out + torch.einsum("ab,nbhw->nahw", w[:, :, ky, kx], _window(xp, ky, kx, Hc, Wc))
    return out


def wgrad_k5s2_ref(gy, x, dtype=torch.float64):
    """dW[a,b,ky,kx] = sum_{n,y,x} gy[n,a,y,x] * X[n,b,2y+ky-2,2x+kx-2]: 25 stride-2 windows, one einsum each."""
    gy, x = gy.to(dtype), x.to(dtype)
    Hc, Wc = coarse_hw(*x.shape[-2:])
    assert tuple(gy.shape[-2:]) == (Hc, Wc) and gy.shape[0] == x.shape[0]
    xp = _padded(x)
    g = torch.zeros(gy.shape[1], x.shape[1], 5, 5, dtype=dtype, device=x.device)
    for ky, kx in TAPS:
        g[:, :, ky, kx] = torch.einsum("nahw,nbhw->ab", gy, _window(xp, ky, kx, Hc, Wc))
    return g


def _dilate(v, ky, kx, H, W):
    """v [N,C,Hc,Wc] placed at (ky, kx) + 2 * (y, x) of a zero [N,C,H,W] frame: interleaved with zeros and padded (no in-place writes)."""
    N, C, Hc, Wc = v.shape
    v = torch.stack((v, torch.zeros_like(v)), 3).reshape(N, C, 2 * Hc, Wc)
    v = torch.stack((v, torch.zeros_like(v)), 4).reshape(N, C, 2 * Hc, 2 * Wc)
    return F.pad(v, (kx, W - 2 * Wc - kx, ky, H - 2 * Hc - ky))


def dgrad_k5s2_ref(gy, w, fine_hw, dtype=torch.float64):
    """dX[n,b,2y+ky-2,2x+kx-2] += sum_a gy[n,a,y,x] * w[a,b,ky,kx], what falls outside the Hf x Wf tensor dropped (differentiable)."""
    gy, w = gy.to(dtype), w.to(dtype)
    Hf, Wf = fine_hw
    Hc, Wc = gy.shape[-2:]
    assert coarse_hw(Hf, Wf) == (Hc, Wc)
    H, W = 2 * Hc + 4, 2 * Wc + 4   # the padded fine frame: index f + 2 holds pixel f
    total = torch.zeros(gy.shape[0], w.shape[1], H, W, dtype=dtype, device=gy.device)
    for ky, kx in TAPS:
        total = total + _dilate(torch.einsum("ab,nahw->nbhw", w[:, :, ky, kx], gy), ky, kx, H, W)
    return total[..., 2:2 + Hf, 2:2 + Wf]


def conv3x3_ref(x, w, dtype=torch.float64):
    """The stride-1 3x3 pad-1 conv of the blocks that follow the layer in FeatureNet's conv1 / conv2 (for the chain test)."""
    x, w = x.to(dtype), w.to(dtype)
    H, W = x.shape[-2:]
    xp = F.pad(x, (1, 1, 1, 1))
    out = torch.zeros(x.shape[0], w.shape[0], H, W, dtype=dtype, device=x.device)
    for ky in range(3):
        for kx in range(3):
            out = out + torch.einsum("ab,nbhw->nahw", w[:, :, ky, kx], xp[..., ky:ky + H, kx:kx + W])
    return out


def planes(t):
    """A bare kernel's tensor [C,D,H,W] as the restatement's [N = D,C,H,W] (and back: the permutation is its own inverse)."""
    return t.permute(1, 0, 2, 3)


def make_case(Cb, Hf, Wf, B, seed):
    """fp32 inputs of one block: x, weight (He-sized), BatchNorm gamma / beta, upstream gradient gy."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * Cb + 5)
    Hc, Wc = coarse_hw(Hf, Wf)
    x = torch.randn(B, Cb, Hf, Wf, generator=g)
    # the weight sits on a 2^-9 grid (it compresses that way); still fp32 data like any other
    w = torch.round(torch.randn(2 * Cb, Cb, 5, 5, generator=g) * (2.0 / (Cb * 25)) ** 0.5 * 512.0) / 512.0
    gamma = 1.0 + 0.2 * torch.randn(2 * Cb, generator=g)
    beta = 0.2 * torch.randn(2 * Cb, generator=g)
    gy = torch.randn(B, 2 * Cb, Hc, Wc, generator=g)
    return dict(Cb=Cb, x=x, w=w, gamma=gamma, beta=beta, gy=gy)


def golden_case(g, name):
    """The stored case ``name`` of op_conv_k5s2_grad.npz as torch tensors (inputs and the reference's recorded fp32 results)."""
    case = dict(Cb=GOLDEN_CASES[name]["Cb"])
    for k in ("x", "w", "gamma", "beta", "gy", "out", "g_x", "g_w", "g_gamma", "g_beta"):
        case[k] = torch.from_numpy(g[f"{name}.{k}"])
    return case


def bn_train(y, gamma, beta):
    """Train-mode BatchNorm of [N,C,H,W] in y's dtype: batch statistics, biased variance, eps 1e-5."""
    mean = y.mean(dim=(0, 2, 3), keepdim=True)
    var = ((y - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
    sh = (1, -1, 1, 1)
    return (y - mean) / torch.sqrt(var + BN_EPS) * gamma.to(y.dtype).reshape(sh) + beta.to(y.dtype).reshape(sh)


def bn_pre_relu_f64(case):
    """The BatchNorm output (before the ReLU) of the block in float64."""
    return bn_train(conv_k5s2_ref(case["x"], case["w"]), case["gamma"], case["beta"])


def kink_violations(case, margin=KINK_MARGIN):
    """Number of BatchNorm outputs within ``margin`` of the ReLU kink (must be 0: a flipped kink dominates every gradient)."""
    return int((bn_pre_relu_f64(case).abs() <= margin).sum().item())


def block_f64(case):
    """layer + train-mode BatchNorm (biased variance, eps 1e-5) + ReLU in float64 and its gradients for the upstream gradient gy."""
    leaves = {k: case[k].double().clone().requires_grad_(True) for k in ("x", "w", "gamma", "beta")}
    out = torch.relu(bn_pre_relu_f64({**case, **leaves}))
    gx, gw, gg, gb = torch.autograd.grad(out, [leaves[k] for k in ("x", "w", "gamma", "beta")], case["gy"].double())
    return dict(out=out.detach(), g_x=gx, g_w=gw, g_gamma=gg, g_beta=gb)


# ------------------------------------------------------------------------------------------ the chain: FeatureNet's conv1, then conv2
CHAIN_BLOCKS = (("conv1.0", 8, 16, 5), ("conv1.1", 16, 16, 3), ("conv1.2", 16, 16, 3),
                ("conv2.0", 16, 32, 5), ("conv2.1", 32, 32, 3), ("conv2.2", 32, 32, 3))
CHAIN_KINK_MARGIN = 1e-4


def make_chain(B, Hf, Wf, seed):
    """fp32 input [B,8,Hf,Wf], per block (weight, gamma, beta), and the upstream gradient on the chain's output."""
    g = torch.Generator().manual_seed(7000 + seed)
    x = torch.randn(B, 8, Hf, Wf, generator=g)
    params = []
    for _, cin, cout, k in CHAIN_BLOCKS:
        params.append((torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5,
                       1.0 + 0.2 * torch.randn(cout, generator=g), 0.2 * torch.randn(cout, generator=g)))
    Hc, Wc = coarse_hw(*coarse_hw(Hf, Wf))
    gy = torch.randn(B, 32, Hc, Wc, generator=g)
    return dict(x=x, params=params, gy=gy)


def chain_f64(chain, dtype=torch.float64, device="cpu"):
    """The six blocks in ``dtype`` (float64: the yardstick; float32 on a GPU: the stock-ATen fp32 run of the same restatement): output,
    gradient on x, the parameter gradients in block order (w, gamma, beta), and the smallest |BatchNorm output| of the chain (the
    distance to the nearest ReLU kink)."""
    x = chain["x"].to(device, dtype).clone().requires_grad_(True)
    leaves = [tuple(p.to(device, dtype).clone().requires_grad_(True) for p in blk) for blk in chain["params"]]
    h, nearest = x, float("inf")
    for (_, _, _, k), (w, gamma, beta) in zip(CHAIN_BLOCKS, leaves):
        pre = bn_train(conv_k5s2_ref(h, w, dtype) if k == 5 else conv3x3_ref(h, w, dtype), gamma, beta)
        nearest = min(nearest, pre.detach().abs().min().item())
        h = torch.relu(pre)
    flat = [t for blk in leaves for t in blk]
    grads = torch.autograd.grad(h, [x] + flat, chain["gy"].to(device, dtype))
    return dict(out=h.detach(), g_x=grads[0], g_params=list(grads[1:]), nearest_kink=nearest)
