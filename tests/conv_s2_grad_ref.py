"""Yardstick of the differentiable stride-2 and transposed convolutions (K3 forward / data gradient, K3h weight gradient): a float64
restatement that uses no convolution library -- zero-padded copies, stride-2 slices and einsum -- and the block the reference builds
around such a layer (conv + train-mode BatchNorm + ReLU: networks/module.py Conv3d / Deconv3d / Conv2d / Deconv2d), restated in float64
with autograd over the restatement.  No product code here.

Every layer is kernel 3, stride 2, padding 1, no bias; the transposed ones have output_padding 1.  Layouts: activations [B,C,D,H,W] (a
2D layer is D = 1 and kd = 1: no z taps, D not strided); the FINE tensor has Cb channels and extents (2 Dc | Dc) x 2 Hc x 2 Wc, the
COARSE one Ca = 2 Cb channels and Dc x Hc x Wc.  Both weights are [Ca,Cb,kd,3,3]: nn.Conv3d's [out][in] and nn.ConvTranspose3d's
[in][out].  The functions run on whatever device their inputs are on, in ``dtype`` (float64 by default; float32 gives the stock-ATen
fp32 run of the same restatement, the ``e_ref`` of the bare-kernel tests)."""
import torch
import torch.nn.functional as F

SHAPES = ((16, 8, 3), (32, 16, 3), (64, 32, 3), (64, 32, 1))   # (Ca, Cb, kdepth): the four shapes of K3h
LAYERS = tuple((mode, ca, cb, kd) for mode in ("conv", "deconv") for ca, cb, kd in SHAPES)   # the eight layers
KINK_MARGIN = 1e-5
BN_EPS = 1e-5

# coarse extents; the fine volume is (2 Dc | Dc) x 2 Hc x 2 Wc.  Seeds: the first for which no BatchNorm output lies within KINK_MARGIN
# of 0 (tests/golden/make_golden_conv_s2_grad.py asserts it, the tests re-assert it).
GOLDEN_CASES = {
    "conv_8to16_2x5x6": dict(mode="conv", Cb=8, kd=3, Dc=2, Hc=5, Wc=6, B=1, seed=0),
    "conv_16to32_b2_1x3x4": dict(mode="conv", Cb=16, kd=3, Dc=1, Hc=3, Wc=4, B=2, seed=0),
    "deconv_32to16_2x3x5": dict(mode="deconv", Cb=16, kd=3, Dc=2, Hc=3, Wc=5, B=1, seed=0),
    "deconv_16to8_1x5x9": dict(mode="deconv", Cb=8, kd=3, Dc=1, Hc=5, Wc=9, B=1, seed=0),
    "conv2d_32to64_5x9": dict(mode="conv", Cb=32, kd=1, Dc=1, Hc=5, Wc=9, B=1, seed=0),
    "deconv2d_64to32_6x7": dict(mode="deconv", Cb=32, kd=1, Dc=1, Hc=6, Wc=7, B=1, seed=0),
}


def rel_dist(a, b):
    """max|a - b| / max|b| in float64."""
    a, b = a.detach().to("cpu", torch.float64), b.detach().to("cpu", torch.float64)
    return ((a - b).abs().max() / b.abs().max()).item()


def _taps(kd):
    return [(kz, ky, kx) for kz in range(kd) for ky in range(3) for kx in range(3)]


def _padded(fine, kd):
    """One zero voxel around the fine tensor (not in z for kd = 1): index f + 1 holds fine voxel f."""
    return F.pad(fine, (1, 1, 1, 1, 1 if kd == 3 else 0, 1 if kd == 3 else 0))


def _window(t, kd, kz, ky, kx, Dc, Hc, Wc):
    """The padded fine tensor at 2z + kz - 1, 2y + ky - 1, 2x + kx - 1 for every coarse (z, y, x): a stride-2 slice."""
    zs = slice(kz, kz + 2 * Dc, 2) if kd == 3 else slice(None)
    return t[:, :, zs, ky:ky + 2 * Hc:2, kx:kx + 2 * Wc:2]


def coarse_extents(fine_shape, kd):
    D, H, W = fine_shape[-3:]
    assert H % 2 == 0 and W % 2 == 0 and (kd == 1 or D % 2 == 0), "even fine extents only"
    return (D // 2 if kd == 3 else D), H // 2, W // 2


def gather_ref(fine, w, kd, dtype=torch.float64):
    """coarse[b,a,z,y,x] = sum_{c,taps} w[a,c,kz,ky,kx] * fine[b,c,2z+kz-1,2y+ky-1,2x+kx-1]  (zero outside; differentiable).
    The stride-2 conv's forward (w = W) and the transposed conv's data gradient (w = Wt, fine = the gradient on its output)."""
    fine, w = fine.to(dtype), w.to(dtype)
    Dc, Hc, Wc = coarse_extents(fine.shape, kd)
    fp = _padded(fine, kd)
    out = torch.zeros(fine.shape[0], w.shape[0], Dc, Hc, Wc, dtype=dtype, device=fine.device)
    for kz, ky, kx in _taps(kd):
        out = out + torch.einsum("ac,bcdhw->badhw", w[:, :, kz, ky, kx], _window(fp, kd, kz, ky, kx, Dc, Hc, Wc))
    return out


def scatter_ref(coarse, w, kd, dtype=torch.float64):
    """fine[b,c,2z+kz-1,2y+ky-1,2x+kx-1] += sum_a w[a,c,kz,ky,kx] * coarse[b,a,z,y,x], what falls outside dropped (differentiable).
    The transposed conv's forward (w = Wt; output_padding 1: fine extent = 2 x coarse) and the stride-2 conv's data gradient (w = W,
    coarse = the gradient on its output)."""
    coarse, w = coarse.to(dtype), w.to(dtype)
    B, _, Dc, Hc, Wc = coarse.shape
    Df = 2 * Dc if kd == 3 else Dc
    shape = (B, w.shape[1], Df + (2 if kd == 3 else 0), 2 * Hc + 2, 2 * Wc + 2)   # the padded fine frame: index f + 1 holds voxel f
    total = torch.zeros(shape, dtype=dtype, device=coarse.device)
    for kz, ky, kx in _taps(kd):
        total = total + _dilate(torch.einsum("ac,badhw->bcdhw", w[:, :, kz, ky, kx], coarse), kd, kz, ky, kx, shape)
    zs = slice(1, Df + 1) if kd == 3 else slice(None)
    return total[:, :, zs, 1:2 * Hc + 1, 1:2 * Wc + 1]


def _dilate(v, kd, kz, ky, kx, shape):
    """v [B,C,Dc,Hc,Wc] placed at the stride-2 positions (kz | :, ky, kx) + 2 * (z, y, x) of a zero tensor of ``shape``: interleaved
    with zeros and padded (no in-place writes: plain autograd)."""
    B, C, Dc, Hc, Wc = v.shape
    if kd == 3:
        v = torch.stack((v, torch.zeros_like(v)), 3).reshape(B, C, 2 * Dc, Hc, Wc)
    D2 = v.shape[2]
    v = torch.stack((v, torch.zeros_like(v)), 4).reshape(B, C, D2, 2 * Hc, Wc)
    v = torch.stack((v, torch.zeros_like(v)), 5).reshape(B, C, D2, 2 * Hc, 2 * Wc)
    zlo = kz if kd == 3 else 0
    return F.pad(v, (kx, shape[4] - 2 * Wc - kx, ky, shape[3] - 2 * Hc - ky, zlo, shape[2] - D2 - zlo))


def conv_s2_ref(x, w, kd, dtype=torch.float64):
    """nn.Conv3d(Cb, Ca, 3, stride=2, padding=1) / nn.Conv2d: x fine -> coarse."""
    return gather_ref(x, w, kd, dtype)


def deconv_s2_ref(x, wt, kd, dtype=torch.float64):
    """nn.ConvTranspose3d(Ca, Cb, 3, stride=2, padding=1, output_padding=1) / nn.ConvTranspose2d: x coarse -> fine."""
    return scatter_ref(x, wt, kd, dtype)


def dgrad_conv_s2_ref(gy, w, kd, dtype=torch.float64):
    """Data gradient of the stride-2 conv: the transposed conv of the gradient with the SAME weight tensor."""
    return scatter_ref(gy, w, kd, dtype)


def dgrad_deconv_s2_ref(gy, wt, kd, dtype=torch.float64):
    """Data gradient of the transposed conv: the stride-2 conv of the gradient with the SAME weight tensor."""
    return gather_ref(gy, wt, kd, dtype)


def wgrad_s2_ref(coarse, fine, kd, dtype=torch.float64):
    """G[a,c,kz,ky,kx] = sum_{b,z,y,x} coarse[b,a,z,y,x] * fine[b,c,2z+kz-1,2y+ky-1,2x+kx-1]: 27 (9) stride-2 windows, one einsum each.
    Stride-2 conv: (coarse, fine) = (dY, X), G = dW.  Transposed conv: (X, dY), G = dWt."""
    coarse, fine = coarse.to(dtype), fine.to(dtype)
    B, Ca, Dc, Hc, Wc = coarse.shape
    assert coarse_extents(fine.shape, kd) == (Dc, Hc, Wc) and fine.shape[0] == B
    fp = _padded(fine, kd)
    a2 = coarse.permute(1, 0, 2, 3, 4).reshape(Ca, -1)
    g = torch.zeros(Ca, fine.shape[1], kd, 3, 3, dtype=dtype, device=coarse.device)
    for kz, ky, kx in _taps(kd):
        win = _window(fp, kd, kz, ky, kx, Dc, Hc, Wc).permute(1, 0, 2, 3, 4).reshape(fine.shape[1], -1)
        g[:, :, kz, ky, kx] = torch.einsum("av,cv->ac", a2, win)
    return g


def layer_ref(mode, x, w, kd, dtype=torch.float64):
    return conv_s2_ref(x, w, kd, dtype) if mode == "conv" else deconv_s2_ref(x, w, kd, dtype)


def in_out_shapes(mode, Cb, kd, Dc, Hc, Wc, B):
    fine = (B, Cb, 2 * Dc if kd == 3 else Dc, 2 * Hc, 2 * Wc)
    coarse = (B, 2 * Cb, Dc, Hc, Wc)
    return (fine, coarse) if mode == "conv" else (coarse, fine)


def make_case(mode, Cb, kd, Dc, Hc, Wc, B, seed):
    """fp32 inputs of one block: x, weight (He-sized), BatchNorm gamma / beta, upstream gradient gy."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * Cb + kd + (500 if mode == "deconv" else 0))
    xs, ys = in_out_shapes(mode, Cb, kd, Dc, Hc, Wc, B)
    x = torch.randn(xs, generator=g)
    # the weight sits on a 2^-9 grid (it compresses that way); still fp32 data like any other
    w = torch.round(torch.randn(2 * Cb, Cb, kd, 3, 3, generator=g) * (2.0 / (xs[1] * 9 * kd)) ** 0.5 * 512.0) / 512.0
    gamma = 1.0 + 0.2 * torch.randn(ys[1], generator=g)
    beta = 0.2 * torch.randn(ys[1], generator=g)
    gy = torch.randn(ys, generator=g)
    return dict(mode=mode, Cb=Cb, kd=kd, x=x, w=w, gamma=gamma, beta=beta, gy=gy)


def golden_case(g, name):
    """The stored case ``name`` of op_conv_s2_grad.npz as torch tensors (inputs and the reference's recorded fp32 results)."""
    kw = GOLDEN_CASES[name]
    case = dict(mode=kw["mode"], Cb=kw["Cb"], kd=kw["kd"])
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
    return bn_train(layer_ref(case["mode"], case["x"], case["w"], case["kd"]), case["gamma"], case["beta"])


def kink_violations(case):
    """Number of BatchNorm outputs within KINK_MARGIN of the ReLU kink (must be 0: a flipped kink dominates every gradient)."""
    return int((bn_pre_relu_f64(case).abs() <= KINK_MARGIN).sum().item())


def block_f64(case):
    """layer + train-mode BatchNorm (biased variance, eps 1e-5) + ReLU in float64 and its gradients for the upstream gradient gy."""
    leaves = {k: case[k].double().clone().requires_grad_(True) for k in ("x", "w", "gamma", "beta")}
    out = torch.relu(bn_pre_relu_f64({**case, **leaves}))
    gx, gw, gg, gb = torch.autograd.grad(out, [leaves[k] for k in ("x", "w", "gamma", "beta")], case["gy"].double())
    return dict(out=out.detach(), g_x=gx, g_w=gw, g_gamma=gg, g_beta=gb)
