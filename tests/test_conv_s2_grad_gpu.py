"""K3h (weight gradient of the stride-2 and transposed convolutions), their data gradients on K3 and the stride-2 forms of
``DiffConv3d`` / ``DiffConv2d`` and ``DiffConvTranspose3d`` / ``DiffConvTranspose2d`` on the MI355X.

Yardsticks, none of which is the code under test: the float64 restatement (tests/conv_s2_grad_ref.py; checked against float64
autograd of F.conv3d / F.conv_transpose3d in tests/test_conv_s2_grad_cpu.py), the reference's recorded fp32 block gradients
(tests/golden/op_conv_s2_grad.npz) and, for the bare kernels, the fp32 run of the same restatement on stock ATen.  No test reads the
reference or the oracle.

  criterion  per tensor: e_ref = max-abs distance of the fp32 yardstick to the float64 restatement over the tensor's max-abs, e_hip
             the same for the kernels; e_hip <= 8 e_ref (K3g's criterion: the factor covers another association of the voxel sums).
             Where e_ref < 4 * 2^-23 the bound is 16 * 2^-23.
  exact      the single-voxel probe, the data gradients against the host-packed K3 launch of the other mode, the forward identity,
             reproducibility, accumulate, cache invalidation: torch.equal.

Every test prints its figures before it asserts (PARITY / BARE / GRID / PROBE / DGRAD / FWD / CHAIN lines);
docs/kernels/K3h_conv_wgrad_s2.md keeps the measured ones.  No test provokes a fault."""
import gc

import pytest
import torch
from torch import nn
import torch.nn.functional as F

import conv_s2_grad_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 8.0
EPS32 = 2.0 ** -23

# coarse volumes: the smallest at which the kernel can go wrong (tile: 1 x 4 (2) x 32 coarse voxels).  kdepth 1 runs them at Dc = 1.
VOLUMES = {
    "1x3x4": (1, 3, 4),       # smaller than any tile; fine depth 2 -> 1: K3's depth-tap-skipping stride-2 / deconv forms in the data gradients
    "2x5x9": (2, 5, 9),       # W % 4 != 0, ragged
    "3x10x18": (3, 10, 18),   # W % 4 == 0
    "2x5x67": (2, 5, 67),     # ragged against 32- and 64-wide tiles
}


@pytest.fixture(autouse=True)
def free_gpu_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def g(golden):
    return golden("op_conv_s2_grad.npz")


def bound_of(e_ref):
    return FACTOR * e_ref if e_ref >= 4 * EPS32 else 16 * EPS32


def vol_of(vol, kd):
    D, H, W = VOLUMES[vol] if isinstance(vol, str) else vol
    return (D if kd == 3 else 1), H, W


def rand_pair(Ca, Cb, kd, Dc, Hc, Wc, B=1, seed=0):
    """coarse [B,Ca,Dc,Hc,Wc], fine [B,Cb,(2Dc|Dc),2Hc,2Wc], weight [Ca,Cb,kd,3,3] (He-sized) on the GPU."""
    gen = torch.Generator().manual_seed(7919 * seed + 31 * Ca + kd + Dc * Hc * Wc)
    fs, cs = R.in_out_shapes("conv", Cb, kd, Dc, Hc, Wc, B)
    coarse, fine = torch.randn(cs, generator=gen).cuda(), torch.randn(fs, generator=gen).cuda()
    w = (torch.randn(Ca, Cb, kd, 3, 3, generator=gen) * (2.0 / (Ca * 9 * kd)) ** 0.5).cuda()
    return coarse, fine, w


def hip_wgrad(coarse, fine, kd, **kw):
    """K3h over a batch, its samples one after the other (accumulate from the second on)."""
    from dmvsnet_amd import ops
    gw = None
    for b in range(coarse.shape[0]):
        gw = ops.conv3d_wgrad_s2(coarse[b], fine[b], kd, out=gw, accumulate=b > 0, **kw)
    return gw


def host_layer(w, kd, k3mode):
    """The bare K3 layer that reads the weight tensor [Ca,Cb,...] in ``k3mode``, packed by the HOST packer (the eval path's packing)."""
    from dmvsnet_amd import ops
    Ca, Cb = w.shape[:2]
    cin, cout = (Cb, Ca) if k3mode == ops.CONV_S2 else (Ca, Cb)
    return ops.ConvLayer("host", k3mode, kd, cin, cout, None, ops.pack_mfma(w.detach().cpu(), cin, cout, k3mode, kd).cuda(), None, None, False)


def make_module(mode, Ca, Cb, kd, w):
    from dmvsnet_amd import DiffConv2d, DiffConv3d, DiffConvTranspose2d, DiffConvTranspose3d
    if mode == "conv":
        m = (DiffConv3d if kd == 3 else DiffConv2d)(Cb, Ca, 3, stride=2, padding=1, bias=False)
    else:
        m = (DiffConvTranspose3d if kd == 3 else DiffConvTranspose2d)(Ca, Cb, 3, stride=2, padding=1, output_padding=1, bias=False)
    m = m.cuda()
    with torch.no_grad():
        m.weight.copy_(w.reshape(m.weight.shape))
    return m


def shaped(t, kd):
    """[B,C,D,H,W] -> what the module of this kdepth takes ([B,C,H,W] for the 2D layers; D must be 1)."""
    return t if kd == 3 else t.squeeze(2)


def layer_io(mode, coarse, fine):
    """(input, gradient on the output) of the layer for a (coarse, fine) pair."""
    return (fine, coarse) if mode == "conv" else (coarse, fine)


# ------------------------------------------------------------------------------------------------ parity on the golden blocks
@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_block_parity_golden_cases(g, name):
    """The reference's block restated: Diff layer + F.batch_norm(training=True) + ReLU, against the reference's recorded fp32 run."""
    case = R.golden_case(g, name)
    assert R.kink_violations(case) == 0
    f64 = R.block_f64(case)
    Cb, kd, mode = case["Cb"], case["kd"], case["mode"]
    m = make_module(mode, 2 * Cb, Cb, kd, case["w"].cuda())
    x = shaped(case["x"].cuda(), kd).contiguous().requires_grad_(True)
    gamma, beta = case["gamma"].cuda().requires_grad_(True), case["beta"].cuda().requires_grad_(True)
    out = F.relu(F.batch_norm(m(x), None, None, gamma, beta, True, 0.1, R.BN_EPS))
    out.backward(shaped(case["gy"].cuda(), kd))
    got = dict(out=out.detach(), g_x=x.grad, g_w=m.weight.grad, g_gamma=gamma.grad, g_beta=beta.grad)
    rows = []
    for k in ("out", "g_x", "g_w", "g_gamma", "g_beta"):
        e_ref, e_hip = R.rel_dist(case[k], f64[k]), R.rel_dist(got[k].reshape(f64[k].shape), f64[k])
        rows.append((k, e_hip, e_ref))
        print(f"PARITY {name} {k}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {bound_of(e_ref):.3e}  (max {f64[k].abs().max().item():.3e})")
    for k, e_hip, e_ref in rows:
        assert e_hip <= bound_of(e_ref), (name, k, e_hip, e_ref)


# ------------------------------------------------------------------------------------------------ bare kernel against float64
def check_wgrad(tag, coarse, fine, kd, gw):
    f64 = R.wgrad_s2_ref(coarse, fine, kd)
    e_ref, e_hip = R.rel_dist(R.wgrad_s2_ref(coarse, fine, kd, torch.float32), f64), R.rel_dist(gw, f64)
    print(f"{tag}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {bound_of(e_ref):.3e}  (|G| max {f64.abs().max().item():.3e})")
    assert gw.dtype == torch.float32 and tuple(gw.shape) == tuple(f64.shape)
    assert e_hip <= bound_of(e_ref), (tag, e_hip, e_ref)


@pytest.mark.parametrize("vol", list(VOLUMES))
@pytest.mark.parametrize("Ca,Cb,kd", R.SHAPES)
def test_bare_wgrad_against_float64(Ca, Cb, kd, vol):
    coarse, fine, _ = rand_pair(Ca, Cb, kd, *vol_of(vol, kd))
    check_wgrad(f"BARE {Ca}/{Cb} kd {kd} {vol}", coarse, fine, kd, hip_wgrad(coarse, fine, kd))


@pytest.mark.parametrize("Ca,Cb,kd", R.SHAPES)
def test_bare_wgrad_accumulates_over_a_batch(Ca, Cb, kd):
    from dmvsnet_amd import ops
    coarse, fine, _ = rand_pair(Ca, Cb, kd, *vol_of((2, 3, 33), kd), B=2, seed=1)
    gw = hip_wgrad(coarse, fine, kd)
    check_wgrad(f"BARE {Ca}/{Cb} kd {kd} B 2", coarse, fine, kd, gw)
    # accumulate adds to a known buffer exactly once
    known = torch.randn(Ca, Cb, kd, 3, 3, generator=torch.Generator().manual_seed(5)).cuda()
    one = ops.conv3d_wgrad_s2(coarse[0], fine[0], kd)
    assert torch.equal(ops.conv3d_wgrad_s2(coarse[0], fine[0], kd, out=known.clone(), accumulate=True), known + one)


# ------------------------------------------------------------------------------------------------ grid-size cases
def plan_of(Ca, Dc, Hc, Wc, kd):
    from dmvsnet_amd import _lib
    plan = _lib.load().dmvs_conv3d_wgrad_s2_plan(Ca, Dc, Hc, Wc, kd)
    assert plan > 0
    return plan >> 9, plan & 511


def test_more_tiles_than_shares():
    for vol in ((2, 48, 176), (4, 48, 176), (4, 64, 176)):
        tiles, wgs = plan_of(16, *vol, 3)
        if tiles > 256:
            break
    else:
        pytest.fail("no volume of the list has more tiles than shares")
    coarse, fine, _ = rand_pair(16, 8, 3, *vol)
    print(f"GRID 16/8 kd 3 {vol}: {tiles} tiles, {wgs} workgroups")
    check_wgrad(f"GRID 16/8 kd 3 {vol} tiles > shares", coarse, fine, 3, hip_wgrad(coarse, fine, 3))


@pytest.mark.parametrize("Ca,Cb,kd", R.SHAPES)
def test_fewer_tiles_than_shares(Ca, Cb, kd):
    """The workgroups past the last share exit at once and own no partial: a NaN-filled workspace must not reach the result."""
    from dmvsnet_amd import _lib
    vol = vol_of((2, 6, 40), kd)
    tiles, wgs = plan_of(Ca, *vol, kd)
    shares = min(tiles, 128 if Ca == 64 else 256)
    assert tiles < (128 if Ca == 64 else 256), tiles
    coarse, fine, _ = rand_pair(Ca, Cb, kd, *vol)
    ws = torch.full((_lib.load().dmvs_conv3d_wgrad_s2_workspace(Ca, *vol, kd),), float("nan"), device="cuda")
    print(f"GRID {Ca}/{Cb} kd {kd} {vol}: {tiles} tiles, {wgs} workgroups")
    check_wgrad(f"GRID {Ca}/{Cb} kd {kd} {vol} tiles < shares", coarse, fine, kd, hip_wgrad(coarse, fine, kd, workspace=ws))
    assert torch.isfinite(ws[:shares * 9 * kd * Ca * Cb]).all(), "a share's partial was not fully written"


# ------------------------------------------------------------------------------------------------ single-voxel probe (exact)
@pytest.mark.parametrize("Ca,Cb,kd", R.SHAPES)
def test_single_voxel_probe(Ca, Cb, kd):
    """A[a] = one 1.0 at a probe voxel (interior, corner, last, tile edges; which one depends on a): G[a][b][tap] is then exactly one
    element of B, or 0 where the tap falls outside B.  Names tap order, x-parity, halo and a / b mistakes without a tolerance."""
    Dc, Hc, Wc = vol_of((2, 6, 37), kd)
    probes = [(Dc // 2, 2, 5), (0, 0, 0), (Dc - 1, Hc - 1, Wc - 1), (0, 3, 31), (Dc - 1, 4, 32), (0, 1, Wc - 1), (Dc - 1, 0, 33), (0, Hc - 1, 0),
              (0, 3, 32), (Dc - 1, 4, 31), (0, 5, 36)]
    Df, Hf, Wf = (2 * Dc if kd == 3 else Dc), 2 * Hc, 2 * Wc
    fine = torch.randn(1, Cb, Df, Hf, Wf, generator=torch.Generator().manual_seed(Ca + kd)).cuda()
    coarse = torch.zeros(1, Ca, Dc, Hc, Wc, device="cuda")
    want = torch.zeros(Ca, Cb, kd, 3, 3, device="cuda")
    for a in range(Ca):
        z, y, x = probes[a % len(probes)]
        coarse[0, a, z, y, x] = 1.0
        for kz in range(kd):
            for ky in range(3):
                for kx in range(3):
                    fz, fy, fx = (2 * z + kz - 1 if kd == 3 else z), 2 * y + ky - 1, 2 * x + kx - 1
                    if 0 <= fz < Df and 0 <= fy < Hf and 0 <= fx < Wf:
                        want[a, :, kz, ky, kx] = fine[0, :, fz, fy, fx]
    got = hip_wgrad(coarse, fine, kd)
    bad = (got != want).nonzero()
    print(f"PROBE {Ca}/{Cb} kd {kd}: {bad.shape[0]} of {want.numel()} elements differ" + (f", first (a, b, kz, ky, kx) = {bad[0].tolist()}" if len(bad) else ""))
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ data gradient and forward
@pytest.mark.parametrize("vol", ["1x3x4", "2x5x9"])
@pytest.mark.parametrize("mode,Ca,Cb,kd", R.LAYERS)
def test_data_gradient_and_forward(mode, Ca, Cb, kd, vol):
    """Forward bit-identical to ops.conv3d on the host-packed bare layer; data gradient bit-identical to the host-packed K3 launch of
    the OTHER mode on the same weight tensor; both within the bound against float64."""
    from dmvsnet_amd import ops
    B = 2
    coarse, fine, w = rand_pair(Ca, Cb, kd, *vol_of(vol, kd), B=B, seed=2)
    x, gy = layer_io(mode, coarse, fine)
    fwd, bwd = (ops.CONV_S2, ops.DECONV_S2) if mode == "conv" else (ops.DECONV_S2, ops.CONV_S2)
    m = make_module(mode, Ca, Cb, kd, w)
    m.weight.requires_grad_(False)
    xin = shaped(x, kd).clone().requires_grad_(True)
    y = m(xin)
    y.backward(shaped(gy, kd).contiguous())
    y, gx = y.detach().reshape(gy.shape), xin.grad.reshape(x.shape)
    lf, lb = host_layer(w, kd, fwd), host_layer(w, kd, bwd)
    assert torch.equal(y, torch.stack([ops.conv3d(x[b], lf, backend="mfma") for b in range(B)])), "the forward is not the host-packed K3 launch"
    assert torch.equal(gx, torch.stack([ops.conv3d(gy[b], lb, backend="mfma") for b in range(B)])), \
        "the data gradient is not the K3 launch of the other mode on the host-packed weight"
    if mode == "conv":
        y64, y32 = R.conv_s2_ref(x, w, kd), R.conv_s2_ref(x, w, kd, torch.float32)
        g64, g32 = R.dgrad_conv_s2_ref(gy, w, kd), R.dgrad_conv_s2_ref(gy, w, kd, torch.float32)
    else:
        y64, y32 = R.deconv_s2_ref(x, w, kd), R.deconv_s2_ref(x, w, kd, torch.float32)
        g64, g32 = R.dgrad_deconv_s2_ref(gy, w, kd), R.dgrad_deconv_s2_ref(gy, w, kd, torch.float32)
    rows = (("FWD", R.rel_dist(y, y64), R.rel_dist(y32, y64)), ("DGRAD", R.rel_dist(gx, g64), R.rel_dist(g32, g64)))
    for tag, e_hip, e_ref in rows:
        print(f"{tag} {mode} {Ca}/{Cb} kd {kd} {vol}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {bound_of(e_ref):.3e}")
    for tag, e_hip, e_ref in rows:
        assert e_hip <= bound_of(e_ref), (tag, e_hip, e_ref)


# ------------------------------------------------------------------------------------------------ reproducibility and poison
@pytest.mark.parametrize("mode,Ca,Cb,kd", (("conv", 16, 8, 3), ("deconv", 64, 32, 3), ("deconv", 32, 16, 3), ("conv", 64, 32, 1)))
def test_reproducible_with_a_poisoned_workspace(mode, Ca, Cb, kd):
    from dmvsnet_amd import ops
    vol = vol_of("2x5x67", kd)
    coarse, fine, w = rand_pair(Ca, Cb, kd, *vol, B=2, seed=4)
    x, gy = layer_io(mode, coarse, fine)
    runs = []
    for _ in range(2):
        ops.conv3d_wgrad_s2_workspace(Ca, *vol, kd, "cuda").fill_(float("nan"))   # the cached workspace the backward will use
        m = make_module(mode, Ca, Cb, kd, w)
        xin = shaped(x, kd).clone().requires_grad_(True)   # a fresh leaf per run: its .grad must not accumulate
        m(xin).backward(shaped(gy, kd).contiguous())
        runs.append((xin.grad.clone(), m.weight.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.isfinite(runs[0][0]).all() and torch.isfinite(runs[0][1]).all()
    # a NaN-filled gw is fully overwritten, and the module's gradient is the bare kernel's over the batch
    gw = ops.conv3d_wgrad_s2(coarse[0], fine[0], kd, out=torch.full((Ca, Cb, kd, 3, 3), float("nan"), device="cuda"))
    assert torch.isfinite(gw).all() and torch.equal(gw, ops.conv3d_wgrad_s2(coarse[0], fine[0], kd))
    assert torch.equal(runs[0][1].reshape(Ca, Cb, kd, 3, 3), hip_wgrad(coarse, fine, kd))
    # the launch log carries the family once per dispatch
    ops.launch_log = log = []
    try:
        ops.conv3d_wgrad_s2(coarse[0], fine[0], kd)
    finally:
        ops.launch_log = None
    assert log == ["conv3d_wgrad_s2", "conv3d_wgrad_s2"]


# ------------------------------------------------------------------------------------------------ cache invalidation
@pytest.mark.parametrize("mode,Ca,Cb,kd", (("conv", 16, 8, 3), ("deconv", 64, 32, 1)))
def test_cache_invalidation_by_an_optimizer_step(mode, Ca, Cb, kd):
    from dmvsnet_amd import ops
    coarse, fine, w = rand_pair(Ca, Cb, kd, *vol_of((2, 3, 5), kd), B=1, seed=6)
    x, gy = layer_io(mode, coarse, fine)
    xs, gys = shaped(x, kd).contiguous(), shaped(gy, kd).contiguous()
    m = make_module(mode, Ca, Cb, kd, w)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)

    def run(mod):
        xin = xs.clone().requires_grad_(True)
        y = mod(xin)
        y.backward(gys)
        return y.detach(), xin.grad

    y0, gx0 = run(m)
    opt.step()
    y1, gx1 = run(m)
    y2, gx2 = run(make_module(mode, Ca, Cb, kd, m.weight.detach().clone()))
    assert not torch.equal(y0, y1), "the step did not change the output: stale packed weight"
    assert torch.equal(y1, y2) and torch.equal(gx1, gx2) and not torch.equal(gx0, gx1)
    # unchanged weight: the packed forms are re-used
    fwd = ops.CONV_S2 if mode == "conv" else ops.DECONV_S2
    packed = m._packed[fwd][1].w_mfma
    m(xs)
    assert m._packed[fwd][1].w_mfma is packed


# ------------------------------------------------------------------------------------------------ plumbing
@pytest.mark.parametrize("mode", ("conv", "deconv"))
def test_frozen_inputs_skip_their_kernel_and_double_backward_raises(mode):
    from dmvsnet_amd import conv
    from dmvsnet_amd._lib import DmvsError
    coarse, fine, w = rand_pair(16, 8, 3, 1, 3, 5, B=2, seed=7)
    x, gy = layer_io(mode, coarse, fine)
    m = make_module(mode, 16, 8, 3, w)
    before = dict(conv.launch_counts)
    m(x.clone().requires_grad_(True)).backward(gy)
    assert conv.launch_counts == {"dgrad": before["dgrad"] + 2, "wgrad": before["wgrad"] + 2}
    m.weight.requires_grad_(False)
    before = dict(conv.launch_counts)
    m(x.clone().requires_grad_(True)).backward(gy)
    assert conv.launch_counts == {"dgrad": before["dgrad"] + 2, "wgrad": before["wgrad"]}
    m.weight.requires_grad_(True)
    before = dict(conv.launch_counts)
    m(x).backward(gy)
    assert conv.launch_counts == {"dgrad": before["dgrad"], "wgrad": before["wgrad"] + 2}
    xin = x.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(m(xin), xin, gy, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()
    with pytest.raises(DmvsError):
        m(x.transpose(3, 4))   # non-contiguous
    if mode == "conv":
        with pytest.raises(DmvsError, match="even"):
            m(torch.zeros(1, 8, 2, 5, 6, device="cuda"))


# ------------------------------------------------------------------------------------------------ the whole U-Net
class Block(nn.Module):
    """The reference's Conv3d / Deconv3d block: layer + BatchNorm3d + ReLU."""

    def __init__(self, conv):
        super().__init__()
        self.conv, self.bn = conv, nn.BatchNorm3d(conv.out_channels)

    def forward(self, x):
        return F.relu(self.bn(self.conv(x)))


class CostRegNetPart(nn.Module):
    """CostRegNet_part of the reference (networks/module.py), base 8 channels: conv1 .. conv11 on the Diff classes (``diff``) or on
    ATen, conv0 / prob / BatchNorm on ATen either way."""

    def __init__(self, diff, in_channels=8, base=8):
        super().__init__()
        import dmvsnet_amd as da
        c3 = da.DiffConv3d if diff else nn.Conv3d
        t3 = da.DiffConvTranspose3d if diff else nn.ConvTranspose3d
        s1 = lambda c: Block(c3(c, c, 3, stride=1, padding=1, bias=False))
        dn = lambda c: Block(c3(c, 2 * c, 3, stride=2, padding=1, bias=False))
        up = lambda c: Block(t3(2 * c, c, 3, stride=2, padding=1, output_padding=1, bias=False))
        self.conv0 = Block(nn.Conv3d(in_channels, base, 3, padding=1, bias=False))
        self.conv1, self.conv2 = dn(base), s1(2 * base)
        self.conv3, self.conv4 = dn(2 * base), s1(4 * base)
        self.conv5, self.conv6 = dn(4 * base), s1(8 * base)
        self.conv7, self.conv9, self.conv11 = up(4 * base), up(2 * base), up(base)
        self.prob = nn.Conv3d(base, 2, 3, stride=1, padding=1, bias=False)
        self.pre = []   # BatchNorm outputs of the last forward (the kink condition)
        for m in self.modules():
            if isinstance(m, nn.BatchNorm3d):
                m.register_forward_hook(lambda mod, inp, out: self.pre.append(out.detach()))

    def forward(self, x):
        self.pre.clear()
        conv0 = self.conv0(x)
        conv2 = self.conv2(self.conv1(conv0))
        conv4 = self.conv4(self.conv3(conv2))
        x = self.conv6(self.conv5(conv4))
        x = conv4 + self.conv7(x)
        x = conv2 + self.conv9(x)
        x = conv0 + self.conv11(x)
        return self.prob(x)


CHAIN_SEED = 0


def chain_inputs(seed):
    gen = torch.Generator().manual_seed(100 + seed)
    x = torch.randn(1, 8, 8, 16, 32, generator=gen)
    gy = torch.randn(1, 2, 8, 16, 32, generator=gen)
    weights = {}
    for k, v in CostRegNetPart(False).state_dict().items():
        if v.dim() == 5:                                  # conv weights, He-sized on the layer's input channels
            fan = (v.shape[0] if "conv7" in k or "conv9" in k or "conv11" in k else v.shape[1]) * 27
            v = torch.randn(v.shape, generator=gen) * (2.0 / fan) ** 0.5
        elif k.endswith("bn.weight"):
            v = 1.0 + 0.2 * torch.randn(v.shape, generator=gen)
        elif k.endswith("bn.bias"):
            v = 0.2 * torch.randn(v.shape, generator=gen)
        weights[k] = v
    return x, gy, weights


def run_chain(diff, dtype, device, x, gy, weights):
    net = CostRegNetPart(diff)
    net.load_state_dict(weights)
    net = net.to(device=device, dtype=dtype).train()
    xin = x.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)   # a fresh leaf per run
    out = net(xin)
    pre = list(net.pre)
    out.backward(gy.to(device=device, dtype=dtype))
    grads = {"x": xin.grad, **{n: p.grad for n, p in net.named_parameters()}}
    return out.detach(), grads, pre


def test_costregnet_part_chain():
    """The whole CostRegNet_part at fine 8 x 16 x 32, base 8 channels, through .backward(): conv1 .. conv11 on the Diff classes with the
    skip additions, conv0 / prob / BatchNorm on ATen; against the all-ATen chain in fp32 (CPU) and float64 (CPU), same criterion, on
    inputs that meet the kink condition."""
    x, gy, weights = chain_inputs(CHAIN_SEED)
    o64, g64, pre64 = run_chain(False, torch.float64, "cpu", x, gy, weights)
    assert all((p.abs() > R.KINK_MARGIN).all() for p in pre64), "a BatchNorm output sits on the ReLU kink: pick another seed"
    o32, g32, _ = run_chain(False, torch.float32, "cpu", x, gy, weights)
    ohip, ghip, _ = run_chain(True, torch.float32, "cuda", x, gy, weights)
    rows = [("out", R.rel_dist(ohip, o64), R.rel_dist(o32, o64))] + [(k, R.rel_dist(ghip[k], g64[k]), R.rel_dist(g32[k], g64[k])) for k in g64]
    for k, e_hip, e_ref in rows:
        print(f"CHAIN {k}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {bound_of(e_ref):.3e}")
    for k, e_hip, e_ref in rows:
        assert e_hip <= bound_of(e_ref), (k, e_hip, e_ref)
