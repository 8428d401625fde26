"""K3k (weight gradient) and K3d (data gradient) of FeatureNet's 5x5 stride-2 convolutions and the kernel-5 form of ``DiffConv2d`` /
``DiffConvBlock2d`` on the MI355X.

Yardsticks, none of which is the code under test: the float64 restatement (tests/conv_k5s2_grad_ref.py; checked against float64
autograd of F.conv2d in tests/test_conv_k5s2_grad_cpu.py), the reference's recorded fp32 block gradients
(tests/golden/op_conv_k5s2_grad.npz) and, for the bare kernels, the fp32 run of the same restatement on stock ATen.  No test reads the
reference or the oracle.

  criterion  per tensor: e_ref = max-abs distance of the fp32 yardstick to the float64 restatement over the tensor's max-abs, e_hip
             the same for the kernels; e_hip <= 8 e_ref (K3g's criterion: the factor covers another association of the sums).
             Where e_ref < 4 * 2^-23 the bound is 16 * 2^-23.
  exact      integer-valued inputs (every partial sum an integer far below 2^24: any summation order gives the same bits), the
             one-hot probes, the forward identity, reproducibility, accumulate, cache invalidation: torch.equal.

Every test prints its figures before it asserts (BARE / EXACT / PROBE / GRID / FWD / PARITY / CHAIN lines);
docs/kernels/K3k_conv_wgrad_k5s2.md keeps the measured ones.  No test provokes a fault."""
import gc

import pytest
import torch
from torch import nn

import conv_k5s2_grad_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 8.0
EPS32 = 2.0 ** -23


@pytest.fixture(autouse=True)
def free_gpu_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def g(golden):
    return golden("op_conv_k5s2_grad.npz")


def bound_of(e_ref):
    return FACTOR * e_ref if e_ref >= 4 * EPS32 else 16 * EPS32


def check(tag, got, f64, e_ref):
    e_hip = R.rel_dist(got.reshape(f64.shape), f64)
    print(f"{tag}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {bound_of(e_ref):.3e}  (max {f64.abs().max().item():.3e})")
    assert got.dtype == torch.float32
    assert e_hip <= bound_of(e_ref), (tag, e_hip, e_ref)


def rand_case(Cb, D, Hf, Wf, seed=0, integer=False):
    """x [Cb,D,Hf,Wf], gy [Ca,D,Hc,Wc], w [Ca,Cb,5,5] on the GPU; ``integer``: integer-valued in [-3, 3]."""
    gen = torch.Generator().manual_seed(7919 * seed + 31 * Cb + D * Hf * Wf)
    Hc, Wc = R.coarse_hw(Hf, Wf)
    if integer:
        mk = lambda *s: torch.randint(-3, 4, s, generator=gen).float()   # noqa: E731
        return mk(Cb, D, Hf, Wf).cuda(), mk(2 * Cb, D, Hc, Wc).cuda(), mk(2 * Cb, Cb, 5, 5).cuda()
    x, gy = torch.randn(Cb, D, Hf, Wf, generator=gen), torch.randn(2 * Cb, D, Hc, Wc, generator=gen)
    w = torch.randn(2 * Cb, Cb, 5, 5, generator=gen) * (2.0 / (Cb * 25)) ** 0.5
    return x.cuda(), gy.cuda(), w.cuda()


def wgrad_f(x, gy, dtype=torch.float64):
    return R.wgrad_k5s2_ref(R.planes(gy), R.planes(x), dtype)


def dgrad_f(gy, w, hw, dtype=torch.float64):
    return R.planes(R.dgrad_k5s2_ref(R.planes(gy), w, hw, dtype))


def make_module(Cb, w):
    from dmvsnet_amd import DiffConv2d
    m = DiffConv2d(Cb, 2 * Cb, 5, stride=2, padding=2, bias=False).cuda()
    with torch.no_grad():
        m.weight.copy_(w)
    return m


# ------------------------------------------------------------------------------------------------ BARE: both kernels against float64
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("Cb", [8, 16])
def test_bare_kernels_against_float64(Cb, shape):
    from dmvsnet_amd import ops
    D, Hf, Wf = shape
    x, gy, w = rand_case(Cb, D, Hf, Wf)
    f64 = wgrad_f(x, gy)
    check(f"BARE K3k {Cb}->{2 * Cb} {shape}", ops.conv2d_k5s2_wgrad(x, gy), f64, R.rel_dist(wgrad_f(x, gy, torch.float32), f64))
    f64 = dgrad_f(gy, w, (Hf, Wf))
    got = ops.conv2d_k5s2_dgrad(gy, w, (Hf, Wf))
    assert tuple(got.shape) == (Cb, D, Hf, Wf)
    check(f"BARE K3d {Cb}->{2 * Cb} {shape}", got, f64, R.rel_dist(dgrad_f(gy, w, (Hf, Wf), torch.float32), f64))


# ------------------------------------------------------------------------------------------------ EXACT: integer inputs
@pytest.mark.parametrize("shape", [(2, 33, 130), (1, 17, 67)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("Cb", [8, 16])
def test_integer_inputs_are_exact(Cb, shape):
    """Every product and partial sum is an integer far below 2^24, so fp32 in any order equals float64: any wrong tap, parity, seam or
    halo index shows as a wrong integer."""
    from dmvsnet_amd import ops
    D, Hf, Wf = shape
    x, gy, w = rand_case(Cb, D, Hf, Wf, seed=1, integer=True)
    gw64, gx64 = wgrad_f(x, gy), dgrad_f(gy, w, (Hf, Wf))
    print(f"EXACT {Cb}->{2 * Cb} {shape}: max |dW| {gw64.abs().max().item():.0f}  max |dX| {gx64.abs().max().item():.0f}")
    assert gw64.abs().max().item() < 2 ** 20 and gx64.abs().max().item() < 2 ** 20
    gw, gx = ops.conv2d_k5s2_wgrad(x, gy), ops.conv2d_k5s2_dgrad(gy, w, (Hf, Wf))
    nw, nx = int((gw.double().cpu() != gw64.cpu()).sum()), int((gx.double().cpu() != gx64.cpu()).sum())
    print(f"EXACT {Cb}->{2 * Cb} {shape}: {nw} of {gw.numel()} dW and {nx} of {gx.numel()} dX elements differ")
    assert torch.equal(gw.double().cpu(), gw64.cpu())
    assert torch.equal(gx.double().cpu(), gx64.cpu())


# ------------------------------------------------------------------------------------------------ PROBE: one-hot dY
def probe_pixels(Hc, Wc):
    """Interior, the four corners, and a pixel either side of each tile seam (K3k: rows of 4, columns of 32; K3d: rows of 8)."""
    px = [(Hc // 2 + 1, Wc // 2 + 3), (0, 0), (0, Wc - 1), (Hc - 1, 0), (Hc - 1, Wc - 1), (3, 31), (4, 32), (7, 31), (8, 32), (8, Wc - 1)]
    return [p for p in px if p[0] < Hc and p[1] < Wc]


@pytest.mark.parametrize("Cb", [8, 16])
def test_one_hot_probe(Cb):
    from dmvsnet_amd import ops
    D, Hf, Wf = 1, 33, 130
    Hc, Wc = R.coarse_hw(Hf, Wf)
    x, _, w = rand_case(Cb, D, Hf, Wf, seed=2)
    a0 = 2 * Cb - 3
    bad = 0
    for (y0, x0) in probe_pixels(Hc, Wc):
        gy = torch.zeros(2 * Cb, D, Hc, Wc, device="cuda")
        gy[a0, 0, y0, x0] = 1.0
        # K3d: the weight of a0 scattered around (2 y0, 2 x0), what falls outside dropped
        want = torch.zeros(Cb, D, Hf + 4, Wf + 4, device="cuda")
        want[:, 0, 2 * y0:2 * y0 + 5, 2 * x0:2 * x0 + 5] = w[a0]
        want = want[:, :, 2:2 + Hf, 2:2 + Wf]
        gx = ops.conv2d_k5s2_dgrad(gy, w, (Hf, Wf))
        # K3k: row a0 holds the fine values around (2 y0, 2 x0), zero outside; every other row is zero
        xp = torch.zeros(Cb, Hf + 6, Wf + 6, device="cuda")
        xp[:, 2:2 + Hf, 2:2 + Wf] = x[:, 0]
        wantw = torch.zeros(2 * Cb, Cb, 5, 5, device="cuda")
        wantw[a0] = xp[:, 2 * y0:2 * y0 + 5, 2 * x0:2 * x0 + 5]
        gw = ops.conv2d_k5s2_wgrad(x, gy)
        nx, nw = int((gx != want).sum()), int((gw != wantw).sum())
        bad += nx + nw
        print(f"PROBE {Cb}->{2 * Cb} dY one-hot at {(y0, x0)}: {nx} of {gx.numel()} dX, {nw} of {gw.numel()} dW elements differ")
    assert bad == 0


# ------------------------------------------------------------------------------------------------ GRID
def test_more_tiles_than_shares():
    """The smallest D = 1 image with more than 256 tiles and a tile count not divisible by 8: shares of one and of two tiles."""
    from dmvsnet_amd import ops, _lib
    _, ty, tx = ops.WGRAD_K5S2_TILE
    ny, nx = 17, 17   # 289 tiles
    Hf, Wf = 2 * ty * ny, 2 * (tx * (nx - 1) + 8)
    plan = _lib.load().dmvs_conv2d_k5s2_wgrad_plan(16, 1, Hf, Wf)
    assert plan // 512 == ny * nx and plan // 512 > 256 and (plan // 512) % 8 and plan % 512 == 256
    x, gy, w = rand_case(8, 1, Hf, Wf, seed=3)
    f64 = wgrad_f(x, gy)
    check(f"GRID K3k 8->16 1x{Hf}x{Wf} ({plan // 512} tiles)", ops.conv2d_k5s2_wgrad(x, gy), f64, R.rel_dist(wgrad_f(x, gy, torch.float32), f64))
    f64 = dgrad_f(gy, w, (Hf, Wf))
    check(f"GRID K3d 8->16 1x{Hf}x{Wf}", ops.conv2d_k5s2_dgrad(gy, w, (Hf, Wf)), f64, R.rel_dist(dgrad_f(gy, w, (Hf, Wf), torch.float32), f64))


def test_poisoned_workspace_and_outputs():
    from dmvsnet_amd import ops
    D, Hf, Wf = 1, 12, 80
    x, gy, w = rand_case(8, D, Hf, Wf, seed=4)
    ws = ops.conv2d_k5s2_wgrad_workspace(16, D, Hf, Wf, x.device)
    ws.fill_(float("nan"))
    gw = torch.full((16, 8, 5, 5), float("nan"), device="cuda")
    gx = torch.full((8, D, Hf, Wf), float("nan"), device="cuda")
    ops.conv2d_k5s2_wgrad(x, gy, out=gw, workspace=ws)
    ops.conv2d_k5s2_dgrad(gy, w, (Hf, Wf), out=gx)
    f64 = wgrad_f(x, gy)
    check("GRID K3k 8->16 1x12x80 NaN-poisoned", gw, f64, R.rel_dist(wgrad_f(x, gy, torch.float32), f64))
    f64 = dgrad_f(gy, w, (Hf, Wf))
    check("GRID K3d 8->16 1x12x80 NaN-poisoned", gx, f64, R.rel_dist(dgrad_f(gy, w, (Hf, Wf), torch.float32), f64))


# ------------------------------------------------------------------------------------------------ reproducibility and reuse
@pytest.mark.parametrize("Cb", [8, 16])
def test_reproducible_accumulate_and_batch(Cb):
    from dmvsnet_amd import ops
    D, Hf, Wf = 2, 18, 70
    x0, gy0, w = rand_case(Cb, D, Hf, Wf, seed=5)
    x1, gy1, _ = rand_case(Cb, D, Hf, Wf, seed=6)
    a, b = ops.conv2d_k5s2_wgrad(x0, gy0), ops.conv2d_k5s2_wgrad(x0, gy0)
    assert torch.equal(a, b)
    assert torch.equal(ops.conv2d_k5s2_dgrad(gy0, w, (Hf, Wf)), ops.conv2d_k5s2_dgrad(gy0, w, (Hf, Wf)))
    second = ops.conv2d_k5s2_wgrad(x1, gy1)
    acc = ops.conv2d_k5s2_wgrad(x1, gy1, out=a.clone(), accumulate=True)
    assert torch.equal(acc, a + second)
    # a batch of 2 through the module: the samples singly, added in order
    m = make_module(Cb, w)
    xb = torch.stack((x0[:, 0], x1[:, 0])).contiguous().requires_grad_(True)
    gyb = torch.stack((gy0[:, 0], gy1[:, 0])).contiguous()
    m(xb).backward(gyb)
    g0 = ops.conv2d_k5s2_wgrad(x0[:, :1].contiguous(), gy0[:, :1].contiguous())
    g1 = ops.conv2d_k5s2_wgrad(x1[:, :1].contiguous(), gy1[:, :1].contiguous())
    assert torch.equal(m.weight.grad, g0 + g1)
    assert torch.equal(xb.grad[1], ops.conv2d_k5s2_dgrad(gy1[:, :1].contiguous(), w, (Hf, Wf))[:, 0])


# ------------------------------------------------------------------------------------------------ FWD
@pytest.mark.parametrize("Cb", [8, 16])
def test_forward_is_the_host_packed_k3_launch(Cb):
    from dmvsnet_amd import ops
    x, _, w = rand_case(Cb, 2, 18, 70, seed=7)
    xb = x.permute(1, 0, 2, 3).contiguous()   # [B = 2, Cb, H, W]
    m = make_module(Cb, w)

    def host(weight):
        layer = ops.make_layer("host", ops.CONV2D_K5S2, weight.detach(), None, None, False, direct=False)
        return torch.stack([ops.conv3d(xb[b].unsqueeze(1), layer, backend="mfma").squeeze(1) for b in range(2)])

    assert torch.equal(m(xb), host(m.weight))
    f64 = R.conv_k5s2_ref(xb, w)
    check(f"FWD {Cb}->{2 * Cb} 2x18x70", m(xb).detach(), f64, R.rel_dist(R.conv_k5s2_ref(xb, w, torch.float32), f64))
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    m(xb).sum().backward()
    before = m.weight.detach().clone()
    opt.step()   # in place: the cached packed weight is stale now
    assert not torch.equal(before, m.weight)
    assert torch.equal(m(xb), host(m.weight))


# ------------------------------------------------------------------------------------------------ PARITY on the golden blocks
@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_block_parity_golden_cases(g, name):
    """The reference's block on DiffConvBlock2d against the reference's recorded fp32 run."""
    from dmvsnet_amd import DiffConvBlock2d
    case = R.golden_case(g, name)
    assert R.kink_violations(case) == 0
    f64 = R.block_f64(case)
    Cb = case["Cb"]
    blk = DiffConvBlock2d(Cb, 2 * Cb, 5, stride=2, padding=2).cuda().train()
    with torch.no_grad():
        blk.conv.weight.copy_(case["w"])
        blk.bn.weight.copy_(case["gamma"])
        blk.bn.bias.copy_(case["beta"])
    x = case["x"].cuda().requires_grad_(True)
    out = blk(x)
    out.backward(case["gy"].cuda())
    got = dict(out=out.detach(), g_x=x.grad, g_w=blk.conv.weight.grad, g_gamma=blk.bn.weight.grad, g_beta=blk.bn.bias.grad)
    rows = []
    for k in ("out", "g_x", "g_w", "g_gamma", "g_beta"):
        e_ref, e_hip = R.rel_dist(case[k], f64[k]), R.rel_dist(got[k], f64[k])
        rows.append((k, e_hip, e_ref))
        print(f"PARITY {name} {k}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {bound_of(e_ref):.3e}  (max {f64[k].abs().max().item():.3e})")
    for k, e_hip, e_ref in rows:
        assert e_hip <= bound_of(e_ref), (name, k, e_hip, e_ref)


# ------------------------------------------------------------------------------------------------ CHAIN: FeatureNet's conv1, conv2
def test_featurenet_conv1_conv2_chain():
    from dmvsnet_amd import DiffConvBlock2d
    chain = R.make_chain(2, 20, 28, 0)
    f64 = R.chain_f64(chain)
    print(f"CHAIN nearest BatchNorm output to the kink: {f64['nearest_kink']:.3e}")
    assert f64["nearest_kink"] > R.CHAIN_KINK_MARGIN
    r32 = R.chain_f64(chain, torch.float32, "cuda")   # e_ref: the fp32 run of the restatement on stock ATen
    blocks = []
    for (_, cin, cout, k), (w, gamma, beta) in zip(R.CHAIN_BLOCKS, chain["params"]):
        blk = DiffConvBlock2d(cin, cout, k, stride=2, padding=2) if k == 5 else DiffConvBlock2d(cin, cout, 3, 1, padding=1)
        with torch.no_grad():
            blk.conv.weight.copy_(w), blk.bn.weight.copy_(gamma), blk.bn.bias.copy_(beta)
        blocks.append(blk)
    hip = nn.Sequential(*blocks).cuda().train()

    def step(net):
        net.zero_grad(set_to_none=True)
        x = chain["x"].cuda().requires_grad_(True)
        out = net(x)
        out.backward(chain["gy"].cuda())
        return [out.detach(), x.grad] + [p.grad for p in net.parameters()]

    ref, got, again = [r32["out"], r32["g_x"]] + r32["g_params"], step(hip), step(hip)
    names = ["out", "g_x"] + [f"{n}.{p}" for n, *_ in R.CHAIN_BLOCKS for p in ("conv.weight", "bn.weight", "bn.bias")]
    wants = [f64["out"], f64["g_x"]] + f64["g_params"]
    assert len(names) == len(wants) == len(got) == len(ref)
    rows = []
    for n, r, h, w64 in zip(names, ref, got, wants):
        e_ref, e_hip = R.rel_dist(r, w64), R.rel_dist(h, w64)
        rows.append((n, e_hip, e_ref))
        print(f"CHAIN {n}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {bound_of(e_ref):.3e}")
    for n, e_hip, e_ref in rows:
        assert e_hip <= bound_of(e_ref), (n, e_hip, e_ref)
    for n, h, h2 in zip(names, got, again):
        assert torch.equal(h, h2), n


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_before_any_launch():
    from dmvsnet_amd import ops
    from dmvsnet_amd import conv as dconv
    from dmvsnet_amd._lib import DmvsError
    x, gy, w = rand_case(8, 1, 5, 8, seed=8)
    m = make_module(8, w)
    xb = x.permute(1, 0, 2, 3).contiguous()
    ops.launch_log = []
    before = dict(dconv.launch_counts)
    try:
        for bad in (xb.cpu(), xb.half(), xb.transpose(2, 3), torch.zeros(1, 16, 5, 8, device="cuda")):
            with pytest.raises((DmvsError, RuntimeError)):
                m(bad)
        with pytest.raises(DmvsError):
            ops.conv2d_k5s2_wgrad(x.cpu(), gy)
        with pytest.raises(RuntimeError):
            ops.conv2d_k5s2_dgrad(gy.half(), w, (5, 8))
        with pytest.raises(DmvsError):
            ops.conv2d_k5s2_dgrad(gy, w, (6, 9))    # (6, 9) has another coarse grid
        with pytest.raises(DmvsError):
            ops.conv2d_k5s2_wgrad(x[:4].contiguous(), gy)
        assert ops.launch_log == [] and dconv.launch_counts == before
    finally:
        ops.launch_log = None
