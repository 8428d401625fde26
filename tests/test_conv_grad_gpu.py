"""K3g (weight gradient of the stride-1 square convolutions), their data gradient on K3 and ``DiffConv3d`` / ``DiffConv2d`` on the
MI355X.

Yardsticks, none of which is the code under test: the float64 restatement (tests/conv_grad_ref.py; checked against float64 autograd
of F.conv3d / F.conv2d in tests/test_conv_grad_cpu.py), the reference's recorded fp32 block gradients (tests/golden/op_conv_grad.npz)
and, for the bare kernels, the fp32 run of the same restatement on stock ATen.  No test reads the reference or the oracle.

  criterion  per gradient tensor: e_ref = max-abs distance of the fp32 yardstick to the float64 restatement over the tensor's max-abs,
             e_hip the same for the kernels; e_hip <= 8 e_ref (K1b / K4b's criterion: the factor covers another association of the
             voxel sums).  Where e_ref < 4 * 2^-23 the bound is 16 * 2^-23.
  exact      the single-voxel probe, the data gradient against the host-packed K3 launch, the forward identity, reproducibility,
             accumulate, cache invalidation: torch.equal.

Every test prints its figures before it asserts (PARITY / BARE / GRID / DGRAD / FWD / CHAIN lines); docs/kernels/K3g_conv_wgrad.md is
where the measured ones are kept -- none recorded so far (the document says so).  No test provokes a
fault."""
import gc

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import conv_grad_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 8.0
EPS32 = 2.0 ** -23

# the smallest volumes at which the kernel can go wrong (tile: 1 x 4 x 32 voxels)
VOLUMES = {
    "1x5x7": (1, 5, 7),         # smaller than any tile; with kd = 3 only the centre z tap is live
    "3x19x35": (3, 19, 35),     # W % 4 != 0 (no 16-byte rows), ragged in y and x, several tiles
    "2x20x36": (2, 20, 36),     # W % 4 == 0
    "5x9x131": (5, 9, 131),     # ragged against 32-, 64- and 128-wide tiles; more tiles than shares at C = 64
}


@pytest.fixture(autouse=True)
def free_gpu_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def g(golden):
    return golden("op_conv_grad.npz")


def bound_of(e_ref):
    return FACTOR * e_ref if e_ref >= 4 * EPS32 else 16 * EPS32


def rand_case(C, kd, D, H, W, B=1, seed=0):
    gen = torch.Generator().manual_seed(7919 * seed + 31 * C + kd + D * H * W)
    x = torch.randn(B, C, D, H, W, generator=gen).cuda()
    gy = torch.randn(B, C, D, H, W, generator=gen).cuda()
    w = (torch.randn(C, C, kd, 3, 3, generator=gen) * (2.0 / (C * 9 * kd)) ** 0.5).cuda()
    return x, gy, w


def hip_wgrad(x, gy, kd, **kw):
    """K3g over a batch, its samples one after the other (accumulate from the second on)."""
    from dmvsnet_amd import ops
    gw = None
    for b in range(x.shape[0]):
        gw = ops.conv3d_wgrad(x[b], gy[b], kd, out=gw, accumulate=b > 0, **kw)
    return gw


def host_layer(w, kd, transposed_flipped=False):
    """The bare K3 layer with the weight packed by the HOST packer (the eval path's packing)."""
    from dmvsnet_amd import ops
    C = w.shape[0]
    w5 = w.detach().cpu().reshape(C, C, kd, 3, 3)
    src = w5.transpose(0, 1).flip(2, 3, 4).contiguous() if transposed_flipped else w5
    return ops.ConvLayer("host", ops.CONV_S1, kd, C, C, None, ops.pack_mfma(src, C, C, ops.CONV_S1, kd).cuda(), None, None, False)


def make_module(C, kd, w):
    from dmvsnet_amd import DiffConv2d, DiffConv3d
    m = (DiffConv3d if kd == 3 else DiffConv2d)(C, C, 3, stride=1, padding=1, bias=False).cuda()
    with torch.no_grad():
        m.weight.copy_(w.reshape(m.weight.shape))
    return m


def shaped(t, kd):
    """[B,C,D,H,W] -> what the module of this kdepth takes ([B,C,H,W] for the 2D layers; D must be 1)."""
    return t if kd == 3 else t.squeeze(2)


# ------------------------------------------------------------------------------------------------ parity on the golden blocks
@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_block_parity_golden_cases(g, name):
    """The reference's block restated: DiffConv + F.batch_norm(training=True) + ReLU, against the reference's recorded fp32 run."""
    case = R.golden_case(g, name)
    assert R.kink_violations(case) == 0
    f64 = R.block_f64(case)
    C, kd = case["C"], case["kd"]
    m = make_module(C, kd, case["w"].cuda())
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
def check_wgrad(tag, x, gy, kd, gw):
    f64 = R.wgrad_ref(x, gy, kd)
    e_ref, e_hip = R.rel_dist(R.wgrad_ref(x, gy, kd, torch.float32), f64), R.rel_dist(gw, f64)
    print(f"{tag}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {bound_of(e_ref):.3e}  (|dW| max {f64.abs().max().item():.3e})")
    assert gw.dtype == torch.float32 and tuple(gw.shape) == tuple(f64.shape)
    assert e_hip <= bound_of(e_ref), (tag, e_hip, e_ref)


@pytest.mark.parametrize("vol", list(VOLUMES))
@pytest.mark.parametrize("C,kd", R.SHAPES)
def test_bare_wgrad_against_float64(C, kd, vol):
    D, H, W = VOLUMES[vol]
    x, gy, _ = rand_case(C, kd, D, H, W)
    check_wgrad(f"BARE C {C} kd {kd} {vol}", x, gy, kd, hip_wgrad(x, gy, kd))


@pytest.mark.parametrize("C,kd", R.SHAPES)
def test_bare_wgrad_accumulates_over_a_batch(C, kd):
    x, gy, _ = rand_case(C, kd, 2, 6, 33, B=3, seed=1)
    check_wgrad(f"BARE C {C} kd {kd} B 3", x, gy, kd, hip_wgrad(x, gy, kd))


# ------------------------------------------------------------------------------------------------ grid-size cases
def plan_of(C, D, H, W, kd):
    from dmvsnet_amd import _lib
    plan = _lib.load().dmvs_conv3d_wgrad_plan(C, D, H, W, kd)
    assert plan > 0
    return plan >> 9, plan & 511


def test_more_tiles_than_workgroups():
    for vol in ((4, 96, 352), (4, 128, 352), (8, 96, 352)):
        tiles, wgs = plan_of(16, *vol, 3)
        if tiles > wgs:
            break
    else:
        pytest.fail("no shape of the list has more tiles than workgroups")
    x, gy, _ = rand_case(16, 3, *vol)
    print(f"GRID C 16 kd 3 {vol}: {tiles} tiles, {wgs} workgroups")
    check_wgrad(f"GRID C 16 kd 3 {vol} tiles > workgroups", x, gy, 3, hip_wgrad(x, gy, 3))


@pytest.mark.parametrize("C,kd", ((16, 3), (64, 3), (32, 1)))
def test_fewer_tiles_than_workgroups(C, kd):
    """The workgroups past the last share exit at once and own no partial: a NaN-filled workspace must not reach the result."""
    from dmvsnet_amd import _lib
    vol = (1, 6, 40)
    tiles, wgs = plan_of(C, *vol, kd)
    assert tiles < wgs, (tiles, wgs)
    x, gy, _ = rand_case(C, kd, *vol)
    ws = torch.full((_lib.load().dmvs_conv3d_wgrad_workspace(C, *vol, kd),), float("nan"), device="cuda")
    print(f"GRID C {C} kd {kd} {vol}: {tiles} tiles, {wgs} workgroups")
    check_wgrad(f"GRID C {C} kd {kd} {vol} tiles < workgroups", x, gy, kd, hip_wgrad(x, gy, kd, workspace=ws))


# ------------------------------------------------------------------------------------------------ single-voxel probe (exact)
@pytest.mark.parametrize("C,kd", R.SHAPES)
def test_single_voxel_probe(C, kd):
    """X[ci] = one 1.0 at a probe voxel (interior, faces, edges, corners; which one depends on ci): dW[co][ci][tap] is then exactly one
    element of dY, or 0 where the tap falls outside the volume.  Names tap order, halo and co / ci mistakes without a tolerance."""
    D, H, W = 3, 6, 37
    probes = [(1, 2, 5), (0, 0, 0), (D - 1, H - 1, W - 1), (1, 3, 31), (1, 4, 32), (0, 2, W - 1), (2, 0, 33), (1, H - 1, 0), (0, 3, 32),
              (2, 4, 31), (1, 0, 36)]
    gy = torch.randn(1, C, D, H, W, generator=torch.Generator().manual_seed(C + kd)).cuda()
    x = torch.zeros(1, C, D, H, W, device="cuda")
    want = torch.zeros(C, C, kd, 3, 3, device="cuda")
    for ci in range(C):
        z, y, xx = probes[ci % len(probes)]
        x[0, ci, z, y, xx] = 1.0
        for kz in range(kd):
            for ky in range(3):
                for kx in range(3):
                    # X[ci][oz + kz - 1][oy + ky - 1][ox + kx - 1] is the probe for the output voxel (oz, oy, ox):
                    oz, oy, ox = (z - kz + 1 if kd == 3 else z), y - ky + 1, xx - kx + 1
                    if 0 <= oz < D and 0 <= oy < H and 0 <= ox < W:
                        want[:, ci, kz, ky, kx] = gy[0, :, oz, oy, ox]
    got = hip_wgrad(x, gy, kd)
    bad = (got != want).nonzero()
    print(f"PROBE C {C} kd {kd}: {bad.shape[0]} of {want.numel()} elements differ" + (f", first (co, ci, kz, ky, kx) = {bad[0].tolist()}" if len(bad) else ""))
    assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------ data gradient
@pytest.mark.parametrize("vol", ["3x19x35", "2x20x36"])
@pytest.mark.parametrize("C,kd", R.SHAPES)
def test_data_gradient(C, kd, vol):
    from dmvsnet_amd import ops
    D, H, W = VOLUMES[vol]
    B = 2
    x, gy, w = rand_case(C, kd, D, H, W, B=B, seed=2)
    if kd == 1:   # the 2D module takes [B,C,H,W]: the D slices become samples
        x, gy = [t.permute(0, 2, 1, 3, 4).reshape(B * D, C, 1, H, W).contiguous() for t in (x, gy)]
    m = make_module(C, kd, w)
    m.weight.requires_grad_(False)
    xin = shaped(x, kd).clone().requires_grad_(True)
    m(xin).backward(shaped(gy, kd).contiguous())
    gx = xin.grad.reshape(x.shape)
    layer = host_layer(w, kd, transposed_flipped=True)
    want = torch.stack([ops.conv3d(gy[b], layer, backend="mfma") for b in range(x.shape[0])])
    assert torch.equal(gx, want), "the data gradient is not the K3 launch on the host-packed transposed-flipped weight"
    f64 = R.dgrad_ref(gy, w, kd)
    e_ref, e_hip = R.rel_dist(R.dgrad_ref(gy, w, kd, torch.float32), f64), R.rel_dist(gx, f64)
    print(f"DGRAD C {C} kd {kd} {vol}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {bound_of(e_ref):.3e}")
    assert e_hip <= bound_of(e_ref), (e_hip, e_ref)


# ------------------------------------------------------------------------------------------------ forward identity
@pytest.mark.parametrize("C,kd", R.SHAPES)
def test_forward_identity(C, kd):
    from dmvsnet_amd import ops
    D, H, W = (3, 19, 35) if kd == 3 else (1, 19, 35)
    x, _, w = rand_case(C, kd, D, H, W, B=2, seed=3)
    m = make_module(C, kd, w)
    with torch.no_grad():
        y = m(shaped(x, kd).contiguous()).reshape(x.shape)
    layer = host_layer(w, kd)
    want = torch.stack([ops.conv3d(x[b], layer, backend="mfma") for b in range(2)])
    assert torch.equal(y, want), "the forward is not ops.conv3d(..., backend='mfma') on the host-packed weight"
    f64 = R.conv_ref(x, w, kd)
    aten = F.conv3d(x, w, padding=1) if kd == 3 else F.conv2d(x.squeeze(2), w.squeeze(2), padding=1).unsqueeze(2)
    e_ref, e_hip = R.rel_dist(aten, f64), R.rel_dist(y, f64)
    print(f"FWD C {C} kd {kd}: e_hip {e_hip:.3e}  e_ref (F.conv) {e_ref:.3e}  bound {bound_of(e_ref):.3e}")
    assert e_hip <= bound_of(e_ref), (e_hip, e_ref)


# ------------------------------------------------------------------------------------------------ reproducibility and poison
@pytest.mark.parametrize("C,kd", ((16, 3), (64, 3), (32, 1)))
def test_reproducible_poison_and_accumulate(C, kd):
    from dmvsnet_amd import _lib, ops
    D, H, W = (3, 19, 35) if kd == 3 else (1, 19, 35)
    x, gy, w = rand_case(C, kd, D, H, W, B=2, seed=4)
    nan = float("nan")
    # two whole backward runs through the module are bit-equal
    runs = []
    for _ in range(2):
        m = make_module(C, kd, w)
        xin = shaped(x, kd).clone().requires_grad_(True)   # a fresh leaf per run: its .grad must not accumulate
        m(xin).backward(shaped(gy, kd).contiguous())
        runs.append((xin.grad.clone(), m.weight.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.isfinite(runs[0][0]).all() and torch.isfinite(runs[0][1]).all()
    # NaN-filled gw / workspace / gx are fully overwritten
    n_ws = _lib.load().dmvs_conv3d_wgrad_workspace(C, D, H, W, kd)
    ws = torch.full((n_ws,), nan, device="cuda")
    gw = ops.conv3d_wgrad(x[0], gy[0], kd, out=torch.full((C, C, kd, 3, 3), nan, device="cuda"), workspace=ws)
    fresh = ops.conv3d_wgrad(x[0], gy[0], kd)
    assert torch.isfinite(gw).all() and torch.equal(gw, fresh)
    tiles = _lib.load().dmvs_conv3d_wgrad_plan(C, D, H, W, kd) >> 9
    shares = min(tiles, 256 // ((C // 32) ** 2 if C > 32 else 1))
    assert torch.isfinite(ws[:shares * 9 * kd * C * C]).all(), "a share's partial was not fully written"
    gx = ops.conv3d(gy[0], host_layer(w, kd, True), out=torch.full_like(x[0], nan), backend="mfma")
    assert torch.isfinite(gx).all()
    # accumulate adds to a known gw exactly once
    known = torch.randn(C, C, kd, 3, 3, generator=torch.Generator().manual_seed(5)).cuda()
    acc = ops.conv3d_wgrad(x[0], gy[0], kd, out=known.clone(), accumulate=True)
    assert torch.equal(acc, known + fresh)
    # the launch log carries the family once per dispatch
    ops.launch_log = log = []
    try:
        ops.conv3d_wgrad(x[0], gy[0], kd)
    finally:
        ops.launch_log = None
    assert log == ["conv3d_wgrad", "conv3d_wgrad"]


# ------------------------------------------------------------------------------------------------ cache invalidation
@pytest.mark.parametrize("C,kd", ((16, 3), (32, 1)))
def test_cache_invalidation_by_an_optimizer_step(C, kd):
    D, H, W = (2, 9, 13) if kd == 3 else (1, 9, 13)
    x, gy, w = rand_case(C, kd, D, H, W, B=1, seed=6)
    xs, gys = shaped(x, kd).contiguous(), shaped(gy, kd).contiguous()
    m = make_module(C, kd, w)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    xin = xs.clone().requires_grad_(True)
    y0 = m(xin)
    y0.backward(gys)
    gx0 = xin.grad.clone()
    opt.step()
    xin2 = xs.clone().requires_grad_(True)
    y1 = m(xin2)
    y1.backward(gys)
    fresh = make_module(C, kd, m.weight.detach().clone())
    xin3 = xs.clone().requires_grad_(True)
    y2 = fresh(xin3)
    y2.backward(gys)
    assert not torch.equal(y0, y1), "the step did not change the output: stale packed weight"
    assert torch.equal(y1, y2) and torch.equal(xin2.grad, xin3.grad) and not torch.equal(gx0, xin2.grad)
    # unchanged weight: the packed forms are re-used
    packed = m._packed[False][1].w_mfma
    m(xs)
    assert m._packed[False][1].w_mfma is packed


# ------------------------------------------------------------------------------------------------ plumbing
def test_frozen_inputs_skip_their_kernel_and_double_backward_raises():
    from dmvsnet_amd import conv
    x, gy, w = rand_case(16, 3, 2, 6, 9, B=2, seed=7)
    m = make_module(16, 3, w)
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
    # a non-contiguous input is refused, as everywhere in the package
    from dmvsnet_amd._lib import DmvsError
    with pytest.raises(DmvsError):
        m(x.transpose(3, 4))


def build_chain(diff, dtype, device, weights):
    from dmvsnet_amd import DiffConv3d
    mk = (lambda C: DiffConv3d(C, C, 3, stride=1, padding=1, bias=False)) if diff else (lambda C: nn.Conv3d(C, C, 3, stride=1, padding=1, bias=False))
    net = nn.Sequential(mk(16), nn.BatchNorm3d(16), nn.ReLU(), nn.Conv3d(16, 32, 3, stride=2, padding=1, bias=False), nn.BatchNorm3d(32),
                        nn.ReLU(), mk(32), nn.BatchNorm3d(32), nn.ReLU())
    net.load_state_dict(weights)
    return net.to(device=device, dtype=dtype).train()


def test_chained_unet_fragment():
    """DiffConv3d 16 -> 16, ATen stride-2 nn.Conv3d 16 -> 32, DiffConv3d 32 -> 32, each followed by BatchNorm3d (train) and ReLU, through
    .backward(); against the all-ATen chain in fp32 (CPU) and float64 (CPU), same criterion, on a volume that meets the kink condition."""
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(1, 16, 4, 10, 12, generator=gen)
    gy = torch.randn(1, 32, 2, 5, 6, generator=gen)
    proto = nn.Sequential(nn.Conv3d(16, 16, 3, padding=1, bias=False), nn.BatchNorm3d(16), nn.ReLU(), nn.Conv3d(16, 32, 3, stride=2, padding=1, bias=False),
                          nn.BatchNorm3d(32), nn.ReLU(), nn.Conv3d(32, 32, 3, padding=1, bias=False), nn.BatchNorm3d(32), nn.ReLU())
    weights = {}
    for k, v in proto.state_dict().items():
        if v.dim() == 5:                                  # conv weights, He-sized
            v = torch.randn(v.shape, generator=gen) * (2.0 / v[0].numel()) ** 0.5
        elif k.endswith(".weight"):                       # BatchNorm gamma
            v = 1.0 + 0.2 * torch.randn(v.shape, generator=gen)
        elif k.endswith(".bias"):                         # BatchNorm beta
            v = 0.2 * torch.randn(v.shape, generator=gen)
        weights[k] = v

    def run(diff, dtype, device):
        net = build_chain(diff, dtype, device, weights)
        xin = x.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)   # a fresh leaf per run
        pre = []
        hooks = [net[i].register_forward_hook(lambda mod, inp, out: pre.append(out.detach())) for i in (1, 4, 7)]
        out = net(xin)
        for h in hooks:
            h.remove()
        out.backward(gy.to(device=device, dtype=dtype))
        grads = {"x": xin.grad, **{n: p.grad for n, p in net.named_parameters()}}
        return out.detach(), grads, pre

    o64, g64, pre64 = run(False, torch.float64, "cpu")
    assert all((p.abs() > R.KINK_MARGIN).all() for p in pre64), "a BatchNorm output sits on the ReLU kink: pick another seed"
    o32, g32, _ = run(False, torch.float32, "cpu")
    ohip, ghip, _ = run(True, torch.float32, "cuda")
    rows = [("out", R.rel_dist(ohip, o64), R.rel_dist(o32, o64))] + [(k, R.rel_dist(ghip[k], g64[k]), R.rel_dist(g32[k], g64[k])) for k in g64]
    for k, e_hip, e_ref in rows:
        print(f"CHAIN {k}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {bound_of(e_ref):.3e}")
    for k, e_hip, e_ref in rows:
        assert e_hip <= bound_of(e_ref), (k, e_hip, e_ref)
