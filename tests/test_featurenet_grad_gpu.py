"""K3f (weight and bias gradient of FeatureNet's rectangular stride-1 layers), their data gradients on K3's new rows, and
``DiffFeatureConv2d`` / ``DiffFeatureConvBlock2d`` / ``DiffFeatureNet`` on the MI355X.

Yardsticks, none of which is the code under test: the float64 restatement (tests/featurenet_grad_ref.py; checked against float64
autograd of F.conv2d and the stock nn network in tests/test_featurenet_grad_cpu.py), the fp32 run of the same restatement on stock ATen,
and the reference's recorded fp32 results (tests/golden/op_featurenet_grad.npz).  No test reads the reference or the oracle.

  criterion  per tensor: e = max|a - f64| / max|f64|; e_ref from the fp32 yardstick, e_hip from the kernels; e_hip <= 8 e_ref, and
             16 * 2^-23 where e_ref < 4 * 2^-23.
  exact      integer-valued inputs (every partial sum an integer below 2^20: any summation order gives the same bits), the one-hot
             probes, the forward identity, reproducibility, accumulate, the user workspace: torch.equal.

Every test prints its figures before it asserts (BARE / EXACT / PROBE / GRID / FWD / PARITY / WHOLE lines);
docs/kernels/K3f_conv_wgrad_fpn.md keeps the measured ones.  No test provokes a fault."""
import copy
import gc

import pytest
import torch

import featurenet_grad_ref as R

pytestmark = pytest.mark.gpu
LAYER_IDS = [l[0] for l in R.LAYERS]


@pytest.fixture(autouse=True)
def free_gpu_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def g(golden):
    return golden("op_featurenet_grad.npz")


def check(tag, got, f64, e_ref):
    e_hip = R.rel_dist(got.reshape(f64.shape), f64)
    print(f"{tag}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {R.bound(e_ref):.3e}  (max {f64.abs().max().item():.3e})")
    assert got.dtype == torch.float32
    assert e_hip <= R.bound(e_ref), (tag, e_hip, e_ref)
    return e_hip


def gpu_case(cin, cout, k, bias, shape, seed=0, integer=False):
    return {key: (None if v is None else v.cuda()) for key, v in R.layer_case(cin, cout, k, bias, shape, seed, integer).items()}


def bare(case, workspace=None, out=None, bias_out=None, accumulate=False):
    """K3f on the case: (dW, db or None)."""
    from dmvsnet_amd import ops
    k = case["w"].shape[-1]
    if case["bias"] is not None and bias_out is None:
        bias_out = torch.empty_like(case["bias"])
    gw = ops.conv2d_wgrad_fpn(case["x"], case["gy"], k, out=out, bias_out=bias_out, accumulate=accumulate, workspace=workspace)
    return gw, bias_out


def bare_dgrad(case):
    """The data gradient's K3 launch on the case's planes: the layer out -> in on the transposed, tap-flipped weight."""
    from dmvsnet_amd import featurenet, ops
    layer = featurenet._build_fpn(case["w"], 1, True)
    return ops.conv3d(case["gy"], layer, backend="mfma")


def make_module(case):
    from dmvsnet_amd import DiffFeatureConv2d
    cout, cin, k, _ = case["w"].shape
    m = DiffFeatureConv2d(cin, cout, k, padding=k // 2, bias=case["bias"] is not None).cuda()
    with torch.no_grad():
        m.weight.copy_(case["w"])
        if case["bias"] is not None:
            m.bias.copy_(case["bias"])
    return m


def module_run(m, case):
    """Forward + backward of the module on the case's planes as a batch: y, dX (None for conv0.0), dW, db (None without bias)."""
    x = R.planes(case["x"]).contiguous().requires_grad_(m.in_channels != 3)
    y = m(x)
    leaves = ([x] if x.requires_grad else []) + list(m.parameters())
    grads = list(torch.autograd.grad(y, leaves, R.planes(case["gy"]).contiguous()))
    gx = grads.pop(0) if x.requires_grad else None
    return y.detach(), gx, grads[0], (grads[1] if len(grads) > 1 else None)


# ------------------------------------------------------------------------------------------------ BARE: against float64
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name,cin,cout,k,bias", R.LAYERS, ids=LAYER_IDS)
def test_bare_kernels_against_float64(name, cin, cout, k, bias, shape):
    case = gpu_case(cin, cout, k, bias, shape)
    f64, f32 = R.layer_f64(case, device="cuda"), R.layer_f64(case, torch.float32, device="cuda")
    gw, gb = bare(case)
    assert tuple(gw.shape) == (cout, cin, k, k)
    check(f"BARE K3f dW {name} {shape}", gw, f64["g_w"], R.rel_dist(f32["g_w"], f64["g_w"]))
    if bias:
        check(f"BARE K3f db {name} {shape}", gb, f64["g_b"], R.rel_dist(f32["g_b"], f64["g_b"]))
    if cin != 3:
        gx = bare_dgrad(case)
        assert tuple(gx.shape) == tuple(case["x"].shape)
        check(f"BARE K3 dX {name} {shape}", gx, f64["g_x"], R.rel_dist(f32["g_x"], f64["g_x"]))


# ------------------------------------------------------------------------------------------------ EXACT: integer inputs
@pytest.mark.parametrize("shape", [(2, 33, 130), (1, 17, 67)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name,cin,cout,k,bias", R.LAYERS, ids=LAYER_IDS)
def test_integer_inputs_are_exact(name, cin, cout, k, bias, shape):
    """Every product and partial sum is an integer below 2^20, so fp32 in any order equals float64: any wrong tap, channel, seam or halo
    index shows as a wrong integer."""
    case = gpu_case(cin, cout, k, bias, shape, seed=1, integer=True)
    f64 = R.layer_f64(case, device="cuda")
    # the sums of the absolute values bound every partial sum, whatever the order
    mags = R.layer_f64({key: (None if v is None else v.abs()) for key, v in case.items()}, device="cuda")
    top = max(mags[key].max().item() for key in ("g_w", "g_x") + (("g_b",) if bias else ()))
    print(f"EXACT {name} {shape}: largest sum of magnitudes {top:.0f}")
    assert top < 2 ** 20
    gw, gb = bare(case)
    assert torch.equal(gw.double(), f64["g_w"])
    if bias:
        assert torch.equal(gb.double(), f64["g_b"])
    if cin != 3:
        assert torch.equal(bare_dgrad(case).double(), f64["g_x"])


# ------------------------------------------------------------------------------------------------ PROBE: one-hot upstream gradients
PROBE_SHAPE = (1, 9, 70)
PROBES = [(4, 33), (0, 0), (0, 69), (8, 0), (8, 69), (3, 31), (4, 32), (3, 32), (4, 31), (7, 63), (8, 64)]


@pytest.mark.parametrize("name,cin,cout,k,bias", R.LAYERS, ids=LAYER_IDS)
def test_one_hot_probes(name, cin, cout, k, bias):
    """dY = 1 at one (co, y, x): dW[co] is the zero-padded k x k window of X around the pixel (for 1x1 the pixel's channel vector), db
    the one-hot, and dX the weight scattered around the pixel (for 1x1 the weight's row co at the pixel), all exactly."""
    _, H, W = PROBE_SHAPE
    case = gpu_case(cin, cout, k, bias, PROBE_SHAPE, seed=2)
    xp = torch.nn.functional.pad(case["x"], (k // 2,) * 4)
    for i, (y, x) in enumerate(PROBES):
        co = (5 * i + 3) % cout
        case["gy"] = torch.zeros(cout, 1, H, W, device="cuda")
        case["gy"][co, 0, y, x] = 1.0
        gw, gb = bare(case)
        want = torch.zeros_like(gw)
        want[co] = xp[:, 0, y:y + k, x:x + k]
        assert torch.equal(gw, want), (name, y, x)
        if bias:
            assert torch.equal(gb, torch.nn.functional.one_hot(torch.tensor(co), cout).float().cuda())
        if cin != 3:
            gx = bare_dgrad(case)
            wantx = torch.zeros(cin, 1, H + 2, W + 2, device="cuda")   # a frame around the plane takes what falls outside
            h = k // 2
            wantx[:, 0, y + 1 - h:y + 2 + h, x + 1 - h:x + 2 + h] = case["w"][co]   # dX[ci][y + ky - h][x + kx - h] = w[co][ci][ky][kx]
            assert torch.equal(gx, wantx[:, :, 1:-1, 1:-1]), (name, y, x)
    print(f"PROBE {name}: {len(PROBES)} one-hot gradients exact (interior, corners, tile seams)")


# ------------------------------------------------------------------------------------------------ GRID: shares, workspace, accumulate
@pytest.mark.parametrize("shape", [(3, 40, 300), (1, 9, 40)], ids=["many_tiles", "few_tiles"])
@pytest.mark.parametrize("name,cin,cout,k,bias", R.LAYERS, ids=LAYER_IDS)
def test_grid_workspace_and_accumulate(name, cin, cout, k, bias, shape):
    from dmvsnet_amd import _lib, ops
    plan = _lib.load().dmvs_conv2d_wgrad_fpn_plan(cin, cout, k, *shape)
    tiles, wgs = plan // 512, plan % 512
    print(f"GRID {name} {shape}: {tiles} tiles, {wgs} workgroups")
    assert wgs <= 256 and (tiles > 256 if shape[0] == 3 else tiles < 256)
    case = gpu_case(cin, cout, k, bias, shape, seed=3)
    f64, f32 = R.layer_f64(case, device="cuda"), R.layer_f64(case, torch.float32, device="cuda")
    gw, gb = bare(case)
    check(f"GRID K3f dW {name} {shape}", gw, f64["g_w"], R.rel_dist(f32["g_w"], f64["g_w"]))
    if bias:
        check(f"GRID K3f db {name} {shape}", gb, f64["g_b"], R.rel_dist(f32["g_b"], f64["g_b"]))
    # a user workspace (poisoned) gives the cached one's bits
    ws = torch.full((_lib.load().dmvs_conv2d_wgrad_fpn_workspace(cin, cout, k, *shape) + 3,), float("nan"), device="cuda")
    gw2, gb2 = bare(case, workspace=ws)
    assert torch.equal(gw2, gw) and (not bias or torch.equal(gb2, gb))
    # accumulate on integer inputs: the sum of two calls, bit for bit
    a, b = (gpu_case(cin, cout, k, bias, shape, seed=s, integer=True) for s in (4, 5))
    (gwa, gba), (gwb, gbb) = bare(a), bare(b)
    acc_w, acc_b = gwa.clone(), (gba.clone() if bias else None)
    bare(b, out=acc_w, bias_out=acc_b, accumulate=True)
    assert torch.equal(acc_w, gwa + gwb) and (not bias or torch.equal(acc_b, gba + gbb))


# ------------------------------------------------------------------------------------------------ the modules
@pytest.mark.parametrize("name,cin,cout,k,bias", R.LAYERS, ids=LAYER_IDS)
def test_forward_identity_and_reproducibility(name, cin, cout, k, bias):
    """The module's output is ops.conv3d on the host-packed layer, bit for bit; two runs of forward + backward are the same bits."""
    from dmvsnet_amd import ops
    shape = (2, 18, 70)
    case = gpu_case(cin, cout, k, bias, shape, seed=6)
    m = make_module(case)
    y, gx, gw, gb = module_run(m, case)
    scale = None if not bias else torch.ones(cout, device="cuda")
    layer = ops.make_layer(name, ops.CONV_S1 if k == 3 else ops.CONV2D_K1, case["w"], scale, case["bias"], False)
    for b in range(shape[0]):
        if cin == 3:
            want = ops.conv3d(case["x"][:, b].unsqueeze(0).contiguous(), layer, backend="mfma", in_views=True)
        else:
            want = ops.conv3d(case["x"][:, b:b + 1].contiguous(), layer, backend="mfma")
        assert torch.equal(y[b], want[:, 0]), (name, b)
    y2, gx2, gw2, gb2 = module_run(m, case)
    assert torch.equal(y2, y) and torch.equal(gw2, gw) and (gx is None or torch.equal(gx2, gx)) and (gb is None or torch.equal(gb2, gb))
    print(f"FWD {name}: identical to ops.conv3d on the host-packed layer; forward + backward reproducible")
    with pytest.raises(RuntimeError):   # once_differentiable
        xx = R.planes(case["x"]).contiguous().requires_grad_(cin != 3)
        (g1,) = torch.autograd.grad(m(xx), [m.weight], R.planes(case["gy"]).contiguous(), create_graph=True)
        g1.sum().backward()


@pytest.mark.parametrize("name,cin,cout,k,bias", R.LAYERS, ids=LAYER_IDS)
def test_layer_parity_against_float64(name, cin, cout, k, bias):
    shape = (2, 17, 67)
    case = gpu_case(cin, cout, k, bias, shape, seed=7)
    f64, f32 = R.layer_f64(case, device="cuda"), R.layer_f64(case, torch.float32, device="cuda")
    y, gx, gw, gb = module_run(make_module(case), case)
    check(f"PARITY {name} y", R.planes(y), f64["y"], R.rel_dist(f32["y"], f64["y"]))
    check(f"PARITY {name} dW", gw, f64["g_w"], R.rel_dist(f32["g_w"], f64["g_w"]))
    if bias:
        check(f"PARITY {name} db", gb, f64["g_b"], R.rel_dist(f32["g_b"], f64["g_b"]))
    if cin != 3:
        check(f"PARITY {name} dX", R.planes(gx), f64["g_x"], R.rel_dist(f32["g_x"], f64["g_x"]))


@pytest.mark.parametrize("name,cin,cout,k,bias", [R.LAYERS[1], R.LAYERS[4]], ids=["conv0.1", "inner1"])
def test_cache_follows_in_place_changes_and_copies(name, cin, cout, k, bias):
    shape = (1, 9, 40)
    case = gpu_case(cin, cout, k, bias, shape, seed=8, integer=True)
    m = make_module(case)
    module_run(m, case)   # fills the cache
    with torch.no_grad():
        m.weight.mul_(2.0)
        if bias:
            m.bias.add_(1.0)
    case["w"] = case["w"] * 2.0
    if bias:
        case["bias"] = case["bias"] + 1.0
    f64 = R.layer_f64(case, device="cuda")
    y, gx, _, _ = module_run(m, case)
    assert torch.equal(R.planes(y).double(), f64["y"]) and torch.equal(R.planes(gx).double(), f64["g_x"])
    m2 = copy.deepcopy(m)
    m3 = make_module(gpu_case(cin, cout, k, bias, shape, seed=9))
    m3.load_state_dict(m.state_dict())
    for other in (m2, m3):
        yo, gxo, gwo, _ = module_run(other, case)
        assert torch.equal(yo, y) and torch.equal(gxo, gx) and torch.equal(gwo.double(), f64["g_w"])
    print(f"CACHE {name}: in-place weight / bias changes seen; deepcopy and state-dict round trip run as the original")


# ------------------------------------------------------------------------------------------------ blocks and the whole network
def compare_net(tag, got, f64, ref, keys_out=R.OUT_KEYS):
    worst = 0.0
    for k in keys_out:
        worst = max(worst, check(f"{tag} out {k}", got["out"][k], f64["out"][k], R.rel_dist(ref["out"][k], f64["out"][k])))
    for k in f64["g"]:
        worst = max(worst, check(f"{tag} g {k}", got["g"][k], f64["g"][k], R.rel_dist(ref["g"][k], f64["g"][k])))
    return worst


def diff_net(case, train=True):
    from dmvsnet_amd import DiffFeatureNet
    net = DiffFeatureNet(8)
    net.load_state_dict(case["sd"], strict=True)
    return net.cuda().train(train)


def run_diff_net(net, case):
    """The differentiable network on the case, its ReLU masks (through forward hooks on the BatchNorm + ReLU modules) included."""
    masks, hooks = {}, []
    for lvl in ("conv0", "conv1", "conv2"):
        for i, blk in enumerate(getattr(net, lvl)):
            hooks.append(blk.bn.register_forward_hook(lambda mod, inp, out, key=f"{lvl}.{i}": masks.__setitem__(key, out.detach() > 0)))
    got = R.run_module(net, case, device="cuda")
    for h in hooks:
        h.remove()
    got["masks"] = masks
    return got


def test_conv0_blocks_against_float64_and_the_recorded_gradients(g):
    """conv0 as its two blocks with train-mode BatchNorm, taken alone: the upstream gradient is the one that reaches conv0's output in
    the float64 run of the whole network, so the blocks' parameter gradients are the network's -- the recorded ones included."""
    from dmvsnet_amd import DiffFeatureConvBlock2d
    case = R.golden_case(g, "b2_16x24")
    f64, aten = R.run_net(case, device="cuda"), R.run_net(case, torch.float32, "cuda")
    blocks = torch.nn.Sequential(DiffFeatureConvBlock2d(3, 8, 3, 1, padding=1), DiffFeatureConvBlock2d(8, 8, 3, 1, padding=1))
    blocks.load_state_dict({k[len("conv0."):]: v for k, v in case["sd"].items() if k.startswith("conv0.")}, strict=True)
    blocks = blocks.cuda().train()
    keys = [k for k in R.param_keys() if k.startswith("conv0.")]
    assert [n for n, _ in blocks.named_parameters()] == [k[len("conv0."):] for k in keys]
    out = blocks(case["x"].cuda())
    got = torch.autograd.grad(out, list(blocks.parameters()), f64["g_conv0"].float())
    check("PARITY conv0 blocks out", out.detach(), f64["conv0"], R.rel_dist(aten["conv0"], f64["conv0"]))
    for k, a in zip(keys, got):
        check(f"PARITY conv0 blocks g {k} vs fp32 ATen restatement", a, f64["g"][k], R.rel_dist(aten["g"][k], f64["g"][k]))
        check(f"PARITY conv0 blocks g {k} vs recorded reference", a, f64["g"][k], R.rel_dist(case["g"][k], f64["g"][k]))


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_whole_network_against_float64_aten_and_the_recorded_results(g, name):
    case = R.golden_case(g, name)
    f64 = R.run_net(case, device="cuda")
    assert f64["nearest_kink"] > R.KINK_MARGIN
    aten = R.run_net(case, torch.float32, "cuda")
    got = run_diff_net(diff_net(case), case)
    assert all(torch.equal(got["masks"][k], f64["masks"][k]) for k in f64["masks"])
    w1 = compare_net(f"WHOLE {name} vs fp32 ATen restatement", got, f64, aten)
    w2 = compare_net(f"WHOLE {name} vs recorded reference", got, f64, {"out": case["out"], "g": case["g"]})
    print(f"WHOLE {name}: worst e_hip {max(w1, w2):.3e}")


def test_whole_network_across_the_tile_seams():
    """(1, 36, 136): 34 / 68 / 136 columns cross the 32-column seam at all three pyramid levels."""
    case = R.make_net_case(seed=R.WIDE_SEED, **R.WIDE_CASE)
    f64 = R.run_net(case, device="cuda")
    print(f"WHOLE wide: nearest kink {f64['nearest_kink']:.3e}")
    assert f64["nearest_kink"] > R.WIDE_MARGIN
    aten = R.run_net(case, torch.float32, "cuda")
    got = run_diff_net(diff_net(case), case)
    assert all(torch.equal(got["masks"][k], f64["masks"][k]) for k in f64["masks"])
    compare_net("WHOLE wide", got, f64, aten)


def test_whole_network_in_eval_mode():
    case = R.eval_case()
    f64 = R.run_net(case, device="cuda", train=False)
    assert f64["nearest_kink"] > R.KINK_MARGIN
    aten = R.run_net(case, torch.float32, "cuda", train=False)
    net = diff_net(case, train=False)
    got = run_diff_net(net, case)
    assert all(torch.equal(got["masks"][k], f64["masks"][k]) for k in f64["masks"])
    compare_net("WHOLE eval", got, f64, aten)
    assert all(torch.equal(v.cpu(), case["sd"][k]) for k, v in net.state_dict().items() if "running" in k or "num_batches" in k)


def test_whole_network_is_reproducible_and_updates_running_statistics():
    case = R.make_net_case(**R.GOLDEN_CASES["b1_20x36"])
    a, b = (run_diff_net(diff_net(case), case) for _ in range(2))
    assert all(torch.equal(a["out"][k], b["out"][k]) for k in R.OUT_KEYS) and all(torch.equal(a["g"][k], b["g"][k]) for k in a["g"])
    net = diff_net(case)
    net(case["x"].cuda())
    assert int(net.conv0[0].bn.num_batches_tracked) == 1 and float(net.conv2[2].bn.running_mean.abs().max()) > 0


def test_refusals_launch_nothing():
    from dmvsnet_amd import DiffFeatureNet, ops
    from dmvsnet_amd._lib import DmvsError
    net = DiffFeatureNet(8).cuda()
    ops.launch_log = []
    try:
        z = lambda *s, **kw: torch.zeros(*s, device="cuda", **kw)   # noqa: E731
        for bad in (z(1, 3, 18, 24), z(1, 3, 16, 26), z(1, 4, 16, 24), z(3, 16, 24), z(1, 3, 16, 24, dtype=torch.float16),
                    z(1, 3, 16, 48)[..., ::2]):
            with pytest.raises(DmvsError):
                net(bad)
        with pytest.raises(DmvsError, match="no CPU fallback"):
            net(torch.zeros(1, 3, 16, 24))
        with pytest.raises(DmvsError, match="no data gradient"):
            net(torch.zeros(1, 3, 16, 24, device="cuda", requires_grad=True))
        assert ops.launch_log == []
    finally:
        ops.launch_log = None
