"""K5 (train- and eval-mode BatchNorm + ReLU, forward and backward), ``DiffBatchNormReLU3d`` / ``DiffBatchNormReLU2d`` and the four
blocks ``DiffConvBlock*`` / ``DiffDeconvBlock*`` on the MI355X.

Yardsticks, none of which is the code under test: the float64 restatement (tests/bn_grad_ref.py; checked against float64 autograd of
F.batch_norm + relu in tests/test_bn_grad_cpu.py), the fp32 run of stock ATen on the CPU for the bare operator, and the reference's
recorded fp32 block results (tests/golden/op_conv_grad.npz, op_conv_s2_grad.npz).  No test reads the reference or the oracle.

  criterion  per tensor: e = max-abs distance to the float64 restatement over the tensor's max-abs; e_hip <= 8 e_ref, and where
             e_ref < 4 * 2^-23 the bound is 16 * 2^-23 (the project's criterion, K3g / K3h).
  exact      the recomputed ReLU mask against the forward's output (integer sums), reproducibility with a NaN-filled workspace, the
             block with the reference's in-place ReLU left in, untouched running buffers in eval mode: torch.equal.

Shapes come from ``ops.bn_plan`` and ``ops.BN_CHUNK`` / ``ops.BN_MAX_WG`` (tests/bn_grad_ref.py: bare_volumes, grid_shape).  ReLU is
compared only on inputs without a pre-activation within 1e-5 of the kink (asserted); the 16 M-element GRID shapes have 9 to 24 such
values per channel at any seed, so their parity runs without ReLU and their mask is checked exactly instead.

Every test prints its figures before it asserts (BARE / OFFSET / GRID / MASK / STATS / EVAL / PARITY / CHAIN lines);
docs/kernels/K5_batchnorm_relu.md keeps the measured ones.  No test provokes a fault."""
import gc

import pytest
import torch
from torch import nn
import torch.nn.functional as F

import bn_grad_ref as R
import conv_grad_ref as R1
import conv_s2_grad_ref as R2

pytestmark = pytest.mark.gpu

FACTOR = 8.0
EPS32 = 2.0 ** -23
TENSORS = ("y", "g_x", "g_gamma", "g_beta", "mean", "invstd")


@pytest.fixture(autouse=True)
def free_gpu_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def bound_of(e_ref):
    return FACTOR * e_ref if e_ref >= 4 * EPS32 else 16 * EPS32


def chunk_constants():
    from dmvsnet_amd import ops
    return ops.BN_CHUNK, ops.BN_MAX_WG


def volumes():
    return R.bare_volumes(chunk_constants()[0])


def make_module(C, nd, relu=True, momentum=0.1, gamma=None, beta=None):
    from dmvsnet_amd import DiffBatchNormReLU2d, DiffBatchNormReLU3d
    m = (DiffBatchNormReLU3d if nd == 3 else DiffBatchNormReLU2d)(C, momentum=momentum, relu=relu).cuda()
    with torch.no_grad():
        if gamma is not None:
            m.weight.copy_(gamma)
        if beta is not None:
            m.bias.copy_(beta)
    return m


def run_module(m, x, gy):
    """One forward + backward of the module on device tensors -> the six compared tensors."""
    m.zero_grad()
    xin = x.detach().requires_grad_(True)
    y = m(xin)
    mean, invstd = (t.clone() for t in y.grad_fn.saved_tensors[3:5])
    y.backward(gy)
    return dict(y=y.detach(), g_x=xin.grad, g_gamma=m.weight.grad.clone(), g_beta=m.bias.grad.clone(), mean=mean, invstd=invstd)


def compare(tag, got, f64, ref, keys=TENSORS):
    rows = []
    for k in keys:
        e_hip, e_ref = R.rel_dist(got[k].reshape(f64[k].shape), f64[k]), R.rel_dist(ref[k].reshape(f64[k].shape), f64[k])
        rows.append((k, e_hip, e_ref))
        print(f"{tag} {k}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {bound_of(e_ref):.3e}  (max {f64[k].abs().max().item():.3e})")
    for k, e_hip, e_ref in rows:
        assert got[k].dtype == torch.float32 and torch.isfinite(got[k]).all(), (tag, k)
        assert e_hip <= bound_of(e_ref), (tag, k, e_hip, e_ref)


def bare_case(C, nd, vol, offset):
    B, spatial = volumes()[vol]
    seed = R.first_clean_seed(C, B, spatial, offset)
    case = R.make_case(C, B, spatial, seed, offset)
    assert R.kink_violations(case) == 0
    if nd == 2:
        shape = (B, C) + R.spatial_2d(spatial)
        case = dict(case, x=case["x"].reshape(shape), gy=case["gy"].reshape(shape))
    return case, seed


def check_bare(tag, C, nd, vol, offset):
    from dmvsnet_amd import ops
    case, seed = bare_case(C, nd, vol, offset)
    B, V = case["x"].shape[0], case["x"][0, 0].numel()
    f64, ref = R.all_f64(**case), R.aten_fp32(**case)
    m = make_module(C, nd, True, 0.1, case["gamma"], case["beta"])
    got = run_module(m, case["x"].cuda(), case["gy"].cuda())
    print(f"{tag} C {C} {nd}D {vol} B {B} V {V} seed {seed}: S {ops.bn_plan(C, B, V)}, {'16-byte' if V % 4 == 0 else 'scalar'} path")
    compare(f"{tag} C {C} {nd}D {vol}", got, f64, ref)


# ------------------------------------------------------------------------------------------------ bare operator against float64
@pytest.mark.parametrize("vol", list(R.bare_volumes(1024)))
@pytest.mark.parametrize("nd", (3, 2))
@pytest.mark.parametrize("C", R.CHANNELS)
def test_bare_against_float64(C, nd, vol):
    assert list(volumes()) == list(R.bare_volumes(1024))   # (the ids above are names only; the shapes come from the chunk constant)
    check_bare("BARE", C, nd, vol, 0.0)


@pytest.mark.parametrize("vol", list(R.bare_volumes(1024)))
@pytest.mark.parametrize("nd", (3, 2))
@pytest.mark.parametrize("C", R.CHANNELS)
def test_offset_input(C, nd, vol):
    """x = 50 + N(0, 1): mean^2 / var = 2500.  A raw E[x^2] - E[x]^2 misses this bound by a factor of 20 and more."""
    check_bare("OFFSET", C, nd, vol, 50.0)


@pytest.mark.parametrize("C", (8, 32))
def test_unaligned_base_pointer(C):
    """A contiguous view at storage offset 1 (4 bytes past a 16-byte boundary) with V % 4 == 0: the scalar path, chosen by alignment."""
    case, _ = bare_case(C, 3, "3x10x18", 0.0)
    f64, ref = R.all_f64(**case), R.aten_fp32(**case)
    n = case["x"].numel()
    xbuf, gbuf = torch.zeros(n + 1, device="cuda"), torch.zeros(n + 1, device="cuda")
    x, gy = xbuf[1:].view(case["x"].shape), gbuf[1:].view(case["x"].shape)
    x.copy_(case["x"]), gy.copy_(case["gy"])
    assert x.is_contiguous() and x.data_ptr() % 16 == 4 and gy.data_ptr() % 16 == 4
    m = make_module(C, 3, True, 0.1, case["gamma"], case["beta"])
    got = run_module(m, x, gy)
    compare(f"BARE C {C} unaligned", got, f64, ref)
    aligned = run_module(m, case["x"].cuda(), case["gy"].cuda())
    for k in ("y", "g_x"):   # both paths are correct; they need not be equal in bits, but the mask must agree
        assert torch.equal(got[k] == 0, aligned[k] == 0)


# ------------------------------------------------------------------------------------------------ grid-size cases
_grid_cache = {}


def grid_case(C):
    """The GRID shape's inputs on the device (shared by the parity and the mask test; never modified)."""
    if C not in _grid_cache:
        from dmvsnet_amd import ops
        chunk, max_wg = chunk_constants()
        B, spatial = R.grid_shape(C, chunk, max_wg)
        V = R.volume(spatial)
        S = ops.bn_plan(C, B, V)
        assert B == 2 and S == max_wg // C and B * V >= 2 * chunk * S and V % 4 == 0
        inside = [s for s in range(S) if ops.bn_share_range(C, B, V, s)[0] < V < ops.bn_share_range(C, B, V, s)[1]]
        assert len(inside) == 1, "the sample boundary must fall inside a share"
        case = R.make_case(C, B, spatial, 0)
        _grid_cache[C] = (B, V, S, {k: v.cuda() for k, v in case.items()})
    return _grid_cache[C]


@pytest.mark.parametrize("C", (8, 64))
def test_full_grid_parity_and_reproducibility(C):
    """S == Smax, several chunks per share, a sample boundary inside a share; without ReLU (see the module text).  The cached
    workspace is NaN-filled before each of the two runs: every partial that is read was written, and the bits repeat."""
    from dmvsnet_amd import ops
    B, V, S, case = grid_case(C)
    print(f"GRID C {C}: B {B} V {V} ({B * C * V / 1e6:.1f} M floats), S {S}, {(B * V + ops.BN_CHUNK - 1) // ops.BN_CHUNK} chunks per channel")
    m = make_module(C, 3, False, 0.1, case["gamma"], case["beta"])
    x = case["x"]
    ws = ops.bn_workspace(C, B, V, x.device)   # the cached buffer the module's calls get: same key, same storage
    assert ws.data_ptr() == ops.bn_workspace(C, B, V, x.device).data_ptr() == ops.bn_workspace(C, B, V, "cuda").data_ptr()
    used = 2 * C * S + C                       # [C][S][2] partials and [C] pivots
    runs = []
    for _ in range(2):
        ws.fill_(float("nan"))
        runs.append(run_module(m, x, case["gy"]))
        assert torch.isfinite(ws[:2 * C * S]).all(), "the module did not write its partials into the NaN-filled workspace"
        assert torch.isnan(ws[used:]).all(), "the kernels wrote past the part of the workspace they own"
    for k in TENSORS:
        assert torch.equal(runs[0][k], runs[1][k]), f"{k} differs between two runs"
    # the same through ops with an explicit NaN-filled workspace: same bits as the module's path, nothing read that was not written
    own = torch.full((ws.numel(),), float("nan"), device=x.device)
    y, mean, invstd = ops.bn_relu_forward(x, m.weight.detach(), m.bias.detach(), torch.zeros(C, device=x.device), torch.ones(C, device=x.device),
                                          0.1, m.eps, False, True, workspace=own)
    assert torch.isfinite(own[:used]).all() and torch.isnan(own[used:]).all()   # forward: partials and pivots
    own.fill_(float("nan"))
    gx, gg, gb = ops.bn_relu_backward(x, case["gy"], m.weight.detach(), m.bias.detach(), mean, invstd, False, True, True, workspace=own)
    assert torch.isfinite(own[:2 * C * S]).all() and torch.isnan(own[2 * C * S:]).all()
    for k, t in (("y", y), ("mean", mean), ("invstd", invstd), ("g_x", gx), ("g_gamma", gg), ("g_beta", gb)):
        assert torch.equal(t, runs[0][k]), f"{k}: explicit workspace and cached workspace give different bits"
    print(f"GRID C {C} workspace: {ws.numel()} floats NaN-filled before each run, {used} written, two module runs and the explicit-workspace "
          "run equal in bits")
    cpu = {k: v.cpu() for k, v in case.items()}
    f64, ref = R.all_f64(relu=False, **cpu), R.aten_fp32(relu=False, **cpu)
    compare(f"GRID C {C}", runs[0], f64, ref)


@pytest.mark.parametrize("C", (8, 64))
def test_recomputed_mask_is_the_forwards(C):
    """relu=True, gy = ones: g_beta[c] is the number of elements the backward lets through, y > 0 the number the forward did.  Integer
    sums below 2^24 are exact under any association, so the two are EQUAL unless a single mask bit differs."""
    B, V, S, case = grid_case(C)
    assert B * V < (1 << 24)
    m = make_module(C, 3, True, 0.1, case["gamma"], case["beta"])
    got = run_module(m, case["x"], torch.ones_like(case["x"]))
    want = (got["y"] > 0).transpose(0, 1).reshape(C, -1).sum(1)
    diff = (got["g_beta"].double() - want.double()).abs().max().item()
    print(f"MASK C {C}: {int(want.sum())} of {B * C * V} pass, max |g_beta - count| = {diff}")
    assert torch.equal(got["g_beta"].double(), want.double())
    assert 0 < int(want.min()) and int(want.max()) < B * V


# ------------------------------------------------------------------------------------------------ running statistics and eval mode
@pytest.mark.parametrize("momentum", (0.1, 0.01))
@pytest.mark.parametrize("C,nd", ((8, 3), (64, 2)))
def test_running_statistics(C, nd, momentum):
    B, spatial = 2, (3, 10, 18)
    shape = (B, C) + (spatial if nd == 3 else R.spatial_2d(spatial))
    m = make_module(C, nd, True, momentum)
    ref = (nn.BatchNorm3d if nd == 3 else nn.BatchNorm2d)(C, momentum=momentum).train()
    rm64, rv64 = ref.running_mean.double(), ref.running_var.double()
    rows = []
    for step in (1, 2):
        x = R.make_case(C, B, spatial, 10 + step, offset=0.5 * step)["x"].reshape(shape) * (1.0 + step)
        m(x.cuda())
        ref(x)
        rm64, rv64 = R.running_update(rm64, rv64, x, momentum)
        for k, got, r32, r64 in (("running_mean", m.running_mean, ref.running_mean, rm64), ("running_var", m.running_var, ref.running_var, rv64)):
            rows.append((f"step {step} {k}", R.rel_dist(got, r64), R.rel_dist(r32, r64)))
        assert int(m.num_batches_tracked) == step and m.num_batches_tracked.is_cuda
    for k, e_hip, e_ref in rows:
        print(f"STATS C {C} {nd}D momentum {momentum} {k}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {bound_of(e_ref):.3e}")
    for k, e_hip, e_ref in rows:
        assert e_hip <= bound_of(e_ref), (k, e_hip, e_ref)


@pytest.mark.parametrize("relu", (True, False))
@pytest.mark.parametrize("C,nd,vol", ((8, 3, "2x5x9_b2"), (16, 2, "3x10x18"), (64, 3, "3chunk+1")))
def test_eval_mode(C, nd, vol, relu):
    B, spatial = volumes()[vol]
    g = torch.Generator().manual_seed(C + nd)
    rm, rv = 0.3 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    for seed in range(20):
        case = R.make_case(C, B, spatial, seed)
        if R.kink_violations(case, mean=rm, var=rv) == 0:
            break
    assert R.kink_violations(case, mean=rm, var=rv) == 0
    if nd == 2:
        shape = (B, C) + R.spatial_2d(spatial)
        case = dict(case, x=case["x"].reshape(shape), gy=case["gy"].reshape(shape))
    m = make_module(C, nd, relu, 0.1, case["gamma"], case["beta"])
    with torch.no_grad():
        m.running_mean.copy_(rm), m.running_var.copy_(rv)
    m.eval()
    got = run_module(m, case["x"].cuda(), case["gy"].cuda())
    f64, ref = R.all_f64(relu=relu, mean=rm, var=rv, **case), R.aten_fp32(relu=relu, mean=rm, var=rv, **case)
    compare(f"EVAL C {C} {nd}D {vol} relu {relu}", got, f64, ref)
    assert torch.equal(m.running_mean.cpu(), rm) and torch.equal(m.running_var.cpu(), rv) and int(m.num_batches_tracked) == 0


# ------------------------------------------------------------------------------------------------ parity on the golden blocks
@pytest.fixture(scope="module")
def goldens(golden):
    return {"s1": golden("op_conv_grad.npz"), "s2": golden("op_conv_s2_grad.npz")}


GOLDEN_IDS = [("s1", n) for n in R1.GOLDEN_CASES] + [("s2", n) for n in R2.GOLDEN_CASES]


@pytest.mark.parametrize("family,name", GOLDEN_IDS)
def test_block_parity_golden_cases(goldens, family, name):
    """Whole reference blocks (layer + train-mode BatchNorm + ReLU) on the gfx950 kernels in both directions, against the reference's
    recorded fp32 run."""
    import dmvsnet_amd as da
    Rk = R1 if family == "s1" else R2
    case = Rk.golden_case(goldens[family], name)
    assert Rk.kink_violations(case) == 0
    f64 = Rk.block_f64(case)
    kd = case["kd"]
    if family == "s1":
        C = case["C"]
        blk = (da.DiffConvBlock3d if kd == 3 else da.DiffConvBlock2d)(C, C, 3, padding=1)
    elif case["mode"] == "conv":
        blk = (da.DiffConvBlock3d if kd == 3 else da.DiffConvBlock2d)(case["Cb"], 2 * case["Cb"], 3, stride=2, padding=1)
    else:
        blk = (da.DiffDeconvBlock3d if kd == 3 else da.DiffDeconvBlock2d)(2 * case["Cb"], case["Cb"], 3, stride=2, padding=1, output_padding=1)
    blk = blk.cuda().train()
    assert blk.bn.eps == Rk.BN_EPS
    with torch.no_grad():
        blk.conv.weight.copy_(case["w"].reshape(blk.conv.weight.shape))
        blk.bn.weight.copy_(case["gamma"]), blk.bn.bias.copy_(case["beta"])
    sq = (lambda t: t) if kd == 3 else (lambda t: t.squeeze(2))
    x = sq(case["x"].cuda()).contiguous().requires_grad_(True)
    out = blk(x)
    out.backward(sq(case["gy"].cuda()).contiguous())
    got = dict(out=out.detach(), g_x=x.grad, g_w=blk.conv.weight.grad, g_gamma=blk.bn.weight.grad, g_beta=blk.bn.bias.grad)
    rows = []
    for k in ("out", "g_x", "g_w", "g_gamma", "g_beta"):
        e_ref, e_hip = Rk.rel_dist(case[k], f64[k]), Rk.rel_dist(got[k].reshape(f64[k].shape), f64[k])
        rows.append((k, e_hip, e_ref))
        print(f"PARITY {name} {k}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {bound_of(e_ref):.3e}  (max {f64[k].abs().max().item():.3e})")
    for k, e_hip, e_ref in rows:
        assert e_hip <= bound_of(e_ref), (name, k, e_hip, e_ref)


# ------------------------------------------------------------------------------------------------ the whole U-Net
class DiffCostRegNetPart(nn.Module):
    """CostRegNet_part of the reference, base 8 channels: conv1 .. conv11 on the Diff blocks, conv0 the ATen conv with
    DiffBatchNormReLU3d (the reference's block with only .bn swapped, its ReLU left in), prob on ATen.  Parameter names are those of
    tests/test_conv_s2_grad_gpu.py::CostRegNetPart."""

    def __init__(self, in_channels=8, base=8):
        super().__init__()
        import dmvsnet_amd as da
        import test_conv_s2_grad_gpu as S2
        s1 = lambda c: da.DiffConvBlock3d(c, c, 3, padding=1)
        dn = lambda c: da.DiffConvBlock3d(c, 2 * c, 3, stride=2, padding=1)
        up = lambda c: da.DiffDeconvBlock3d(2 * c, c, 3, stride=2, padding=1, output_padding=1)
        self.conv0 = S2.Block(nn.Conv3d(in_channels, base, 3, padding=1, bias=False))
        self.conv0.bn = da.DiffBatchNormReLU3d(base)
        self.conv1, self.conv2 = dn(base), s1(2 * base)
        self.conv3, self.conv4 = dn(2 * base), s1(4 * base)
        self.conv5, self.conv6 = dn(4 * base), s1(8 * base)
        self.conv7, self.conv9, self.conv11 = up(4 * base), up(2 * base), up(base)
        self.prob = nn.Conv3d(base, 2, 3, stride=1, padding=1, bias=False)

    def forward(self, x):
        conv0 = self.conv0(x)
        conv2 = self.conv2(self.conv1(conv0))
        conv4 = self.conv4(self.conv3(conv2))
        x = self.conv6(self.conv5(conv4))
        x = conv4 + self.conv7(x)
        x = conv2 + self.conv9(x)
        x = conv0 + self.conv11(x)
        return self.prob(x)


def test_costregnet_part_chain():
    """The whole CostRegNet_part at fine 8 x 16 x 32 through .backward(): every block on the gfx950 kernels in both directions, the
    skip additions, conv0's convolution and prob on ATen; against the all-ATen chain in fp32 (CPU) and float64 (CPU), on inputs that meet
    the kink condition."""
    import test_conv_s2_grad_gpu as S2
    x, gy, weights = S2.chain_inputs(S2.CHAIN_SEED)
    o64, g64, pre64 = S2.run_chain(False, torch.float64, "cpu", x, gy, weights)
    assert all((p.abs() > R.KINK_MARGIN).all() for p in pre64), "a BatchNorm output sits on the ReLU kink: pick another seed"
    o32, g32, _ = S2.run_chain(False, torch.float32, "cpu", x, gy, weights)
    net = DiffCostRegNetPart()
    net.load_state_dict(weights)
    net = net.cuda().train()
    xin = x.cuda().requires_grad_(True)
    out = net(xin)
    out.backward(gy.cuda())
    ghip = {"x": xin.grad, **{n: p.grad for n, p in net.named_parameters()}}
    assert set(ghip) == set(g64)
    rows = [("out", R.rel_dist(out, o64), R.rel_dist(o32, o64))] + [(k, R.rel_dist(ghip[k], g64[k]), R.rel_dist(g32[k], g64[k])) for k in g64]
    for k, e_hip, e_ref in rows:
        print(f"CHAIN {k}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {bound_of(e_ref):.3e}")
    for k, e_hip, e_ref in rows:
        assert e_hip <= bound_of(e_ref), (k, e_hip, e_ref)
    assert all(int(m.num_batches_tracked) == 1 for m in net.modules() if isinstance(m, nn.BatchNorm3d))


# ------------------------------------------------------------------------------------------------ contract
def small_inputs(C=16, B=2, spatial=(2, 5, 9), seed=0):
    case = R.make_case(C, B, spatial, R.first_clean_seed(C, B, spatial))
    return case, case["x"].cuda(), case["gy"].cuda()


def test_frozen_parameters_and_frozen_input():
    from dmvsnet_amd import bn, ops
    case, x, gy = small_inputs()
    m = make_module(16, 3, True, 0.1, case["gamma"], case["beta"])
    full = run_module(m, x, gy)
    before = dict(bn.launch_counts)
    m.weight.requires_grad_(False), m.bias.requires_grad_(False)
    xin = x.clone().requires_grad_(True)
    m(xin).backward(gy)
    assert torch.equal(xin.grad, full["g_x"]) and m.weight.grad is not None   # (the earlier .grad stays; nothing new is added to it)
    assert bn.launch_counts == {"reduce": before["reduce"] + 1, "apply": before["apply"] + 1}
    m.weight.requires_grad_(True), m.bias.requires_grad_(True)
    m.zero_grad()
    before = dict(bn.launch_counts)
    ops.launch_log = log = []
    try:
        m(x).backward(gy)   # a frozen input: the apply launch is skipped, the fold kernel writes the two vectors
    finally:
        ops.launch_log = None
    assert bn.launch_counts == {"reduce": before["reduce"] + 1, "apply": before["apply"]}
    assert torch.equal(m.weight.grad, full["g_gamma"]) and torch.equal(m.bias.grad, full["g_beta"])
    assert log == ["batchnorm"] * 4   # one entry per dispatch: statistics, apply; reduce, fold
    m.eval()
    ops.launch_log = log = []
    try:
        m(x)
    finally:
        ops.launch_log = None
    assert log == ["batchnorm"]


def test_double_backward_raises_and_weight_change_raises():
    case, x, gy = small_inputs()
    m = make_module(16, 3, True, 0.1, case["gamma"], case["beta"])
    xin = x.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(m(xin), xin, gy, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()
    y = m(x.clone().requires_grad_(True))
    with torch.no_grad():
        m.weight.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        y.backward(gy)


def test_the_output_is_not_saved():
    case, x, gy = small_inputs()
    m = make_module(16, 3, True, 0.1, case["gamma"], case["beta"])
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = m(x.clone().requires_grad_(True))
    big = [t for t in saved if t.numel() == x.numel()]
    print(f"SAVED {[tuple(t.shape) for t in saved]}")
    assert len(big) == 1 and len(saved) == 5 and big[0].data_ptr() != y.data_ptr()
    y.backward(gy)


class RefStyleBlock(nn.Module):
    """The reference's block with only .bn swapped; ``inplace_relu`` keeps its ``F.relu(x, inplace=True)`` line."""

    def __init__(self, conv, bn, inplace_relu):
        super().__init__()
        self.conv, self.bn, self.inplace_relu = conv, bn, inplace_relu

    def forward(self, x):
        x = self.bn(self.conv(x))
        if self.inplace_relu:
            x = F.relu(x, inplace=True)
        return x


def test_reference_block_with_its_inplace_relu_left_in():
    from dmvsnet_amd import DiffBatchNormReLU3d
    g = torch.Generator().manual_seed(11)
    x, gy = torch.randn(2, 8, 4, 6, 10, generator=g).cuda(), torch.randn(2, 8, 4, 6, 10, generator=g).cuda()
    conv = nn.Conv3d(8, 8, 3, padding=1, bias=False)
    runs = []
    for inplace in (True, False):
        blk = RefStyleBlock(nn.Conv3d(8, 8, 3, padding=1, bias=False), DiffBatchNormReLU3d(8), inplace)
        blk.conv.load_state_dict(conv.state_dict())
        blk = blk.cuda().train()
        xin = x.clone().requires_grad_(True)
        out = blk(xin)
        out.backward(gy)
        runs.append((out.detach(), xin.grad, blk.conv.weight.grad, blk.bn.weight.grad, blk.bn.bias.grad, blk.bn.running_mean, blk.bn.running_var))
    assert (runs[0][0] == 0).any() and (runs[0][0] > 0).any()
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_non_contiguous_and_wrong_inputs_are_refused():
    from dmvsnet_amd._lib import DmvsError
    m = make_module(8, 3)
    for bad in (torch.zeros(1, 8, 2, 4, 6, device="cuda").transpose(3, 4), torch.zeros(1, 8, 4, 6, device="cuda"),
                torch.zeros(1, 16, 2, 4, 6, device="cuda"), torch.zeros(1, 8, 2, 4, 6, device="cuda", dtype=torch.float16),
                torch.zeros(1, 8, 1, 1, 1, device="cuda")):
        with pytest.raises(DmvsError):
            m(bad)
    assert int(m.num_batches_tracked) == 0
    m.eval()
    assert m(torch.zeros(1, 8, 1, 1, 1, device="cuda")).shape == (1, 8, 1, 1, 1)   # eval mode takes one value per channel
