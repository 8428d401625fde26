"""K2g (weight gradient of the 2-channel ends conv0 / prob), ``DiffConv3d(2, 8)`` / ``(8, 2)`` on K2 and the four regularisation
networks of dmvsnet_amd.regnet on the MI355X.

Yardsticks, none of which is the code under test: the float64 restatement (tests/regnet_grad_ref.py; checked against float64 autograd
of F.conv3d in tests/test_regnet_grad_cpu.py), the fp32 run of the same restatement on stock ATen, the stock-layer networks in float64
and the reference's recorded fp32 results (tests/golden/op_regnet_grad.npz, op_costreg.npz).  No test reads the reference or the oracle.

  criterion  K3g's (tests/test_conv_grad_gpu.py): per tensor e = max-abs distance to float64 over the tensor's max-abs; e_hip <= 8 e_ref,
             e_ref the fp32 yardstick's distance; where e_ref < 4 * 2^-23 the bound is 16 * 2^-23.
  exact      the one-hot probes, reproducibility, accumulate, batch = samples, poison, the forward and the data gradient against the
             host-packed K2 launches, cache invalidation: torch.equal.

Every test prints its figures before it asserts (BARE / GRID / PROBE / FWD / DGRAD / MODULE / NET / EVAL lines);
docs/kernels/K2g_conv_wgrad_c2.md is where measured ones are kept.  No test provokes a fault."""
import gc

import pytest
import torch

import regnet_grad_ref as R

pytestmark = pytest.mark.gpu

bound_of = R.bound_of

# the smallest volumes at which the kernel can go wrong (tile: 1 x 4 x 64 voxels)
VOLUMES = {
    "1x3x4": (1, 3, 4),        # below any tile; depth taps 0 and 2 see only padding: those 2 x 144 entries are exactly 0.0
    "2x5x9": (2, 5, 9),        # W % 4 != 0
    "3x10x18": (3, 10, 18),
    "2x5x67": (2, 5, 67),      # ragged against 32- and 64-wide tiles
}


@pytest.fixture(autouse=True)
def free_gpu_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def cuda_case(cin, cout, D, H, W, B=1, seed=0):
    return tuple(t.cuda() for t in R.rand_case(cin, cout, D, H, W, B, seed))


def hip_wgrad(x, gy, **kw):
    """K2g over a batch, its samples one after the other (accumulate from the second on)."""
    from dmvsnet_amd import ops
    gw = None
    for b in range(x.shape[0]):
        gw = ops.conv3d_wgrad_c2(x[b], gy[b], out=gw, accumulate=b > 0, **kw)
    return gw


def host_layer(w, transposed_flipped=False):
    """The bare K2 layer with the weight packed on the HOST by pack_direct (the eval path's packing)."""
    from dmvsnet_amd import ops
    wc = w.detach().cpu()
    src = wc.transpose(0, 1).flip(2, 3, 4).contiguous() if transposed_flipped else wc
    return ops.ConvLayer("host", ops.CONV_S1, 3, src.shape[1], src.shape[0], ops.pack_direct(src, False).cuda(), None, None, None, False)


def make_module(cin, cout, w):
    from dmvsnet_amd import DiffConv3d
    m = DiffConv3d(cin, cout, 3, stride=1, padding=1, bias=False).cuda()
    with torch.no_grad():
        m.weight.copy_(w)
    return m


def plan_of(cin, cout, D, H, W):
    from dmvsnet_amd import _lib
    plan = _lib.load().dmvs_conv3d_wgrad_c2_plan(cin, cout, D, H, W)
    assert plan > 0
    return plan >> 9, plan & 511


# ------------------------------------------------------------------------------------------------ bare kernel against float64
def check_wgrad(tag, x, gy, gw):
    f64 = R.wgrad_ref(x, gy)
    e_ref, e_hip = R.rel_dist(R.wgrad_ref(x, gy, torch.float32), f64), R.rel_dist(gw, f64)
    print(f"{tag}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {bound_of(e_ref):.3e}  (|dW| max {f64.abs().max().item():.3e})")
    assert gw.dtype == torch.float32 and tuple(gw.shape) == tuple(f64.shape)
    assert e_hip <= bound_of(e_ref), (tag, e_hip, e_ref)


@pytest.mark.parametrize("vol", list(VOLUMES))
@pytest.mark.parametrize("cin,cout", R.SHAPES)
def test_bare_wgrad_against_float64(cin, cout, vol):
    D, H, W = VOLUMES[vol]
    x, gy, _ = cuda_case(cin, cout, D, H, W)
    gw = hip_wgrad(x, gy)
    check_wgrad(f"BARE {cin} -> {cout} {vol}", x, gy, gw)
    if D == 1:   # taps kz = 0 and kz = 2 read the padding planes only
        assert torch.equal(gw[:, :, [0, 2]], torch.zeros(cout, cin, 2, 3, 3, device="cuda")) and gw[:, :, [0, 2]].numel() == 2 * 144


@pytest.mark.parametrize("cin,cout", R.SHAPES)
def test_fewer_tiles_than_workgroups(cin, cout):
    """The grid shrinks to the tiles: workgroups past the last share exit at once and own no partial -- a NaN-filled workspace must not
    reach the result."""
    from dmvsnet_amd import _lib
    vol = (3, 10, 18)
    tiles, wgs = plan_of(cin, cout, *vol)
    assert tiles < 256 and wgs < 256 and wgs - 8 < tiles <= wgs, (tiles, wgs)
    x, gy, _ = cuda_case(cin, cout, *vol, seed=1)
    ws = torch.full((_lib.load().dmvs_conv3d_wgrad_c2_workspace(cin, cout, *vol),), float("nan"), device="cuda")
    print(f"GRID {cin} -> {cout} {vol}: {tiles} tiles, {wgs} workgroups")
    check_wgrad(f"GRID {cin} -> {cout} {vol} tiles < workgroups", x, gy, hip_wgrad(x, gy, workspace=ws))


@pytest.mark.parametrize("cin,cout", R.SHAPES)
def test_more_tiles_than_workgroups(cin, cout):
    """Some share walks several tiles (and not all shares the same number)."""
    for vol in ((8, 36, 130), (8, 68, 130), (16, 68, 130)):
        tiles, wgs = plan_of(cin, cout, *vol)
        if tiles > 256 and tiles % 256:
            break
    else:
        pytest.fail("no shape of the list has more tiles than workgroups")
    assert wgs == 256
    x, gy, _ = cuda_case(cin, cout, *vol, seed=2)
    print(f"GRID {cin} -> {cout} {vol}: {tiles} tiles, {wgs} workgroups")
    check_wgrad(f"GRID {cin} -> {cout} {vol} tiles > workgroups", x, gy, hip_wgrad(x, gy))


# ------------------------------------------------------------------------------------------------ one-hot probes (exact)
@pytest.mark.parametrize("cin,cout", R.SHAPES)
def test_one_hot_probes(cin, cout):
    """One voxel of gy and one of x set to 1.0, the x voxel at every tap offset from the gy voxel -- at an interior position and at each
    of the eight corners: dW is a single 1.0 at [co][ci][kz][ky][kx] (all zeros where the offset leaves the volume).  Pins the role
    map, prob's tap flip and the halo without a tolerance."""
    from dmvsnet_amd import ops
    D, H, W = 3, 6, 70   # two tiles in x: the far corners sit in a ragged tile
    spots = [(1, 2, 5)] + [(z, y, xx) for z in (0, D - 1) for y in (0, H - 1) for xx in (0, W - 1)]
    x = torch.zeros(cin, D, H, W, device="cuda")
    gy = torch.zeros(cout, D, H, W, device="cuda")
    bad, n = [], 0
    for si, (z, y, xx) in enumerate(spots):
        for t in range(27):
            kz, ky, kx = t // 9, (t // 3) % 3, t % 3
            co, ci = (t + si) % cout, (t // 2 + si) % cin
            iz, iy, ix = z + kz - 1, y + ky - 1, xx + kx - 1   # dW[co][ci][t] = sum_v gy[co][v] * x[ci][v + t - 1]
            inside = 0 <= iz < D and 0 <= iy < H and 0 <= ix < W
            want = torch.zeros(cout, cin, 3, 3, 3, device="cuda")
            gy[co, z, y, xx] = 1.0
            if inside:
                x[ci, iz, iy, ix] = 1.0
                want[co, ci, kz, ky, kx] = 1.0
            got = ops.conv3d_wgrad_c2(x, gy)
            n += 1
            if not torch.equal(got, want):
                bad.append(((z, y, xx), (kz, ky, kx), co, ci, got.nonzero().tolist()))
            gy[co, z, y, xx] = 0.0
            if inside:
                x[ci, iz, iy, ix] = 0.0
    print(f"PROBE {cin} -> {cout}: {len(bad)} of {n} probes differ" + (f", first (spot, tap, co, ci, nonzeros) = {bad[0]}" if bad else ""))
    assert not bad


# ------------------------------------------------------------------------------------------------ reproducibility, accumulate, poison
@pytest.mark.parametrize("cin,cout", R.SHAPES)
def test_reproducible_accumulate_batch_and_poison(cin, cout):
    from dmvsnet_amd import _lib, ops
    D, H, W = 3, 10, 67
    x, gy, w = cuda_case(cin, cout, D, H, W, B=2, seed=3)
    nan = float("nan")
    a0, a1 = ops.conv3d_wgrad_c2(x[0], gy[0]).clone(), ops.conv3d_wgrad_c2(x[0], gy[0]).clone()
    assert torch.equal(a0, a1) and torch.isfinite(a0).all(), "two runs differ"
    b0 = ops.conv3d_wgrad_c2(x[1], gy[1]).clone()
    # accumulate: the sum of two separate results added in fp32
    acc = ops.conv3d_wgrad_c2(x[1], gy[1], out=a0.clone(), accumulate=True)
    assert torch.equal(acc, a0 + b0)
    # a batch of 2 through the module: sample-by-sample accumulation
    m = make_module(cin, cout, w)
    m(x).backward(gy)
    assert torch.equal(m.weight.grad, acc) and torch.equal(hip_wgrad(x, gy), acc)
    # NaN-filled out / workspace are fully overwritten where read
    ws = torch.full((_lib.load().dmvs_conv3d_wgrad_c2_workspace(cin, cout, D, H, W),), nan, device="cuda")
    got = ops.conv3d_wgrad_c2(x[0], gy[0], out=torch.full((cout, cin, 3, 3, 3), nan, device="cuda"), workspace=ws)
    assert torch.equal(got, a0)
    tiles, _ = plan_of(cin, cout, D, H, W)
    assert torch.isfinite(ws[:min(tiles, 256) * 432]).all(), "a share's partial was not fully written"
    with pytest.raises(_lib.DmvsError):
        ops.conv3d_wgrad_c2(x[0], gy[0], workspace=ws[:100])
    with pytest.raises(_lib.DmvsError):
        ops.conv3d_wgrad_c2(x[0], gy[0], accumulate=True)
    # the launch log carries the family once per dispatch
    ops.launch_log = log = []
    try:
        ops.conv3d_wgrad_c2(x[0], gy[0])
    finally:
        ops.launch_log = None
    assert log == ["conv3d_wgrad_c2", "conv3d_wgrad_c2"]


# ------------------------------------------------------------------------------------------------ modules
@pytest.mark.parametrize("vol", ["2x5x9", "3x10x18", "2x5x67"])
@pytest.mark.parametrize("cin,cout", R.SHAPES)
def test_module_forward_and_gradients(cin, cout, vol):
    """Forward = ops.conv3d(..., backend="direct") on the host-packed layer and data gradient = the host-packed launch of the
    transposed-flipped weight, bit for bit; forward, g_x and g_w against float64 under the criterion."""
    import torch.nn.functional as F
    from dmvsnet_amd import ops
    D, H, W = VOLUMES[vol]
    B = 2
    x, gy, w = cuda_case(cin, cout, D, H, W, B=B, seed=4)
    m = make_module(cin, cout, w)
    xin = x.clone().requires_grad_(True)
    y = m(xin)
    y.backward(gy)
    fwd, bwd = host_layer(w), host_layer(w, True)
    assert (fwd.cin, fwd.cout, bwd.cin, bwd.cout) == (cin, cout, cout, cin)
    want_y = torch.stack([ops.conv3d(x[b], fwd, backend="direct") for b in range(B)])
    want_gx = torch.stack([ops.conv3d(gy[b], bwd, backend="direct") for b in range(B)])
    assert torch.equal(y.detach(), want_y), "the forward is not the K2 launch on the host-packed weight"
    assert torch.equal(xin.grad, want_gx), "the data gradient is not the K2 launch on the host-packed transposed-flipped weight"
    rows = []
    for tag, got, f64, ref in (("FWD", y, R.conv_ref(x, w), F.conv3d(x, w, padding=1)),
                               ("DGRAD", xin.grad, R.dgrad_ref(gy, w), R.dgrad_ref(gy, w, torch.float32)),
                               ("WGRAD", m.weight.grad, R.wgrad_ref(x, gy), R.wgrad_ref(x, gy, torch.float32))):
        e_ref, e_hip = R.rel_dist(ref, f64), R.rel_dist(got, f64)
        rows.append((tag, e_hip, e_ref))
        print(f"MODULE {tag} {cin} -> {cout} {vol}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {bound_of(e_ref):.3e}")
    for tag, e_hip, e_ref in rows:
        assert e_hip <= bound_of(e_ref), (tag, e_hip, e_ref)


@pytest.mark.parametrize("cin,cout", R.SHAPES)
def test_cache_invalidation_by_an_optimizer_step(cin, cout):
    x, gy, w = cuda_case(cin, cout, 2, 9, 13, seed=5)
    m = make_module(cin, cout, w)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    xin = x.clone().requires_grad_(True)
    y0 = m(xin)
    y0.backward(gy)
    gx0 = xin.grad.clone()
    opt.step()
    xin2 = x.clone().requires_grad_(True)
    y1 = m(xin2)
    y1.backward(gy)
    fresh = make_module(cin, cout, m.weight.detach().clone())
    xin3 = x.clone().requires_grad_(True)
    y2 = fresh(xin3)
    y2.backward(gy)
    assert not torch.equal(y0, y1), "the step did not change the output: stale packed weight"
    assert torch.equal(y1, y2) and torch.equal(xin2.grad, xin3.grad) and not torch.equal(gx0, xin2.grad)
    packed = m._packed[False][1].w_direct   # unchanged weight: the packed forms are re-used
    m(x)
    assert m._packed[False][1].w_direct is packed


def test_frozen_inputs_skip_their_kernel_and_double_backward_raises():
    from dmvsnet_amd import conv
    from dmvsnet_amd._lib import DmvsError
    for cin, cout in R.SHAPES:
        x, gy, w = cuda_case(cin, cout, 2, 6, 9, B=2, seed=6)
        m = make_module(cin, cout, w)
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
            m(x.transpose(3, 4))


# ------------------------------------------------------------------------------------------------ whole networks
def diff_part(name, sd):
    import dmvsnet_amd as da
    net = (da.DiffCostRegNetPartRefine if R.GOLDEN_NETS[name]["refine"] else da.DiffCostRegNetPart)(2, 8)
    net.load_state_dict(sd, strict=True)
    return net.cuda().train()


def run_diff(net, x, gy):
    """Forward + backward on a fresh leaf; the blocks' outputs (after the fused ReLU) give the masks."""
    post, hooks = {}, []
    for blk in R.BLOCKS:
        hooks.append(getattr(net, blk).register_forward_hook(lambda mod, inp, out, blk=blk: post.__setitem__(blk, out.detach())))
    xin = x.cuda().clone().requires_grad_(True)
    out = net(xin)
    for h in hooks:
        h.remove()
    out.backward(gy.cuda())
    return out.detach(), {"x": xin.grad, **{n: p.grad for n, p in net.named_parameters()}}, post


@pytest.fixture(scope="module")
def net_refs(golden):
    """Per stored case, computed once: inputs, weights, the float64 and the stock fp32 run (CPU) and the reference's recorded results."""
    g = golden("op_regnet_grad.npz")
    out = {}
    for name in R.GOLDEN_NETS:
        seed = int(g[f"{name}.seed"])
        x, gy = torch.from_numpy(g[f"{name}.x"]), torch.from_numpy(g[f"{name}.gy"])
        beta = {k.split(".")[-1]: v for k, v in g.items() if k.startswith(f"{name}.beta.")}
        sd = R.net_weights(name, seed, beta)
        f64 = R.run_part(R.plain_net(name, sd, torch.float64), x, gy)
        f32 = R.run_part(R.plain_net(name, sd, torch.float32), x, gy)
        stored = {k[len(name) + 3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(f"{name}.g.")}
        out[name] = dict(x=x, gy=gy, sd=sd, f64=f64, f32=f32, stored=stored, out=torch.from_numpy(g[f"{name}.out"]))
    return out


@pytest.mark.parametrize("name", list(R.GOLDEN_NETS))
def test_network_against_the_reference_and_float64(net_refs, name):
    """The reference's CostRegNet_part / _part_refine in train mode, batch 2: the stored tensors against the reference's recorded fp32
    run, every other gradient against the stock fp32 run, all measured from the float64 run; the ReLU masks first."""
    c = net_refs[name]
    (o64, g64, pre64), (o32, g32, pre32) = c["f64"], c["f32"]
    assert R.kink_violations(pre64) == 0 and R.same_masks(pre32, pre64)
    net = diff_part(name, c["sd"])
    out, ghip, post = run_diff(net, c["x"], c["gy"])
    flips = {blk: int(((post[blk].cpu() > 0) != (pre64[blk] > 0)).sum()) for blk in R.BLOCKS}
    print(f"NET {name} mask flips per block: {flips}")
    assert not any(flips.values()), flips
    assert set(ghip) == set(g64)
    rows = [("out", "recorded", R.rel_dist(out, o64), R.rel_dist(c["out"], o64))]
    for k in sorted(g64):
        ref, what = (c["stored"][k], "recorded") if k in c["stored"] else (g32[k], "stock fp32")
        rows.append((k, what, R.rel_dist(ghip[k], g64[k]), R.rel_dist(ref, g64[k])))
    for k, what, e_hip, e_ref in rows:
        print(f"NET {name} {k}: e_hip {e_hip:.3e}  e_ref ({what}) {e_ref:.3e}  bound {bound_of(e_ref):.3e}")
    for k, what, e_hip, e_ref in rows:
        assert e_hip <= bound_of(e_ref), (name, k, e_hip, e_ref)
    assert all(int(m.num_batches_tracked) == 1 for m in net.modules() if hasattr(m, "num_batches_tracked"))


def test_eval_mode_meets_the_costreg_golden(golden):
    """eval(): the Diff networks with the op_costreg.npz seed's weights against the reference's recorded outputs, at the bound
    tests/test_gpu_parity.py::test_costreg_golden uses for the same vectors."""
    import numpy as np
    import dmvsnet_amd as da
    from dmvsnet_amd import synth
    g = golden("op_costreg.npz")
    sd = synth.synth_state_dict(da.MVSNet([8], [4], verbose=False).state_dict(), int(g["seed"]))
    sub = lambda prefix: {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    full, refine = da.DiffCostRegNet(2, 8), da.DiffCostRegNetRefine(2, 8)
    full.load_state_dict(sub("cost_regularization.0."), strict=True)
    refine.load_state_dict(sub("cost_regularization_refine.0."), strict=True)
    full, refine = full.cuda().eval(), refine.cuda().eval()
    x, xr = torch.from_numpy(g["x"]).cuda(), torch.from_numpy(g["xr"]).cuda()
    with torch.no_grad():
        got = dict(y_small=full.cosR_small(x), y_full=full(x), yr_huge=refine.cosR_huge(xr), yr_full=refine(xr))
    for k, v in got.items():
        print(f"EVAL {k}: max-abs distance {np.abs(v.cpu().numpy() - g[k]).max():.3e}  (|y| max {np.abs(g[k]).max():.3e}, bound 1e-4)")
    for k, v in got.items():
        np.testing.assert_allclose(v.cpu().numpy(), g[k], atol=1e-4, rtol=0.0, err_msg=k)
    assert all(int(m.num_batches_tracked) == 0 for m in full.modules() if hasattr(m, "num_batches_tracked"))


def test_network_train_step_is_bitwise_reproducible(net_refs):
    import dmvsnet_amd as da
    c = net_refs["part"]
    sd = {f"{half}.{k}": v for half in ("cosR_small", "cosR_huge") for k, v in c["sd"].items()}
    gy = torch.cat((c["gy"], c["gy"].flip(1)), 1).cuda()
    runs = []
    for _ in range(2):
        net = da.DiffCostRegNet(2, 8)
        net.load_state_dict(sd, strict=True)
        net = net.cuda().train()
        xin = c["x"].cuda().clone().requires_grad_(True)
        out = net(xin)
        out.backward(gy)
        runs.append([out.detach(), xin.grad] + [p.grad for p in net.parameters()] + [b for b in net.buffers()])
    assert tuple(runs[0][0].shape) == (2, 4, 8, 16, 24)
    assert all(torch.isfinite(t.float()).all() for t in runs[0])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
