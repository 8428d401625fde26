"""CPU: the host side of the differentiable 2-channel ends (conv0 / prob: dmvsnet_amd/conv.py, K2g's launcher), of the four
regularisation networks (dmvsnet_amd/regnet.py) and their yardsticks.

  yardstick   the float64 restatement of G with both role maps, prob's tap flip included (tests/regnet_grad_ref.py), equals float64
              autograd of F.conv3d for (2, 8) and (8, 2) on ragged volumes; the stock-layer networks equal the Diff networks' keys;
              the stored network cases meet the kink condition and carry the reference's results at fp32 distance from float64
  packing     ops.pack_index_direct reproduces pack_direct(w) and pack_direct(w.transpose(0, 1).flip(2, 3, 4)) bit for bit
  launcher    dmvs_conv3d_wgrad_c2_plan / _workspace: host only; refused shapes, a workspace that does not grow with the volume, at
              most 256 workgroups, the documented 1 x 4 x 64 tile; argument refusals of dmvs_conv3d_wgrad_c2 itself
  modules     keys and shapes against tests/golden/state_dict_keys.json, strict load_state_dict round trips with the stock stack,
              constructor / input / extent refusals, the C ABI agreement
"""
import ctypes
import json
import os
import re

import pytest
import torch
import torch.nn.functional as F

import regnet_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dmvs_conv3d_wgrad_c2", "dmvs_conv3d_wgrad_c2_workspace", "dmvs_conv3d_wgrad_c2_plan")
RAGGED = ((1, 3, 4), (2, 5, 9), (3, 10, 18), (2, 5, 67))


# ------------------------------------------------------------------------------------------------ yardstick
@pytest.mark.parametrize("vol", RAGGED)
@pytest.mark.parametrize("cin,cout", R.SHAPES)
def test_restatement_equals_float64_autograd(cin, cout, vol):
    D, H, W = vol
    g = torch.Generator().manual_seed(cin + 10 * cout + D * H * W)
    x = torch.randn(2, cin, D, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(2, cout, D, H, W, generator=g, dtype=torch.float64)
    y = F.conv3d(x, w, padding=1)
    gx, gw = torch.autograd.grad(y, [x, w], gy)
    for name, got, want in (("conv", R.conv_ref(x, w), y), ("wgrad", R.wgrad_ref(x, gy), gw), ("dgrad", R.dgrad_ref(gy, w), gx)):
        e = R.rel_dist(got, want)
        print(f"RESTATEMENT {cin} -> {cout} {vol} {name}: {e:.2e}")
        assert tuple(got.shape) == tuple(want.shape) and e <= 1e-12, (name, e)
    # the two layers are ONE formula: G of (P, Q) = (8-channel, 2-channel) tensor, whichever of them is the input
    P, Q = (gy, x) if cin == 2 else (x, gy)
    G = R.g_ref(P, Q)
    want = gw if cin == 2 else gw.transpose(0, 1).flip(2, 3, 4)
    assert tuple(G.shape) == (8, 2, 3, 3, 3) and R.rel_dist(G, want) <= 1e-12


def test_the_data_gradient_of_each_end_is_the_other_end():
    """conv0's data gradient is the 8 -> 2 convolution with the transposed-flipped weight, prob's the 2 -> 8 one (float64, exact form)."""
    for cin, cout in R.SHAPES:
        _, gy, w = R.rand_case(cin, cout, 2, 5, 9, B=2)
        wt = w.transpose(0, 1).flip(2, 3, 4).contiguous()
        assert tuple(wt.shape) == (cin, cout, 3, 3, 3)
        assert R.rel_dist(R.conv_ref(gy, wt), R.dgrad_ref(gy, w)) <= 1e-12


@pytest.mark.parametrize("name", list(R.GOLDEN_NETS))
def test_stored_networks_meet_the_kink_condition(golden, name):
    g = golden("op_regnet_grad.npz")
    kw, seed = R.GOLDEN_NETS[name], int(g[f"{name}.seed"])
    x, gy = torch.from_numpy(g[f"{name}.x"]), torch.from_numpy(g[f"{name}.gy"])
    assert tuple(x.shape) == tuple(gy.shape) == (kw["B"], 2, kw["D"], kw["H"], kw["W"]) and kw["B"] == 2
    fx, fgy = R.net_inputs(name, seed)
    assert torch.equal(x, fx) and torch.equal(gy, fgy)
    beta = {k.split(".")[-1]: v for k, v in g.items() if k.startswith(f"{name}.beta.")}
    assert set(beta) in (set(), set(R.BLOCKS))
    sd = R.net_weights(name, seed, beta)
    o64, g64, pre64 = R.run_part(R.plain_net(name, sd, torch.float64), x, gy)
    assert R.kink_violations(pre64) == 0, "a BatchNorm output of the float64 run lies within 1e-4 of the ReLU kink"
    o32, g32, pre32 = R.run_part(R.plain_net(name, sd, torch.float32), x, gy)
    assert R.same_masks(pre32, pre64)
    stored = {k[len(name) + 3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith(f"{name}.g.")}
    want = {"x"} | set(R.STORED_WEIGHT_GRADS) | {f"{b}.bn.{p}" for b in R.BLOCKS for p in ("weight", "bias")}
    assert set(stored) == want
    rows = [("out", R.rel_dist(torch.from_numpy(g[f"{name}.out"]), o64))] + [(k, R.rel_dist(v, g64[k])) for k, v in sorted(stored.items())]
    for k, e in rows:
        print(f"GOLDEN {name} {k}: e_ref {e:.2e}")
    for k, e in rows:
        assert e < 1e-4, (k, e)   # the recorded fp32 run is the same function (measured up to 2.1e-6)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "op_regnet_grad.npz")) < (1 << 20)


# ------------------------------------------------------------------------------------------------ packing
@pytest.mark.parametrize("cin,cout", R.SHAPES)
def test_pack_index_is_pack_direct(cin, cout):
    from dmvsnet_amd import ops
    n = cin * cout * 27
    iota = torch.arange(n, dtype=torch.float32).reshape(cout, cin, 3, 3, 3)
    w = torch.randn(cout, cin, 3, 3, 3, generator=torch.Generator().manual_seed(cin))
    for src in (iota, w):
        for tf in (False, True):
            idx = ops.pack_index_direct(cin, cout, tf)
            assert idx.dtype == torch.int64 and idx.device.type == "cpu" and idx.numel() == n
            assert torch.equal(torch.sort(idx).values, torch.arange(n)), "not a permutation"
            assert ops.pack_index_direct(cin, cout, tf) is idx, "not cached"
            host = ops.pack_direct(src.transpose(0, 1).flip(2, 3, 4) if tf else src, False)
            assert tuple(host.shape) == ((3, 3, 3, cout, cin) if tf else (3, 3, 3, cin, cout))
            assert torch.equal(src.reshape(-1)[idx], host.reshape(-1))
    assert not torch.equal(ops.pack_index_direct(cin, cout, False), ops.pack_index_direct(cin, cout, True))


def test_packed_cache_follows_the_weight():
    """The per-module packed weights (host logic, no kernel): equal to pack_direct, re-used while the weight is unchanged, re-packed
    after an in-place update."""
    from dmvsnet_amd import DiffConv3d, conv, ops
    for cin, cout in R.SHAPES:
        m = DiffConv3d(cin, cout, 3, padding=1, bias=False)
        for tf in (False, True):
            w = m.weight.detach()
            want = ops.pack_direct(w.transpose(0, 1).flip(2, 3, 4) if tf else w, False)
            layer = conv._packed_layer_c2(m._packed, m.weight, tf)
            assert torch.equal(layer.w_direct, want.reshape(-1)) and layer.w_mfma is None and layer.scale is None and not layer.relu
            assert (layer.cin, layer.cout) == ((cout, cin) if tf else (cin, cout)) and layer.mode == ops.CONV_S1 and layer.kdepth == 3
            assert conv._packed_layer_c2(m._packed, m.weight, tf) is layer
        stale = conv._packed_layer_c2(m._packed, m.weight, False)
        m.weight.grad = torch.ones_like(m.weight)
        torch.optim.SGD(m.parameters(), lr=0.5).step()
        fresh = conv._packed_layer_c2(m._packed, m.weight, False)
        assert fresh is not stale and torch.equal(fresh.w_direct, ops.pack_direct(m.weight.detach(), False).reshape(-1))


# ------------------------------------------------------------------------------------------------ launcher
def test_plan_and_workspace():
    from dmvsnet_amd import _lib, ops
    lib = _lib.load()
    tz, ty, tx = ops.WGRAD_C2_TILE
    assert (tz, ty, tx) == (1, 4, 64)   # docs/kernels/K2g_conv_wgrad_c2.md
    assert tuple(ops.WGRAD_C2_SHAPES) == R.SHAPES
    for cin, cout in R.SHAPES:
        small, large = lib.dmvs_conv3d_wgrad_c2_workspace(cin, cout, 1, 3, 4), lib.dmvs_conv3d_wgrad_c2_workspace(cin, cout, 32, 592, 800)
        assert small > 0 and small == large == lib.dmvs_conv3d_wgrad_c2_workspace(cin, cout, 8, 1184, 1600), (small, large)
        assert small % 432 == 0 and small // 432 <= 256   # whole partials [27][8][2], at most one per workgroup
        for D, H, W in ((1, 1, 1), (1, 3, 4), (2, 5, 9), (3, 10, 18), (2, 5, 67), (8, 36, 130), (64, 296, 400), (32, 592, 800),
                        (8, 1184, 1600)):
            plan = lib.dmvs_conv3d_wgrad_c2_plan(cin, cout, D, H, W)
            assert plan > 0, (cin, cout, D, H, W, plan)
            tiles, wgs = plan >> 9, plan & 511
            assert tiles == D * -(-H // ty) * -(-W // tx)   # a regular grid of 1 x 4 x 64 boxes: every voxel in exactly one
            shares = min(tiles, 256)
            assert wgs % 8 == 0 and 0 < wgs <= 256 and wgs - 8 < shares <= wgs
            assert shares * 432 <= small                     # every share's partial has its place
    for cin, cout in ((2, 2), (8, 8), (2, 16), (16, 2), (3, 8), (8, 1), (0, 8), (1, 8)):
        assert lib.dmvs_conv3d_wgrad_c2_workspace(cin, cout, 4, 8, 8) == 0
        assert lib.dmvs_conv3d_wgrad_c2_plan(cin, cout, 4, 8, 8) == _lib.EUNSUPPORTED
    for D, H, W in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4)):
        assert lib.dmvs_conv3d_wgrad_c2_workspace(2, 8, D, H, W) == 0
        assert lib.dmvs_conv3d_wgrad_c2_plan(2, 8, D, H, W) == _lib.EINVAL
    assert lib.dmvs_conv3d_wgrad_c2_plan(2, 8, 4096, 4096, 64) == _lib.EINVAL   # 2^22 tiles: past what the plan can say


def test_wgrad_c2_entry_refuses_bad_arguments():
    """Argument checks happen before anything is launched: no GPU needed (the pointers are never followed)."""
    from dmvsnet_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for cin, cout in ((8, 8), (2, 2), (16, 16), (2, 16)):
        assert lib.dmvs_conv3d_wgrad_c2(p, p, p, p, cin, cout, 2, 4, 4, 0, None) == _lib.EUNSUPPORTED
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.dmvs_conv3d_wgrad_c2(*args, 2, 8, 2, 4, 4, 0, None) == _lib.EINVAL
    for dims in ((0, 4, 4), (2, 0, 4), (2, 4, 0)):
        assert lib.dmvs_conv3d_wgrad_c2(p, p, p, p, 8, 2, *dims, 0, None) == _lib.EINVAL


def test_abi_agreement():
    from dmvsnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "dmvs.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/dmvs.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["dmvs_conv3d_wgrad_c2"][1]) == 11
    assert lib.dmvs_version() == _lib.ABI_VERSION == 140   # additive: the ABI version does not move
    text = open(os.path.join(ROOT, "scripts", "pmc_summary.py")).read()
    assert "conv_wgrad_c2_kernel" in text and "conv_wgrad_c2_reduce_kernel" in text
    src = open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "conv3d_wgrad_c2.h")).read()
    assert set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src)) == {"conv_wgrad_c2_kernel", "conv_wgrad_c2_reduce_kernel"}
    assert "atomic" not in src.lower().replace("no atomics", "")
    shared = open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "wgrad_share.h")).read()
    assert "atomic" not in shared.lower().replace("no atomics", "")
    assert '#include "conv3d_wgrad_c2.h"' in open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "conv3d_direct.hip")).read()


# ------------------------------------------------------------------------------------------------ modules
def test_constructor_refusals_and_contract():
    import dmvsnet_amd
    from dmvsnet_amd import DiffConv2d, DiffConv3d, DiffConvBlock3d, conv
    from dmvsnet_amd._lib import DmvsError
    assert set(conv.launch_counts) == {"dgrad", "wgrad"}
    assert tuple(conv.CHANNELS_C2) == R.SHAPES
    for cin, cout in R.SHAPES:
        m = DiffConv3d(cin, cout, 3, stride=1, padding=1, bias=False)
        ref = torch.nn.Conv3d(cin, cout, 3, stride=1, padding=1, bias=False)
        assert isinstance(m, torch.nn.Conv3d) and list(m.state_dict()) == ["weight"] and m.weight.shape == ref.weight.shape
        m.load_state_dict(ref.state_dict())
        assert torch.equal(m.weight, ref.weight)
        with pytest.raises(DmvsError):
            DiffConv2d(cin, cout, 3, stride=1, padding=1, bias=False)
        bad = (dict(stride=2), dict(bias=True), dict(dilation=2, padding=2), dict(groups=2), dict(padding=0), dict(padding_mode="reflect"),
               dict(kernel_size=5, padding=2), dict(kernel_size=(1, 3, 3), padding=(0, 1, 1)))
        for kw in bad:
            args = {"kernel_size": 3, "stride": 1, "padding": 1, "bias": False, **kw}
            with pytest.raises(DmvsError):
                DiffConv3d(cin, cout, **args)
    for cin, cout in ((2, 2), (8, 8), (2, 16), (4, 8), (8, 4), (1, 8), (8, 1), (16, 32)):
        with pytest.raises(DmvsError):
            DiffConv3d(cin, cout, 3, stride=1, padding=1, bias=False)
    blk = DiffConvBlock3d(2, 8, 3, padding=1)   # conv0 as the reference builds it
    assert isinstance(blk.conv, DiffConv3d) and blk.conv.weight.shape == (8, 2, 3, 3, 3) and blk.bn.num_features == 8
    assert all(n in dmvsnet_amd.__all__ for n in ("regnet", "DiffCostRegNetPart", "DiffCostRegNetPartRefine", "DiffCostRegNet",
                                                  "DiffCostRegNetRefine"))


NETS = (("DiffCostRegNet", "cost_regularization", False), ("DiffCostRegNetRefine", "cost_regularization_refine", True))


@pytest.mark.parametrize("cls,prefix,refine", NETS)
def test_networks_have_the_reference_keys_and_load_strictly(cls, prefix, refine):
    import dmvsnet_amd as da
    from dmvsnet_amd import synth
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "state_dict_keys.json")))
    net = getattr(da, cls)(2, 8)
    got = {k: list(v.shape) for k, v in net.state_dict().items()}
    for n in (0, 1, 2):
        want = {k[len(f"{prefix}.{n}."):]: v for k, v in keys.items() if k.startswith(f"{prefix}.{n}.")}
        assert len(want) == 122 and got == want
    assert list(net.state_dict()) == list(R.PlainPair(refine).state_dict())   # the same names in the same order
    part = net.cosR_small
    assert [n for n, _ in part.named_children()] == ["conv0", "conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv9", "conv11", "prob"]
    assert isinstance(part.prob, da.DiffConv3d) and isinstance(part.conv0, da.DiffConvBlock3d)
    assert isinstance(part.conv6, da.DiffConvBlock2d if refine else da.DiffConvBlock3d)
    assert not any(type(m) in (torch.nn.Conv3d, torch.nn.Conv2d, torch.nn.ConvTranspose3d, torch.nn.ConvTranspose2d, torch.nn.BatchNorm3d,
                               torch.nn.BatchNorm2d) for m in net.modules()), "a stock ATen layer is left in the network"
    # a strict round trip with the same-named stock stack, both ways
    plain = R.PlainPair(refine)
    sd = synth.synth_state_dict(plain.state_dict(), 3)
    plain.load_state_dict(sd, strict=True)
    res = net.load_state_dict(plain.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(v, sd[k].reshape(v.shape)) for k, v in net.state_dict().items())
    R.PlainPair(refine).load_state_dict(net.state_dict(), strict=True)
    one = getattr(da, "DiffCostRegNetPartRefine" if refine else "DiffCostRegNetPart")(2, 8, stage=1)
    one.load_state_dict({k[len("cosR_huge."):]: v for k, v in sd.items() if k.startswith("cosR_huge.")}, strict=True)


def test_network_refusals():
    import dmvsnet_amd as da
    from dmvsnet_amd._lib import DmvsError
    for cls in (da.DiffCostRegNetPart, da.DiffCostRegNetPartRefine, da.DiffCostRegNet, da.DiffCostRegNetRefine):
        for cin, base in ((1, 8), (2, 16), (8, 8), (2, 4), (32, 8)):
            with pytest.raises(DmvsError, match="in_channels == 2, base_channels == 8"):
                cls(cin, base)
    full, refine = da.DiffCostRegNet(2, 8), da.DiffCostRegNetRefine(2, 8)
    for vol in ((4, 16, 16), (8, 12, 16), (8, 16, 20), (12, 16, 16), (0, 16, 16)):
        with pytest.raises(DmvsError, match="multiples of 8"):
            full(torch.zeros(1, 2, *vol))
    for vol in ((2, 16, 16), (6, 16, 16), (8, 16, 16), (4, 12, 16), (4, 16, 20)):
        with pytest.raises(DmvsError, match="D must be 4"):
            refine(torch.zeros(1, 2, *vol))
    for net, vol in ((full, (8, 16, 24)), (refine, (4, 16, 24))):
        with pytest.raises(DmvsError, match="no CPU fallback"):
            net(torch.zeros(1, 2, *vol))
        with pytest.raises(DmvsError):
            net(torch.zeros(1, 3, *vol))
        with pytest.raises(DmvsError):
            net(torch.zeros(2, *vol))
        with pytest.raises(DmvsError):
            net("x")


def test_input_refusals():
    from dmvsnet_amd import DiffConv3d, ops
    from dmvsnet_amd._lib import DmvsError
    for cin, cout in R.SHAPES:
        m = DiffConv3d(cin, cout, 3, padding=1, bias=False)
        with pytest.raises(DmvsError, match="no CPU fallback"):
            m(torch.zeros(1, cin, 2, 4, 4))
        with pytest.raises(DmvsError):
            m(torch.zeros(1, cin, 2, 4, 4, dtype=torch.float16))
        with pytest.raises(DmvsError):
            m(torch.zeros(1, cout, 2, 4, 4))
        with pytest.raises(DmvsError):
            m("x")
        with pytest.raises(DmvsError, match="no CPU fallback"):
            ops.conv3d_wgrad_c2(torch.zeros(cin, 2, 4, 4), torch.zeros(cout, 2, 4, 4))
    with pytest.raises(DmvsError):
        ops.conv3d_wgrad_c2_workspace(8, 8, 2, 4, 4, "cpu")


def test_no_training_mode_for_the_whole_network():
    from dmvsnet_amd import MVSNet
    with pytest.raises(NotImplementedError):
        MVSNet([8], [4], verbose=False).train()
