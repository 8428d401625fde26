"""CPU: the host side of the differentiable stride-1 square convolutions (dmvsnet_amd/conv.py, K3g's launcher) and their yardstick.

  yardstick   the float64 restatement (tests/conv_grad_ref.py) equals float64 autograd of F.conv3d / F.conv2d for all six shapes; the
              stored goldens meet the kink condition and carry the reference's gradients at fp32 distance from the restatement
  packing     ops.pack_index_mfma is a permutation, its gather equals the host packer bit for bit, and the transposed-flipped index
              equals packing w.transpose(0, 1).flip(2, 3, 4)
  launcher    dmvs_conv3d_wgrad_plan / _workspace: positive for the six shapes, refused otherwise, a workspace that does not grow with
              the volume, tiles that cover a ragged volume exactly once; argument refusals of dmvs_conv3d_wgrad itself
  module      constructor and input refusals, the parameter / state-dict contract, the C ABI agreement
"""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import conv_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dmvs_conv3d_wgrad", "dmvs_conv3d_wgrad_workspace", "dmvs_conv3d_wgrad_plan")


# ------------------------------------------------------------------------------------------------ yardstick
@pytest.mark.parametrize("C,kd", R.SHAPES)
def test_restatement_equals_float64_autograd(C, kd):
    B, D, H, W = 2, (3 if kd == 3 else 1), 5, 6
    g = torch.Generator().manual_seed(C + kd)
    x = torch.randn(B, C, D, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(C, C, kd, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(B, C, D, H, W, generator=g, dtype=torch.float64)
    if kd == 3:
        y = F.conv3d(x, w, padding=1)
    else:
        y = F.conv2d(x.squeeze(2), w.squeeze(2), padding=1).unsqueeze(2)
    gx, gw = torch.autograd.grad(y, [x, w], gy)
    for name, got, want in (("conv", R.conv_ref(x, w, kd), y), ("wgrad", R.wgrad_ref(x, gy, kd), gw), ("dgrad", R.dgrad_ref(gy, w, kd), gx)):
        e = R.rel_dist(got, want)
        print(f"RESTATEMENT C {C} kd {kd} {name}: {e:.2e}")
        assert e <= 1e-12, (name, e)


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_goldens_meet_the_kink_condition(golden, name):
    g = golden("op_conv_grad.npz")
    case, kw = R.golden_case(g, name), R.GOLDEN_CASES[name]
    assert tuple(case["x"].shape) == (kw["B"], kw["C"], kw["D"], kw["H"], kw["W"]) and tuple(case["w"].shape) == (kw["C"], kw["C"], kw["kd"], 3, 3)
    fresh = R.make_case(**kw)
    assert all(torch.equal(case[k], fresh[k]) for k in ("x", "w", "gamma", "beta", "gy"))
    assert R.kink_violations(case) == 0
    f64 = R.block_f64(case)
    for k in ("out", "g_x", "g_w", "g_gamma", "g_beta"):
        e = R.rel_dist(case[k], f64[k])
        print(f"GOLDEN {name} {k}: e_ref {e:.2e}")
        assert e < 1e-5, (k, e)   # the recorded fp32 run is the same function (measured 0.8e-7 .. 3.9e-7)
    # the block's gradients for x and w are the restated data / weight gradient of the gradient that reaches the conv
    y = R.conv_ref(case["x"], case["w"], case["kd"]).requires_grad_(True)
    g_y = torch.autograd.grad(torch.relu(R.bn_train(y, case["gamma"], case["beta"])), y, case["gy"].double())[0]
    assert R.rel_dist(R.wgrad_ref(case["x"], g_y, case["kd"]), f64["g_w"]) <= 1e-12
    assert R.rel_dist(R.dgrad_ref(g_y, case["w"], case["kd"]), f64["g_x"]) <= 1e-12


# ------------------------------------------------------------------------------------------------ packing
@pytest.mark.parametrize("C,kd", R.SHAPES)
def test_pack_index_is_the_host_packing(C, kd):
    from dmvsnet_amd import ops
    n = C * C * 9 * kd
    w = torch.randn(C, C, kd, 3, 3, generator=torch.Generator().manual_seed(C * kd))
    for tf in (False, True):
        idx = ops.pack_index_mfma(C, kd, tf)
        assert idx.dtype == torch.int64 and idx.device.type == "cpu" and idx.numel() == n
        assert torch.equal(torch.sort(idx).values, torch.arange(n)), "not a permutation"
        assert ops.pack_index_mfma(C, kd, tf) is idx, "not cached"
        src = w.transpose(0, 1).flip(2, 3, 4).contiguous() if tf else w
        host = ops.pack_mfma(src, C, C, ops.CONV_S1, kd)
        assert host.numel() == n
        assert torch.equal(w.reshape(-1)[idx], host)
    # the 2D weight layout [C,C,3,3] is the same memory
    if kd == 1:
        assert torch.equal(w.squeeze(2).reshape(-1)[ops.pack_index_mfma(C, 1, False)], ops.pack_mfma(w.squeeze(2), C, C, ops.CONV_S1, 1))
    assert not torch.equal(ops.pack_index_mfma(C, kd, False), ops.pack_index_mfma(C, kd, True))


def test_pack_index_refuses_other_shapes():
    from dmvsnet_amd import ops
    from dmvsnet_amd._lib import DmvsError
    for C, kd in ((8, 3), (48, 1), (16, 2), (128, 3)):
        with pytest.raises(DmvsError):
            ops.pack_index_mfma(C, kd, False)


# ------------------------------------------------------------------------------------------------ launcher
def test_plan_and_workspace():
    from dmvsnet_amd import _lib, ops
    lib = _lib.load()
    tz, ty, tx = ops.WGRAD_TILE
    assert tz == 1
    for C, kd in R.SHAPES:
        small, large = lib.dmvs_conv3d_wgrad_workspace(C, 4, 96, 352, kd), lib.dmvs_conv3d_wgrad_workspace(C, 32, 592, 800, kd)
        assert small > 0 and small == large == lib.dmvs_conv3d_wgrad_workspace(C, 1, 1, 1, kd), (C, kd, small, large)
        assert small % (9 * kd * C * C) == 0 and small // (9 * kd * C * C) <= 256   # whole partials, at most one per workgroup
        for D, H, W in ((1, 1, 1), (1, 5, 7), (3, 19, 35), (2, 20, 36), (5, 9, 131), (4, 96, 352), (7, 33, 65), (32, 592, 800)):
            plan = lib.dmvs_conv3d_wgrad_plan(C, D, H, W, kd)
            assert plan > 0, (C, kd, D, H, W, plan)
            tiles, wgs = plan >> 9, plan & 511
            # the tiles are a regular grid of 1 x ty x tx boxes over [0,D) x [0,H) x [0,W): every voxel in exactly one of them
            assert tiles == D * -(-H // ty) * -(-W // tx)
            assert tiles * ty * tx >= D * H * W
            blocks = (C // 32) ** 2 if C > 32 else 1
            shares = min(tiles, 256 // blocks)
            assert wgs % 8 == 0 and 0 < wgs <= 256 and wgs - 8 < shares * blocks <= wgs
            assert shares * 9 * kd * C * C <= small   # every share's partial has its place
    for C, kd in ((8, 3), (24, 1), (16, 2), (16, 0), (128, 3), (0, 3)):
        assert lib.dmvs_conv3d_wgrad_workspace(C, 4, 8, 8, kd) == 0
        assert lib.dmvs_conv3d_wgrad_plan(C, 4, 8, 8, kd) == _lib.EUNSUPPORTED
    for D, H, W in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4)):
        assert lib.dmvs_conv3d_wgrad_workspace(16, D, H, W, 3) == 0
        assert lib.dmvs_conv3d_wgrad_plan(16, D, H, W, 3) == _lib.EINVAL


def test_wgrad_entry_refuses_bad_arguments():
    """Argument checks happen before anything is launched: no GPU needed (the pointers are never followed)."""
    from dmvsnet_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.dmvs_conv3d_wgrad(p, p, p, p, 8, 2, 4, 4, 3, 0, None) == _lib.EUNSUPPORTED
    assert lib.dmvs_conv3d_wgrad(p, p, p, p, 16, 2, 4, 4, 2, 0, None) == _lib.EUNSUPPORTED
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.dmvs_conv3d_wgrad(*args, 16, 2, 4, 4, 3, 0, None) == _lib.EINVAL
    for dims in ((0, 4, 4), (2, 0, 4), (2, 4, 0)):
        assert lib.dmvs_conv3d_wgrad(p, p, p, p, 16, *dims, 3, 0, None) == _lib.EINVAL


def test_abi_agreement():
    from dmvsnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "dmvs.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/dmvs.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["dmvs_conv3d_wgrad"][1]) == 11
    declared = set(re.findall(r"\b(dmvs_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SIGNATURES)
    assert lib.dmvs_version() == _lib.ABI_VERSION == 140
    text = open(os.path.join(ROOT, "scripts", "pmc_summary.py")).read()
    assert "conv_wgrad_kernel" in text and "conv_wgrad_reduce_kernel" in text
    src = open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "conv3d_wgrad.h")).read()
    assert set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src)) == {"conv_wgrad_kernel", "conv_wgrad_reduce_kernel"}
    assert "atomic" not in src.lower().replace("no atomics", "")
    shared = open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "wgrad_share.h")).read()
    assert "atomic" not in shared.lower().replace("no atomics", "")


# ------------------------------------------------------------------------------------------------ module
def test_constructor_refusals_and_contract():
    import dmvsnet_amd
    from dmvsnet_amd import DiffConv2d, DiffConv3d, conv
    from dmvsnet_amd._lib import DmvsError
    assert dmvsnet_amd.conv is conv and "DiffConv3d" in dmvsnet_amd.__all__ and "DiffConv2d" in dmvsnet_amd.__all__
    assert set(conv.launch_counts) == {"dgrad", "wgrad"}
    for cls, nn_cls in ((DiffConv3d, torch.nn.Conv3d), (DiffConv2d, torch.nn.Conv2d)):
        for C in (16, 32, 64):
            m = cls(C, C, 3, stride=1, padding=1, bias=False)
            ref = nn_cls(C, C, 3, stride=1, padding=1, bias=False)
            assert isinstance(m, nn_cls) and list(m.state_dict()) == ["weight"] and m.weight.shape == ref.weight.shape
            assert [n for n, _ in m.named_parameters()] == ["weight"]
            m.load_state_dict(ref.state_dict())
            assert torch.equal(m.weight, ref.weight)
        bad = (dict(stride=2), dict(bias=True), dict(dilation=2, padding=2), dict(groups=2), dict(padding=0), dict(padding_mode="reflect"))
        for kw in bad:
            with pytest.raises(DmvsError):
                cls(16, 16, 3, **{"stride": 1, "padding": 1, "bias": False, **kw})
        with pytest.raises(DmvsError):
            cls(8, 8, 3, padding=1, bias=False)
        with pytest.raises(DmvsError):
            cls(16, 32, 3, padding=1, bias=False)
        with pytest.raises(DmvsError):
            cls(16, 16, 5, padding=2, bias=False)
        with pytest.raises(DmvsError):
            cls(16, 16, 3, padding=1)   # nn.Conv's default has a bias
    with pytest.raises(DmvsError):
        DiffConv3d(16, 16, (1, 3, 3), padding=(0, 1, 1), bias=False)


def test_input_refusals():
    from dmvsnet_amd import DiffConv2d, DiffConv3d, ops
    from dmvsnet_amd._lib import DmvsError
    m3, m2 = DiffConv3d(16, 16, 3, padding=1, bias=False), DiffConv2d(16, 16, 3, padding=1, bias=False)
    with pytest.raises(DmvsError, match="no CPU fallback"):
        m3(torch.zeros(1, 16, 2, 4, 4))
    with pytest.raises(DmvsError, match="no CPU fallback"):
        m2(torch.zeros(1, 16, 4, 4))
    with pytest.raises(DmvsError):
        m3(torch.zeros(1, 16, 2, 4, 4, dtype=torch.float16))
    with pytest.raises(DmvsError):
        m3("x")
    with pytest.raises(DmvsError):
        ops.conv3d_wgrad(torch.zeros(16, 2, 4, 4), torch.zeros(16, 2, 4, 4), 3)


def test_no_training_mode_for_the_whole_network():
    from dmvsnet_amd import MVSNet
    with pytest.raises(NotImplementedError):
        MVSNet([8], [4], verbose=False).train()


def test_packed_cache_follows_the_weight():
    """The per-module packed weights (host logic, no kernel): equal to the host packing, re-used while the weight is unchanged,
    re-packed after an in-place update, a load_state_dict and a replaced parameter."""
    from dmvsnet_amd import DiffConv2d, DiffConv3d, conv, ops
    for cls, C, kd in ((DiffConv3d, 32, 3), (DiffConv2d, 16, 1)):
        m = cls(C, C, 3, padding=1, bias=False)
        for tf in (False, True):
            w5 = m.weight.detach().reshape(C, C, kd, 3, 3)
            want = ops.pack_mfma(w5.transpose(0, 1).flip(2, 3, 4).contiguous() if tf else w5, C, C, ops.CONV_S1, kd)
            layer = conv._packed_layer(m._packed, m.weight, kd, tf)
            assert torch.equal(layer.w_mfma, want) and layer.scale is None and layer.shift is None and not layer.relu
            assert layer.mode == ops.CONV_S1 and layer.kdepth == kd and layer.cin == layer.cout == C
            assert conv._packed_layer(m._packed, m.weight, kd, tf) is layer
        stale = conv._packed_layer(m._packed, m.weight, kd, False)
        torch.optim.SGD(m.parameters(), lr=0.5).zero_grad()
        m.weight.grad = torch.ones_like(m.weight)
        torch.optim.SGD(m.parameters(), lr=0.5).step()
        fresh = conv._packed_layer(m._packed, m.weight, kd, False)
        assert fresh is not stale and torch.equal(fresh.w_mfma, ops.pack_mfma(m.weight.detach().reshape(C, C, kd, 3, 3), C, C, ops.CONV_S1, kd))
        m.load_state_dict({"weight": torch.zeros_like(m.weight)})
        assert not conv._packed_layer(m._packed, m.weight, kd, False).w_mfma.any()
        m.weight = torch.nn.Parameter(torch.ones_like(m.weight))
        assert conv._packed_layer(m._packed, m.weight, kd, False).w_mfma.all()
