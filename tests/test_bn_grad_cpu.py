"""CPU: the host side of the differentiable BatchNorm + ReLU (dmvsnet_amd/bn.py, K5's launchers) and its yardstick.

  yardstick   the float64 restatement (tests/bn_grad_ref.py: no batch_norm call) equals float64 autograd of F.batch_norm + relu, train
              and eval mode, and nn.BatchNorm3d's running-statistics update, to 1e-12
  partition   dmvs_bn_plan / dmvs_bn_share_range: for every shape of the GPU tests the shares tile [0, B * V) exactly once and in
              order, on multiples of 4 when V % 4 == 0; S is 1 below one chunk and capped at Smax
  launcher    EINVAL paths of the entry points (checked before anything is launched), the C ABI agreement
  module      constructor and input refusals, the state-dict contract of the modules and of the four blocks
"""
import ctypes
import os
import re

import pytest
import torch
from torch import nn
import torch.nn.functional as F

import bn_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dmvs_bn_relu_forward", "dmvs_bn_relu_backward", "dmvs_bn_workspace", "dmvs_bn_plan", "dmvs_bn_share_range")
KERNELS = {"bn_stats_kernel", "bn_apply_kernel", "bn_bwd_reduce_kernel", "bn_bwd_apply_kernel", "bn_bwd_fold_kernel"}


# ------------------------------------------------------------------------------------------------ yardstick
@pytest.mark.parametrize("relu", (True, False))
@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("shape", ((2, 8, 2, 3, 5), (1, 16, 7, 9), (3, 8, 4, 4)))
def test_restatement_equals_float64_autograd(shape, training, relu):
    g = torch.Generator().manual_seed(sum(shape) + training + 2 * relu)
    C = shape[1]
    x = torch.randn(shape, generator=g, dtype=torch.float64, requires_grad=True) * 1.5 + 0.7
    x = x.detach().requires_grad_(True)
    gamma = (1.0 + 0.2 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_(True)
    beta = (0.2 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_(True)
    gy = torch.randn(shape, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    stats = {} if training else dict(mean=rm, var=rv)
    pre = F.batch_norm(x, None if training else rm, None if training else rv, gamma, beta, training, 0.1, R.BN_EPS)
    y = torch.relu(pre) if relu else pre
    gx, gg, gb = torch.autograd.grad(y, [x, gamma, beta], gy)
    got = R.all_f64(x, gy, gamma, beta, relu, R.BN_EPS, **stats)
    for name, a, b in (("y", got["y"], y), ("g_x", got["g_x"], gx), ("g_gamma", got["g_gamma"], gg), ("g_beta", got["g_beta"], gb)):
        e = R.rel_dist(a, b)
        print(f"RESTATEMENT {shape} train {training} relu {relu} {name}: {e:.2e}")
        assert a.shape == b.shape and e <= 1e-12, (name, e)
    if training:
        _, mean, invstd = torch.native_batch_norm(x.detach(), gamma.detach(), beta.detach(), None, None, True, 0.1, R.BN_EPS)
        assert R.rel_dist(got["mean"], mean) <= 1e-12 and R.rel_dist(got["invstd"], invstd) <= 1e-12


@pytest.mark.parametrize("momentum", (0.1, 0.01))
def test_running_update_equals_the_module(momentum):
    g = torch.Generator().manual_seed(3)
    m = nn.BatchNorm3d(8, momentum=momentum).double().train()
    rm, rv = m.running_mean.clone(), m.running_var.clone()
    for step in range(2):
        x = torch.randn(2, 8, 2, 3, 5, generator=g, dtype=torch.float64) * 2.0 + 1.0
        m(x)
        rm, rv = R.running_update(rm, rv, x, momentum)
        assert R.rel_dist(rm, m.running_mean) <= 1e-12 and R.rel_dist(rv, m.running_var) <= 1e-12
    assert int(m.num_batches_tracked) == 2


def test_case_generator_and_kink_count():
    from dmvsnet_amd import ops
    case = R.make_case(8, 2, (2, 5, 9), 0)
    again = R.make_case(8, 2, (2, 5, 9), 0)
    assert all(torch.equal(case[k], again[k]) for k in case) and case["x"].dtype == torch.float32
    assert R.kink_violations(case) == 0
    gamma, beta = case["gamma"].clone(), case["beta"].clone()
    gamma[3] = beta[3] = 0.0   # channel 3 sits on the kink everywhere
    assert R.kink_violations(dict(case, gamma=gamma, beta=beta)) == 2 * 90
    # the small shapes of the GPU tests are clean at their first seeds (the tests re-assert it)
    for name, (B, spatial) in R.bare_volumes(ops.BN_CHUNK).items():
        for offset in (0.0, 50.0):
            assert R.first_clean_seed(8, B, spatial, offset) < 20


# ------------------------------------------------------------------------------------------------ partition
def gpu_test_shapes():
    from dmvsnet_amd import ops
    shapes = [(C, B, R.volume(sp)) for C in R.CHANNELS for B, sp in R.bare_volumes(ops.BN_CHUNK).values()]
    shapes += [(C, B, R.volume(sp)) for C in (8, 64) for B, sp in (R.grid_shape(C, ops.BN_CHUNK, ops.BN_MAX_WG),)]
    shapes += [(8, 1, 8 * 16 * 32), (16, 1, 4 * 8 * 16), (32, 1, 2 * 4 * 8), (64, 1, 1 * 2 * 4)]   # the chain's volumes
    return shapes


def test_shares_tile_every_gpu_test_shape():
    from dmvsnet_amd import _lib, ops
    lib = _lib.load()
    chunk = ops.BN_CHUNK
    for C, B, V in gpu_test_shapes():
        n, smax = B * V, ops.BN_MAX_WG // C
        S = ops.bn_plan(C, B, V)
        assert S == min(-(-n // chunk), smax), (C, B, V, S)
        end = 0
        for s in range(S):
            lo, hi = ops.bn_share_range(C, B, V, s)
            assert lo == end and hi > lo, (C, B, V, s, lo, hi)   # in order, no gap, no overlap, none empty
            assert lo % chunk == 0 and (hi % chunk == 0 or hi == n)
            if V % 4 == 0:
                assert lo % 4 == 0 and hi % 4 == 0
            end = hi
        assert end == n, (C, B, V, end)
        lo, hi = ctypes.c_long(), ctypes.c_long()
        for s in (-1, S):
            assert lib.dmvs_bn_share_range(C, B, V, s, ctypes.byref(lo), ctypes.byref(hi)) == _lib.EINVAL
        assert lib.dmvs_bn_workspace(C, B, V) >= 2 * C * S + C
    B, sp = R.grid_shape(8, chunk, ops.BN_MAX_WG)
    V = R.volume(sp)
    inside = [s for s in range(ops.bn_plan(8, B, V)) if ops.bn_share_range(8, B, V, s)[0] < V < ops.bn_share_range(8, B, V, s)[1]]
    assert len(inside) == 1, "the sample boundary of the GRID shape must fall inside a share"


def test_plan_limits():
    from dmvsnet_amd import _lib, ops
    lib = _lib.load()
    chunk = ops.BN_CHUNK
    for C in R.CHANNELS:
        smax = ops.BN_MAX_WG // C
        assert C * smax == ops.BN_MAX_WG
        assert ops.bn_plan(C, 1, 2) == 1 and ops.bn_plan(C, 1, chunk) == 1 and ops.bn_plan(C, 1, chunk - 1) == 1
        assert ops.bn_plan(C, 1, chunk + 1) == 2 and ops.bn_plan(C, 3, chunk) == 3
        assert ops.bn_plan(C, 1, smax * chunk) == smax == ops.bn_plan(C, 1, smax * chunk + 1) == ops.bn_plan(C, 7, 100 * smax * chunk)
        ws = lib.dmvs_bn_workspace(C, 1, 2)
        assert ws == lib.dmvs_bn_workspace(C, 4, 1 << 24) >= 2 * C * smax + C   # does not grow with the volume
    for C in (0, 4, 12, 24, 128, -8):
        assert lib.dmvs_bn_plan(C, 1, 64) == _lib.EINVAL and lib.dmvs_bn_workspace(C, 1, 64) == 0
        with pytest.raises(_lib.DmvsError):
            ops.bn_plan(C, 1, 64)
    for B, V in ((0, 8), (1, 0), (-1, 8), (2, 1 << 30)):
        assert lib.dmvs_bn_plan(8, B, V) == _lib.EINVAL and lib.dmvs_bn_workspace(8, B, V) == 0


def test_entries_refuse_bad_arguments():
    """Argument checks happen before anything is launched: no GPU needed (the pointers are never followed)."""
    from dmvsnet_amd import _lib, ops
    lib = _lib.load()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    train = ops.RELU | ops.BN_TRAIN
    fwd = lambda ptrs, B, C, V, flags, mom=0.1, eps=1e-5: lib.dmvs_bn_relu_forward(*ptrs, B, C, V, mom, eps, flags, None)
    bwd = lambda ptrs, B, C, V, flags: lib.dmvs_bn_relu_backward(*ptrs, B, C, V, flags, None)
    for C in (4, 12, 128, 0):
        assert fwd([p] * 9, 1, C, 64, train) == _lib.EINVAL and bwd([p] * 10, 1, C, 64, train) == _lib.EINVAL
    for i in range(9):
        assert fwd([None if j == i else p for j in range(9)], 1, 8, 64, train) == _lib.EINVAL
    for i in range(10):
        if i != 6:   # gx may be NULL (g_gamma / g_beta alone)
            assert bwd([None if j == i else p for j in range(10)], 1, 8, 64, train) == _lib.EINVAL
    for B, V in ((1, 1), (0, 8), (1, 0), (2, 1 << 30)):
        assert fwd([p] * 9, B, 8, V, train) == _lib.EINVAL and bwd([p] * 10, B, 8, V, train) == _lib.EINVAL
    assert fwd([p] * 9, 1, 8, 64, train | 2) == _lib.EINVAL and bwd([p] * 10, 1, 8, 64, 64) == _lib.EINVAL
    assert fwd([p] * 9, 1, 8, 64, train, mom=1.5) == _lib.EINVAL and fwd([p] * 9, 1, 8, 64, train, eps=-1.0) == _lib.EINVAL
    with pytest.raises(_lib.DmvsError, match="no CPU fallback"):
        ops.bn_relu_forward(torch.zeros(1, 8, 4, 4), torch.ones(8), torch.zeros(8), torch.zeros(8), torch.ones(8), 0.1, 1e-5, True, True)
    with pytest.raises(_lib.DmvsError, match="no CPU fallback"):
        ops.bn_relu_backward(torch.zeros(1, 8, 4, 4), torch.zeros(1, 8, 4, 4), torch.ones(8), torch.zeros(8), torch.zeros(8), torch.ones(8),
                             True, True)


def test_abi_agreement():
    from dmvsnet_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "dmvs.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/dmvs.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["dmvs_bn_relu_forward"][1]) == 16 and len(_lib.SIGNATURES["dmvs_bn_relu_backward"][1]) == 15
    assert _lib.SIGNATURES["dmvs_bn_workspace"][0] is ctypes.c_long
    declared = set(re.findall(r"\b(dmvs_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SIGNATURES)
    assert lib.dmvs_version() == _lib.ABI_VERSION == 140
    assert int(re.search(r"#define DMVS_BN_TRAIN (\d+)", header).group(1)) == ops.BN_TRAIN
    assert int(re.search(r"#define DMVS_RELU (\d+)", header).group(1)) == ops.RELU
    text = open(os.path.join(ROOT, "scripts", "pmc_summary.py")).read()
    assert all(k in text for k in KERNELS)
    src = open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "batchnorm.h")).read()
    assert set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src)) == KERNELS
    assert "atomic" not in src.lower().replace("nothing is atomic", "").replace("no atomics", "")
    assert int(re.search(r"kChunk = 4 \* kLanes", src) is not None) and ops.BN_CHUNK == 4 * int(re.search(r"kLanes = (\d+)", src).group(1))
    assert ops.BN_MAX_WG == int(re.search(r"kMaxWg = (\d+)", src).group(1))
    make = open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "Makefile")).read()
    assert "batchnorm.h" in make
    assert not os.path.exists(os.path.join(ROOT, "dmvsnet_amd", "csrc", "batchnorm.hip"))


# ------------------------------------------------------------------------------------------------ module
def test_constructor_refusals_and_state_dict_contract():
    import dmvsnet_amd
    from dmvsnet_amd import DiffBatchNormReLU2d, DiffBatchNormReLU3d, bn
    from dmvsnet_amd._lib import DmvsError
    assert all(n in dmvsnet_amd.__all__ for n in ("DiffBatchNormReLU3d", "DiffBatchNormReLU2d", "DiffConvBlock3d", "DiffDeconvBlock3d",
                                                  "DiffConvBlock2d", "DiffDeconvBlock2d"))
    assert bn.launch_counts == {"reduce": 0, "apply": 0} or set(bn.launch_counts) == {"reduce", "apply"}
    for cls, parent in ((DiffBatchNormReLU3d, nn.BatchNorm3d), (DiffBatchNormReLU2d, nn.BatchNorm2d)):
        for C in R.CHANNELS:
            m, ref = cls(C, momentum=0.01), parent(C, momentum=0.01)
            assert isinstance(m, parent) and m.relu is True and m.momentum == 0.01 and m.eps == ref.eps
            sd, rd = m.state_dict(), ref.state_dict()
            assert list(sd) == list(rd) == ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
            assert all(sd[k].shape == rd[k].shape and sd[k].dtype == rd[k].dtype for k in sd)
            assert [n for n, _ in m.named_parameters()] == ["weight", "bias"]
            with torch.no_grad():
                ref.weight.normal_(), ref.bias.normal_(), ref.running_mean.normal_(), ref.running_var.uniform_(0.5, 2.0)
                ref.num_batches_tracked.fill_(7)
            m.load_state_dict(ref.state_dict())
            assert all(torch.equal(m.state_dict()[k], ref.state_dict()[k]) for k in sd)
            back = parent(C)
            back.load_state_dict(m.state_dict())
            assert all(torch.equal(back.state_dict()[k], ref.state_dict()[k]) for k in sd)
        assert cls(8, relu=False).relu is False and "relu=False" in repr(cls(8, relu=False))
        for kw in (dict(affine=False), dict(track_running_stats=False), dict(momentum=None)):
            with pytest.raises(DmvsError):
                cls(8, **kw)
        for C in (1, 2, 4, 12, 24, 128):
            with pytest.raises(DmvsError):
                cls(C)


def test_input_refusals():
    from dmvsnet_amd import DiffBatchNormReLU2d, DiffBatchNormReLU3d, bn
    from dmvsnet_amd._lib import DmvsError
    m3, m2 = DiffBatchNormReLU3d(8), DiffBatchNormReLU2d(16)
    for m, x in ((m3, torch.zeros(1, 8, 2, 4, 4)), (m2, torch.zeros(2, 16, 4, 4))):
        with pytest.raises(DmvsError, match="no CPU fallback"):
            m(x)
        with pytest.raises(DmvsError):
            m("x")
    assert int(m3.num_batches_tracked) == 0   # a refused call does not count as a batch
    with pytest.raises(DmvsError, match="no CPU fallback"):
        bn._check_input("bn", torch.empty((1, 8, 2, 4, 4), device="meta"), 3, 8, True)
    # the refusals behind the device check, on the input's properties alone
    dev, f32 = torch.device("cuda", 0), torch.float32
    chk = lambda dtype, shape, contiguous, nd, C, training: bn._check_layout("bn", True, dev, dtype, torch.Size(shape), contiguous, nd, C, training)
    chk(f32, (1, 8, 2, 4, 4), True, 3, 8, True)
    chk(f32, (2, 16, 4, 4), True, 2, 16, True)
    chk(f32, (1, 8, 1, 1, 1), True, 3, 8, False)   # eval mode takes one value per channel
    for args in ((torch.float16, (1, 8, 2, 4, 4), True, 3, 8, True), (torch.float64, (1, 8, 2, 4, 4), True, 3, 8, True),
                 (f32, (1, 8, 4, 4), True, 3, 8, True), (f32, (1, 8, 2, 4, 4), True, 2, 8, True), (f32, (1, 16, 2, 4, 4), True, 3, 8, True),
                 (f32, (1, 8, 2, 4, 4), False, 3, 8, True), (f32, (1, 8, 1, 1, 1), True, 3, 8, True)):
        with pytest.raises(DmvsError):
            chk(*args)
    with pytest.raises(DmvsError, match="no CPU fallback"):
        bn._check_layout("bn", False, torch.device("cpu"), f32, torch.Size((1, 8, 2, 4, 4)), True, 3, 8, True)


class RefBlock(nn.Module):
    """The reference's block: layer + BatchNorm + ReLU."""

    def __init__(self, conv, bn):
        super().__init__()
        self.conv, self.bn = conv, bn


def test_blocks_have_the_reference_blocks_keys():
    from dmvsnet_amd import (DiffBatchNormReLU2d, DiffBatchNormReLU3d, DiffConv2d, DiffConv3d, DiffConvBlock2d, DiffConvBlock3d,
                             DiffConvTranspose2d, DiffConvTranspose3d, DiffDeconvBlock2d, DiffDeconvBlock3d)
    from dmvsnet_amd._lib import DmvsError
    keys = ["conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked"]
    cases = ((DiffConvBlock3d, (16, 16, 3), dict(padding=1), nn.Conv3d, nn.BatchNorm3d, DiffConv3d, DiffBatchNormReLU3d),
             (DiffConvBlock3d, (8, 16, 3), dict(stride=2, padding=1), nn.Conv3d, nn.BatchNorm3d, DiffConv3d, DiffBatchNormReLU3d),
             (DiffDeconvBlock3d, (16, 8, 3), dict(stride=2, padding=1, output_padding=1), nn.ConvTranspose3d, nn.BatchNorm3d,
              DiffConvTranspose3d, DiffBatchNormReLU3d),
             (DiffConvBlock2d, (64, 64, 3), dict(padding=1), nn.Conv2d, nn.BatchNorm2d, DiffConv2d, DiffBatchNormReLU2d),
             (DiffConvBlock2d, (32, 64, 3), dict(stride=2, padding=1), nn.Conv2d, nn.BatchNorm2d, DiffConv2d, DiffBatchNormReLU2d),
             (DiffDeconvBlock2d, (64, 32, 3), dict(stride=2, padding=1, output_padding=1), nn.ConvTranspose2d, nn.BatchNorm2d,
              DiffConvTranspose2d, DiffBatchNormReLU2d))
    for cls, args, kw, nn_conv, nn_bn, d_conv, d_bn in cases:
        m = cls(*args, bn_momentum=0.01, **kw)
        ref = RefBlock(nn_conv(*args, bias=False, **kw), nn_bn(args[1], momentum=0.01))
        assert list(m.state_dict()) == list(ref.state_dict()) == keys
        assert all(m.state_dict()[k].shape == ref.state_dict()[k].shape for k in keys)
        assert type(m.conv) is d_conv and type(m.bn) is d_bn and m.bn.momentum == 0.01 and m.bn.relu is True and m.conv.bias is None
        m.load_state_dict(ref.state_dict())
        ref.load_state_dict(m.state_dict())
        assert cls(*args, relu=False, **kw).bn.relu is False
        with pytest.raises(DmvsError):
            cls(*args, bn=False, **kw)
        m.init_weights("xavier")
        assert torch.equal(m.bn.weight, torch.ones(args[1])) and torch.equal(m.bn.bias, torch.zeros(args[1]))
    for cls, args, kw in ((DiffConvBlock3d, (8, 8, 3), dict(padding=1)), (DiffConvBlock3d, (1, 8, 3), dict(padding=1)),
                          (DiffConvBlock3d, (16, 16, 5), dict(padding=2)), (DiffDeconvBlock3d, (16, 8, 3), dict(stride=2, padding=1)),
                          (DiffConvBlock2d, (16, 32, 3), dict(stride=2, padding=1)), (DiffDeconvBlock2d, (32, 16, 3), dict(stride=2, padding=1, output_padding=1))):
        with pytest.raises(DmvsError):
            cls(*args, **kw)
