"""CPU (-m "not gpu"): the synchronised BatchNorm + ReLU without a GPU -- the yardstick (tests/bn_sync_ref.py: the combine of per-rank
moments in float64 against ``bn_grad_ref.stats`` of the concatenated batch, and a raw-sums combine in fp32 that fails the same table),
the ABI surface of the four new entries and their refusals, the converter on whole networks, the guard behind the stock converter, and
what the wrappers and the autograd Function launch, in which order, with the recording library of tests/test_train_dispatch.py."""
import ctypes
import os
import re
import types

import pytest
import torch
from torch import nn

import bn_grad_ref as G
import bn_sync_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dmvs_bn_sync_moments", "dmvs_bn_sync_forward", "dmvs_bn_sync_backward_sums", "dmvs_bn_sync_backward_apply")

# pieces (whole samples per rank) x per-rank offsets of the combine table; std 0.1 (variance 1e-2) where offsets are given
TABLE = {"two_equal": ((1, 1), None), "uneven": ((1, 2, 1), None), "eight": ((1,) * 8, None), "one_rank": ((3,), None),
         "offset_pm1e3": ((1, 1), (1e3, -1e3)), "offset_mixed": ((1, 2, 1, 1, 1), (1e3, -1e3, 1.0, -1.0, 0.0)),
         "offset_same_1e3": ((2, 1), (1e3, 1e3))}


def _table_case(name, spatial=(2, 5, 9)):
    pieces, offsets = TABLE[name]
    return pieces, S.make_pieces(8, pieces, spatial, 3, offsets, 0.1 if offsets else 1.0)["x"].double()


# ------------------------------------------------------------------------------------------------ yardstick
@pytest.mark.parametrize("name", list(TABLE))
def test_combine_equals_the_statistics_of_the_concatenated_batch(name):
    pieces, x = _table_case(name)
    gathered = torch.stack([S.moments(p) for p in S.split(x, pieces)])
    assert gathered.dtype == torch.float64 and tuple(gathered.shape) == (len(pieces), 8, 3)
    N, mean, var, M2 = S.combine(gathered)
    m64, v64, _ = G.stats(x)
    e_mean = ((mean - m64).abs().max() / m64.abs().max().clamp_min(1.0)).item()
    e_var = ((var - v64).abs().max() / v64.abs().max()).item()
    print(f"COMBINE {name}: N {int(N[0])}, mean {e_mean:.3e}, var {e_var:.3e} (bound 1e-12)")
    assert torch.equal(N, torch.full_like(N, x.numel() // 8))
    assert e_mean <= 1e-12 and e_var <= 1e-12


def test_single_value_ranks():
    """n_r = 1: M2_r = 0 and the variance is all between the ranks."""
    x = torch.tensor([[[3.0]] * 8, [[5.0]] * 8], dtype=torch.float64)   # [2, 8, 1]
    gathered = torch.stack([S.moments(p) for p in S.split(x, (1, 1))])
    assert torch.equal(gathered[:, :, 2], torch.zeros(2, 8, dtype=torch.float64))
    N, mean, var, M2 = S.combine(gathered)
    assert torch.equal(N, torch.full((8,), 2.0, dtype=torch.float64)) and torch.equal(mean, torch.full_like(mean, 4.0))
    assert torch.equal(var, torch.full_like(var, 1.0)) and torch.equal(M2 / (N - 1), torch.full_like(var, 2.0))


@pytest.mark.parametrize("name", ["offset_pm1e3", "offset_mixed", "offset_same_1e3"])
def test_raw_sums_in_fp32_fail_the_same_table(name):
    """The table discriminates: (n, sum x, sum x^2) shipped in fp32 misses the variance by orders of magnitude where fp32 MOMENTS (the
    combine formula run in fp32 on fp32 moments) still hold it to fp32 accuracy."""
    pieces, x = _table_case(name)
    x = x.float()                 # (the fp32 tensor is the input: its float64 statistics are the yardstick)
    _, v64, _ = G.stats(x)
    _, var_raw = S.combine_raw_sums_fp32(S.split(x, pieces))
    _, _, var_mom, _ = S.combine(torch.stack([S.moments(p, torch.float32) for p in S.split(x, pieces)]))
    e_raw, e_mom = G.rel_dist(var_raw, v64), G.rel_dist(var_mom, v64)
    print(f"RAW {name}: var max {v64.max():.3e}; raw fp32 sums {e_raw:.3e}, fp32 moments {e_mom:.3e}")
    # fp32 moments: a piece mean near 1e3 carries a few ulp(1e3) = 6e-5 of error (delta <= 2.4e-4), which enters the between-piece term
    # as 2 d delta / var with |d| <= 0.02 between piece means at std 0.1: 1e-3 of a variance of 1e-2, less elsewhere
    assert e_mom <= 1e-3
    if name == "offset_same_1e3":   # total variance 1e-2 at a mean of 1e3: the raw form has no correct digit
        assert e_raw > 1e3 * max(e_mom, 1e-12) and e_raw > 0.1


def test_per_rank_yardstick_adds_up():
    """The per-rank slices of the float64 restatement: local parameter gradients sum to the global ones, slices concatenate back."""
    pieces = (1, 2, 1)
    case, _ = S.first_clean_pieces(8, pieces, (2, 5, 9))
    assert G.kink_violations(case) == 0
    ranks = S.f64_per_rank(case, pieces, 0.1)
    f64 = G.all_f64(**case)
    assert torch.equal(torch.cat([r["y"] for r in ranks]), f64["y"]) and torch.equal(torch.cat([r["g_x"] for r in ranks]), f64["g_x"])
    for k in ("g_gamma", "g_beta"):
        assert G.rel_dist(sum(r[k] for r in ranks), f64[k]) <= 1e-13


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_surface():
    from dmvsnet_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "dmvs.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/dmvs.h"
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert set(re.findall(r"\b(dmvs_[a-z0-9_]+)\s*\(", header)) == set(_lib.SIGNATURES)
    assert lib.dmvs_version() == _lib.ABI_VERSION == 140   # additive: the ABI version does not move
    src = open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "batchnorm_sync.h")).read()
    assert re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src) == ["bn_moments_kernel"]
    k5 = open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "batchnorm.h")).read()
    assert ops.BN_MAX_RANKS == int(re.search(r"kMaxRanks = (\d+)", k5).group(1)) >= 16
    assert '#include "batchnorm_sync.h"' in k5
    assert "atomic" not in src.lower()


def test_entries_refuse_bad_arguments():
    """Checked before any launch and before the gathered buffer is read: no GPU needed (the pointers are never followed)."""
    from dmvsnet_amd import _lib, ops
    lib, EINVAL = _lib.load(), _lib.EINVAL
    buf = (ctypes.c_double * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    n = ctypes.c_long(-7)
    mom = lambda ptrs, B, C, V: lib.dmvs_bn_sync_moments(*ptrs, B, C, V, None)
    fwd = lambda ptrs, B, C, V, R, flags=1, m=0.1, eps=1e-5: lib.dmvs_bn_sync_forward(*ptrs, ctypes.byref(n), B, C, V, R, m, eps, flags, None)
    sums = lambda ptrs, B, C, V, flags=1: lib.dmvs_bn_sync_backward_sums(*ptrs, B, C, V, flags, None)
    app = lambda ptrs, B, C, V, R, N, flags=1: lib.dmvs_bn_sync_backward_apply(*ptrs, B, C, V, R, N, flags, None)
    for C in (4, 12, 128, 0):
        assert mom([p] * 3, 1, C, 64) == EINVAL and fwd([p] * 9, 1, C, 64, 2) == EINVAL
        assert sums([p] * 10, 1, C, 64) == EINVAL and app([p] * 8, 1, C, 64, 2, 128) == EINVAL
    for i in range(3):
        assert mom([None if j == i else p for j in range(3)], 1, 8, 64) == EINVAL
    for i in range(9):
        assert fwd([None if j == i else p for j in range(9)], 1, 8, 64, 2) == EINVAL
    assert lib.dmvs_bn_sync_forward(*[p] * 9, None, 1, 8, 64, 2, 0.1, 1e-5, 1, None) == EINVAL
    for i in range(10):
        assert sums([None if j == i else p for j in range(10)], 1, 8, 64) == EINVAL
    for i in range(8):   # gx too: a caller that wants no gx does not call the apply entry
        assert app([None if j == i else p for j in range(8)], 1, 8, 64, 2, 128) == EINVAL
    for B, V in ((0, 8), (1, 0), (2, 1 << 30)):
        assert mom([p] * 3, B, 8, V) == EINVAL and fwd([p] * 9, B, 8, V, 2) == EINVAL
        assert sums([p] * 10, B, 8, V) == EINVAL and app([p] * 8, B, 8, V, 2, 1 << 20) == EINVAL
    for R in (0, -1, ops.BN_MAX_RANKS + 1, 1 << 20):
        assert fwd([p] * 9, 1, 8, 64, R) == EINVAL and app([p] * 8, 1, 8, 64, R, 128) == EINVAL
    for N in (1, 0, -5, 63):   # below two, or below this rank's own 64 values
        assert app([p] * 8, 1, 8, 64, 2, N) == EINVAL
    assert app([p] * 8, 1, 8, 1, 2, 1) == EINVAL   # one value on this rank is fine, one value in all is not
    for flags in (2, 32, 33, 64):   # DMVS_RELU alone: there is no eval form, DMVS_BN_TRAIN is not an argument
        assert fwd([p] * 9, 1, 8, 64, 2, flags) == EINVAL and sums([p] * 10, 1, 8, 64, flags) == EINVAL
        assert app([p] * 8, 1, 8, 64, 2, 128, flags) == EINVAL
    assert fwd([p] * 9, 1, 8, 64, 2, m=1.5) == EINVAL and fwd([p] * 9, 1, 8, 64, 2, eps=-1.0) == EINVAL
    assert n.value == -7   # a refused forward leaves the count alone
    x = torch.zeros(1, 8, 4, 4)
    v = [torch.ones(8), torch.zeros(8), torch.zeros(8), torch.ones(8)]
    with pytest.raises(_lib.DmvsError, match="no CPU fallback"):
        ops.bn_sync_moments(x)
    with pytest.raises(_lib.DmvsError, match="no CPU fallback"):
        ops.bn_sync_forward(x, *v, torch.zeros(2, 8, 3, dtype=torch.float64), 0.1, 1e-5, True)
    with pytest.raises(_lib.DmvsError, match="no CPU fallback"):
        ops.bn_sync_backward_sums(x, x, *v, True)
    with pytest.raises(_lib.DmvsError, match="no CPU fallback"):
        ops.bn_sync_backward_apply(x, x, *v, torch.zeros(2, 8, 2, dtype=torch.float64), 32, True)


# ------------------------------------------------------------------------------------------------ modules and converter
def test_all_and_module_contract():
    import dmvsnet_amd
    from dmvsnet_amd import (DiffBatchNormReLU2d, DiffBatchNormReLU3d, DiffSyncBatchNormReLU2d, DiffSyncBatchNormReLU3d, bn,
                             convert_sync_batchnorm)
    from dmvsnet_amd._lib import DmvsError
    for n in ("DiffSyncBatchNormReLU3d", "DiffSyncBatchNormReLU2d", "convert_sync_batchnorm"):
        assert n in dmvsnet_amd.__all__ and n in bn.__all__ and getattr(dmvsnet_amd, n) is getattr(bn, n)
    assert set(bn.sync_launch_counts) == {"moments", "sums", "apply", "gather"} and set(bn.launch_counts) == {"reduce", "apply"}
    for cls, plain, parent in ((DiffSyncBatchNormReLU3d, DiffBatchNormReLU3d, nn.BatchNorm3d),
                               (DiffSyncBatchNormReLU2d, DiffBatchNormReLU2d, nn.BatchNorm2d)):
        m, ref = cls(16, momentum=0.01, relu=False, process_group=None), plain(16, momentum=0.01, relu=False)
        assert isinstance(m, parent) and not isinstance(m, plain) and m.relu is False and m.momentum == 0.01 and m.process_group is None
        assert list(m.state_dict()) == list(ref.state_dict()) == ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
        with torch.no_grad():
            ref.weight.normal_(), ref.bias.normal_(), ref.running_mean.normal_(), ref.num_batches_tracked.fill_(7)
        m.load_state_dict(ref.state_dict(), strict=True)
        back = plain(16)
        back.load_state_dict(m.state_dict(), strict=True)
        assert all(torch.equal(back.state_dict()[k], ref.state_dict()[k]) for k in ref.state_dict())
        assert "relu=False" in repr(m) and "process_group" in repr(m)
        for kw in (dict(affine=False), dict(track_running_stats=False), dict(momentum=None)):
            with pytest.raises(DmvsError):
                cls(8, **kw)
        for C in (1, 4, 12, 128):
            with pytest.raises(DmvsError):
                cls(C)
        with pytest.raises(DmvsError, match="no CPU fallback"):
            cls(8)(torch.zeros((2, 8) + (2,) * m._nd))
        assert bn._sync_world(None) == 1 and cls(8).train()._sync() is None and cls(8).eval()._sync() is None


def _nets():
    import dmvsnet_amd as da
    return {"regnet_part": da.DiffCostRegNetPart(2, 8), "featurenet": da.DiffFeatureNet(8)}


@pytest.mark.parametrize("which", ["regnet_part", "featurenet"])
def test_converter_on_whole_networks(which):
    import dmvsnet_amd as da
    from dmvsnet_amd.bn import _DiffBatchNormReLU, _DiffSyncBatchNormReLU
    net = _nets()[which]
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for t in list(net.parameters()) + [b for b in net.buffers() if b.dtype.is_floating_point]:
            t.copy_(torch.rand(t.shape, generator=g) + 0.5)
    plain = {n: m for n, m in net.named_modules() if isinstance(m, _DiffBatchNormReLU)}
    assert len(plain) >= 5 and not any(isinstance(m, _DiffSyncBatchNormReLU) for m in plain.values())
    first = next(iter(plain.values()))
    first.momentum, first.relu, first.eps = 0.37, False, 3e-4
    first.eval()                                              # a frozen layer stays frozen
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    params = dict(net.named_parameters())
    others = {n: m for n, m in net.named_modules() if not isinstance(m, _DiffBatchNormReLU) and not list(m.children())}
    group = object()
    out = da.convert_sync_batchnorm(net, group)
    assert out is net
    after = {n: m for n, m in net.named_modules() if isinstance(m, _DiffBatchNormReLU)}
    assert list(after) == list(plain)
    for n, m in after.items():
        old = plain[n]
        assert type(m) is (da.DiffSyncBatchNormReLU3d if isinstance(old, nn.BatchNorm3d) else da.DiffSyncBatchNormReLU2d)
        assert (m.relu, m.momentum, m.eps, m.training, m.num_features) == (old.relu, old.momentum, old.eps, old.training, old.num_features)
        assert m.process_group is group
        assert m.weight is old.weight and m.bias is old.bias and m.running_mean is old.running_mean and m.running_var is old.running_var
        assert m.num_batches_tracked is old.num_batches_tracked
    new_first = next(iter(after.values()))
    assert (new_first.momentum, new_first.relu, new_first.eps, new_first.training) == (0.37, False, 3e-4, False)
    assert all(m is dict(net.named_modules())[n] for n, m in others.items())          # everything else is left alone
    assert list(net.state_dict()) == list(sd) and all(torch.equal(net.state_dict()[k], v) for k, v in sd.items())
    assert all(p is params[n] for n, p in net.named_parameters())                     # the parameter objects are kept
    fresh = _nets()[which]
    fresh.load_state_dict(net.state_dict(), strict=True)                              # sync -> plain
    da.convert_sync_batchnorm(_nets()[which]).load_state_dict(fresh.state_dict(), strict=True)   # plain -> sync
    again = da.convert_sync_batchnorm(net, None)                                      # already converted: left alone
    assert all(m is dict(again.named_modules())[n] for n, m in after.items())


def test_converter_on_a_bare_module_and_foreign_modules():
    import dmvsnet_amd as da
    m = da.DiffBatchNormReLU2d(32, momentum=0.2, relu=False).eval()
    s = da.convert_sync_batchnorm(m)
    assert type(s) is da.DiffSyncBatchNormReLU2d and s is not m and s.weight is m.weight and not s.training and s.process_group is None
    stock = nn.Sequential(nn.Conv3d(2, 8, 3), nn.BatchNorm3d(8), nn.ReLU())
    kids = list(stock.children())
    assert da.convert_sync_batchnorm(stock) is stock and list(stock.children()) == kids   # a stock BatchNorm is not ours to convert


@pytest.mark.parametrize("which", ["regnet_part", "featurenet"])
def test_stock_converter_is_refused_at_the_first_block(which):
    """torch.nn.SyncBatchNorm.convert_sync_batchnorm swaps this package's BatchNorm + ReLU for ATen's and drops the fused ReLU: every
    block it went over raises and names the converter to use (before the change it ran, and computed another function)."""
    from dmvsnet_amd._lib import DmvsError
    from dmvsnet_amd.bn import _DiffBlock
    net = torch.nn.SyncBatchNorm.convert_sync_batchnorm(_nets()[which])
    blocks = [m for m in net.modules() if isinstance(m, _DiffBlock)]
    assert blocks and all(type(b.bn) is torch.nn.SyncBatchNorm for b in blocks)
    if which == "regnet_part":   # (DiffFeatureNet looks at the input's device before its first block)
        with pytest.raises(DmvsError, match=r"dmvsnet_amd\.convert_sync_batchnorm"):
            net(torch.zeros(1, 2, 8, 8, 8))
    for b in blocks:
        nd = 2 if isinstance(b.conv, (nn.Conv2d, nn.ConvTranspose2d)) else 3
        with pytest.raises(DmvsError, match=r"dmvsnet_amd\.convert_sync_batchnorm"):
            b(torch.zeros((1, b.conv.in_channels) + (4,) * nd))


def test_train_still_raises():
    import dmvsnet_amd as da
    with pytest.raises(NotImplementedError):
        da.MVSNet([8], [4], verbose=False).train()
