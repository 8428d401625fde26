"""CPU (-m "not gpu"): the differentiable FeatureNet (K3f, the four new K3 rows, ``dmvsnet_amd.featurenet``) without a GPU.

* the float64 restatement (tests/featurenet_grad_ref.py) against float64 autograd of F.conv2d / the stock nn network to 1e-12;
* the stored fixture (tests/golden/op_featurenet_grad.npz): its condition (no BatchNorm output on the ReLU kink) and its sanity;
* ops.pack_index_mfma_fpn against the host packer, bit for bit, and cached; the plan and workspace entries; the C ABI;
* the constructor contracts and refusals of the three classes, the strict state-dict load, the refusals of CPU inputs;
* with a fake library (the pattern of tests/test_conv_k5s2_grad_cpu.py): the exact entry and integer arguments of every launch of a
  forward + backward of each layer, and the launches of the whole network."""
import contextlib
import copy
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import featurenet_grad_ref as R
import dmvsnet_amd
from dmvsnet_amd import _lib, bn, conv, featurenet, ops
from dmvsnet_amd import DiffConv2d, DiffConvBlock2d, DiffFeatureConv2d, DiffFeatureConvBlock2d, DiffFeatureNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = _lib.EINVAL, _lib.EUNSUPPORTED
ENTRIES = ("dmvs_conv2d_wgrad_fpn", "dmvs_conv2d_wgrad_fpn_workspace", "dmvs_conv2d_wgrad_fpn_plan")
KERNELS = {"conv_wgrad_fpn_kernel", "conv_wgrad_fpn_reduce_kernel"}
LAYER_IDS = [l[0] for l in R.LAYERS]


def _ctor(cin, cout, k, bias):
    return DiffFeatureConv2d(cin, cout, k, padding=k // 2, bias=bias)


# ------------------------------------------------------------------------------------------ the yardstick itself
@pytest.mark.parametrize("shape", R.SHAPES[:5], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name,cin,cout,k,bias", R.LAYERS, ids=LAYER_IDS)
def test_restatement_against_float64_autograd(name, cin, cout, k, bias, shape):
    D, H, W = shape
    gen = torch.Generator().manual_seed(cin + H * W)
    x = torch.randn(D, cin, H, W, dtype=torch.float64, generator=gen).requires_grad_(True)
    w = torch.randn(cout, cin, k, k, dtype=torch.float64, generator=gen).requires_grad_(True)
    b = torch.randn(cout, dtype=torch.float64, generator=gen).requires_grad_(True) if bias else None
    y = F.conv2d(x, w, b, padding=k // 2)
    gy = torch.randn(y.shape, dtype=torch.float64, generator=gen)
    leaves = [x, w] + ([b] if bias else [])
    grads = torch.autograd.grad(y, leaves, gy)
    assert R.rel_dist(R.conv_ref(x, w, b), y) <= 1e-12
    assert R.rel_dist(R.dgrad_ref(gy, w), grads[0]) <= 1e-12
    assert R.rel_dist(R.wgrad_ref(gy, x, k), grads[1]) <= 1e-12
    if bias:
        assert R.rel_dist(R.bgrad_ref(gy), grads[2]) <= 1e-12
    # autograd over the restatement is the gradient restatements
    grads2 = torch.autograd.grad(R.conv_ref(x, w, b), leaves, gy)
    assert all(R.rel_dist(a, c) <= 1e-12 for a, c in zip(grads2, grads))


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_network_restatement_against_the_stock_network(train):
    case = R.make_net_case(2, 8, 12, 1)
    if not train:   # running statistics that are not the identity
        gen = torch.Generator().manual_seed(5)
        for k in case["sd"]:
            if k.endswith("running_mean"):
                case["sd"][k] = 0.1 * torch.randn(case["sd"][k].shape, generator=gen)
            elif k.endswith("running_var"):
                case["sd"][k] = 0.5 + torch.rand(case["sd"][k].shape, generator=gen)
    net = R.StockFeatureNet()
    net.load_state_dict(case["sd"], strict=True)
    net = net.double().train(train)
    want = R.run_module(net, case, dtype=torch.float64)
    got = R.run_net(case, train=train)
    assert list(want["g"]) == R.param_keys() == list(got["g"])
    for k in R.OUT_KEYS:
        assert tuple(got["out"][k].shape) == R.out_shapes(2, 8, 12)[k] and R.rel_dist(got["out"][k], want["out"][k]) <= 1e-12, k
    for k in R.param_keys():
        assert R.rel_dist(got["g"][k], want["g"][k]) <= 1e-12, k


def test_up2_is_nearest_interpolation():
    t = torch.randn(2, 3, 4, 5, dtype=torch.float64)
    assert torch.equal(R.up2(t), F.interpolate(t, scale_factor=2, mode="nearest"))


# ------------------------------------------------------------------------------------------ the fixture
@pytest.fixture(scope="module")
def g():
    path = os.path.join(ROOT, "tests", "golden", "op_featurenet_grad.npz")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "op_conv_grad.npz"))
    return np.load(path)


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_fixture_condition_and_sanity(g, name):
    kw = R.GOLDEN_CASES[name]
    case = R.golden_case(g, name)
    made = R.make_net_case(**kw)
    assert torch.equal(made["x"], case["x"]) and tuple(case["x"].shape) == (kw["B"], 3, kw["H"], kw["W"])
    assert list(case["sd"]) == R.state_dict_keys()
    for k in R.state_dict_keys():
        assert torch.equal(made["sd"][k], case["sd"][k]), k   # the stored inputs are the generator's
    f64 = R.run_net(case)
    assert f64["nearest_kink"] > R.KINK_MARGIN
    for k in R.OUT_KEYS:
        assert torch.equal(made["gys"][k], case["gys"][k])
        assert tuple(case["out"][k].shape) == R.out_shapes(kw["B"], kw["H"], kw["W"])[k] and case["out"][k].dtype == torch.float32
        assert R.rel_dist(case["out"][k], f64["out"][k]) < 1e-5, k   # sanity: the same function
    for k in R.param_keys():
        assert case["g"][k].shape == case["sd"][k].shape and R.rel_dist(case["g"][k], f64["g"][k]) < 1e-5, k
    if name == "b1_20x36":
        assert tuple(case["out"]["stage1"].shape[-2:]) == (5, 9)   # odd extents at the conv2 level


def test_fixture_keys(g):
    want = {f"sd.{k}" for k in R.state_dict_keys()}
    for n in R.GOLDEN_CASES:
        want |= {f"{n}.x"} | {f"{n}.{p}.{k}" for p in ("gy", "out") for k in R.OUT_KEYS} | {f"{n}.g.{k}" for k in R.param_keys()}
    assert set(g.files) == want


# ------------------------------------------------------------------------------------------ host-side library entries
@pytest.mark.parametrize("tf", [False, True], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("name,cin,cout,k,bias", R.LAYERS, ids=LAYER_IDS)
def test_pack_index_is_the_host_packer(name, cin, cout, k, bias, tf):
    if tf and cin == 3:
        with pytest.raises(_lib.DmvsError, match="no data gradient"):
            ops.pack_index_mfma_fpn(cin, cout, k, True)
        return
    w = torch.randn(cout, cin, k, k, generator=torch.Generator().manual_seed(cin + cout))
    idx = ops.pack_index_mfma_fpn(cin, cout, k, tf)
    wl, lin, lout = (w.transpose(0, 1).flip(2, 3).contiguous(), cout, cin) if tf else (w, cin, cout)
    mode = ops.CONV_S1 if k == 3 else ops.CONV2D_K1
    if lin == 3:
        want = ops.make_layer("l", mode, wl, None, None, False).w_mfma   # make_layer adds the zero fourth channel
    else:
        want = ops.pack_mfma(wl, lin, lout, mode, 1)
    got = torch.cat((w.reshape(-1), torch.zeros(1)))[idx]
    assert idx.dtype == torch.int64 and got.shape == want.shape
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert ops.pack_index_mfma_fpn(cin, cout, k, tf) is idx
    n = cin * cout * k * k
    assert int((idx == n).sum()) == idx.numel() - n   # every zero of the packed form is the appended slot


def test_pack_index_refusals_and_existing_rows():
    for bad in ((8, 3, 3), (16, 16, 3), (32, 64, 3), (8, 32, 3), (3, 8, 1)):
        with pytest.raises(_lib.DmvsError):
            ops.pack_index_mfma_fpn(*bad, False)
    with pytest.raises(_lib.DmvsError):
        ops.pack_index_mfma(8, 3, False)   # the square index keeps refusing C = 8
    lib = _lib.load()
    # the new rows: the data gradients' layers, and nothing else
    for cin, cout, mode in ((16, 32, ops.CONV_S1), (64, 32, ops.CONV2D_K1), (32, 16, ops.CONV2D_K1), (32, 8, ops.CONV2D_K1)):
        assert lib.dmvs_conv3d_mfma_weight_floats(cin, cout, mode, 1) > 0
        assert lib.dmvs_conv3d_mfma_weight_floats(cin, cout, mode, 3) == 0
    assert lib.dmvs_conv3d_mfma_weight_floats(8, 4, ops.CONV_S1, 1) == 0 and lib.dmvs_conv3d_mfma_weight_floats(64, 16, ops.CONV2D_K1, 1) == 0
    # the rows an existing (Cin, Cout, mode, kdepth) finds are what they were
    assert lib.dmvs_conv3d_mfma_weight_floats(32, 16, ops.CONV_S1, 1) == 9 * 8 * 64
    assert lib.dmvs_conv3d_mfma_weight_floats(32, 64, ops.CONV2D_K1, 1) == 16 * 2 * 64
    assert lib.dmvs_conv3d_mfma_weight_floats(8, 32, ops.CONV2D_K1, 1) == 4 * 64


def test_plan_and_workspace():
    lib = _lib.load()
    assert ops.FPN_SHAPES == R.SHAPES3 and ops.WGRAD_FPN_TILE == (1, 4, 32)
    _, ty, tx = ops.WGRAD_FPN_TILE
    for name, cin, cout, k, bias in R.LAYERS:
        ws = lib.dmvs_conv2d_wgrad_fpn_workspace(cin, cout, k, 1, 5, 8)
        assert ws == 256 * cout * (cin * k * k + int(bias))
        for D, H, W in R.SHAPES + ((1, 136, 1040), (3, 512, 640), (1, 1184, 1600)):
            tiles = D * -(-H // ty) * -(-W // tx)
            plan = lib.dmvs_conv2d_wgrad_fpn_plan(cin, cout, k, D, H, W)
            assert plan // 512 == tiles and plan % 512 == 8 * -(-min(tiles, 256) // 8) <= 256, (name, D, H, W, plan)
            assert lib.dmvs_conv2d_wgrad_fpn_workspace(cin, cout, k, D, H, W) == ws   # whatever the planes
        for bad in ((0, 5, 8), (1, 0, 8), (1, 5, 0), (-1, 5, 8)):
            assert lib.dmvs_conv2d_wgrad_fpn_plan(cin, cout, k, *bad) == EINVAL and lib.dmvs_conv2d_wgrad_fpn_workspace(cin, cout, k, *bad) == 0
    assert lib.dmvs_conv2d_wgrad_fpn_plan(8, 8, 3, 1 << 20, 64, 64) == EINVAL   # 2^22 tiles
    for cin, cout, k in ((8, 8, 1), (3, 8, 1), (8, 3, 3), (16, 16, 3), (32, 64, 3), (32, 16, 1), (8, 32, 5), (64, 32, 1)):
        assert lib.dmvs_conv2d_wgrad_fpn_plan(cin, cout, k, 1, 5, 8) == EUNSUPPORTED
        assert lib.dmvs_conv2d_wgrad_fpn_workspace(cin, cout, k, 1, 5, 8) == 0
    # null pointers are refused on the host, before any launch
    assert lib.dmvs_conv2d_wgrad_fpn(None, None, None, None, None, 8, 8, 1, 5, 8, 3, 0, None) == EINVAL
    # the existing refusals stay
    assert lib.dmvs_conv3d_wgrad_plan(8, 1, 5, 8, 1) == EUNSUPPORTED


def test_c_abi_and_sources():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dmvs.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/dmvs.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for line in (":284", ":285", ":301", ":305", ":306", ":309"):
        assert line in header[header.index("K3f:"):header.index("dmvs_conv2d_wgrad_fpn_plan(")]
    assert len(_lib.SIGNATURES["dmvs_conv2d_wgrad_fpn"][1]) == 13 and len(_lib.SIGNATURES["dmvs_conv2d_wgrad_fpn_plan"][1]) == 6
    src = open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "conv2d_wgrad_fpn.h")).read()
    assert set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src)) == KERNELS
    assert "atomic" not in src.lower().replace("no atomics", "")
    shared = open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "wgrad_share.h")).read()
    assert "atomic" not in shared.lower().replace("no atomics", "")
    doc = open(os.path.join(ROOT, "docs", "kernels", "K3f_conv_wgrad_fpn.md")).read()
    assert set(re.findall(r"`(conv_\w+_kernel)`", doc)) == KERNELS
    direct = open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "conv3d_direct.hip")).read()
    assert direct.index('#include "conv2d_wgrad_fpn.h"') > direct.index('#include "conv2d_k5s2_bwd.h"')
    assert "conv2d_wgrad_fpn.h" in open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "Makefile")).read()
    for name in ("featurenet", "DiffFeatureConv2d", "DiffFeatureConvBlock2d", "DiffFeatureNet"):
        assert name in dmvsnet_amd.__all__ and hasattr(dmvsnet_amd, name)


# ------------------------------------------------------------------------------------------ the constructors
@pytest.mark.parametrize("name,cin,cout,k,bias", R.LAYERS, ids=LAYER_IDS)
def test_constructor_contract(name, cin, cout, k, bias):
    assert featurenet.SHAPES == R.SHAPES3 and featurenet.BIAS_SHAPES == tuple(s[1:4] for s in R.LAYERS if s[4])
    m = _ctor(cin, cout, k, bias)
    assert isinstance(m, nn.Conv2d) and list(m.state_dict()) == ["weight"] + (["bias"] if bias else [])
    stock = nn.Conv2d(cin, cout, k, padding=k // 2, bias=bias)
    m.load_state_dict(stock.state_dict())
    assert torch.equal(m.weight, stock.weight)
    with pytest.raises(_lib.DmvsError, match="no ATen fallback"):
        _ctor(cin, cout, k, not bias)   # a bias exactly where the reference has one
    with pytest.raises(_lib.DmvsError, match="no ATen fallback"):
        DiffConv2d(cin, cout, k, padding=k // 2, bias=False)   # DiffConv2d keeps refusing the six shapes


@pytest.mark.parametrize("kw", [dict(stride=2), dict(padding=0), dict(padding=2), dict(dilation=2), dict(groups=2), dict(padding_mode="reflect")],
                         ids=lambda kw: "%s%s" % next(iter(kw.items())))
def test_constructor_refusals_by_argument(kw):
    args = dict(padding=1, bias=False)
    args.update(kw)
    with pytest.raises(_lib.DmvsError, match="no ATen fallback"):
        DiffFeatureConv2d(8, 8, 3, **args)


@pytest.mark.parametrize("cin,cout,k", [(16, 16, 3), (32, 32, 3), (8, 16, 3), (8, 3, 3), (32, 16, 1), (8, 8, 1), (8, 16, 5), (64, 32, 1)])
def test_constructor_refusals_by_shape(cin, cout, k):
    with pytest.raises(_lib.DmvsError, match="no ATen fallback"):
        DiffFeatureConv2d(cin, cout, k, padding=k // 2, bias=False)


def test_block_and_network_contract():
    blk = DiffFeatureConvBlock2d(3, 8, 3, 1, padding=1)
    assert isinstance(blk.conv, DiffFeatureConv2d) and isinstance(blk.bn, bn.DiffBatchNormReLU2d)
    assert list(blk.state_dict()) == list(R.StockBlock(3, 8, 3, 1).state_dict())
    with pytest.raises(_lib.DmvsError):
        DiffFeatureConvBlock2d(3, 8, 3, 1, padding=1, bn=False)
    with pytest.raises(_lib.DmvsError, match="no ATen fallback"):
        DiffFeatureConvBlock2d(16, 16, 3, 1, padding=1)
    with pytest.raises(_lib.DmvsError, match="no ATen fallback"):
        DiffConvBlock2d(8, 8, 3, 1, padding=1)
    net = DiffFeatureNet(8)
    assert net.out_channels == [32, 16, 8] and (net.mode, net.stride, net.base_channels, net.num_stage, net.layernorm) == ("fpn", 4, 8, 3, False)
    assert [n for n, _ in net.named_children()] == ["conv0", "conv1", "conv2", "out1", "inner1", "inner2", "out2", "out3"]
    assert list(net.state_dict()) == R.state_dict_keys()
    assert isinstance(net.out2, DiffConv2d) and not isinstance(net.out2, DiffFeatureConv2d)
    assert all(isinstance(b, DiffFeatureConvBlock2d) for b in net.conv0) and all(isinstance(b, DiffConvBlock2d) for b in (*net.conv1, *net.conv2))
    assert all(isinstance(m, DiffFeatureConv2d) for m in (net.out1, net.inner1, net.inner2, net.out3))
    for bad in (dict(base_channels=16), dict(base_channels=8, num_stage=2), dict(base_channels=8, mode="unet")):
        with pytest.raises(_lib.DmvsError, match="no ATen fallback"):
            DiffFeatureNet(**bad)
    with pytest.raises(NotImplementedError):
        dmvsnet_amd.MVSNet([8], [4], verbose=False).train()


def test_strict_state_dict_load_from_a_stock_replica(g):
    stock = R.StockFeatureNet()
    net = DiffFeatureNet(8)
    assert list(stock.state_dict()) == list(net.state_dict())
    net.load_state_dict(stock.state_dict(), strict=True)
    net.load_state_dict(R.golden_case(g, "b2_16x24")["sd"], strict=True)
    for (ka, a), (kb, b) in zip(net.state_dict().items(), R.golden_case(g, "b2_16x24")["sd"].items()):
        assert ka == kb and torch.equal(a, b)
    net2 = copy.deepcopy(net)
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), net2.state_dict().values()))


def test_cpu_inputs_are_refused():
    net = DiffFeatureNet(8)
    with pytest.raises(_lib.DmvsError, match="no CPU fallback"):
        net(torch.zeros(1, 3, 8, 8))
    for name, cin, cout, k, bias in R.LAYERS:
        with pytest.raises(_lib.DmvsError, match="no CPU fallback"):
            _ctor(cin, cout, k, bias)(torch.zeros(1, cin, 4, 4))
    with pytest.raises(_lib.DmvsError, match="no CPU fallback"):
        DiffFeatureConvBlock2d(8, 8, 3, 1, padding=1)(torch.zeros(1, 8, 4, 4))
    with pytest.raises(_lib.DmvsError):
        net("x")


# ------------------------------------------------------------------------------------------ what gets launched (fake library)
HOST_ONLY = ("_plan", "_workspace", "_weight_floats")


class _FakeLib:
    def __init__(self, real, codes):
        self.real, self.codes, self.calls = real, dict(codes), []

    def __getattr__(self, name):
        if name.endswith(HOST_ONLY) or name.startswith(("dmvs_pack_", "dmvs_error_string")):
            return getattr(self.real, name)

        def launch(*args):
            self.calls.append((name, tuple(a for a in args if type(a) is int)))
            return self.codes.get(name, 0)
        return launch


class _Ev:
    def record(self):
        pass


class _Timer(ops.KernelTimer):
    def _event(self):
        return self._pool.pop() if self._pool else _Ev()


@pytest.fixture
def fake(monkeypatch):
    real = _lib.load()

    def install(codes=()):
        lib = _FakeLib(real, codes)
        monkeypatch.setattr(ops._lib, "load", lambda: lib)
        return lib

    monkeypatch.setattr(ops, "_req", lambda *ts: None)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "timer", _Timer())
    monkeypatch.setattr(ops, "launch_log", [])
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(featurenet, "_check_input", lambda *a: None)
    monkeypatch.setattr(conv, "_check_input", lambda *a: None)
    monkeypatch.setattr(bn, "_check_input", lambda *a: None)
    install()
    return install


def _records():
    t = ops.timer
    return [(r[0], lab, r[3], r[4]) for r, lab in zip(t.records, t.labels)]


D, H, W = 2, 5, 8


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("name,cin,cout,k,bias", R.LAYERS, ids=LAYER_IDS)
def test_wgrad_wrapper(fake, name, cin, cout, k, bias, accumulate):
    lib = fake()
    x, gy = torch.zeros(cin, D, H, W), torch.zeros(cout, D, H, W)
    ws = torch.zeros(_lib.load().dmvs_conv2d_wgrad_fpn_workspace(cin, cout, k, D, H, W))
    out = torch.zeros(cout, cin, k, k) if accumulate else None
    gb = torch.zeros(cout) if bias else None
    gw = ops.conv2d_wgrad_fpn(x, gy, k, out=out, bias_out=gb, accumulate=accumulate, workspace=ws)
    assert tuple(gw.shape) == (cout, cin, k, k) and (out is None or gw is out)
    assert lib.calls == [("dmvs_conv2d_wgrad_fpn", (cin, cout, D, H, W, k, int(accumulate)))]
    assert ops.launch_log == ["conv2d_wgrad_fpn"] * 2
    nt = k * k * cin * cout
    assert _records() == [("conv2d_wgrad_fpn", f"wgrad_fpn_{cin}to{cout}k{k}", 2.0 * nt * D * H * W, 4.0 * ((cin + cout) * D * H * W + nt))]


def test_wgrad_wrapper_refusals(fake):
    lib = fake()
    x, gy = torch.zeros(8, D, H, W), torch.zeros(8, D, H, W)
    ws = torch.zeros(_lib.load().dmvs_conv2d_wgrad_fpn_workspace(8, 8, 3, D, H, W))
    with pytest.raises(_lib.DmvsError, match="accumulate needs the buffer"):
        ops.conv2d_wgrad_fpn(x, gy, 3, accumulate=True, workspace=ws)
    with pytest.raises(_lib.DmvsError, match=re.escape("is not a [8,8,3,3] weight")):
        ops.conv2d_wgrad_fpn(x, gy, 3, out=torch.zeros(8 * 8 * 9 - 1), workspace=ws)
    with pytest.raises(_lib.DmvsError, match="workspace too small"):
        ops.conv2d_wgrad_fpn(x, gy, 3, workspace=ws[1:])
    with pytest.raises(_lib.DmvsError, match="has no bias"):
        ops.conv2d_wgrad_fpn(x, gy, 3, bias_out=torch.zeros(8), workspace=ws)
    with pytest.raises(_lib.DmvsError, match=re.escape("is not a [32] bias")):
        ops.conv2d_wgrad_fpn(x, torch.zeros(32, D, H, W), 1, bias_out=torch.zeros(31))
    with pytest.raises(_lib.DmvsError):
        ops.conv2d_wgrad_fpn(x, gy, 1, workspace=ws)                                  # 8 -> 8 at kernel 1
    with pytest.raises(_lib.DmvsError):
        ops.conv2d_wgrad_fpn(x, torch.zeros(8, D, H + 1, W), 3, workspace=ws)          # other planes
    with pytest.raises(_lib.DmvsError):
        ops.conv2d_wgrad_fpn(torch.zeros(16, D, H, W), torch.zeros(16, D, H, W), 3)   # a square layer: K3g's
    with pytest.raises(_lib.DmvsError, match="not covered"):
        ops.conv2d_wgrad_fpn_workspace(16, 16, 3, D, H, W, "cpu")
    assert lib.calls == [] and ops.launch_log == [] and ops.timer.records == []
    lib = fake({"dmvs_conv2d_wgrad_fpn": EINVAL})
    with pytest.raises(_lib.DmvsError):
        ops.conv2d_wgrad_fpn(x, gy, 3, workspace=ws)
    assert lib.calls == [("dmvs_conv2d_wgrad_fpn", (8, 8, D, H, W, 3, 0))] and ops.launch_log == [] and ops.timer.records == []


def _launches(cin, cout, k):
    """(forward, data gradient, weight gradient(accumulate)) of one sample of the layer at H x W."""
    mode = ops.CONV_S1 if k == 3 else ops.CONV2D_K1
    fwd = ("dmvs_conv3d_mfma", (max(cin, 4), cout, 1, H, W, mode, 1, ops.IN_VIEWS if cin == 3 else 0))
    dgrad = ("dmvs_conv3d_mfma", (cout, cin, 1, H, W, mode, 1, 0))
    return fwd, dgrad, lambda acc: ("dmvs_conv2d_wgrad_fpn", (cin, cout, 1, H, W, k, acc))


@pytest.mark.parametrize("x_grad,w_grad", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("name,cin,cout,k,bias", R.LAYERS, ids=LAYER_IDS)
def test_layer_forward_backward_launches(fake, name, cin, cout, k, bias, x_grad, w_grad):
    m = _ctor(cin, cout, k, bias)
    m.weight.requires_grad_(w_grad)
    if bias:
        m.bias.requires_grad_(w_grad)
    lib = fake()
    fwd, dgrad, wgrad = _launches(cin, cout, k)
    x_grad = x_grad and cin != 3   # conv0.0: the image takes no gradient
    x = torch.zeros(2, cin, H, W, requires_grad=x_grad)
    before = dict(conv.launch_counts)
    y = m(x)
    assert tuple(y.shape) == (2, cout, H, W) and lib.calls == [fwd] * 2 and conv.launch_counts == before
    leaves = ([x] if x_grad else []) + ([m.weight] + ([m.bias] if bias else []) if w_grad else [])
    if not leaves:
        assert not y.requires_grad
        return
    grads = torch.autograd.grad(y, leaves, torch.zeros_like(y))
    assert [tuple(t.shape) for t in grads] == [tuple(t.shape) for t in leaves]
    assert lib.calls == [fwd] * 2 + ([dgrad] * 2 if x_grad else []) + ([wgrad(0), wgrad(1)] if w_grad else [])
    assert {k_: conv.launch_counts[k_] - before[k_] for k_ in before} == {"dgrad": 2 * int(x_grad), "wgrad": 2 * int(w_grad)}


def test_conv00_refuses_an_input_that_requires_a_gradient(fake):
    lib = fake()
    with pytest.raises(_lib.DmvsError, match="no data gradient"):
        _ctor(3, 8, 3, False)(torch.zeros(1, 3, H, W, requires_grad=True))
    assert lib.calls == []


def test_bias_alone_launches_the_weight_gradient_kernel(fake):
    m = _ctor(8, 32, 1, True)
    m.weight.requires_grad_(False)
    lib = fake()
    y = m(torch.zeros(1, 8, H, W))
    (gb,) = torch.autograd.grad(y, [m.bias], torch.zeros_like(y))
    assert tuple(gb.shape) == (32,) and lib.calls[-1] == ("dmvs_conv2d_wgrad_fpn", (8, 32, 1, H, W, 1, 0))


def test_a_moved_bias_leaves_one_forward_layer_behind(fake):
    """The forward layer of a lateral is cached under a slot that carries the bias's data pointer and device: a bias that moved to a new
    tensor between two forwards evicts the old entry, so exactly one bias-keyed entry stays in the module's cache; the launches of a
    forward + backward on a batch of 2 are those test_layer_forward_backward_launches lists."""
    m = _ctor(16, 32, 1, True)
    lib = fake()
    fwd, dgrad, wgrad = _launches(16, 32, 1)
    x = torch.zeros(2, 16, H, W, requires_grad=True)
    m(x)
    (slot,) = [s for s in m._packed if isinstance(s, tuple)]
    assert slot == (False, m.bias.data_ptr(), m.bias.device) and m._packed[slot][1].shift.data_ptr() == m.bias.data_ptr()
    m(x)
    assert [s for s in m._packed if isinstance(s, tuple)] == [slot]   # the same bias: the same entry
    old = m.bias.data    # (kept alive: the new tensor cannot take its address)
    m.bias.data = old.clone()
    del lib.calls[:]
    y = m(x)
    (moved,) = [s for s in m._packed if isinstance(s, tuple)]
    assert moved == (False, m.bias.data_ptr(), m.bias.device) and moved != slot
    assert m._packed[moved][1].shift.data_ptr() == m.bias.data_ptr() != old.data_ptr()
    torch.autograd.grad(y, [x, m.weight, m.bias], torch.zeros_like(y))
    assert lib.calls == [fwd] * 2 + [dgrad] * 2 + [wgrad(0), wgrad(1)]
    assert sorted(map(str, m._packed)) == sorted(map(str, [moved, True]))   # ... beside the data gradient's layer


def test_conv_fn_keeps_its_signature(fake):
    lib = fake()
    x, w = torch.zeros((1, 16, 1, H, W), requires_grad=True), torch.zeros((16, 16, 3, 3), requires_grad=True)
    y = conv._ConvFn.apply(x, w, {}, conv._SQUARE)
    torch.autograd.grad(y, [x, w], torch.zeros_like(y))
    assert [c[0] for c in lib.calls] == ["dmvs_conv3d_mfma", "dmvs_conv3d_mfma", "dmvs_conv3d_wgrad"]


def test_network_launches(fake):
    net = DiffFeatureNet(8)
    lib = fake()
    Hn, Wn = 8, 12
    outs = net(torch.zeros(2, 3, Hn, Wn))
    assert tuple(outs) == R.OUT_KEYS and {k: tuple(v.shape) for k, v in outs.items()} == R.out_shapes(2, Hn, Wn)
    names = [c[0] for c in lib.calls]
    assert names.count("dmvs_conv3d_mfma") == 2 * 13 and names.count("dmvs_bn_relu_forward") == 8 and len(names) == 34
    assert lib.calls[0] == ("dmvs_conv3d_mfma", (4, 8, 1, Hn, Wn, ops.CONV_S1, 1, ops.IN_VIEWS))
    del lib.calls[:]
    before = dict(conv.launch_counts)
    torch.autograd.grad(list(outs.values()), list(net.parameters()), [torch.zeros_like(v) for v in outs.values()])
    names = [c[0] for c in lib.calls]
    # 13 convolutions: every one a weight gradient per sample, all but conv0.0 a data gradient per sample
    assert {k: conv.launch_counts[k] - before[k] for k in before} == {"dgrad": 2 * 12, "wgrad": 2 * 13}
    assert names.count("dmvs_conv2d_wgrad_fpn") == 2 * 6 and names.count("dmvs_conv3d_wgrad") == 2 * 5
    assert names.count("dmvs_conv2d_k5s2_wgrad") == 2 * 2 == names.count("dmvs_conv2d_k5s2_dgrad")
    assert names.count("dmvs_conv3d_mfma") == 2 * 10 and names.count("dmvs_bn_relu_backward") == 8
    assert ("dmvs_conv3d_mfma", (8, 3, 1, Hn, Wn, ops.CONV_S1, 1, 0)) not in lib.calls
    fpn = [c[1] for c in lib.calls if c[0] == "dmvs_conv2d_wgrad_fpn"]
    assert sorted(fpn) == sorted((cin, cout, 1, Hn // s, Wn // s, k, acc) for (cin, cout, k), s in
                                 zip(R.SHAPES3, (1, 1, 1, 4, 2, 1)) for acc in (0, 1))


@pytest.mark.parametrize("H_,W_", [(6, 8), (8, 10), (2, 4)])
def test_network_refuses_extents_that_do_not_add_back(fake, H_, W_):
    lib = fake()
    with pytest.raises(_lib.DmvsError, match="multiples of 4"):
        DiffFeatureNet(8)(torch.zeros(1, 3, H_, W_))
    assert lib.calls == []
