"""CPU (-m "not gpu"): the differentiable 5x5 stride-2 convolutions (K3k / K3d, the kernel-5 form of ``DiffConv2d``) without a GPU.

* the float64 restatement (tests/conv_k5s2_grad_ref.py) against float64 autograd of F.conv2d to 1e-12 at every shape;
* the stored fixture (tests/golden/op_conv_k5s2_grad.npz): its condition (no BatchNorm output on the ReLU kink) and its sanity;
* ops.pack_index_mfma_k5s2 against the host packer, bit for bit; the plan and workspace entries; the C ABI;
* the constructor contract and refusals of DiffConv2d at kernel 5, and DiffConvBlock2d's state-dict keys;
* with a fake library of its own (the pattern of tests/test_train_dispatch.py): what the two wrappers and one forward + backward through
  ``_ConvFn`` launch, log and time, and that nothing is logged or timed when a launch fails or a refusal fires;
* the header: exactly the kernels docs/kernels/K3k_conv_wgrad_k5s2.md names, and no atomic."""
import contextlib
import copy
import io
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import conv_k5s2_grad_ref as R
from dmvsnet_amd import _lib, conv, ops
from dmvsnet_amd import DiffConv2d, DiffConv3d, DiffConvBlock2d, DiffConvTranspose2d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = _lib.EINVAL
ENTRIES = ("dmvs_conv2d_k5s2_wgrad", "dmvs_conv2d_k5s2_wgrad_workspace", "dmvs_conv2d_k5s2_wgrad_plan", "dmvs_conv2d_k5s2_dgrad")
KERNELS = {"conv_wgrad_k5s2_kernel", "conv_wgrad_k5s2_reduce_kernel", "conv_dgrad_k5s2_kernel"}


# ------------------------------------------------------------------------------------------ the yardstick itself
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("Cb,Ca", R.PAIRS)
def test_restatement_against_float64_autograd(Cb, Ca, shape):
    D, Hf, Wf = shape
    gen = torch.Generator().manual_seed(Cb + Hf * Wf)
    x = torch.randn(D, Cb, Hf, Wf, dtype=torch.float64, generator=gen).requires_grad_(True)
    w = torch.randn(Ca, Cb, 5, 5, dtype=torch.float64, generator=gen).requires_grad_(True)
    y = F.conv2d(x, w, stride=2, padding=2)
    assert tuple(y.shape[-2:]) == R.coarse_hw(Hf, Wf)
    gy = torch.randn(y.shape, dtype=torch.float64, generator=gen)
    gx, gw = torch.autograd.grad(y, (x, w), gy)
    assert R.rel_dist(R.conv_k5s2_ref(x, w), y) <= 1e-12
    assert R.rel_dist(R.dgrad_k5s2_ref(gy, w, (Hf, Wf)), gx) <= 1e-12
    assert R.rel_dist(R.wgrad_k5s2_ref(gy, x), gw) <= 1e-12
    # autograd over the restatement is the two gradient restatements
    y2 = R.conv_k5s2_ref(x, w)
    gx2, gw2 = torch.autograd.grad(y2, (x, w), gy)
    assert R.rel_dist(gx2, gx) <= 1e-12 and R.rel_dist(gw2, gw) <= 1e-12


def test_conv3x3_restatement():
    gen = torch.Generator().manual_seed(3)
    x, w = torch.randn(2, 16, 5, 7, dtype=torch.float64, generator=gen), torch.randn(16, 16, 3, 3, dtype=torch.float64, generator=gen)
    assert R.rel_dist(R.conv3x3_ref(x, w), F.conv2d(x, w, padding=1)) <= 1e-12


# ------------------------------------------------------------------------------------------ the fixture
@pytest.fixture(scope="module")
def g():
    path = os.path.join(ROOT, "tests", "golden", "op_conv_k5s2_grad.npz")
    assert os.path.getsize(path) < (1 << 20)
    return np.load(path)


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_fixture_condition_and_sanity(g, name):
    kw = R.GOLDEN_CASES[name]
    case = R.golden_case(g, name)
    Cb, Hc, Wc = kw["Cb"], *R.coarse_hw(kw["Hf"], kw["Wf"])
    assert tuple(case["x"].shape) == (kw["B"], Cb, kw["Hf"], kw["Wf"]) and tuple(case["w"].shape) == (2 * Cb, Cb, 5, 5)
    assert tuple(case["out"].shape) == tuple(case["gy"].shape) == (kw["B"], 2 * Cb, Hc, Wc)
    assert all(v.dtype == torch.float32 for k, v in case.items() if k != "Cb")
    made = R.make_case(**kw)
    for k in ("x", "w", "gamma", "beta", "gy"):
        assert torch.equal(made[k], case[k]), k   # the stored inputs are the generator's
    assert R.kink_violations(case) == 0
    f64 = R.block_f64(case)
    for k in ("out", "g_x", "g_w", "g_gamma", "g_beta"):
        assert case[k].shape == f64[k].shape
        assert R.rel_dist(case[k], f64[k]) < 1e-5, k   # sanity: the same function
    assert set(g.files) == {f"{n}.{k}" for n in R.GOLDEN_CASES for k in ("x", "w", "gamma", "beta", "gy", "out", "g_x", "g_w", "g_gamma", "g_beta")}


def test_chain_inputs_stay_off_the_kink():
    assert R.chain_f64(R.make_chain(2, 20, 28, 0))["nearest_kink"] > R.CHAIN_KINK_MARGIN


# ------------------------------------------------------------------------------------------ host-side library entries
@pytest.mark.parametrize("cin,cout", R.PAIRS)
def test_pack_index_is_the_host_packer(cin, cout):
    w = torch.randn(cout, cin, 5, 5, generator=torch.Generator().manual_seed(cin))
    idx = ops.pack_index_mfma_k5s2(cin, cout)
    want = ops.pack_mfma(w, cin, cout, ops.CONV2D_K5S2, 1)
    got = torch.cat((w.reshape(-1), torch.zeros(1)))[idx]
    assert idx.dtype == torch.int64 and got.shape == want.shape
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert ops.pack_index_mfma_k5s2(cin, cout) is idx
    with pytest.raises(_lib.DmvsError):
        ops.pack_index_mfma_k5s2(cout, cin)


def test_plan_and_workspace():
    lib = _lib.load()
    _, ty, tx = ops.WGRAD_K5S2_TILE
    for Ca in (16, 32):
        ws = lib.dmvs_conv2d_k5s2_wgrad_workspace(Ca, 1, 5, 8)
        assert ws == 256 * 25 * Ca * (Ca // 2)
        for D, Hf, Wf in R.SHAPES + ((1, 136, 1040), (3, 512, 640)):
            Hc, Wc = R.coarse_hw(Hf, Wf)
            tiles = D * -(-Hc // ty) * -(-Wc // tx)
            plan = lib.dmvs_conv2d_k5s2_wgrad_plan(Ca, D, Hf, Wf)
            assert plan // 512 == tiles and plan % 512 == 8 * -(-min(tiles, 256) // 8), (Ca, D, Hf, Wf, plan)
            assert lib.dmvs_conv2d_k5s2_wgrad_workspace(Ca, D, Hf, Wf) == ws   # whatever the image
    assert lib.dmvs_conv2d_k5s2_wgrad_plan(16, 1, 136, 1040) // 512 == 289
    assert lib.dmvs_conv2d_k5s2_wgrad_plan(24, 1, 5, 8) == _lib.EUNSUPPORTED and lib.dmvs_conv2d_k5s2_wgrad_workspace(24, 1, 5, 8) == 0
    for bad in ((0, 5, 8), (1, 0, 8), (1, 5, 0)):
        assert lib.dmvs_conv2d_k5s2_wgrad_plan(16, *bad) == EINVAL and lib.dmvs_conv2d_k5s2_wgrad_workspace(16, *bad) == 0
    assert lib.dmvs_conv2d_k5s2_wgrad_plan(16, 1 << 20, 64, 64) == EINVAL   # 2^22 tiles
    # null pointers and unsupported channels are refused on the host, before any launch
    assert lib.dmvs_conv2d_k5s2_wgrad(None, None, None, None, 16, 1, 5, 8, 0, None) == EINVAL
    assert lib.dmvs_conv2d_k5s2_dgrad(None, None, None, 16, 1, 5, 8, None) == EINVAL


def test_c_abi_and_sources():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "dmvs.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/dmvs.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "module.py:289" in header and ":295" in header
    assert len(_lib.SIGNATURES["dmvs_conv2d_k5s2_wgrad"][1]) == 10 and len(_lib.SIGNATURES["dmvs_conv2d_k5s2_dgrad"][1]) == 8
    src = open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "conv2d_k5s2_bwd.h")).read()
    assert set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src)) == KERNELS
    assert "atomic" not in src.lower()
    shared = open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "wgrad_share.h")).read()
    assert "atomic" not in shared.lower().replace("no atomics", "")
    doc = open(os.path.join(ROOT, "docs", "kernels", "K3k_conv_wgrad_k5s2.md")).read()
    assert set(re.findall(r"`(conv_\w+_kernel)`", doc)) == KERNELS
    text = open(os.path.join(ROOT, "scripts", "pmc_summary.py")).read()
    assert all(k in text for k in KERNELS)
    direct = open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "conv3d_direct.hip")).read()
    assert direct.index('#include "conv2d_k5s2_bwd.h"') > direct.index('#include "conv3d_wgrad_s2.h"')
    assert "conv2d_k5s2_bwd.h" in open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "Makefile")).read()


# ------------------------------------------------------------------------------------------ the constructor
@pytest.mark.parametrize("cin,cout", R.PAIRS)
def test_constructor_contract(cin, cout):
    assert conv.CHANNELS_K5S2 == R.PAIRS
    m = DiffConv2d(cin, cout, 5, stride=2, padding=2, bias=False)
    assert isinstance(m, nn.Conv2d) and list(m.state_dict()) == ["weight"] and tuple(m.weight.shape) == (cout, cin, 5, 5)
    stock = nn.Conv2d(cin, cout, 5, stride=2, padding=2, bias=False)
    m.load_state_dict(stock.state_dict())
    assert torch.equal(m.weight, stock.weight)
    blk = DiffConvBlock2d(cin, cout, 5, stride=2, padding=2)
    want = nn.Sequential()
    want.conv, want.bn = stock, nn.BatchNorm2d(cout)
    assert list(blk.state_dict()) == list(want.state_dict())
    assert isinstance(blk.conv, DiffConv2d) and blk.conv.kernel_size == (5, 5)


@pytest.mark.parametrize("kw", [dict(stride=1), dict(padding=1), dict(bias=True), dict(dilation=2), dict(groups=2), dict(padding_mode="reflect")],
                         ids=lambda kw: next(iter(kw)))
def test_constructor_refusals_by_argument(kw):
    args = dict(stride=2, padding=2, bias=False)
    args.update(kw)
    with pytest.raises(_lib.DmvsError, match="no ATen fallback"):
        DiffConv2d(8, 16, 5, **args)


@pytest.mark.parametrize("cin,cout", [(8, 8), (16, 16), (32, 64), (16, 8)])
def test_constructor_refusals_by_channels(cin, cout):
    with pytest.raises(_lib.DmvsError, match="no ATen fallback"):
        DiffConv2d(cin, cout, 5, stride=2, padding=2, bias=False)


def test_constructor_refusals_other_classes():
    with pytest.raises(_lib.DmvsError):
        DiffConv3d(8, 16, 5, stride=2, padding=2, bias=False)
    with pytest.raises(_lib.DmvsError):
        DiffConvTranspose2d(16, 8, 5, stride=2, padding=2, output_padding=1, bias=False)
    with pytest.raises(_lib.DmvsError):
        DiffConv2d(16, 16, 5, padding=2, bias=False)
    with pytest.raises(_lib.DmvsError):
        DiffConvBlock2d(8, 16, 5, stride=2, padding=2, bn=False)


# ------------------------------------------------------------------------------------------ what the wrappers launch (fake library)
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
    def __init__(self):
        super().__init__()
        self.made = []

    def _event(self):
        if self._pool:
            return self._pool.pop()
        self.made.append(_Ev())
        return self.made[-1]

    def held(self):
        """Every event this timer made is in a record or back in the pool."""
        return sorted(map(id, [r[1] for r in self.records] + [r[2] for r in self.records] + self._pool)) == sorted(map(id, self.made))


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
    install()
    return install


def _records():
    t = ops.timer
    return [(r[0], lab, r[3], r[4], r[5]) for r, lab in zip(t.records, t.labels)]


def _refused(lib, launches=()):
    assert lib.calls == list(launches) and ops.launch_log == [] and ops.timer.records == []
    assert ops.timer.held()


D, HF, WF = 2, 5, 8
HC, WC = 3, 4


def _tensors(Cb):
    return torch.zeros(Cb, D, HF, WF), torch.zeros(2 * Cb, D, HC, WC), torch.zeros(2 * Cb, Cb, 5, 5)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("Cb", [8, 16])
def test_wgrad_wrapper(fake, Cb, accumulate):
    lib = fake()
    Ca = 2 * Cb
    x, gy, _ = _tensors(Cb)
    ws = torch.zeros(_lib.load().dmvs_conv2d_k5s2_wgrad_workspace(Ca, D, HF, WF))
    out = torch.zeros(Ca, Cb, 5, 5) if accumulate else None
    gw = ops.conv2d_k5s2_wgrad(x, gy, out=out, accumulate=accumulate, workspace=ws)
    assert tuple(gw.shape) == (Ca, Cb, 5, 5) and (out is None or gw is out)
    assert lib.calls == [("dmvs_conv2d_k5s2_wgrad", (Ca, D, HF, WF, int(accumulate)))]
    assert ops.launch_log == ["conv2d_k5s2_wgrad"] * 2
    fl = 2.0 * 25 * Ca * Cb * D * HC * WC
    assert _records() == [("conv2d_k5s2_wgrad", f"wgrad_k5s2_{Ca}", fl, 4.0 * (Ca * D * HC * WC + Cb * D * HF * WF + 25 * Ca * Cb), fl)]
    assert ops.timer.held()


@pytest.mark.parametrize("Cb", [8, 16])
def test_dgrad_wrapper(fake, Cb):
    lib = fake()
    Ca = 2 * Cb
    _, gy, w = _tensors(Cb)
    gx = ops.conv2d_k5s2_dgrad(gy, w, (HF, WF))
    assert tuple(gx.shape) == (Cb, D, HF, WF)
    assert lib.calls == [("dmvs_conv2d_k5s2_dgrad", (Ca, D, HF, WF))]
    assert ops.launch_log == ["conv2d_k5s2_dgrad"]
    fl = 2.0 * 25 * Ca * Cb * D * HC * WC
    assert _records() == [("conv2d_k5s2_dgrad", f"dgrad_k5s2_{Ca}", fl, 4.0 * (Ca * D * HC * WC + Cb * D * HF * WF + 25 * Ca * Cb), fl)]
    out = torch.zeros(Cb, D, HF + 1, WF)   # 6 x 8 has the same coarse grid: the fine extent is the caller's to name
    assert ops.conv2d_k5s2_dgrad(gy, w, (HF + 1, WF), out=out) is out and lib.calls[-1] == ("dmvs_conv2d_k5s2_dgrad", (Ca, D, HF + 1, WF))
    assert ops.timer.held()


def test_wrappers_log_nothing_when_the_launch_fails(fake):
    x, gy, w = _tensors(8)
    ws = torch.zeros(_lib.load().dmvs_conv2d_k5s2_wgrad_workspace(16, D, HF, WF))
    lib = fake({"dmvs_conv2d_k5s2_wgrad": EINVAL, "dmvs_conv2d_k5s2_dgrad": EINVAL})
    with pytest.raises(_lib.DmvsError):
        ops.conv2d_k5s2_wgrad(x, gy, workspace=ws)
    _refused(lib, [("dmvs_conv2d_k5s2_wgrad", (16, D, HF, WF, 0))])
    lib = fake({"dmvs_conv2d_k5s2_dgrad": EINVAL})
    with pytest.raises(_lib.DmvsError):
        ops.conv2d_k5s2_dgrad(gy, w, (HF, WF))
    _refused(lib, [("dmvs_conv2d_k5s2_dgrad", (16, D, HF, WF))])


def test_wrapper_refusals(fake):
    lib = fake()
    x, gy, w = _tensors(8)
    ws = torch.zeros(_lib.load().dmvs_conv2d_k5s2_wgrad_workspace(16, D, HF, WF))
    with pytest.raises(_lib.DmvsError, match="accumulate needs the buffer"):
        ops.conv2d_k5s2_wgrad(x, gy, accumulate=True, workspace=ws)
    with pytest.raises(_lib.DmvsError, match=re.escape("is not a [16,8,5,5] weight")):
        ops.conv2d_k5s2_wgrad(x, gy, out=torch.zeros(16 * 8 * 25 - 1), workspace=ws)
    with pytest.raises(_lib.DmvsError, match="workspace too small"):
        ops.conv2d_k5s2_wgrad(x, gy, workspace=ws[1:])
    with pytest.raises(_lib.DmvsError):
        ops.conv2d_k5s2_wgrad(torch.zeros(8, D, HF + 2, WF), gy, workspace=ws)      # another coarse grid
    with pytest.raises(_lib.DmvsError):
        ops.conv2d_k5s2_wgrad(torch.zeros(12, D, HF, WF), torch.zeros(24, D, HC, WC), workspace=ws)   # 24 channels
    with pytest.raises(_lib.DmvsError, match="not covered"):
        ops.conv2d_k5s2_wgrad_workspace(24, D, HF, WF, "cpu")
    with pytest.raises(_lib.DmvsError, match=re.escape("is not a [16,8,5,5] weight")):
        ops.conv2d_k5s2_dgrad(gy, torch.zeros(16, 8, 3, 3), (HF, WF))
    with pytest.raises(_lib.DmvsError):
        ops.conv2d_k5s2_dgrad(gy, w, (HF + 2, WF))
    with pytest.raises(_lib.DmvsError):
        ops.conv2d_k5s2_dgrad(gy, w, (HF, WF), out=torch.zeros(8, D, HF, WF + 1))
    _refused(lib)


# ------------------------------------------------------------------------------------------ the autograd Function
FWD = ("dmvs_conv3d_mfma", (8, 16, 1, HF, WF, ops.CONV2D_K5S2, 1, 0))
DGRAD = ("dmvs_conv2d_k5s2_dgrad", (16, 1, HF, WF))


def _wgrad(acc):
    return ("dmvs_conv2d_k5s2_wgrad", (16, 1, HF, WF, acc))


@pytest.mark.parametrize("x_grad,w_grad", [(True, True), (False, True), (True, False)])
def test_autograd_function(fake, x_grad, w_grad):
    lib = fake()
    x, w = torch.zeros((1, 8, 1, HF, WF), requires_grad=x_grad), torch.zeros((16, 8, 5, 5), requires_grad=w_grad)
    before = dict(conv.launch_counts)
    y = conv._ConvFn.apply(x, w, {}, conv._DOWN5)
    assert tuple(y.shape) == (1, 16, 1, HC, WC)
    assert lib.calls == [FWD] and conv.launch_counts == before
    grads = torch.autograd.grad(y, [t for t in (x, w) if t.requires_grad], torch.zeros_like(y))
    assert [tuple(t.shape) for t in grads] == [s for s, on in ((tuple(x.shape), x_grad), (tuple(w.shape), w_grad)) if on]
    assert lib.calls == [FWD] + ([DGRAD] if x_grad else []) + ([_wgrad(0)] if w_grad else [])
    assert {k: conv.launch_counts[k] - before[k] for k in before} == {"dgrad": int(x_grad), "wgrad": int(w_grad)}
    assert set(conv.launch_counts) == {"dgrad", "wgrad"}
    assert ops.timer.held()


def test_autograd_function_batch_accumulates(fake):
    lib = fake()
    x, w = torch.zeros((2, 8, 1, HF, WF), requires_grad=True), torch.zeros((16, 8, 5, 5), requires_grad=True)
    y = conv._ConvFn.apply(x, w, {}, conv._DOWN5)
    torch.autograd.grad(y, [x, w], torch.zeros_like(y))
    assert lib.calls == [FWD] * 2 + [DGRAD] * 2 + [_wgrad(0), _wgrad(1)]


@pytest.mark.parametrize("how", ["made", "deepcopy", "reloaded"])
def test_copied_modules_launch_the_same(fake, monkeypatch, how):
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(conv, "_check_input", lambda *a: None)
    m = DiffConv2d(8, 16, 5, stride=2, padding=2, bias=False)
    if how == "deepcopy":
        m = copy.deepcopy(m)
    elif how == "reloaded":
        buf = io.BytesIO()
        torch.save(m, buf)
        buf.seek(0)
        m = torch.load(buf, weights_only=False)
    lib = fake()
    x = torch.zeros(1, 8, HF, WF, requires_grad=True)   # odd height: accepted
    y = m(x)
    assert tuple(y.shape) == (1, 16, HC, WC)
    gx, gw = torch.autograd.grad(y, [x, m.weight], torch.zeros_like(y))
    assert tuple(gx.shape) == tuple(x.shape) and tuple(gw.shape) == (16, 8, 5, 5)
    assert lib.calls == [FWD, DGRAD, _wgrad(0)]
