"""CPU (-m "not gpu"): what the training-path host wrappers launch, without a GPU -- the three weight-gradient wrappers
(ops.conv3d_wgrad, conv3d_wgrad_s2, conv3d_wgrad_c2), K5 (ops.bn_relu_forward / bn_relu_backward), the plane-sweep and depth-head
wrappers (ops.warp_corr, depth_select, depth_regress, depth_regress_backward) and the autograd Function of the differentiable convs
(dmvsnet_amd.conv).  A fake library on the pattern of test_conv_dispatch.py records every kernel launch with its integer arguments and
returns scripted codes; host-only queries (plans, workspace and weight lengths, packers, the BatchNorm partition, error strings) go to
the real library.  Pinned per case: the C entry called and its integer arguments, the launch_log families, the one timer record with
its cost written out here, and that no timer event leaks -- on success and when the launch fails; the refusals that come before any
launch; the launch order and the launch_counts of one forward + backward through every layer kind.

Stubs, so that CPU tensors serve: ``ops._req`` (accepts every tensor) and ``ops._stream`` (None) everywhere; in the autograd tests also
``torch.cuda.current_stream`` (an object whose ``cuda_stream`` is 0) and ``torch.cuda.current_device`` (0), which the default workspace
of a weight gradient asks for.  Every other test passes ``workspace=`` explicitly."""
import contextlib
import copy
import io
import re
import types

import pytest
import torch

from dmvsnet_amd import _lib, conv, ops
from dmvsnet_amd.ops import BN_TRAIN, CONV_S1, CONV_S2, DECONV_S2, RELU

EINVAL = _lib.EINVAL
HOST_ONLY = ("_plan", "_workspace", "_weight_floats")


class _FakeLib:
    def __init__(self, real, codes):
        self.real, self.codes, self.calls = real, dict(codes), []

    def __getattr__(self, name):
        if name.endswith(HOST_ONLY) or name.startswith(("dmvs_pack_", "dmvs_bn_share_range", "dmvs_error_string")):
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
    install()
    return install


def _records():
    t = ops.timer
    return [(r[0], lab, r[3], r[4], r[5]) for r, lab in zip(t.records, t.labels)]


def _ok(lib, launches, families, record):
    assert lib.calls == launches
    assert ops.launch_log == families
    assert _records() == [record]
    assert ops.timer.held()


def _refused(lib, launches=()):
    """Nothing ran: no launch beyond ``launches`` (the failing one), nothing logged or timed, every timer event given back."""
    assert lib.calls == list(launches) and ops.launch_log == [] and ops.timer.records == []
    assert ops.timer.held()


def _ws(entry, *shape):
    n = getattr(_lib.load(), entry)(*shape)
    assert n > 0, (entry, shape)
    return torch.zeros(n)


# ------------------------------------------------------------------------------------------ the weight gradients
D, H, W = 2, 4, 6   # every wgrad case: this volume (K3h: the coarse one)


def _k3g(C, kd):
    x = torch.zeros(C, D, H, W)
    fl = 2.0 * 9 * kd * C * C * D * H * W
    return dict(fn=ops.conv3d_wgrad, args=(x, x.clone(), kd), oshape=(C, C, kd, 3, 3), entry="dmvs_conv3d_wgrad", ints=(C, D, H, W, kd),
                family="conv3d_wgrad", label=f"wgrad{C}k{kd}", cost=(fl, 4.0 * (2 * C * D * H * W + 9 * kd * C * C), fl),
                bad=(torch.zeros(C, D, H, W), torch.zeros(C, D, H, W + 1), kd))


def _k3h(Ca, kd):
    coarse, fine = torch.zeros(Ca, D, H, W), torch.zeros(Ca // 2, 2 * D if kd == 3 else D, 2 * H, 2 * W)
    nt = 9 * kd * Ca * (Ca // 2)
    fl = 2.0 * nt * D * H * W
    return dict(fn=ops.conv3d_wgrad_s2, args=(coarse, fine, kd), oshape=(Ca, Ca // 2, kd, 3, 3), entry="dmvs_conv3d_wgrad_s2",
                ints=(Ca, D, H, W, kd), family="conv3d_wgrad_s2", label=f"wgrad_s2_{Ca}k{kd}",
                cost=(fl, 4.0 * (Ca * D * H * W + (Ca // 2) * (2 * D if kd == 3 else D) * 4 * H * W + nt), fl),
                bad=(coarse, torch.zeros(Ca // 2, D, H, W), kd))


def _k2g(cin, cout):
    x, gy = torch.zeros(cin, D, H, W), torch.zeros(cout, D, H, W)
    fl = 2.0 * 27 * cin * cout * D * H * W
    return dict(fn=ops.conv3d_wgrad_c2, args=(x, gy), oshape=(cout, cin, 3, 3, 3), entry="dmvs_conv3d_wgrad_c2", ints=(cin, cout, D, H, W),
                family="conv3d_wgrad_c2", label=f"wgrad{cin}to{cout}", cost=(fl, 4.0 * ((cin + cout) * D * H * W + 27 * cin * cout), fl),
                bad=(torch.zeros(3, D, H, W), gy))


WGRAD = {"k3g_16_kd3": _k3g(16, 3), "k3g_64_kd1": _k3g(64, 1), "k3h_16_kd3": _k3h(16, 3), "k3h_64_kd1": _k3h(64, 1),
         "k2g_2to8": _k2g(2, 8), "k2g_8to2": _k2g(8, 2)}


@pytest.fixture(params=list(WGRAD))
def wg(request):
    c = WGRAD[request.param]
    return types.SimpleNamespace(ws=_ws(c["entry"] + "_workspace", *c["ints"]), **c)


@pytest.mark.parametrize("accumulate", [False, True])
def test_wgrad_launch(fake, wg, accumulate):
    lib = fake()
    out = torch.zeros(wg.oshape) if accumulate else None
    gw = wg.fn(*wg.args, out=out, accumulate=accumulate, workspace=wg.ws)
    assert tuple(gw.shape) == wg.oshape and (out is None or gw is out)
    _ok(lib, [(wg.entry, wg.ints + (int(accumulate),))], [wg.family, wg.family], (wg.family, wg.label) + wg.cost)


def test_wgrad_launch_fails(fake, wg):
    lib = fake({wg.entry: EINVAL})
    with pytest.raises(_lib.DmvsError):
        wg.fn(*wg.args, workspace=wg.ws)
    _refused(lib, [(wg.entry, wg.ints + (0,))])


def test_wgrad_refusals(fake, wg):
    lib = fake()
    with pytest.raises(_lib.DmvsError, match="accumulate needs the buffer"):
        wg.fn(*wg.args, accumulate=True, workspace=wg.ws)
    with pytest.raises(_lib.DmvsError, match=re.escape(f"is not a [{','.join(map(str, wg.oshape))}] weight")):
        wg.fn(*wg.args, out=torch.zeros(wg.oshape).reshape(-1)[1:], workspace=wg.ws)
    with pytest.raises(_lib.DmvsError, match="workspace too small"):
        wg.fn(*wg.args, workspace=wg.ws[1:])
    with pytest.raises(_lib.DmvsError):
        wg.fn(*wg.bad, workspace=wg.ws)
    _refused(lib)


def test_wgrad_uncovered_channels(fake):
    """24 channels: the default workspace's size query refuses, before any device is asked for."""
    lib = fake()
    x = torch.zeros(24, D, H, W)
    with pytest.raises(_lib.DmvsError, match="not covered by the weight-gradient kernel"):
        ops.conv3d_wgrad(x, x, 3)
    with pytest.raises(_lib.DmvsError, match="not covered by the strided weight-gradient kernel"):
        ops.conv3d_wgrad_s2(x, torch.zeros(12, 2 * D, 2 * H, 2 * W), 3)
    _refused(lib)


# ------------------------------------------------------------------------------------------ K5
B, C5, V5 = 2, 8, (3, 5)
NV = B * C5 * 15


def _bn_vec():
    return [torch.zeros(C5) for _ in range(4)]


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu", [True, False])
def test_bn_forward(fake, training, relu):
    lib = fake()
    x = torch.zeros(B, C5, *V5)
    y, mean, invstd = ops.bn_relu_forward(x, *_bn_vec(), 0.1, 1e-5, relu, training, workspace=_ws("dmvs_bn_workspace", C5, B, 15))
    assert y.shape == x.shape and mean.shape == invstd.shape == (C5,)
    flags = (RELU if relu else 0) | (BN_TRAIN if training else 0)
    _ok(lib, [("dmvs_bn_relu_forward", (B, C5, 15, flags))], ["batchnorm"] * (2 if training else 1),
        ("batchnorm", "bn8", 5.0 * NV, 4.0 * NV * (3 if training else 2), 5.0 * NV))


@pytest.mark.parametrize("need_gx", [True, False])
@pytest.mark.parametrize("training", [True, False])
def test_bn_backward(fake, need_gx, training):
    lib = fake()
    x = torch.zeros(B, C5, *V5)
    gx, gg, gb = ops.bn_relu_backward(x, x.clone(), *_bn_vec(), True, training, need_gx=need_gx, workspace=_ws("dmvs_bn_workspace", C5, B, 15))
    assert (gx.shape == x.shape if need_gx else gx is None) and gg.shape == gb.shape == (C5,)
    _ok(lib, [("dmvs_bn_relu_backward", (B, C5, 15, RELU | (BN_TRAIN if training else 0)))], ["batchnorm"] * 2,
        ("batchnorm", "bn8", 12.0 * NV, 4.0 * NV * (5 if need_gx else 2), 12.0 * NV))


def test_bn_launch_fails(fake):
    x, ws = torch.zeros(B, C5, *V5), _ws("dmvs_bn_workspace", C5, B, 15)
    lib = fake({"dmvs_bn_relu_forward": EINVAL, "dmvs_bn_relu_backward": EINVAL})
    with pytest.raises(_lib.DmvsError):
        ops.bn_relu_forward(x, *_bn_vec(), 0.1, 1e-5, True, True, workspace=ws)
    _refused(lib, [("dmvs_bn_relu_forward", (B, C5, 15, RELU | BN_TRAIN))])
    lib = fake({"dmvs_bn_relu_forward": EINVAL, "dmvs_bn_relu_backward": EINVAL})
    with pytest.raises(_lib.DmvsError):
        ops.bn_relu_backward(x, x, *_bn_vec(), True, True, workspace=ws)
    _refused(lib, [("dmvs_bn_relu_backward", (B, C5, 15, RELU | BN_TRAIN))])


def test_bn_refusals(fake):
    lib = fake()
    x, ws = torch.zeros(B, C5, *V5), _ws("dmvs_bn_workspace", C5, B, 15)
    with pytest.raises(_lib.DmvsError, match="workspace too small"):
        ops.bn_relu_forward(x, *_bn_vec(), 0.1, 1e-5, True, True, workspace=ws[1:])
    with pytest.raises(_lib.DmvsError, match="workspace too small"):
        ops.bn_relu_backward(x, x, *_bn_vec(), True, True, workspace=ws[1:])
    with pytest.raises(_lib.DmvsError, match="per-channel vector"):
        ops.bn_relu_forward(x, torch.zeros(C5 + 1), *_bn_vec()[1:], 0.1, 1e-5, True, True, workspace=ws)
    with pytest.raises(_lib.DmvsError, match="more than one value per channel"):
        ops.bn_relu_forward(torch.zeros(1, C5, 1), *_bn_vec(), 0.1, 1e-5, True, True, workspace=ws)
    with pytest.raises(_lib.DmvsError, match="same shape"):
        ops.bn_relu_backward(x, torch.zeros(B, C5, 15), *_bn_vec(), True, True, workspace=ws)
    x24 = torch.zeros(B, 24, *V5)   # the default workspace's size query refuses, before any device is asked for
    with pytest.raises(_lib.DmvsError, match="not covered by the BatchNorm kernels"):
        ops.bn_relu_forward(x24, *(torch.zeros(24) for _ in range(4)), 0.1, 1e-5, True, True)
    with pytest.raises(_lib.DmvsError, match="not covered by the BatchNorm kernels"):
        ops.bn_relu_backward(x24, x24, *(torch.zeros(24) for _ in range(4)), True, True)
    _refused(lib)


# ------------------------------------------------------------------------------------------ K1 / K4 wrappers
KC, KD, KH, KW, NSRC = 8, 3, 4, 6, 2
VOX = KD * KH * KW


def _k1_cost(hyp):
    fl = NSRC * VOX * (10.0 * KC + 25)
    return fl, 4.0 * (NSRC + 1) * KC * KH * KW + 4.0 * (2 * VOX + hyp), fl


def _k1_case(form):
    """-> (ref, src, depth, entry, int args, cost) of one K1 form."""
    proj = torch.zeros(NSRC, 12)
    if form == "q4":
        f = lambda: torch.zeros(KC // 4, KH, KW, 4)   # noqa: E731
        return f(), [f(), f()], proj, torch.zeros(KD, KH, KW), "dmvs_warp_corr_q4", (NSRC, KC, KD, KH, KW, 0, 0), _k1_cost(VOX)
    f = lambda: torch.zeros(KH, KW, KC)   # noqa: E731
    if form == "hwc":
        return f(), [f(), f()], proj, torch.zeros(KD, KH, KW), "dmvs_warp_corr", (NSRC, KC, KC, KD, KH, KW, 0), _k1_cost(VOX)
    planes = ops.AffinePlanes(torch.zeros(KH, KW), torch.zeros(()), KD)
    return f(), [f(), f()], proj, planes, "dmvs_warp_corr_affine", (NSRC, KC, KC, KD, KH, KW, 0), _k1_cost(KH * KW)


@pytest.mark.parametrize("form", ["q4", "hwc", "affine_hwc"])
def test_warp_corr(fake, form):
    ref, src, proj, depth, entry, ints, cost = _k1_case(form)
    lib = fake()
    sim = ops.warp_corr(ref, src, proj, depth)
    assert tuple(sim.shape) == (2, KD, KH, KW)
    _ok(lib, [(entry, ints)], ["warp_corr"], ("warp_corr", "warp_corr") + cost)
    lib = fake({entry: EINVAL})
    n = len(ops.launch_log), len(ops.timer.records)
    with pytest.raises(_lib.DmvsError):
        ops.warp_corr(ref, src, proj, depth)
    assert lib.calls == [(entry, ints)] and (len(ops.launch_log), len(ops.timer.records)) == n
    assert ops.timer.held()


def test_warp_corr_accumulate_family(fake):
    ref, src, proj, depth, entry, ints, cost = _k1_case("q4")
    lib = fake()
    out = torch.zeros(2, KD, KH, KW)
    assert ops.warp_corr(ref, src, proj, depth, out=out, accumulate=True, variant=3, family="shard") is out
    _ok(lib, [(entry, ints[:5] + (1, 3))], ["shard"], ("shard", "shard") + cost)


def test_warp_corr_no_source_view(fake):
    lib = fake()
    ref = torch.zeros(KC // 4, KH, KW, 4)
    out = torch.ones(2, KD, KH, KW)
    assert ops.warp_corr(ref, [], torch.zeros(0, 12), torch.zeros(KD, KH, KW), out=out) is out and not out.any()
    out.fill_(1.0)
    assert ops.warp_corr(ref, [], torch.zeros(0, 12), torch.zeros(KD, KH, KW), out=out, accumulate=True).all()
    _refused(lib)


@pytest.mark.parametrize("mode", [0, 1])
def test_depth_select(fake, mode):
    lib = fake()
    sel, conf = ops.depth_select(torch.zeros(4, KH, KW), torch.zeros(()), mode)
    assert tuple(sel.shape) == ((4, KH, KW) if mode == 0 else (KH, KW)) and tuple(conf.shape) == (KH, KW)
    _ok(lib, [("dmvs_depth_select", (mode, KH, KW))], ["depth_regress"],
        ("depth_regress", "depth_regress", 0.0, 4.0 * (4 + (5 if mode == 0 else 2)) * KH * KW, 0.0))
    lib = fake({"dmvs_depth_select": EINVAL})
    with pytest.raises(_lib.DmvsError):
        ops.depth_select(torch.zeros(4, KH, KW), torch.zeros(()), mode)
    assert len(lib.calls) == 1 and len(ops.launch_log) == 1 and len(ops.timer.records) == 1
    assert ops.timer.held()


@pytest.mark.parametrize("want_prob", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("affine", [False, True])
def test_depth_regress(fake, affine, mode, want_prob):
    lib = fake()
    itv = torch.zeros(())
    hyp = ops.AffinePlanes(torch.zeros(KH, KW), itv, KD) if affine else torch.zeros(KD, KH, KW)
    entry = "dmvs_depth_regress_affine" if affine else "dmvs_depth_regress"
    dsp, sel, conf, prob = ops.depth_regress(torch.zeros(4, KD, KH, KW), hyp, itv, 1.0, mode, want_prob)
    assert tuple(dsp.shape) == (4, KH, KW) and tuple(sel.shape) == ((4, KH, KW) if mode == 0 else (KH, KW))
    assert tuple(conf.shape) == (KH, KW) and (tuple(prob.shape) == (4, KD, KH, KW) if want_prob else prob is None)
    nb = 4.0 * (4 * VOX + (KH * KW if affine else VOX) + (9 if mode == 0 else 6) * KH * KW + (4 * VOX if want_prob else 0))
    _ok(lib, [(entry, (mode, KD, KH, KW))], ["depth_regress"], ("depth_regress", "depth_regress", 0.0, nb, 0.0))
    lib = fake({entry: EINVAL})
    with pytest.raises(_lib.DmvsError):
        ops.depth_regress(torch.zeros(4, KD, KH, KW), hyp, itv, 1.0, mode, want_prob)
    assert len(lib.calls) == 1 and len(ops.launch_log) == 1 and len(ops.timer.records) == 1
    assert ops.timer.held()


@pytest.mark.parametrize("mode,dsp_grad,sel_grad,want_hyp,planes", [(0, True, True, True, 12), (1, False, True, False, 5), (1, True, False, True, 8)])
def test_depth_regress_backward(fake, mode, dsp_grad, sel_grad, want_hyp, planes):
    lib = fake()
    lg, hyp, dsp = torch.zeros(4, KD, KH, KW), torch.zeros(KD, KH, KW), torch.zeros(4, KH, KW)
    g_dsp = torch.zeros(4, KH, KW) if dsp_grad else None
    g_sel = (torch.zeros(4, KH, KW) if mode == 0 else torch.zeros(KH, KW)) if sel_grad else None
    g_lg, g_hyp = ops.depth_regress_backward(lg, hyp, 1.0, mode, dsp, g_dsp, g_sel, want_hyp)
    assert g_lg.shape == lg.shape and (g_hyp.shape == hyp.shape if want_hyp else g_hyp is None)
    _ok(lib, [("dmvs_depth_regress_backward", (mode, KD, KH, KW))], ["depth_regress"],
        ("depth_regress", "depth_regress", 0.0, 4.0 * (8 * VOX + (2 if want_hyp else 1) * VOX + planes * KH * KW), 0.0))
    lib = fake({"dmvs_depth_regress_backward": EINVAL})
    n = len(ops.timer.records)
    with pytest.raises(_lib.DmvsError):
        ops.depth_regress_backward(lg, hyp, 1.0, mode, dsp, g_dsp, g_sel, want_hyp)
    assert len(lib.calls) == 1 and len(ops.launch_log) == 1 and len(ops.timer.records) == n and ops.timer.held()
    with pytest.raises(_lib.DmvsError, match="no upstream gradient"):
        ops.depth_regress_backward(lg, hyp, 1.0, mode, dsp, None, None, want_hyp)
    assert len(lib.calls) == 1


# ------------------------------------------------------------------------------------------ the autograd Functions
def _apply(kind, x, w, cache):
    kinds = {"square": conv._SQUARE, "strided": conv._DOWN, "transposed": conv._UP, "ends": conv._ENDS}
    return conv._ConvFn.apply(x, w, cache, kinds[kind])


# kind -> (x shape, weight shape, forward / data-gradient entry, weight-gradient entry and its int arguments)
FN = {"square": ((1, 16, 2, 4, 4), (16, 16, 3, 3, 3), "dmvs_conv3d_mfma", ("dmvs_conv3d_wgrad", (16, 2, 4, 4, 3, 0))),
      "strided": ((1, 8, 2, 4, 4), (16, 8, 3, 3, 3), "dmvs_conv3d_mfma", ("dmvs_conv3d_wgrad_s2", (16, 1, 2, 2, 3, 0))),
      "transposed": ((1, 16, 2, 4, 4), (16, 8, 3, 3, 3), "dmvs_conv3d_mfma", ("dmvs_conv3d_wgrad_s2", (16, 2, 4, 4, 3, 0))),
      "ends": ((1, 2, 2, 4, 4), (8, 2, 3, 3, 3), "dmvs_conv3d_direct", ("dmvs_conv3d_wgrad_c2", (2, 8, 2, 4, 4, 0)))}
# the (Cin, Cout, D, H, W, mode, kdepth, flags) of the forward launch and of the data-gradient launch
FN_K3 = {"square": ((16, 16, 2, 4, 4, CONV_S1, 3, 0), (16, 16, 2, 4, 4, CONV_S1, 3, 0)),
         "strided": ((8, 16, 2, 4, 4, CONV_S2, 3, 0), (16, 8, 1, 2, 2, DECONV_S2, 3, 0)),
         "transposed": ((16, 8, 2, 4, 4, DECONV_S2, 3, 0), (8, 16, 4, 8, 8, CONV_S2, 3, 0)),
         "ends": ((2, 8, 2, 4, 4, CONV_S1, 3, 0), (8, 2, 2, 4, 4, CONV_S1, 3, 0))}


@pytest.mark.parametrize("x_grad,w_grad", [(True, True), (False, True), (True, False)])
@pytest.mark.parametrize("kind", list(FN))
def test_autograd_function(fake, monkeypatch, kind, x_grad, w_grad):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    lib = fake()
    xshape, wshape, k3, wgrad = FN[kind]
    fwd, dgrad = FN_K3[kind]
    x, w = torch.zeros(xshape, requires_grad=x_grad), torch.zeros(wshape, requires_grad=w_grad)
    before = dict(conv.launch_counts)
    y = _apply(kind, x, w, {})
    assert lib.calls == [(k3, fwd)] and conv.launch_counts == before
    grads = torch.autograd.grad(y, [t for t in (x, w) if t.requires_grad], torch.zeros_like(y))
    assert [tuple(g.shape) for g in grads] == [s for s, on in ((xshape, x_grad), (wshape, w_grad)) if on]
    assert lib.calls == [(k3, fwd)] + ([(k3, dgrad)] if x_grad else []) + ([wgrad] if w_grad else [])
    assert {k: conv.launch_counts[k] - before[k] for k in before} == {"dgrad": int(x_grad), "wgrad": int(w_grad)}
    assert ops.timer.held()


def test_autograd_function_batch_accumulates(fake, monkeypatch):
    """Two samples: per-sample launches in batch order, the second weight gradient added to the first."""
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    lib = fake()
    x, w = torch.zeros((2, 2, 2, 4, 4), requires_grad=True), torch.zeros((8, 2, 3, 3, 3), requires_grad=True)
    y = _apply("ends", x, w, {})
    torch.autograd.grad(y, [x, w], torch.zeros_like(y))
    fwd, dgrad = FN_K3["ends"]
    assert lib.calls == [("dmvs_conv3d_direct", fwd)] * 2 + [("dmvs_conv3d_direct", dgrad)] * 2 + \
        [("dmvs_conv3d_wgrad_c2", (2, 8, 2, 4, 4, 0)), ("dmvs_conv3d_wgrad_c2", (2, 8, 2, 4, 4, 1))]


def _copies(m):
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    return {"made": m, "deepcopy": copy.deepcopy(m), "reloaded": torch.load(buf, weights_only=False)}


@pytest.mark.parametrize("how", ["made", "deepcopy", "reloaded"])
def test_copied_modules_run_as_the_one_they_were_made_from(fake, monkeypatch, how):
    """A copied or reloaded module (an EMA copy, a checkpoint of the whole model) keeps its kind: the stride-2 layer still refuses odd
    extents before any launch, and every kind launches what the module it was copied from launches.  Further stubs: conv._check_input
    (accepts CPU tensors) and torch.cuda.device (a null context)."""
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    monkeypatch.setattr(conv, "_check_input", lambda *a: None)
    lib = fake()
    down = _copies(conv.DiffConv3d(8, 16, 3, stride=2, padding=1, bias=False))[how]
    with pytest.raises(_lib.DmvsError, match="needs even D, H, W"):
        down(torch.zeros(1, 8, 2, 3, 4))
    down2d = _copies(conv.DiffConv2d(32, 64, 3, stride=2, padding=1, bias=False))[how]
    with pytest.raises(_lib.DmvsError, match="needs even H, W"):
        down2d(torch.zeros(1, 32, 4, 3))
    _refused(lib)
    mods = {"square": conv.DiffConv3d(16, 16, 3, padding=1, bias=False), "strided": down,
            "transposed": conv.DiffConvTranspose3d(16, 8, 3, stride=2, padding=1, output_padding=1, bias=False),
            "ends": conv.DiffConv3d(2, 8, 3, padding=1, bias=False)}
    for kind, m in mods.items():
        m = m if kind == "strided" else _copies(m)[how]
        lib = fake()
        xshape, wshape, k3, wgrad = FN[kind]
        fwd, dgrad = FN_K3[kind]
        x = torch.zeros(xshape, requires_grad=True)
        y = m(x)
        gx, gw = torch.autograd.grad(y, [x, m.weight], torch.zeros_like(y))
        assert tuple(gx.shape) == xshape and tuple(gw.shape) == wshape
        assert lib.calls == [(k3, fwd), (k3, dgrad), wgrad]
