"""CPU: the host side of the differentiable stride-2 and transposed convolutions (dmvsnet_amd/conv.py, K3h's launcher) and their
yardstick.

  yardstick   the float64 restatement (tests/conv_s2_grad_ref.py) equals float64 autograd of F.conv3d / F.conv_transpose3d and the 2D
              forms for all eight layers, including the two "same tensor, other mode" data-gradient identities; the stored goldens meet
              the kink condition and carry the reference's gradients at fp32 distance from the restatement
  packing     ops.pack_index_mfma_s2 selects every weight element exactly once, its zero slots are the host packer's zeros, and its
              gather equals the host packing bit for bit in both modes of all eight layers
  launcher    dmvs_conv3d_wgrad_s2_plan / _workspace: positive for the four shapes, refused otherwise, a workspace that does not grow
              with the volume, tiles that cover a ragged coarse volume exactly once; argument refusals of dmvs_conv3d_wgrad_s2 itself
  module      constructor, odd-extent and CPU-input refusals, the parameter / state-dict contract, the C ABI agreement
"""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import conv_s2_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dmvs_conv3d_wgrad_s2", "dmvs_conv3d_wgrad_s2_workspace", "dmvs_conv3d_wgrad_s2_plan")


# ------------------------------------------------------------------------------------------------ yardstick
@pytest.mark.parametrize("mode,Ca,Cb,kd", R.LAYERS)
def test_restatement_equals_float64_autograd(mode, Ca, Cb, kd):
    B, Dc, Hc, Wc = 2, (2 if kd == 3 else 1), 3, 4
    g = torch.Generator().manual_seed(Ca + kd + (mode == "conv"))
    xs, ys = R.in_out_shapes(mode, Cb, kd, Dc, Hc, Wc, B)
    x = torch.randn(xs, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Ca, Cb, kd, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(ys, generator=g, dtype=torch.float64)
    sq = (lambda t: t) if kd == 3 else (lambda t: t.squeeze(2))
    usq = (lambda t: t) if kd == 3 else (lambda t: t.unsqueeze(2))
    conv, deconv = (F.conv3d, F.conv_transpose3d) if kd == 3 else (F.conv2d, F.conv_transpose2d)
    if mode == "conv":
        y = usq(conv(sq(x), sq(w), stride=2, padding=1))
        # identity 1: the data gradient is the TRANSPOSED conv of gy with the same tensor w (no flip, no transposition)
        other = usq(deconv(sq(gy), sq(w.detach()), stride=2, padding=1, output_padding=1))
        coarse, fine = gy, x
        got_y, got_gx = R.conv_s2_ref(x, w, kd), R.dgrad_conv_s2_ref(gy, w, kd)
    else:
        y = usq(deconv(sq(x), sq(w), stride=2, padding=1, output_padding=1))
        # identity 2: the data gradient is the STRIDE-2 conv of gy with the same tensor w read as [out][in]
        other = usq(conv(sq(gy), sq(w.detach()), stride=2, padding=1))
        coarse, fine = x, gy
        got_y, got_gx = R.deconv_s2_ref(x, w, kd), R.dgrad_deconv_s2_ref(gy, w, kd)
    assert y.shape == gy.shape
    gx, gw = torch.autograd.grad(y, [x, w], gy)
    rows = (("forward", got_y, y), ("wgrad G", R.wgrad_s2_ref(coarse, fine, kd), gw), ("dgrad", got_gx, gx), ("dgrad = other mode", other, gx))
    for name, got, want in rows:
        e = R.rel_dist(got, want)
        print(f"RESTATEMENT {mode} {Ca}/{Cb} kd {kd} {name}: {e:.2e}")
        assert got.shape == want.shape and e <= 1e-12, (name, e)
    # autograd over the restatement (what block_f64 relies on)
    gx2, gw2 = torch.autograd.grad(got_y, [x, w], gy)
    assert R.rel_dist(gx2, gx) <= 1e-12 and R.rel_dist(gw2, gw) <= 1e-12


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_goldens_meet_the_kink_condition(golden, name):
    g = golden("op_conv_s2_grad.npz")
    case, kw = R.golden_case(g, name), R.GOLDEN_CASES[name]
    xs, ys = R.in_out_shapes(kw["mode"], kw["Cb"], kw["kd"], kw["Dc"], kw["Hc"], kw["Wc"], kw["B"])
    assert tuple(case["x"].shape) == xs and tuple(case["gy"].shape) == ys == tuple(case["out"].shape)
    assert tuple(case["w"].shape) == (2 * kw["Cb"], kw["Cb"], kw["kd"], 3, 3) == tuple(case["g_w"].shape)
    fresh = R.make_case(**kw)
    assert all(torch.equal(case[k], fresh[k]) for k in ("x", "w", "gamma", "beta", "gy"))
    assert R.kink_violations(case) == 0
    f64 = R.block_f64(case)
    for k in ("out", "g_x", "g_w", "g_gamma", "g_beta"):
        e = R.rel_dist(case[k], f64[k])
        print(f"GOLDEN {name} {k}: e_ref {e:.2e}")
        assert e < 1e-5, (k, e)   # the recorded fp32 run is the same function (measured 0.5e-7 .. 6.0e-7)
    # the block's gradients for x and w are the restated data / weight gradient of the gradient that reaches the layer
    y = R.layer_ref(case["mode"], case["x"], case["w"], case["kd"]).requires_grad_(True)
    g_y = torch.autograd.grad(torch.relu(R.bn_train(y, case["gamma"], case["beta"])), y, case["gy"].double())[0]
    if case["mode"] == "conv":
        gw, gx = R.wgrad_s2_ref(g_y, case["x"], case["kd"]), R.dgrad_conv_s2_ref(g_y, case["w"], case["kd"])
    else:
        gw, gx = R.wgrad_s2_ref(case["x"], g_y, case["kd"]), R.dgrad_deconv_s2_ref(g_y, case["w"], case["kd"])
    assert R.rel_dist(gw, f64["g_w"]) <= 1e-12 and R.rel_dist(gx, f64["g_x"]) <= 1e-12


def test_golden_file_size():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "op_conv_s2_grad.npz")) < (1 << 20)


# ------------------------------------------------------------------------------------------------ packing
def modes_of(mode, Ca, Cb):
    """(cin, cout, K3 mode) of the layer's forward and of its data gradient; the weight tensor [Ca,Cb,...] serves both."""
    from dmvsnet_amd import ops
    conv, deconv = (Cb, Ca, ops.CONV_S2), (Ca, Cb, ops.DECONV_S2)
    return (conv, deconv) if mode == "conv" else (deconv, conv)


@pytest.mark.parametrize("mode,Ca,Cb,kd", R.LAYERS)
def test_pack_index_is_the_host_packing(mode, Ca, Cb, kd):
    from dmvsnet_amd import ops
    n = Ca * Cb * 9 * kd
    w = torch.randn(Ca, Cb, kd, 3, 3, generator=torch.Generator().manual_seed(Ca * kd))
    assert not (w == 0).any()
    flat = torch.cat((w.reshape(-1), torch.zeros(1)))
    for cin, cout, k3mode in modes_of(mode, Ca, Cb):
        idx = ops.pack_index_mfma_s2(cin, cout, k3mode, kd)
        host = ops.pack_mfma(w, cin, cout, k3mode, kd)
        assert idx.dtype == torch.int64 and idx.device.type == "cpu" and idx.numel() == host.numel() >= n
        assert ops.pack_index_mfma_s2(cin, cout, k3mode, kd) is idx, "not cached"
        assert int(idx.min()) >= 0 and int(idx.max()) <= n
        counts = torch.bincount(idx, minlength=n + 1)
        assert torch.equal(counts[:n], torch.ones(n, dtype=torch.int64)), "a weight element is not selected exactly once"
        assert int(counts[n]) == idx.numel() - n, "the zero slots are not exactly the rest"
        assert torch.equal(idx == n, host == 0), "the zero slots are not the host packer's zeros"
        assert torch.equal(flat[idx], host), "the gather is not the host packing"
        print(f"PACK {mode} {cin}->{cout} mode {k3mode} kd {kd}: {idx.numel()} packed floats, {int(counts[n])} zero slots")
    if kd == 1:   # the 2D weight layout [Ca,Cb,3,3] is the same memory
        cin, cout, k3mode = modes_of(mode, Ca, Cb)[0]
        assert torch.equal(ops.pack_mfma(w.squeeze(2), cin, cout, k3mode, 1), ops.pack_mfma(w, cin, cout, k3mode, 1))


def test_pack_index_refusals_and_the_square_index_unchanged():
    from dmvsnet_amd import ops
    from dmvsnet_amd._lib import DmvsError
    bad = ((16, 16, ops.CONV_S2, 3), (16, 32, ops.CONV_S1, 3), (16, 32, ops.DECONV_S2, 3), (32, 16, ops.CONV_S2, 3), (8, 16, ops.CONV_S2, 2),
           (4, 8, ops.CONV_S2, 3), (16, 32, ops.CONV_S2, 1), (128, 64, ops.DECONV_S2, 3))
    for cin, cout, mode, kd in bad:
        with pytest.raises(DmvsError):
            ops.pack_index_mfma_s2(cin, cout, mode, kd)
    for C, kd in ((8, 3), (48, 1)):   # pack_index_mfma keeps refusing what it refused
        with pytest.raises(DmvsError):
            ops.pack_index_mfma(C, kd, False)


# ------------------------------------------------------------------------------------------------ launcher
def test_plan_and_workspace():
    from dmvsnet_amd import _lib, ops
    lib = _lib.load()
    assert set(ops.WGRAD_S2_TILE) == {(Ca, kd) for Ca, _, kd in R.SHAPES}
    for Ca, Cb, kd in R.SHAPES:
        tz, ty, tx = ops.WGRAD_S2_TILE[(Ca, kd)]
        assert tz == 1
        per = 9 * kd * Ca * Cb
        small, large = lib.dmvs_conv3d_wgrad_s2_workspace(Ca, 2, 48, 176, kd), lib.dmvs_conv3d_wgrad_s2_workspace(Ca, 16, 296, 400, kd)
        assert small > 0 and small == large == lib.dmvs_conv3d_wgrad_s2_workspace(Ca, 1, 1, 1, kd), (Ca, kd, small, large)
        assert small % per == 0 and small // per <= 256   # whole partials, at most one per workgroup
        blocks = 2 if Ca == 64 else 1
        for Dc, Hc, Wc in ((1, 1, 1), (1, 3, 4), (2, 5, 9), (3, 10, 18), (2, 5, 67), (2, 48, 176), (7, 33, 65), (16, 296, 400)):
            plan = lib.dmvs_conv3d_wgrad_s2_plan(Ca, Dc, Hc, Wc, kd)
            assert plan > 0, (Ca, kd, Dc, Hc, Wc, plan)
            tiles, wgs = plan >> 9, plan & 511
            # the tiles are a regular grid of 1 x ty x tx boxes over [0,Dc) x [0,Hc) x [0,Wc): every coarse voxel in exactly one
            assert tiles == Dc * -(-Hc // ty) * -(-Wc // tx)
            assert tiles * ty * tx >= Dc * Hc * Wc
            shares = min(tiles, 256 // blocks)
            assert wgs % 8 == 0 and 0 < wgs <= 256 and wgs - 8 < shares * blocks <= wgs
            assert shares * per <= small   # every share's partial has its place
    for Ca, kd in ((8, 3), (24, 3), (16, 1), (32, 1), (16, 2), (16, 0), (128, 3), (0, 3), (64, 2)):
        assert lib.dmvs_conv3d_wgrad_s2_workspace(Ca, 4, 8, 8, kd) == 0
        assert lib.dmvs_conv3d_wgrad_s2_plan(Ca, 4, 8, 8, kd) == _lib.EUNSUPPORTED
    for Dc, Hc, Wc in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1, 4, (1 << 20) + 1)):
        assert lib.dmvs_conv3d_wgrad_s2_workspace(16, Dc, Hc, Wc, 3) == 0
        assert lib.dmvs_conv3d_wgrad_s2_plan(16, Dc, Hc, Wc, 3) == _lib.EINVAL


def test_wgrad_s2_entry_refuses_bad_arguments():
    """Argument checks happen before anything is launched: no GPU needed (the pointers are never followed)."""
    from dmvsnet_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.dmvs_conv3d_wgrad_s2(p, p, p, p, 8, 2, 4, 4, 3, 0, None) == _lib.EUNSUPPORTED
    assert lib.dmvs_conv3d_wgrad_s2(p, p, p, p, 16, 2, 4, 4, 1, 0, None) == _lib.EUNSUPPORTED
    assert lib.dmvs_conv3d_wgrad_s2(p, p, p, p, 64, 2, 4, 4, 2, 0, None) == _lib.EUNSUPPORTED
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert lib.dmvs_conv3d_wgrad_s2(*args, 16, 2, 4, 4, 3, 0, None) == _lib.EINVAL
    for dims in ((0, 4, 4), (2, 0, 4), (2, 4, 0)):
        assert lib.dmvs_conv3d_wgrad_s2(p, p, p, p, 16, *dims, 3, 0, None) == _lib.EINVAL


def test_abi_agreement():
    from dmvsnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "dmvs.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/dmvs.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert len(_lib.SIGNATURES["dmvs_conv3d_wgrad_s2"][1]) == 11
    assert _lib.SIGNATURES["dmvs_conv3d_wgrad_s2_workspace"][0] is ctypes.c_long
    declared = set(re.findall(r"\b(dmvs_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.SIGNATURES)
    assert lib.dmvs_version() == _lib.ABI_VERSION == 140
    text = open(os.path.join(ROOT, "scripts", "pmc_summary.py")).read()
    assert "conv_wgrad_s2_kernel" in text and "conv_wgrad_s2_reduce_kernel" in text
    src = open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "conv3d_wgrad_s2.h")).read()
    assert set(re.findall(r"__global__[^;{]*?void\s+(\w+)\s*\(", src)) == {"conv_wgrad_s2_kernel", "conv_wgrad_s2_reduce_kernel"}
    assert "atomic" not in src.lower().replace("no atomics", "")
    shared = open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "wgrad_share.h")).read()
    assert "atomic" not in shared.lower().replace("no atomics", "")


# ------------------------------------------------------------------------------------------------ module
def test_constructor_refusals_and_contract():
    import dmvsnet_amd
    from dmvsnet_amd import DiffConv2d, DiffConv3d, DiffConvTranspose2d, DiffConvTranspose3d, conv
    from dmvsnet_amd._lib import DmvsError
    assert all(n in dmvsnet_amd.__all__ for n in ("DiffConvTranspose3d", "DiffConvTranspose2d"))
    assert set(conv.launch_counts) == {"dgrad", "wgrad"}
    nn = torch.nn
    good = [(DiffConv3d, nn.Conv3d, ci, 2 * ci, {}) for ci in (8, 16, 32)] + [(DiffConv2d, nn.Conv2d, 32, 64, {})] \
        + [(DiffConvTranspose3d, nn.ConvTranspose3d, 2 * co, co, dict(output_padding=1)) for co in (32, 16, 8)] \
        + [(DiffConvTranspose2d, nn.ConvTranspose2d, 64, 32, dict(output_padding=1))]
    for cls, nn_cls, ci, co, extra in good:
        m = cls(ci, co, 3, stride=2, padding=1, bias=False, **extra)
        ref = nn_cls(ci, co, 3, stride=2, padding=1, bias=False, **extra)
        assert isinstance(m, nn_cls) and list(m.state_dict()) == ["weight"] and m.weight.shape == ref.weight.shape
        assert m.weight.shape[0] == 2 * m.weight.shape[1]   # [coarse][fine] in both forms
        assert [n for n, _ in m.named_parameters()] == ["weight"]
        m.load_state_dict(ref.state_dict())
        assert torch.equal(m.weight, ref.weight)
    # everything refused before stays refused, and the new forms take nothing else
    for cls in (DiffConv3d, DiffConv2d):
        for ci, co, kw in ((16, 16, dict(stride=2)), (16, 32, dict(stride=1)), (32, 16, dict(stride=2)), (8, 8, dict(stride=2)),
                           (64, 128, dict(stride=2)), (16, 32, dict(stride=2, bias=True)), (16, 32, dict(stride=2, padding=0)),
                           (16, 32, dict(stride=2, dilation=2)), (16, 32, dict(stride=2, groups=2)), (16, 32, dict(stride=3)),
                           (16, 32, dict(stride=2, padding_mode="reflect"))):
            if cls is DiffConv2d and (ci, co) == (32, 64):
                continue
            with pytest.raises(DmvsError):
                cls(ci, co, 3, **{"padding": 1, "bias": False, **kw})
    with pytest.raises(DmvsError):
        DiffConv2d(16, 32, 3, stride=2, padding=1, bias=False)   # a 3D shape only
    with pytest.raises(DmvsError):
        DiffConv3d(16, 32, 3, stride=(1, 2, 2), padding=1, bias=False)
    with pytest.raises(DmvsError):
        DiffConv3d(16, 32, 5, stride=2, padding=2, bias=False)
    base = dict(stride=2, padding=1, output_padding=1, bias=False)
    for cls, ci, co in ((DiffConvTranspose3d, 32, 16), (DiffConvTranspose2d, 64, 32)):
        for kw in (dict(output_padding=0), dict(stride=1, output_padding=0), dict(bias=True), dict(padding=0), dict(groups=2), dict(dilation=2)):
            with pytest.raises(DmvsError):
                cls(ci, co, 3, **{**base, **kw})
        for a, b in ((16, 32), (32, 32), (128, 64), (8, 4)):
            with pytest.raises(DmvsError):
                cls(a, b, 3, **base)
        with pytest.raises(DmvsError):
            cls(ci, co, 3, stride=2, padding=1, output_padding=1)   # the default has a bias
    with pytest.raises(DmvsError):
        DiffConvTranspose2d(32, 16, 3, **base)   # a 3D shape only


def test_input_refusals():
    from dmvsnet_amd import DiffConv2d, DiffConv3d, DiffConvTranspose2d, DiffConvTranspose3d, ops
    from dmvsnet_amd._lib import DmvsError
    c3, c2 = DiffConv3d(8, 16, 3, stride=2, padding=1, bias=False), DiffConv2d(32, 64, 3, stride=2, padding=1, bias=False)
    t3 = DiffConvTranspose3d(16, 8, 3, stride=2, padding=1, output_padding=1, bias=False)
    t2 = DiffConvTranspose2d(64, 32, 3, stride=2, padding=1, output_padding=1, bias=False)
    for m, x in ((c3, torch.zeros(1, 8, 2, 4, 4)), (c2, torch.zeros(1, 32, 4, 4)), (t3, torch.zeros(1, 16, 1, 2, 2)), (t2, torch.zeros(1, 64, 2, 2))):
        with pytest.raises(DmvsError, match="no CPU fallback"):
            m(x)
        with pytest.raises(DmvsError):
            m(x.half())
        with pytest.raises(DmvsError):
            m("x")
        with pytest.raises(DmvsError):
            m(x[:, :-1])
    with pytest.raises(DmvsError):
        t3(torch.zeros(1, 16, 1, 2, 2), output_size=(2, 4, 4))
    with pytest.raises(DmvsError):
        ops.conv3d_wgrad_s2(torch.zeros(16, 1, 2, 2), torch.zeros(8, 2, 4, 4), 3)   # CPU tensors
    # odd extents are refused before any launch (checked on the shape alone)
    from dmvsnet_amd import conv
    for shape, nd in (((1, 8, 3, 4, 4), 3), ((1, 8, 2, 5, 4), 3), ((1, 8, 2, 4, 7), 3), ((1, 32, 5, 4), 2), ((1, 32, 4, 3), 2)):
        with pytest.raises(DmvsError, match="even"):
            conv._check_even("DiffConv", torch.empty(shape, device="meta"), nd)
    conv._check_even("DiffConv", torch.empty((1, 8, 2, 4, 6), device="meta"), 3)
    conv._check_even("DiffConv", torch.empty((3, 32, 4, 6), device="meta"), 2)   # the batch may be odd


def test_wgrad_s2_shape_refusals():
    from dmvsnet_amd import ops
    from dmvsnet_amd._lib import DmvsError
    meta = lambda *s: torch.empty(s, device="meta")
    assert ops._wgrad_s2_dims(meta(16, 2, 3, 4), meta(8, 4, 6, 8), 3) == (16, 2, 3, 4)
    assert ops._wgrad_s2_dims(meta(64, 1, 3, 4), meta(32, 1, 6, 8), 1) == (64, 1, 3, 4)
    for coarse, fine, kd in ((meta(16, 2, 3, 4), meta(8, 2, 6, 8), 3), (meta(16, 2, 3, 4), meta(16, 4, 6, 8), 3), (meta(16, 2, 3, 4), meta(8, 4, 6, 7), 3),
                             (meta(64, 1, 3, 4), meta(32, 2, 6, 8), 1), (meta(1, 16, 2, 3, 4), meta(1, 8, 4, 6, 8), 3)):
        with pytest.raises(DmvsError):
            ops._wgrad_s2_dims(coarse, fine, kd)


def test_no_training_mode_for_the_whole_network():
    from dmvsnet_amd import MVSNet
    with pytest.raises(NotImplementedError):
        MVSNet([8], [4], verbose=False).train()


def test_packed_cache_follows_the_weight():
    """The per-module packed weights (host logic, no kernel): equal to the host packing in both modes, re-used while the weight is
    unchanged, re-packed after an in-place update."""
    from dmvsnet_amd import DiffConv3d, DiffConvTranspose2d, conv, ops
    mods = ((DiffConv3d(8, 16, 3, stride=2, padding=1, bias=False), 3), (DiffConvTranspose2d(64, 32, 3, stride=2, padding=1, output_padding=1, bias=False), 1))
    for m, kd in mods:
        Ca, Cb = m.weight.shape[:2]
        for mode, cin, cout in ((ops.CONV_S2, Cb, Ca), (ops.DECONV_S2, Ca, Cb)):
            layer = conv._packed_layer_s2(m._packed, m.weight, kd, mode)
            assert torch.equal(layer.w_mfma, ops.pack_mfma(m.weight.detach(), cin, cout, mode, kd))
            assert (layer.mode, layer.kdepth, layer.cin, layer.cout) == (mode, kd, cin, cout)
            assert layer.scale is None and layer.shift is None and not layer.relu
            assert conv._packed_layer_s2(m._packed, m.weight, kd, mode) is layer
        stale = conv._packed_layer_s2(m._packed, m.weight, kd, ops.CONV_S2)
        m.weight.grad = torch.ones_like(m.weight)
        torch.optim.SGD(m.parameters(), lr=0.5).step()
        fresh = conv._packed_layer_s2(m._packed, m.weight, kd, ops.CONV_S2)
        assert fresh is not stale and torch.equal(fresh.w_mfma, ops.pack_mfma(m.weight.detach(), Cb, Ca, ops.CONV_S2, kd))
