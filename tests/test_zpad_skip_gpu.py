"""GPU (-m gpu): dmvs_tune("zpad_skip") -- the kernel instantiations that leave out the depth taps of a 3x3x3 layer that only meet
zero padding (csrc/common.h: zpad_live_mask): K3w conv2 per tile, K3r conv4 / conv6 per output plane, and K3's stride-2 and
transposed layers where the volume is so shallow that every wave has the same dead tap (2 planes -> 1, 1 plane -> 2).  K3 on deeper
volumes and the `prob` head have no skipping form (measured: no gain, docs/kernels/); the K3 cases below cover those depths too, as
"the knob changes nothing there".

The products left out are exact zeros and the live ones keep their order, so with FINITE inputs the output is value-equal
(torch.equal) to the knob-off path; 0 * Inf / 0 * NaN at a border is out of scope (the knob-off path would give NaN there, the
skipping one would not).  Each case also holds the bound against ATen that the kernel's own parity test uses (2e-5 at an output scale
of ~1), writes into a NaN-filled buffer and must come back finite.  Shapes: 20 x 40 and the ragged 12 x 52 (partial tile rows and
columns), 10 x 50 for K3r (W % 4 != 0: its dword-loader form, which has no skipping instantiation and must simply be unchanged);
depths such that a tile or unit is first-only, last-only, both and neither, with odd depths leaving a partial z tile."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from dmvsnet_amd import MVSNet, _lib, ops, synth  # noqa: E402

DEV = "cuda:0"
HW = [(20, 40), (12, 52)]


def cu(a):
    return a.to(DEV).contiguous()


def rnd(*shape, seed=0, scale=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(g.standard_normal(shape, dtype=np.float32) * np.float32(scale))


def _layer(w, mode, kd=3, bn=True, seed=0):
    tr = mode == ops.DECONV_S2
    cin, cout = (w.shape[0], w.shape[1]) if tr else (w.shape[1], w.shape[0])
    g = np.random.Generator(np.random.PCG64(seed))
    scale = torch.from_numpy((0.5 + g.random(cout)).astype(np.float32)) if bn else None
    shift = torch.from_numpy((0.2 * g.standard_normal(cout)).astype(np.float32)) if bn else None
    wm = ops.pack_mfma(w, cin, cout, mode, kd)
    layer = ops.ConvLayer("t", mode, kd, cin, cout, cu(ops.pack_direct(w, tr)), None if wm is None else cu(wm),
                          None if scale is None else cu(scale), None if shift is None else cu(shift), bn)
    return layer, scale, shift


def _aten(x, w, mode, scale, shift, skip=None):
    if mode == ops.DECONV_S2:
        y = F.conv_transpose3d(x[None], w, None, 2, 1, 1)[0]
    else:
        y = F.conv3d(x[None], w, None, 1 if mode == ops.CONV_S1 else 2, 1)[0]
    if scale is not None:
        y = torch.relu(y * scale.view(-1, 1, 1, 1) + shift.view(-1, 1, 1, 1))
    return y if skip is None else y + skip


def _knob(value):
    _lib.check(_lib.load().dmvs_tune(b"zpad_skip", value), "dmvs_tune(zpad_skip)")


def _on_off(run):
    """run() with the knob off, then on (the default); the knob is back on whatever happens."""
    try:
        _knob(0)
        off = run()
        off = {k: v.clone() for k, v in off.items()} if isinstance(off, dict) else off.clone()
        _knob(1)
        on = run()
    finally:
        _lib.load().dmvs_tune(b"zpad_skip", 1)
    return on, off


def _check_conv(x, w, layer, mode, scale, shift, backend, skip=None, what=""):
    Do, Ho, Wo = layer.out_shape(*x.shape[1:])
    xs, sk = cu(x), None if skip is None else cu(skip)

    def run():
        out = torch.full((layer.cout, Do, Ho, Wo), float("nan"), device=DEV)   # every output must be written
        return ops.conv3d(xs, layer, skip=sk, out=out, backend=backend)
    on, off = _on_off(run)
    assert torch.isfinite(on).all() and torch.isfinite(off).all(), what
    assert torch.equal(on, off), what
    np.testing.assert_allclose(on.cpu().numpy(), _aten(x, w, mode, scale, shift, skip).numpy(), atol=2e-5, rtol=0.0, err_msg=what)
    return on


# ------------------------------------------------------------------------------------------ K3w: conv2
@pytest.mark.parametrize("H,W", HW)
def test_conv2_wino(H, W):
    """16 -> 16 on K3w (two output planes per tile): D = 2 one tile, first and last at once; 3 adds a tile whose second plane is past
    the end; 4 a first-only and a last-only tile; 5 is past the depth the skipping form is dispatched for (the plain kernel, a tile
    that is neither and a partial one).  Planar and quad-planar output."""
    w = rnd(16, 16, 3, 3, 3, seed=11, scale=1.0 / np.sqrt(16 * 27))
    layer, scale, shift = _layer(w, ops.CONV_S1, seed=3)
    layer.w_wino = cu(ops.pack_wino(w, 16, 16, 3))
    for D in (2, 3, 4, 5):
        x = rnd(16, D, H, W, seed=D)
        got = _check_conv(x, w, layer, ops.CONV_S1, scale, shift, "wino", what=f"conv2 D={D} {H}x{W}")
        xs = cu(x)
        on, off = _on_off(lambda: ops.conv3d(xs, layer, backend="wino", out_q4=True,
                                             out=torch.full((2, D, 2, H, W, 4), float("nan"), device=DEV)))
        assert torch.equal(on, off) and torch.isfinite(on).all(), (D, H, W)
        planar = on.permute(0, 2, 5, 1, 3, 4).reshape(16, D, H, W)   # [half][D][C/8][H][W][4] -> channel = half * 8 + quad * 4 + e
        assert torch.equal(planar, got), (D, H, W)


# ------------------------------------------------------------------------------------------ K3r: conv4 / conv6
@pytest.mark.parametrize("H,W", HW + [(10, 50)])
@pytest.mark.parametrize("C", [32, 64])
def test_conv4_conv6_coarse(C, H, W):
    """K3r's unit is one output plane: D = 2 has a first and a last plane, 3 also one that is neither; 5 is past the depth the skipping
    form is dispatched for.  10 x 50: the dword-loader form (unchanged by the knob)."""
    w = rnd(C, C, 3, 3, 3, seed=C, scale=1.0 / np.sqrt(C * 27))
    layer, scale, shift = _layer(w, ops.CONV_S1, seed=5)
    layer.w_coarse = cu(ops.pack_coarse(w, C, C, 3))
    for D in (2, 3, 5):
        _check_conv(rnd(C, D, H, W, seed=D + 10), w, layer, ops.CONV_S1, scale, shift, "coarse", what=f"K3r {C} D={D} {H}x{W}")


# ------------------------------------------------------------------------------------------ K3: stride-2 and transposed layers
@pytest.mark.parametrize("H,W", HW)
@pytest.mark.parametrize("cin,cout", [(8, 16), (16, 32), (32, 64)], ids=["conv1", "conv3", "conv5"])
def test_stride2_mfma(cin, cout, H, W):
    """D -> (D + 1) / 2.  D = 2: the flat one-output-plane tile, tap 0 reads plane -1 for every wave: the skipping instantiation (conv1
    is the packed-K form, 4 taps per k-step: taps 0-7 go, tap 8's step stays).  D = 1 (taps 0 and 2 dead) and 3 .. 6 (two-plane
    tiles) run the plain kernel whatever the knob says."""
    w = rnd(cout, cin, 3, 3, 3, seed=cin + cout, scale=1.0 / np.sqrt(cin * 27))
    layer, scale, shift = _layer(w, ops.CONV_S2, seed=7)
    assert layer.w_mfma is not None
    for D in (1, 2, 3, 4, 5, 6):
        _check_conv(rnd(cin, D, H, W, seed=D + 20), w, layer, ops.CONV_S2, scale, shift, "mfma", what=f"s2 {cin}->{cout} D={D} {H}x{W}")


@pytest.mark.parametrize("H,W", HW)
@pytest.mark.parametrize("cin,cout", [(64, 32), (32, 16), (16, 8)], ids=["conv7", "conv9", "conv11"])
def test_transposed_mfma(cin, cout, H, W):
    """D_in -> 2 D_in with the residual.  D_in = 1: the flat tile, every wave's input offset 1 is the padding plane (tap 0 reads plane
    D_in): the skipping instantiation, conv11 in its residual-prefetching form.  D_in = 2, 3: two-plane tiles, the plain kernel."""
    w = rnd(cin, cout, 3, 3, 3, seed=cin + cout + 1, scale=1.0 / np.sqrt(cin * 27))
    layer, scale, shift = _layer(w, ops.DECONV_S2, seed=9)
    assert layer.w_mfma is not None
    for D in (1, 2, 3):
        skip = rnd(cout, 2 * D, 2 * H, 2 * W, seed=D + 30)
        _check_conv(rnd(cin, D, H, W, seed=D + 40), w, layer, ops.DECONV_S2, scale, shift, "mfma", skip=skip,
                    what=f"deconv {cin}->{cout} D={D} {H}x{W}")


# ------------------------------------------------------------------------------------------ the whole forward
def test_forward_is_equal_with_and_without_the_skip():
    """Quarter-size test shape (synth c2_small: 288 x 416, 5 views, 16 / 8 / 8 planes: stage-3 and refine volumes of depth 8, 4, 2, 1):
    every tensor MVSNet.forward returns is equal with the knob on and off."""
    cfg = synth.CONFIGS["c2_small"]
    net = MVSNet(cfg["ndepths"], cfg["ratios"], verbose=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 0))
    net = net.to(DEV)
    imgs, proj, dv = synth.synth_inputs(cfg["H"], cfg["W"], cfg["V"], 0)
    args = (cu(imgs), {k: cu(v) for k, v in proj.items()}, cu(dv))

    def flat(out, prefix=""):
        res = {}
        for k, v in out.items():
            if torch.is_tensor(v):
                res[prefix + k] = v
            elif isinstance(v, dict):
                res.update(flat(v, prefix + k + "."))
        return res
    on, off = _on_off(lambda: flat(net(*args)))
    assert set(on) == set(off) and len(on) > 10
    for k in on:
        assert torch.isfinite(on[k]).all(), k
        assert torch.equal(on[k], off[k]), k
