"""The FeatureNet kernels on the MI355X -- K3s (``conv2d_c8_kernel``) and the fused ``conv0_fused_kernel``, K3 in its 2D modes with
the SKIP_UP2 / OUT_Q4 / IN_VIEWS epilogues and loaders, K3w's three 2D rows, ``fpn_wino_kernel`` and FeatureNet.run as a whole --
held to the float64 restatement tests/featurenet_ref.py at strip, row-block, tile and tile-walk seams.
tests/test_featurenet_cpu.py checks that restatement, what the case tables claim and which mistakes the criterion catches.

  criterion   e_max and e_mean (distance to float64 over its max-abs), each <= 8 e_ref, 16 * 2^-23 where e_ref < 4 * 2^-23; e_ref
              from fp32 ATen on the CPU (oracle.dmvs_oracle.feature_net for the whole net).  The Winograd forms get the same bound.
  knobs       dmvs_tune("c8_rows") puts K3s' row-block seams where the product has them; "k3_min_blocks" / "k3_split_blocks"
              force each tile form of K3 at a small shape, dmvs_conv3d_mfma_plan proving which one runs; "wino_persistent" /
              "wino_stages" A/B K3w's persistent tile walk.  Every change sits in try / finally and a fixture resets them all.
  exact       K3s and the fused kernel across all row-block sizes; IN_VIEWS against the planar form; the fused kernel against the
              two K3s launches; K3w with and without the persistent walk and with one or two LDS stages (the per-tile arithmetic
              does not depend on which workgroup, or which stage, holds the tile).
  guards      wherever the wrapper takes ``out=``: every output element written, nothing on either side of it.

Every check prints its figures before it asserts (FEAT lines) and the worst ratio per kernel family, with its case, is printed at
the end of the module; docs/kernels/K3s_conv2d_c8.md, K3_conv_mfma.md and K3w_conv_wino.md keep the measured ones.  No test
provokes a fault: declined shapes are host-side argument checks that launch nothing."""
import ctypes
import gc

import pytest
import torch

import featurenet_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = R.F32, R.F64
GUARD = 64          # sentinel floats on either side of an output (256 bytes: the output stays 16-byte aligned)
SENTINEL = -12345.0
WORST = {}          # family -> [worst e_max / bound, its case, worst e_mean / bound, its case]
KNOB_DEFAULTS = {"c8_rows": 0, "k3_min_blocks": 768, "k3_split_blocks": 1024, "wino_persistent": 1, "wino_stages": 0}
SWITCH_DEFAULTS = {"use_c8": True, "use_c8_fused": True, "use_wino": True}


def _tune(**kw):
    from dmvsnet_amd import _lib
    for k, v in kw.items():
        if v is not None:
            _lib.check(_lib.load().dmvs_tune(k.encode(), int(v)), f"dmvs_tune({k})")


@pytest.fixture(autouse=True)
def reset_knobs():
    yield
    from dmvsnet_amd import ops
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device error is sticky: nothing more is launched on the card from this module
        pytest.exit(f"device error after a test, ending the session: {e}", returncode=3)
    _tune(**KNOB_DEFAULTS)
    for k, v in SWITCH_DEFAULTS.items():
        setattr(ops, k, v)
    ops.launch_log = None
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    for key in sorted(WORST):
        w = WORST[key]
        print(f"FEAT worst {key}: e_hip / bound  max {w[0]:.3f} ({w[1]})  mean {w[2]:.3f} ({w[3]})")


def compare(tag, key, got, f64, e_ref):
    e, b = R.errors(got, f64), R.bounds(e_ref)
    r = (e[0] / b[0], e[1] / b[1])
    print(f"FEAT {key} {tag}: e_hip max {e[0]:.3e} mean {e[1]:.3e}  e_ref max {e_ref[0]:.3e} mean {e_ref[1]:.3e}  "
          f"bound max {b[0]:.3e} mean {b[1]:.3e}  ratio max {r[0]:.3f} mean {r[1]:.3f}")
    w = WORST.setdefault(key, [0.0, "", 0.0, ""])
    if r[0] > w[0]:
        w[0], w[1] = r[0], tag
    if r[1] > w[2]:
        w[2], w[3] = r[1], tag
    assert got.dtype == F32 and torch.isfinite(got).all(), f"{key} {tag}: non-finite output"
    assert e[0] <= b[0], (key, tag, "max", e[0], e_ref[0])
    assert e[1] <= b[1], (key, tag, "mean", e[1], e_ref[1])


def cu(t):
    t = t.to("cuda:0", F32).contiguous()
    assert t.data_ptr() % 16 == 0
    return t


def _guarded(shape):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda:0")
    out = buf[GUARD:GUARD + n].view(shape)
    out.fill_(float("nan"))
    assert out.data_ptr() % 16 == 0 and out.is_contiguous()
    return buf, out


def _check_guarded(tag, buf, out):
    torch.cuda.synchronize()
    n = out.numel()
    assert torch.isfinite(out).all(), f"{tag}: output not fully written"
    assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + n:] == SENTINEL).all(), f"{tag}: wrote outside the output"


def _layer(name, mode, w, scale=None, shift=None, relu=False):
    """A ConvLayer with every kernel form the library packs for the shape (a 3-channel weight gets K3's zero fourth channel)."""
    from dmvsnet_amd import ops
    return ops.make_layer(name, mode, cu(w), None if scale is None else cu(scale), None if shift is None else cu(shift), relu,
                          direct=False, coarse=False)


def _conv(x, layer, backend, oshape, tag, **kw):
    """ops.conv3d into a guarded output; -> a clone of the result."""
    from dmvsnet_amd import ops
    buf, out = _guarded(oshape)
    got = ops.conv3d(x, layer, out=out, backend=backend, **kw)
    assert got.data_ptr() == out.data_ptr()
    _check_guarded(tag, buf, out)
    return out.clone()


def _stack(x):
    """[3,V,H,W] -> the loader's image stack [V,3,H,W]."""
    return cu(x.permute(1, 0, 2, 3))


# ------------------------------------------------------------------------------------------------ K3s
@pytest.mark.parametrize("V,H,W", R.C8_SHAPES)
@pytest.mark.parametrize("cin", [3, 8])
def test_c8_rowsweep(cin, V, H, W):
    """conv2d_c8<3> (planar through the raw entry, IN_VIEWS through ops.conv3d) and conv2d_c8<8> at every row-block size of
    C8_ROWS: against float64 under the criterion, the same bits at every R (R only changes which wave computes a row), IN_VIEWS the
    same bits as planar."""
    from dmvsnet_amd import _lib, ops
    x, w, scale, shift = R.conv_case(cin, 8, 3, V, H, W)
    f64, e_ref = R.conv_reference(cin, 8, 3, 1, V, H, W)
    layer = _layer("c8", ops.CONV_S1, w, scale, shift, True)
    assert layer.w_c8 is not None
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    xc, first = cu(x), None
    for rows in R.C8_ROWS:
        tag = f"cin{cin} {V}x{H}x{W} rows{rows}"
        try:
            _tune(c8_rows=rows)
            if cin == 8:
                got = _conv(xc, layer, "c8", (8, V, H, W), tag)
            else:
                buf, out = _guarded((8, V, H, W))
                _lib.check(_lib.load().dmvs_conv2d_c8(P(xc), P(out), P(layer.w_c8), P(layer.scale), P(layer.shift), 3, V, H, W,
                                                      ops.RELU, None), "dmvs_conv2d_c8")
                _check_guarded(tag, buf, out)
                got = out.clone()
                views = _conv(_stack(x), layer, "c8", (8, V, H, W), tag + " in_views", in_views=True)
                assert torch.equal(views, got), f"{tag}: IN_VIEWS differs from the planar form"
        finally:
            _tune(c8_rows=0)
        compare(tag, f"K3s.c8<{cin}>", got, f64, e_ref)
        first = got if first is None else first
        assert torch.equal(got, first), f"{tag}: bits differ from rows{R.C8_ROWS[0]}"


@pytest.mark.parametrize("W", R.FUSED_W)
def test_conv0_fused(W):
    """dmvs_featurenet_conv0 at FUSED_W x the heights of C8_SHAPES x C8_ROWS: against float64, and bit for bit equal to the two
    K3s launches at every R (today's parity test asserts that at R = 8 only), hence to itself across R."""
    from dmvsnet_amd import ops
    for V, H in R.fused_vh():
        x, l0, l1 = R.fused_case(V, H, W)
        f64, e_ref = R.fused_reference(V, H, W)
        L0, L1 = _layer("conv0.0", ops.CONV_S1, *l0, True), _layer("conv0.1", ops.CONV_S1, *l1, True)
        imgs, first = _stack(x), None
        for rows in R.C8_ROWS:
            tag = f"{V}x{H}x{W} rows{rows}"
            try:
                _tune(c8_rows=rows)
                got = ops.featurenet_conv0(imgs, L0, L1)
                assert got is not None
                mid = _conv(imgs, L0, "c8", (8, V, H, W), tag + " conv0.0", in_views=True)
                two = _conv(mid, L1, "c8", (8, V, H, W), tag + " conv0.1")
            finally:
                _tune(c8_rows=0)
            assert tuple(got.shape) == (8, V, H, W)
            compare(tag, "K3s.fused", got, f64, e_ref)
            assert torch.equal(got, two), f"{tag}: the fused kernel differs from the two K3s launches"
            first = got if first is None else first
            assert torch.equal(got, first), f"{tag}: bits differ from rows{R.C8_ROWS[0]}"


# ------------------------------------------------------------------------------------------------ K3, 2D rows
def _assert_plan(name, form, V, H, W):
    """The tile form dmvs_conv3d_mfma_plan reports under the knobs in force is the one the table expects."""
    from dmvsnet_amd import _lib
    cin, cout, mode, _, _ = R.K3_ROWS[name]
    plan = _lib.load().dmvs_conv3d_mfma_plan(cin, cout, V, H, W, mode, 1)
    tz, ty, split = R.k3_expected_plan(name, form)
    assert plan >= 0 and (plan & 0xffff) == tz * 256 + ty and bool(plan & R.PLAN_MBS) == bool(split), (name, form, V, H, W, hex(plan))
    assert bool(plan & R.PLAN_V4) == (W % 4 == 0)


def _between_forms(tag, key, outs, f64, e_ref):
    """The forms of one row on one input: each is within the bound of float64, so any two lie within two bounds of each other --
    re-association level; whether they are the same bits is printed, not claimed."""
    b = R.bounds(e_ref)
    names = list(outs)
    for i, a in enumerate(names):
        for c in names[i + 1:]:
            e = R.errors(outs[a], outs[c].double())
            scale = outs[c].abs().max().item() / max(f64.abs().max().item(), 1e-300)
            print(f"FEAT {key} {tag}: {a} vs {c}: e max {e[0]:.3e} mean {e[1]:.3e}  same bits {torch.equal(outs[a], outs[c])}")
            assert e[0] * scale <= 2 * b[0] and e[1] * scale <= 2 * b[1], (tag, a, c, e)


@pytest.mark.parametrize("name,shape", R.k3_2d_cases(), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_k3_2d(name, shape):
    """Every FeatureNet row of K3's table in each of its tile forms, planar and quad-planar (and IN_VIEWS on conv0.0), against
    float64; the plan is asserted right before each launch."""
    from dmvsnet_amd import ops
    V, H, W = shape
    cin, cout, mode, k, _ = R.K3_ROWS[name]
    views = name == "conv0.0"
    stride = 2 if mode == R.CONV2D_K5S2 else 1
    x, w, scale, shift = R.conv_case(3 if views else cin, cout, k, V, H, W)
    f64, e_ref = R.conv_reference(3 if views else cin, cout, k, stride, V, H, W)
    layer = _layer(name, mode, w, scale, shift, True)
    assert layer.w_mfma is not None and layer.cin == cin
    Ho, Wo = f64.shape[-2:]
    xc = cu(torch.cat((x, torch.zeros_like(x[:1]))) if views else x)
    planar, quads = {}, {}
    for form in R.k3_forms(name):
        mb, sb = R.K3_KNOBS[form]
        tag = f"{name} {V}x{H}x{W} {form}"
        try:
            _tune(k3_min_blocks=mb, k3_split_blocks=sb)
            _assert_plan(name, form, V, H, W)
            planar[form] = _conv(xc, layer, "mfma", (cout, V, Ho, Wo), tag)
            _assert_plan(name, form, V, H, W)
            quads[form] = _conv(xc, layer, "mfma", (2, V, cout // 8, Ho, Wo, 4), tag + " q4", out_q4=True)
            if views:
                _assert_plan(name, form, V, H, W)
                sv = _conv(_stack(x), layer, "mfma", (cout, V, Ho, Wo), tag + " in_views", in_views=True)
                assert torch.equal(sv, planar[form]), f"{tag}: IN_VIEWS differs from the planar form"
                sq = _conv(_stack(x), layer, "mfma", (2, V, cout // 8, Ho, Wo, 4), tag + " in_views q4", in_views=True, out_q4=True)
                assert torch.equal(sq, quads[form]), f"{tag}: IN_VIEWS + OUT_Q4 differs from the planar input's"
        finally:
            _tune(k3_min_blocks=R.K3_DEFAULTS["k3_min_blocks"], k3_split_blocks=R.K3_DEFAULTS["k3_split_blocks"])
        key = f"K3.{'k5s2' if mode == R.CONV2D_K5S2 else 'k1' if mode == R.CONV2D_K1 else 's1'}.{form}"
        compare(tag, key, planar[form], f64, e_ref)
        compare(tag + " q4", key + ".q4", R.q4_halves_to_planar(quads[form].cpu()), f64, e_ref)
    _between_forms(f"{name} {V}x{H}x{W}", "K3.forms", planar, f64, e_ref)


@pytest.mark.parametrize("name,shape", R.k3_skip_cases(), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_k3_skip_up2(name, shape):
    """The CONV2D_K1 rows with the fused nearest x2 upsample-add (DMVS_SKIP_UP2), in each tile form, against float64."""
    from dmvsnet_amd import ops
    V, H, W = shape
    cin, cout = R.K3_ROWS[name][:2]
    x, w, scale, shift, sk = R.skip_case(cin, cout, V, H, W)
    f64, e_ref = R.skip_reference(cin, cout, V, H, W)
    layer = _layer(name, ops.CONV2D_K1, w, scale, shift, False)
    xc, skc, outs = cu(x), cu(sk), {}
    for form in R.k3_forms(name):
        mb, sb = R.K3_KNOBS[form]
        tag = f"{name} {V}x{H}x{W} {form} skip_up2"
        try:
            _tune(k3_min_blocks=mb, k3_split_blocks=sb)
            _assert_plan(name, form, V, H, W)
            outs[form] = _conv(xc, layer, "mfma", (cout, V, H, W), tag, skip=skc, skip_up2=True)
        finally:
            _tune(k3_min_blocks=R.K3_DEFAULTS["k3_min_blocks"], k3_split_blocks=R.K3_DEFAULTS["k3_split_blocks"])
        compare(tag, f"K3.k1.skip_up2.{form}", outs[form], f64, e_ref)
    _between_forms(f"{name} {V}x{H}x{W} skip_up2", "K3.forms", outs, f64, e_ref)


# ------------------------------------------------------------------------------------------------ K3w, 2D rows
@pytest.mark.parametrize("name,shape", R.wino_cases(), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_wino_2d(name, shape):
    """K3w's kdepth = 1 rows, planar and quad-planar, against float64 under the plain criterion.  On the shapes with more tiles
    than persistent workgroups: one tile per workgroup (wino_persistent = 0) and one / two LDS stages give the default's bits --
    a tile's arithmetic does not depend on which workgroup walks to it or which stage holds it."""
    from dmvsnet_amd import _lib, ops
    V, H, W = shape
    cin, cout, ty = R.WINO_ROWS[name]
    bn = R.WINO_BN[name]
    x, w, scale, shift = R.conv_case(cin, cout, 3, V, H, W, bn)
    f64, e_ref = R.conv_reference(cin, cout, 3, 1, V, H, W, bn)
    layer = _layer(name, ops.CONV_S1, w, scale, shift, bn)
    assert layer.w_wino is not None
    multi = shape in R.WINO_MULTI[ty]
    plan = _lib.load().dmvs_conv3d_wino_plan(cin, cout, V, H, W, 1)
    assert (plan > R.WINO_RESIDENT) == multi
    xc = cu(x)
    tag = f"{name} {V}x{H}x{W}"
    base = {}
    for q4 in (False, True):
        oshape = (2, V, cout // 8, H, W, 4) if q4 else (cout, V, H, W)
        got = _conv(xc, layer, "wino", oshape, tag + (" q4" if q4 else ""), out_q4=q4)
        base[q4] = got
        compare(tag + (" q4" if q4 else ""), f"K3w.{name}" + (".q4" if q4 else ""), R.q4_halves_to_planar(got.cpu()) if q4 else got,
                f64, e_ref)
    if not multi:
        return
    for knob, value in (("wino_persistent", 0), ("wino_stages", 1), ("wino_stages", 2)):
        for q4 in (False, True):
            oshape = (2, V, cout // 8, H, W, 4) if q4 else (cout, V, H, W)
            try:
                _tune(**{knob: value})
                got = _conv(xc, layer, "wino", oshape, f"{tag} {knob}={value}", out_q4=q4)
            finally:
                _tune(**{knob: KNOB_DEFAULTS[knob]})
            assert torch.equal(got, base[q4]), f"{tag} q4={q4}: {knob}={value} differs from the default's bits"


# ------------------------------------------------------------------------------------------------ fpn_wino_kernel
def _fpn_layer(w_lat, b_lat, w3):
    from dmvsnet_amd import ops
    layer = _layer("out3", ops.CONV_S1, w3)
    layer.w_wino_fpn = cu(ops.pack_wino_fpn(w3, w_lat, b_lat))
    return layer


@pytest.mark.parametrize("V,H,W", R.FPN_SHAPES)
def test_fpn(V, H, W):
    """inner2 (1x1 + bias) + nearest x2 upsample-add + out3 (3x3) as one Winograd convolution, planar and quad-planar, against
    float64 under the plain criterion; (9,82,168) has more tiles than the 256 persistent workgroups and a ragged last tile."""
    from dmvsnet_amd import ops
    lat, td, w_lat, b_lat, w3 = R.fpn_case(V, H, W)
    f64, e_ref = R.fpn_reference(V, H, W)
    layer = _fpn_layer(w_lat, b_lat, w3)
    got = ops.conv3d_fpn(cu(lat), cu(td), layer)
    assert got is not None and tuple(got.shape) == (16, V, H, W)
    compare(f"{V}x{H}x{W}", "fpn", got, f64, e_ref)
    q4 = ops.conv3d_fpn(cu(lat), cu(td), layer, out_q4=True)
    assert q4 is not None and tuple(q4.shape) == (2, V, 2, H, W, 4)
    compare(f"{V}x{H}x{W} q4", "fpn.q4", R.q4_halves_to_planar(q4.cpu()), f64, e_ref)


def test_fpn_declined_shapes():
    from dmvsnet_amd import ops
    _, _, w_lat, b_lat, w3 = R.fpn_case(*R.FPN_SHAPES[0])
    layer = _fpn_layer(w_lat, b_lat, w3)
    ops.launch_log = log = []
    for V, H, W in R.FPN_DECLINED:
        lat, td = torch.zeros((8, V, H, W), device="cuda:0"), torch.zeros((32, V, H // 2, W // 2), device="cuda:0")
        for q4 in (False, True):
            assert ops.conv3d_fpn(lat, td, layer, out_q4=q4) is None, (V, H, W)
    assert log == []     # nothing ran


def test_fpn_ones_buffer_small_large_small():
    """The layer's constant-one buffer (ops._ones_hw) serves every image size by prefix and only ever grows: small, large, small
    again on ONE layer give the right values, the second small call the first one's bits."""
    from dmvsnet_amd import ops
    small, large = R.FPN_SHAPES[1], R.FPN_SHAPES[3]
    _, _, w_lat, b_lat, w3 = R.fpn_case(*small)
    layer = _fpn_layer(w_lat, b_lat, w3)
    outs, sizes = [], []
    for V, H, W in (small, large, small):
        lat, td = R.fpn_case(V, H, W)[:2]
        got = ops.conv3d_fpn(cu(lat), cu(td), layer)
        assert got is not None
        f64 = R.fpn_head(lat, td, w_lat, b_lat, w3)
        e_ref = R.errors(R.aten_fpn_head(lat, td, w_lat, b_lat, w3), f64)
        compare(f"ones {V}x{H}x{W}", "fpn", got, f64, e_ref)
        outs.append(got)
        bufs = layer.ones["cuda:0"]
        sizes.append(bufs[-1].numel())
        assert sizes[-1] >= H * W and all((b == 1).all() for b in bufs)
    assert sizes[0] < sizes[1] == sizes[2]
    assert torch.equal(outs[0], outs[2])


# ------------------------------------------------------------------------------------------------ FeatureNet.run
LAUNCHES = ("dmvs_featurenet_conv0", "dmvs_conv2d_c8", "dmvs_conv3d_mfma", "dmvs_conv3d_wino", "dmvs_conv3d_wino_fpn2")


class _Spy:
    """The library with its conv launches recorded: (entry, return code) per call, in host order."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if name not in LAUNCHES:
            return f

        def call(*args):
            code = f(*args)
            self._log.append((name.replace("dmvs_", ""), code))
            return code
        return call


@pytest.fixture(scope="module")
def feature_net():
    from dmvsnet_amd.mvsnet import FeatureNet
    net = FeatureNet()
    missing = net.load_state_dict({k[len("feature."):]: v for k, v in R.net_state_dict().items()})
    assert not missing.missing_keys and not missing.unexpected_keys
    net = net.to("cuda:0")
    net.pack()
    return net


def _expected_launches(setting, H, W):
    """The C entry of every launch of FeatureNet.run, in order.  K3w takes a stride-1 3x3 layer where its width is a multiple of
    4 (`auto`: the plan is negative otherwise), K3s the two full-resolution layers, K3 everything else."""
    from dmvsnet_amd import _lib
    s3 = lambda w: "conv3d_wino" if w % 4 == 0 else "conv3d_mfma"  # noqa: E731
    ok = lambda n: (n, 0)  # noqa: E731
    if setting == "no_c8":
        seq = [ok("conv3d_mfma"), ok("conv3d_mfma")]
    elif setting == "no_c8_fused":
        seq = [ok("conv2d_c8"), ok("conv2d_c8")]
    else:
        seq = [ok("featurenet_conv0")]
    seq += [ok("conv3d_mfma"), ok(s3(W // 2)), ok(s3(W // 2)), ok("conv3d_mfma"), ok(s3(W // 4)), ok(s3(W // 4))]
    seq += [ok("conv3d_mfma"), ok("conv3d_mfma"), ok(s3(W // 2))]         # out1, inner1 + up2, out2
    if setting != "no_fuse_topdown":
        if R.net_level3_fused(H, W):
            return seq + [ok("conv3d_wino_fpn2")]
        seq.append(("conv3d_wino_fpn2", _lib.EUNSUPPORTED))
    return seq + [ok("conv3d_mfma"), ok(s3(W))]                            # inner2 + up2, out3


@pytest.mark.parametrize("setting", ["default", "no_fuse_topdown", "no_c8_fused", "no_c8"])
@pytest.mark.parametrize("V,H,W", R.NET_SHAPES)
def test_featurenet_run(feature_net, V, H, W, setting):
    """FeatureNet.run on the NET shapes in four settings: all three levels, both channel halves, against ``fpn`` in float64 with
    e_ref from the oracle; the launches are the expected kernels in the expected order."""
    from dmvsnet_amd import _lib, ops
    f64, e_ref = R.net_reference(V, H, W)
    imgs = cu(R.net_images(V, H, W))
    real_load, calls = _lib.load, []
    spy = _Spy(real_load(), calls)
    ops.launch_log = log = []
    try:
        feature_net.fuse_topdown = setting != "no_fuse_topdown"
        ops.use_c8_fused = setting != "no_c8_fused"
        ops.use_c8 = setting != "no_c8"
        _lib.load = lambda: spy
        outs = feature_net.run(imgs)
        torch.cuda.synchronize()
    finally:
        _lib.load = real_load
        feature_net.fuse_topdown = True
        ops.use_c8_fused = ops.use_c8 = True
        ops.launch_log = None
    want = _expected_launches(setting, H, W)
    assert calls == want, (setting, calls, want)
    assert log == ["feature_mfma"] * sum(code == 0 for _, code in want)
    for k, (o, y, er) in enumerate(zip(outs, f64, e_ref), 1):
        C = y.shape[0]
        assert tuple(o.shape) == (2, V, C // 8, y.shape[2], y.shape[3], 4) and o.is_contiguous()
        both = R.q4_halves_to_planar(o.cpu())
        for half, got, yh, eh in zip(("", "_c"), R.halves(both), R.halves(y), er):
            compare(f"{V}x{H}x{W} {setting}", f"net.stage{k}{half}", got, yh, eh)
