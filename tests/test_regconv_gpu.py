"""K3's regularisation convs on the MI355X -- the thirteen regularisation rows of ``kCfgs`` (csrc/conv3d_mfma.hip): conv1 / conv3 /
conv5, conv7 / conv9 / conv11, the K3 fall-backs of conv0 / conv2 / conv4 / conv6 and the three 2D refine rows -- in every tile form,
held to the float64 restatement tests/regconv_ref.py at tile seams, ragged volumes and both loaders.  tests/test_regconv_cpu.py
checks that restatement, what the case tables claim and which mistakes the criterion catches.

  criterion   e_max and e_mean (distance to float64 over its max-abs), each <= 8 e_ref, 16 * 2^-23 where e_ref < 4 * 2^-23; e_ref
              from fp32 ATen on the CPU.  The unfloored e_mean_hip / e_mean_ref is printed, not asserted.
  forms       dmvs_tune("k3_min_blocks" / "k3_split_blocks") force the big, the plain small and the M-block-split tile at a small
              shape, dmvs_conv3d_mfma_plan proving which one runs right before each launch; "k3_single_buf_min_blocks" one or two
              LDS stages; "zpad_skip" and "k3_deconv_prefetch" their A/B arms.  Every change sits in try / finally, a fixture resets
              them all and the last test sets them once more.
  guards      every output lies inside a NaN-filled buffer: every element written and finite, the bands on both sides still NaN.
  exact       small-integer inputs and weights: the result equals the restatement with no tolerance.

Every launch goes through ops.conv3d(..., backend="mfma").  Every check prints its figures before it asserts (REGCONV lines) and the
worst ratio per mode and form, with its case, is printed at the end of the module; docs/kernels/K3_conv_mfma.md keeps the measured
ones.  No test provokes a fault."""
import gc

import pytest
import torch

import regconv_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = R.F32, R.F64
GUARD = 64          # NaN floats on either side of an output (256 bytes: the output stays 16-byte aligned)
WORST = {}          # (mode, form) -> [worst e_max / bound, its case, worst e_mean / bound, its case, worst unfloored mean ratio, its case]
BITS = {}           # what was compared bit for bit -> [pairs equal, pairs]
IDS = lambda v: v if isinstance(v, str) else "x".join(map(str, v))  # noqa: E731
MODE_NAME = {R.CONV_S1: "s1", R.CONV_S2: "s2", R.DECONV_S2: "t2"}


def _tune(**kw):
    from dmvsnet_amd import _lib
    for k, v in kw.items():
        if v is not None:
            _lib.check(_lib.load().dmvs_tune(k.encode(), int(v)), f"dmvs_tune({k})")


@pytest.fixture(autouse=True)
def reset_knobs():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device error is sticky: nothing more is launched on the card from this module
        pytest.exit(f"device error after a test, ending the session: {e}", returncode=3)
    _tune(**R.KNOB_DEFAULTS)
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    for key in sorted(WORST):
        w = WORST[key]
        print(f"REGCONV worst {key[0]} {key[1]}: e_hip / bound  max {w[0]:.3f} ({w[1]})  mean {w[2]:.3f} ({w[3]})  "
              f"unfloored e_mean_hip / e_mean_ref {w[4]:.3f} ({w[5]})")
    for key in sorted(BITS):
        print(f"REGCONV same bits {key}: {BITS[key][0]} of {BITS[key][1]} pairs")


def _bits(key, a, b):
    same = torch.equal(a, b)
    n = BITS.setdefault(key, [0, 0])
    n[0] += same
    n[1] += 1
    return same


def compare(tag, key, got, f64, e_ref):
    e, b = R.errors(got, f64), R.bounds(e_ref)
    r = (e[0] / b[0], e[1] / b[1])
    raw = e[1] / e_ref[1] if e_ref[1] > 0 else 0.0
    print(f"REGCONV {key[0]} {key[1]} {tag}: e_hip max {e[0]:.3e} mean {e[1]:.3e}  e_ref max {e_ref[0]:.3e} mean {e_ref[1]:.3e}  "
          f"bound max {b[0]:.3e} mean {b[1]:.3e}  ratio max {r[0]:.3f} mean {r[1]:.3f}  e_mean_hip / e_mean_ref {raw:.3f}")
    w = WORST.setdefault(key, [0.0, "", 0.0, "", 0.0, ""])
    for i, v in ((0, r[0]), (2, r[1]), (4, raw)):
        if v > w[i]:
            w[i], w[i + 1] = v, tag
    assert got.dtype == F32 and torch.isfinite(got).all(), f"{tag}: non-finite output"
    assert e[0] <= b[0], (key, tag, "max", e[0], e_ref[0])
    assert e[1] <= b[1], (key, tag, "mean", e[1], e_ref[1])


def cu(t, off=0):
    """The tensor on the device, 16-byte aligned; ``off`` floats past a 16-byte boundary otherwise."""
    t = t.to(F32).contiguous()
    if off == 0:
        d = t.to("cuda:0")
    else:
        buf = torch.empty(t.numel() + 8, device="cuda:0")
        assert buf.data_ptr() % 16 == 0
        d = buf[off:off + t.numel()].view(t.shape)
        d.copy_(t)
    assert d.data_ptr() % 16 == 4 * off and d.is_contiguous()
    return d


def _guarded(shape, off=0):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD + 8,), float("nan"), device="cuda:0")
    out = buf[GUARD + off:GUARD + off + n].view(shape)
    assert buf.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 4 * off and out.is_contiguous()
    return buf, out, (GUARD + off, GUARD + off + n)


def _check_guarded(tag, buf, out, span):
    torch.cuda.synchronize()
    assert torch.isfinite(out).all(), f"{tag}: output not fully written (or not finite)"
    assert torch.isnan(buf[:span[0]]).all() and torch.isnan(buf[span[1]:]).all(), f"{tag}: wrote outside the output"


def _layer(name, w, scale, shift, relu):
    """The layer as tests/test_gpu_parity.py::_layer builds it."""
    from dmvsnet_amd import ops
    cin, cout, mode, kd = R.ROWS[name][:4]
    wm = ops.pack_mfma(w, cin, cout, mode, kd)
    assert wm is not None
    return ops.ConvLayer(name, mode, kd, cin, cout, cu(ops.pack_direct(w, mode == R.DECONV_S2)), cu(wm),
                         None if scale is None else cu(scale), None if shift is None else cu(shift), relu)


def _assert_plan(name, form, D, H, W):
    """The tile form dmvs_conv3d_mfma_plan reports under the knobs in force is the one the table expects."""
    from dmvsnet_amd import _lib
    cin, cout, mode, kd = R.ROWS[name][:4]
    plan = _lib.load().dmvs_conv3d_mfma_plan(cin, cout, D, H, W, mode, kd)
    assert plan == R.expected_plan(name, form, D, H, W), (name, form, D, H, W, hex(plan))


def _conv(name, form, x, layer, shape, tag, skip=None, out_off=0):
    """ops.conv3d on K3 into a guarded output, the plan asserted right before the launch; -> a clone of the result."""
    from dmvsnet_amd import ops
    buf, out, span = _guarded((layer.cout,) + R.out_shape(name, *shape), out_off)
    _assert_plan(name, form, *shape)
    got = ops.conv3d(x, layer, skip=skip, out=out, backend="mfma")
    assert got.data_ptr() == out.data_ptr()
    _check_guarded(tag, buf, out, span)
    return out.clone()


def _form_knobs(form):
    mb, sb = R.K3_KNOBS[form]
    _tune(**R.K3_DEFAULTS)
    _tune(k3_min_blocks=mb, k3_split_blocks=sb)


def _between_forms(tag, outs, f64, e_ref):
    """The forms of one row on one input: each is within the bound of float64, so any two lie within two bounds of each other --
    re-association level; whether they are the same bits is printed, not claimed."""
    b = R.bounds(e_ref)
    names = list(outs)
    for i, a in enumerate(names):
        for c in names[i + 1:]:
            e = R.errors(outs[a], outs[c].double())
            scale = outs[c].abs().max().item() / max(f64.abs().max().item(), 1e-300)
            print(f"REGCONV forms {tag}: {a} vs {c}: e max {e[0]:.3e} mean {e[1]:.3e}  same bits {_bits('forms', outs[a], outs[c])}")
            assert e[0] * scale <= 2 * b[0] and e[1] * scale <= 2 * b[1], (tag, a, c, e)


def _device_case(name, shape):
    x, w, scale, shift, skip = R.case(name, *shape)
    return cu(x), _layer(name, w, scale, shift, True), cu(skip)


# ------------------------------------------------------------------------------------------------ every row, form and shape
@pytest.mark.parametrize("name,shape", R.cases(), ids=IDS)
def test_regconv(name, shape):
    """Every form of the row on one input, planar output, without and with the residual, against float64."""
    xc, layer, skc = _device_case(name, shape)
    mode = MODE_NAME[R.mode_of(name)]
    for with_skip in (False, True):
        f64, e_ref = R.reference(name, *shape, with_skip)
        outs = {}
        for form in R.forms_of(name):
            tag = f"{name} {IDS(shape)} {form}{' +skip' if with_skip else ''}"
            try:
                _form_knobs(form)
                outs[form] = _conv(name, form, xc, layer, shape, tag, skc if with_skip else None)
            finally:
                _tune(**R.K3_DEFAULTS)
            compare(tag, (mode, form), outs[form], f64, e_ref)
        _between_forms(f"{name} {IDS(shape)}{' +skip' if with_skip else ''}", outs, f64, e_ref)


# ------------------------------------------------------------------------------------------------ LDS stages
@pytest.mark.parametrize("name,shape", R.single_buf_cases(), ids=IDS)
def test_lds_stages(name, shape):
    """The 3D conv rows with one LDS stage (`k3_single_buf_min_blocks` = 0, the default) and with two (2^30: no launch reaches it),
    every form: both against float64; whether the bits agree is printed."""
    xc, layer, skc = _device_case(name, shape)
    f64, e_ref = R.reference(name, *shape, True)
    for form in R.forms_of(name):
        outs = {}
        for stages, value in ((1, 0), (2, R.HUGE)):
            tag = f"{name} {IDS(shape)} {form} stages{stages}"
            try:
                _form_knobs(form)
                _tune(k3_single_buf_min_blocks=value)
                outs[stages] = _conv(name, form, xc, layer, shape, tag, skc)
            finally:
                _tune(k3_single_buf_min_blocks=0, **R.K3_DEFAULTS)
            compare(tag, (MODE_NAME[R.mode_of(name)], f"{form}.stages{stages}"), outs[stages], f64, e_ref)
        print(f"REGCONV stages {name} {IDS(shape)} {form}: one vs two LDS stages: same bits {_bits('stages', outs[1], outs[2])}")


# ------------------------------------------------------------------------------------------------ zero-padding skip
@pytest.mark.parametrize("name,shape", R.zpad_cases(), ids=IDS)
def test_zpad_skip(name, shape):
    """`zpad_skip` off and on at the shapes that take a skipping instantiation (ZDEAD = 1, ZSKIP) and at their plain twins, every
    form, with the residual: EACH arm against float64 (a mistake common to both is not hidden), and the two arms equal."""
    xc, layer, skc = _device_case(name, shape)
    f64, e_ref = R.reference(name, *shape, True)
    assert R.skipping(name, *shape) == (shape in R.ZDEAD_SHAPES + R.ZSKIP_SHAPES)
    for form in R.forms_of(name):
        outs = {}
        for knob in (0, 1):
            tag = f"{name} {IDS(shape)} {form} zpad_skip={knob}"
            try:
                _form_knobs(form)
                _tune(zpad_skip=knob)
                outs[knob] = _conv(name, form, xc, layer, shape, tag, skc)
            finally:
                _tune(zpad_skip=1, **R.K3_DEFAULTS)
            compare(tag, (MODE_NAME[R.mode_of(name)], f"{form}.zpad{knob}"), outs[knob], f64, e_ref)
        assert torch.equal(outs[0], outs[1]), f"{name} {IDS(shape)} {form}: zpad_skip changes the result"


# ------------------------------------------------------------------------------------------------ residual prefetch
@pytest.mark.parametrize("shape", R.T2_SHAPES, ids=IDS)
def test_deconv_prefetch(shape):
    """conv11 with the residual, `k3_deconv_prefetch` off and on: each against float64, the two bit for bit equal."""
    xc, layer, skc = _device_case("conv11", shape)
    f64, e_ref = R.reference("conv11", *shape, True)
    outs = {}
    for knob in (0, 1):
        tag = f"conv11 {IDS(shape)} prefetch={knob}"
        try:
            _tune(k3_deconv_prefetch=knob)
            outs[knob] = _conv("conv11", "only", xc, layer, shape, tag, skc)
        finally:
            _tune(k3_deconv_prefetch=1)
        compare(tag, ("t2", f"only.prefetch{knob}"), outs[knob], f64, e_ref)
    assert torch.equal(outs[0], outs[1]), f"conv11 {IDS(shape)}: the residual prefetch changes the bits"


# ------------------------------------------------------------------------------------------------ misaligned views
@pytest.mark.parametrize("name,shape", R.MISALIGNED_CASES, ids=IDS)
def test_misaligned_views(name, shape):
    """W % 4 == 0 with the input one float past a 16-byte boundary (`can_v4` false: the dword loader), then the output (`st4` false:
    dword stores), then both -- ops.conv3d takes such views: the aligned run's bits, and the float64 bound."""
    x, w, scale, shift, skip = R.case(name, *shape)
    layer, skc = _layer(name, w, scale, shift, True), cu(skip)
    f64, e_ref = R.reference(name, *shape, True)
    for form in R.forms_of(name):
        outs = {}
        for in_off, out_off in ((0, 0), (1, 0), (0, 1), (1, 1)):
            tag = f"{name} {IDS(shape)} {form} in+{in_off} out+{out_off}"
            try:
                _form_knobs(form)
                outs[in_off, out_off] = _conv(name, form, cu(x, in_off), layer, shape, tag, skc, out_off)
            finally:
                _tune(**R.K3_DEFAULTS)
            compare(tag, (MODE_NAME[R.mode_of(name)], f"{form}.in{in_off}out{out_off}"), outs[in_off, out_off], f64, e_ref)
            assert torch.equal(outs[in_off, out_off], outs[0, 0]), f"{tag}: differs from the aligned run"


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("name,shape", R.EXACT_CASES, ids=IDS)
def test_exact_small_integers(name, shape):
    """Integer inputs and weights, scale 1, shift 0, no ReLU, an integer residual: every form equals the restatement exactly -- a
    tile seam, the parity map or the padding edge off by one tap shows with no tolerance at all."""
    x, w, skip = R.exact_case(name, *shape)
    cout = R.ROWS[name][1]
    want = R.run(name, x, w, None, None, False, skip)
    layer = _layer(name, w, torch.ones(cout), torch.zeros(cout), False)
    xc, skc = cu(x), cu(skip)
    for form in R.forms_of(name):
        tag = f"{name} {IDS(shape)} {form} exact"
        try:
            _form_knobs(form)
            got = _conv(name, form, xc, layer, shape, tag, skc)
        finally:
            _tune(**R.K3_DEFAULTS)
        diff = (got.cpu().double() - want).abs()
        print(f"REGCONV exact {tag}: max |diff| {diff.max().item():g} at {diff.argmax().item()} of {tuple(want.shape)}")
        assert torch.equal(got.cpu().double(), want), tag


def test_knobs_are_back_at_their_defaults():
    """Last in the file: the library has no getter, so the knobs are set once more; the two that steer the plan are read back."""
    from dmvsnet_amd import _lib
    _tune(**R.KNOB_DEFAULTS)
    lib = _lib.load()
    assert lib.dmvs_conv3d_mfma_plan(64, 64, 3, 9, 36, R.CONV_S1, 3) == R.expected_plan("conv6", "split", 3, 9, 36)
    assert lib.dmvs_conv3d_mfma_plan(16, 16, 32, 296, 400, R.CONV_S1, 3) == 2 * 256 + 8 + R.PLAN_V4
