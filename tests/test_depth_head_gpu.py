"""The depth head's forward on the MI355X -- the `prob` convolution (K2, ``conv_cout2_kernel``, both loader forms), its fused form
``dmvs_prob_regress`` and K4 (``depth_regress_kernel``, ``depth_regress_split_kernel``, ``depth_select_kernel``) -- held to the
float64 restatement tests/depth_head_ref.py at tile, block and map edges.  tests/test_depth_head_cpu.py checks that restatement,
the conditions of the case tables and which mistakes the criterion catches.

  criterion    per output tensor e_max and e_mean (distance to float64 over its max-abs), each <= 8 e_ref, 16 * 2^-23 where
               e_ref < 4 * 2^-23; e_ref from the fp32 oracle on the CPU (F.conv3d; depth_regress_main / _refine).
  conditional  the kernel's own fp32 expectations through the float64 tail: mode 1's pick bit for bit, mode 0's hypotheses and the
               confidence under caps that count the tail's roundings (depth_head_ref.sel_cap / conf_cap).
  exact        the impulse response of `prob`; with / without the softmax volume; AffinePlanes against their volume; depth_select
               against K4's own tail; SPECIAL (a), (d), (e).
  guards       every output element written, nothing on either side of it.

Every check prints its figures before it asserts (HEAD lines) and the worst ratio per tensor and kernel form is printed at the end
of the module; docs/kernels/K4_depth_regress.md and K2_prob_and_direct.md keep the measured ones.  No test provokes a fault: the
refusals are host-side argument checks that launch nothing."""
import ctypes
import gc

import pytest
import torch

import depth_head_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = R.F32, R.F64
GUARD = 1024
NAN = float("nan")
WORST = {}    # "form.tensor" -> [worst e_max / bound, worst e_mean / bound]


@pytest.fixture(autouse=True)
def free_gpu_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    for key in sorted(WORST):
        print(f"HEAD worst {key}: e_hip / bound  max {WORST[key][0]:.3f}  mean {WORST[key][1]:.3f}")


def compare(tag, key, got, f64, e_ref, keep=None):
    e, b = R.errors(got, f64, keep), R.bounds(e_ref)
    r = (e[0] / b[0], e[1] / b[1])
    print(f"HEAD {tag} {key}: e_hip max {e[0]:.3e} mean {e[1]:.3e}  e_ref max {e_ref[0]:.3e} mean {e_ref[1]:.3e}  "
          f"bound max {b[0]:.3e} mean {b[1]:.3e}  ratio max {r[0]:.3f} mean {r[1]:.3f}")
    w = WORST.setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], r[0]), max(w[1], r[1])
    assert got.dtype == F32 and tuple(got.shape) == tuple(f64.shape), tag
    if keep is None:
        assert torch.isfinite(got).all(), f"{tag} {key}: non-finite output"
    assert e[0] <= b[0], (tag, key, "max", e[0], e_ref[0])
    assert e[1] <= b[1], (tag, key, "mean", e[1], e_ref[1])


def conditional(tag, form, dsp, sel, conf, interval, mode):
    """The kernel's tail against the float64 tail of the kernel's own expectations."""
    d32 = dsp.cpu()
    want_sel, want_conf = R.tail(d32.double(), interval.cpu().double(), mode)
    if mode == 1:
        assert torch.equal(sel.cpu().double(), want_sel), f"{tag}: mode 1 is a pure selection"
    else:
        over = ((sel.cpu().double() - want_sel).abs() / R.sel_cap(d32, want_sel)).max().item()
        print(f"HEAD {tag} sel | dsp: worst error / cap {over:.3f}")
        w = WORST.setdefault(f"{form}.sel|dsp", [0.0, 0.0])
        w[0] = max(w[0], over)
        assert over <= 1.0, (tag, "sel | dsp", over)
    if float(interval) > 0:
        over = ((conf.cpu().double() - want_conf).abs() / R.conf_cap(d32, interval.cpu())).max().item()
        print(f"HEAD {tag} conf | dsp: worst error / cap {over:.3f}")
        w = WORST.setdefault(f"{form}.conf|dsp", [0.0, 0.0])
        w[0] = max(w[0], over)
        assert over <= 1.0, (tag, "conf | dsp", over)


def _layer(w):
    """The `prob` layer with the K2 weights alone (no other kernel form may answer)."""
    from dmvsnet_amd import ops
    return ops.ConvLayer("prob", ops.CONV_S1, 3, w.shape[1], 2, ops.pack_direct(w, False).cuda(), None, None, None, False)


def _on_gpu(x, misaligned=False):
    """A contiguous device copy; ``misaligned``: a view starting one float into a larger buffer (4-byte, not 16-byte aligned)."""
    if not misaligned:
        t = x.cuda().contiguous()
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.zeros(x.numel() + 8, device="cuda")
    t = buf[1:1 + x.numel()].view(x.shape)
    t.copy_(x)
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


def _guarded(shape):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), NAN, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(shape)


def _check_guarded(tag, buf, out):
    torch.cuda.synchronize()
    n = out.numel()
    assert torch.isfinite(out).all(), f"{tag}: output not fully written"
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all(), f"{tag}: wrote outside the output"


def _planes(case, itv):
    """What the kernels are handed: the volume, or AffinePlanes on the case's base with ``itv`` as their step."""
    from dmvsnet_amd import ops
    D = case["logits"].shape[1]
    return ops.AffinePlanes(case["base"].cuda(), itv, D) if case["base"] is not None else case["hyp"].cuda()


# ------------------------------------------------------------------------------------------------ plain `prob`
@pytest.mark.parametrize("Cin,D,H,W,misaligned", R.PROB_SHAPES)
def test_prob_plain(Cin, D, H, W, misaligned):
    from dmvsnet_amd import ops
    x, w = R.prob_case(Cin, D, H, W)
    f64 = R.prob_conv(x, w)
    e_ref = R.errors(R.oracle_conv(x, w), f64)
    buf, out = _guarded((2, D, H, W))
    got = ops.conv3d(_on_gpu(x, misaligned), _layer(w), out=out, backend="direct")
    assert got is out
    tag = f"prob Cin={Cin} {D}x{H}x{W}{' misaligned' if misaligned else ''}"
    _check_guarded(tag, buf, out)
    compare(tag, ("v4" if W % 4 == 0 and not misaligned else "dword") + ".logits", out, f64, e_ref)


@pytest.mark.parametrize("misaligned", [False, True], ids=["v4", "dword"])
def test_prob_impulse_response_is_exact(misaligned):
    """Unit impulses with pairwise disjoint supports at the tile seams, the map's borders and the 4-plane blocks' ends: every output
    voxel is one weight or 0, so there is nothing to round."""
    from dmvsnet_amd import ops
    x, w = R.impulse_case()
    want = R.prob_conv(x, w).float()
    buf, out = _guarded(tuple(want.shape))
    ops.conv3d(_on_gpu(x, misaligned), _layer(w), out=out, backend="direct")
    _check_guarded("impulse", buf, out)
    diff = (out.cpu() != want).nonzero()
    assert torch.equal(out.cpu(), want), f"first differing voxels (co, z, y, x): {diff[:8].tolist()}"


# ------------------------------------------------------------------------------------------------ fused head
def _fused_dsp(tag, xg, layers, planes, itv, alpha, H, W):
    from dmvsnet_amd import ops
    halves = []
    for b, layer in enumerate(layers):
        buf, out = _guarded((2, H, W))
        assert ops.prob_regress(xg, layer, planes, itv, alpha, out) is True, f"{tag}: declined"
        _check_guarded(f"{tag} branch {b}", buf, out)
        halves.append(out)
    return torch.cat(halves).contiguous()


@pytest.mark.parametrize("D,H,W", R.FUSED_SHAPES)
def test_fused_head(D, H, W):
    from dmvsnet_amd import ops
    c = R.fused_case(D, H, W)
    xg, layers = _on_gpu(c["x"]), [_layer(w) for w in c["w"]]
    for kind in ("synth", "affine"):
        k = c[kind]
        itv = k["interval"].cuda()
        planes = _planes(k, itv)
        for alpha in (1.0, 5.0):
            tag = f"fused {D}x{H}x{W} {kind} alpha={alpha:g}"
            dsp = _fused_dsp(tag, xg, layers, planes, itv, alpha, H, W)
            for mode in (0, 1):
                y, e_ref = R.fused_reference(D, H, W, kind, mode, alpha)
                if mode == 0:
                    compare(tag, f"fused{D}.dsp", dsp, y["dsp"], e_ref["dsp"])
                sel, conf = ops.depth_select(dsp, itv, mode)
                compare(f"{tag} mode={mode}", f"fused{D}.sel{mode}", sel, y["sel"], e_ref["sel"])
                compare(f"{tag} mode={mode}", f"fused{D}.conf", conf, y["conf"], e_ref["conf"])
                conditional(f"{tag} mode={mode}", "select", dsp, sel, conf, itv, mode)


@pytest.mark.parametrize("Cin,D,H,W,misaligned", R.FUSED_DECLINED)
def test_fused_head_declines_what_it_does_not_cover(Cin, D, H, W, misaligned):
    from dmvsnet_amd import ops
    x, w = R.prob_case(Cin, D, H, W)
    itv = torch.tensor(0.5, device="cuda")
    hyp = torch.full((D, H, W), 600.0, device="cuda")
    for planes in (hyp, ops.AffinePlanes(hyp[0].contiguous(), itv, D)):
        buf, out = _guarded((2, H, W))
        assert ops.prob_regress(_on_gpu(x, misaligned), _layer(w), planes, itv, 1.0, out) is False
        torch.cuda.synchronize()
        assert torch.isnan(buf).all(), "a declined call wrote to its output"


def test_fused_head_one_nan_voxel_spoils_its_3x3_neighbourhood_only():
    """SPECIAL (g): the non-finite expectations are the 3 x 3 pixels around the voxel, cut to the map, in both channels -- at a map
    corner, on both sides of a tile seam in x and y, and at the far corner; everything else obeys the criterion."""
    D, H, W = 8, 33, 68
    c = R.fused_case(D, H, W)
    k = c["synth"]
    from dmvsnet_amd import ops
    itv, layer = k["interval"].cuda(), _layer(c["w"][0])
    y, e_ref = R.fused_reference(D, H, W, "synth", 0, 1.0)
    for px, py in ((0, 0), (32, 15), (33, 16), (W - 1, H - 1)):
        x = c["x"].clone()
        x[3, 1, py, px] = NAN
        want = torch.zeros((H, W), dtype=torch.bool)
        want[max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = True
        f64 = R.head(torch.cat([R.prob_conv(x, c["w"][0])] * 2), k["hyp"].double(), k["interval"].double(), 1.0, 0)["dsp"][:2]
        assert torch.equal(~torch.isfinite(f64), want.expand(2, H, W)), "the yardstick's own set"
        buf, out = _guarded((2, H, W))
        assert ops.prob_regress(_on_gpu(x), layer, k["hyp"].cuda(), itv, 1.0, out) is True
        torch.cuda.synchronize()
        assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + out.numel():]).all()
        got = out.cpu()
        assert torch.equal(~torch.isfinite(got), want.expand(2, H, W)), (px, py, (~torch.isfinite(got)).nonzero()[:12].tolist())
        compare(f"fused nan voxel at ({px},{py})", "fused8.dsp", got, y["dsp"][:2], e_ref["dsp"], keep=~want.expand(2, H, W))


# ------------------------------------------------------------------------------------------------ K4
@pytest.mark.parametrize("D,H,W", R.K4_SHAPES)
def test_k4(D, H, W):
    from dmvsnet_amd import ops
    form = R.K4_FORM[D]
    for kind in R.DEPTHS:
        c = R.k4_case(D, H, W, kind)
        logits, itv = c["logits"].cuda(), c["interval"].cuda()
        planes = _planes(c, itv)
        vol = planes.volume() if kind == "affine" else None
        if vol is not None:
            assert torch.equal(vol.cpu(), c["hyp"])
        for mode, alpha in R.K4_RUNS:
            tag = f"K4 {D}x{H}x{W} {kind} mode={mode} alpha={alpha:g}"
            y, e_ref = R.k4_reference(D, H, W, kind, mode, alpha)
            dsp, sel, conf, none = ops.depth_regress(logits, planes, itv, alpha, mode, False)
            dsp_p, sel_p, conf_p, prob = ops.depth_regress(logits, planes, itv, alpha, mode, True)
            assert none is None and prob is not None
            assert torch.equal(dsp, dsp_p) and torch.equal(sel, sel_p) and torch.equal(conf, conf_p), f"{tag}: with / without prob"
            if vol is not None:   # the affine branch forms the volume's bits
                for a, v in zip((dsp, sel, conf), ops.depth_regress(logits, vol, itv, alpha, mode, False)[:3]):
                    assert torch.equal(a, v), f"{tag}: affine != volume"
                assert torch.equal(prob, ops.depth_regress(logits, vol, itv, alpha, mode, True)[3]), f"{tag}: affine != volume (prob)"
            s2, c2 = ops.depth_select(dsp, itv, mode)
            assert torch.equal(s2, sel) and torch.equal(c2, conf), f"{tag}: depth_select != K4's own tail"
            compare(tag, f"{form}.dsp", dsp, y["dsp"], e_ref["dsp"])
            compare(tag, f"{form}.sel{mode}", sel, y["sel"], e_ref["sel"])
            compare(tag, f"{form}.conf", conf, y["conf"], e_ref["conf"])
            compare(tag, "generic.prob", prob, y["prob"], e_ref["prob"])
            conditional(tag, form, dsp, sel, conf, itv, mode)


SPECIAL_SHAPES = ((4, 7, 255), (8, 5, 256), (32, 7, 63), (64, 3, 65), (5, 7, 255))


@pytest.mark.parametrize("D,H,W", SPECIAL_SHAPES)
def test_k4_special_logits(D, H, W):
    """SPECIAL (a) one-hot, (b) equal logits."""
    from dmvsnet_amd import ops
    form = R.K4_FORM[D]
    c = R.k4_case(D, H, W, "synth")
    hyp, itv = c["hyp"].cuda(), c["interval"].cuda()
    L, hot = R.special_one_hot(D, H, W)
    want_dsp = c["hyp"][None].expand(4, -1, -1, -1).gather(1, hot[:, None])[:, 0]
    for mode in (0, 1):
        for want_prob in (False, True):
            dsp, sel, conf, prob = ops.depth_regress(L.cuda(), hyp, itv, 5.0, mode, want_prob)
            assert torch.equal(dsp.cpu(), want_dsp), f"(a) mode {mode}: dsp is the chosen plane's depth"
            assert torch.isfinite(sel).all() and torch.isfinite(conf).all()
            if want_prob:
                assert torch.equal(prob.cpu(), torch.zeros((4, D, H, W)).scatter_(1, hot[:, None], 1.0)), "(a) p is one-hot"
            conditional(f"K4 {D}x{H}x{W} one-hot mode={mode}", form, dsp, sel, conf, itv, mode)
    L = R.special_equal(D, H, W)
    for mode, alpha in R.K4_RUNS[:2]:
        y = R.head(L.double(), c["hyp"].double(), c["interval"].double(), alpha, mode)
        o = R.oracle_head(L, c["hyp"], c["interval"], alpha, mode)
        dsp, sel, conf, _ = ops.depth_regress(L.cuda(), hyp, itv, alpha, mode, False)
        prob = ops.depth_regress(L.cuda(), hyp, itv, alpha, mode, True)[3]
        tag = f"K4 {D}x{H}x{W} equal logits mode={mode}"
        for name, got in (("dsp", dsp), ("sel", sel), ("conf", conf), ("prob", prob)):
            compare(tag, f"{form if name != 'prob' else 'generic'}.{name}{mode if name == 'sel' else ''}", got, y[name],
                    R.errors(o[name], y[name]))
        assert (prob.cpu().double() - 1.0 / D).abs().max().item() <= R.EPS32 / D, "(b) p = 1 / D to one rounding"


@pytest.mark.parametrize("D,H,W", SPECIAL_SHAPES)
def test_k4_special_confidence(D, H, W):
    """SPECIAL (c), (d), (e): four identical channels pin the 1e-5 and the saturated end; interval 0 pins the other end."""
    from dmvsnet_amd import ops
    form = R.K4_FORM[D]
    c = R.k4_case(D, H, W, "synth")
    hyp = c["hyp"].cuda()
    L = R.special_identical(c).cuda()
    for mode, alpha in R.K4_RUNS[:2]:
        itv = torch.tensor(2e-5, device="cuda")
        dsp, sel, conf, _ = ops.depth_regress(L, hyp, itv, alpha, mode, False)
        assert all(torch.equal(dsp[k], dsp[0]) for k in range(1, 4)), "(c) identical channels give the same bits"
        # var == 0: z = 2e-5f / 1e-5f, then conf_cap's count behind std (8 u = 4 * 2^-23)
        off = (conf.cpu().double() - R.CONF_AT_Z2).abs().max().item()
        print(f"HEAD K4 {D}x{H}x{W} (c) mode={mode}: |conf - 2 (sigmoid(2) - 0.5)| = {off / R.EPS32:.2f} * 2^-23")
        assert off <= 4 * R.EPS32
        itv = torch.tensor(2.65, device="cuda")
        dsp, sel, conf, _ = ops.depth_regress(L, hyp, itv, alpha, mode, False)
        assert torch.equal(conf, torch.ones_like(conf)), "(d) conf == 1"
        if mode == 1:
            assert torch.equal(sel, dsp[0]), "(d) every pick is the expectation"
        else:   # lo == hi: each stack entry is the expectation up to the roundings sel_cap counts (3 e need not be a float)
            assert ((sel - dsp[0]).abs().cpu().double() <= R.sel_cap(dsp.cpu(), sel.cpu().double())).all()
            pair = torch.where(((torch.arange(H).view(-1, 1) + torch.arange(W)) % 2 == 1).cuda(), sel[:2], sel[2:])
            assert torch.equal(pair, dsp[:2]), "(d) the (lo, hi) entries are the expectation itself"
        conditional(f"K4 {D}x{H}x{W} (d) mode={mode}", form, dsp, sel, conf, itv, mode)
        itv = torch.zeros((), device="cuda")
        conf = ops.depth_regress(c["logits"].cuda(), hyp, itv, alpha, mode, False)[2]
        assert torch.equal(conf, torch.zeros_like(conf)), "(e) interval 0: conf == 0"


@pytest.mark.parametrize("D,H,W", SPECIAL_SHAPES)
def test_k4_one_nan_logit_spoils_its_pixel_only(D, H, W):
    """SPECIAL (f).  At the pixel: the channel's expectation, the channel's softmax column and the confidence are non-finite, the
    other three expectations are not.  The pixel's ``sel`` is not pinned: fminf / fmaxf return their finite operand where
    torch.min / max hand the NaN on, and either way the NaN confidence flags the pixel.  Every other pixel obeys the criterion."""
    from dmvsnet_amd import ops
    form = R.K4_FORM[D]
    c = R.k4_case(D, H, W, "synth")
    ch, d0, y0, x0 = 2, D // 2, H - 1, W - 1
    L = c["logits"].clone()
    L[ch, d0, y0, x0] = NAN
    ok = torch.ones((H, W), dtype=torch.bool)
    ok[y0, x0] = False
    for mode, alpha in R.K4_RUNS[:2]:
        y, e_ref = R.k4_reference(D, H, W, "synth", mode, alpha)
        dsp, sel, conf, _ = ops.depth_regress(L.cuda(), c["hyp"].cuda(), c["interval"].cuda(), alpha, mode, False)
        dsp_p, sel_p, conf_p, prob = ops.depth_regress(L.cuda(), c["hyp"].cuda(), c["interval"].cuda(), alpha, mode, True)
        tag = f"K4 {D}x{H}x{W} nan logit mode={mode}"
        for got in ((dsp, sel, conf), (dsp_p, sel_p, conf_p)):
            bad = torch.zeros((4, H, W), dtype=torch.bool)
            bad[ch, y0, x0] = True
            assert torch.equal(~torch.isfinite(got[0].cpu()), bad), f"{tag}: dsp"
            assert torch.equal(~torch.isfinite(got[2].cpu()), ~ok), f"{tag}: conf"
            assert torch.isfinite(got[1].cpu()[..., ok]).all(), f"{tag}: sel"
        bad = torch.zeros((4, D, H, W), dtype=torch.bool)
        bad[ch, :, y0, x0] = True
        assert torch.equal(~torch.isfinite(prob.cpu()), bad), f"{tag}: prob"
        compare(tag, f"{form}.dsp", dsp, y["dsp"], e_ref["dsp"], keep=ok.expand(4, H, W))
        compare(tag, f"{form}.sel{mode}", sel, y["sel"], e_ref["sel"], keep=ok.expand_as(y["sel"]))
        compare(tag, f"{form}.conf", conf, y["conf"], e_ref["conf"], keep=ok)
        compare(tag, "generic.prob", prob, y["prob"], e_ref["prob"], keep=ok.expand(4, D, H, W))


# ------------------------------------------------------------------------------------------------ fully written outputs
def _p(t, offset=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * offset)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _carve(sizes):
    """One NaN-filled allocation, the regions of ``sizes`` floats separated (and framed) by GUARD-float gaps -> (buffer, offsets)."""
    offs, at = [], GUARD
    for n in sizes:
        offs.append(at)
        at += n + GUARD
    return torch.full((at,), NAN, device="cuda"), offs


def _check_carved(tag, buf, offs, sizes):
    torch.cuda.synchronize()
    written = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
    for o, n in zip(offs, sizes):
        written[o:o + n] = True
        assert torch.isfinite(buf[o:o + n]).all(), f"{tag}: an output is not fully written"
    assert torch.isnan(buf[~written]).all(), f"{tag}: wrote into a gap"


@pytest.mark.parametrize("D,H,W", [(32, 5, 65), (64, 5, 65), (4, 3, 257), (8, 3, 257), (5, 3, 257)])
def test_k4_entries_write_their_outputs_and_nothing_else(D, H, W):
    from dmvsnet_amd import _lib
    lib = _lib.load()
    c = R.k4_case(D, H, W, "affine")
    logits, hyp, base, itv = c["logits"].cuda(), c["hyp"].cuda(), c["base"].cuda(), c["interval"].cuda()
    hw = H * W
    for mode in (0, 1):
        for want_prob in (False, True):
            sizes = [4 * hw, 4 * hw if mode == 0 else hw, hw] + ([4 * D * hw] if want_prob else [])
            for affine in (False, True):
                buf, offs = _carve(sizes)
                fn = lib.dmvs_depth_regress_affine if affine else lib.dmvs_depth_regress
                code = fn(_p(logits), _p(base if affine else hyp), _p(itv), 1.0, mode, D, H, W, _p(buf, offs[0]), _p(buf, offs[1]),
                          _p(buf, offs[2]), _p(buf, offs[3]) if want_prob else None, _stream())
                assert code == 0
                _check_carved(f"K4 {D}x{H}x{W} mode={mode} prob={want_prob} affine={affine}", buf, offs, sizes)


@pytest.mark.parametrize("H,W", [(5, 65), (3, 257)])
def test_depth_select_entry_writes_its_outputs_and_nothing_else(H, W):
    from dmvsnet_amd import _lib
    lib = _lib.load()
    dsp = (600.0 + 8.0 * torch.randn((4, H, W), generator=torch.Generator().manual_seed(H * W))).cuda()
    itv = torch.tensor(0.5, device="cuda")
    for mode in (0, 1):
        sizes = [4 * H * W if mode == 0 else H * W, H * W]
        buf, offs = _carve(sizes)
        assert lib.dmvs_depth_select(_p(dsp), _p(itv), mode, H, W, _p(buf, offs[0]), _p(buf, offs[1]), _stream()) == 0
        _check_carved(f"depth_select {H}x{W} mode={mode}", buf, offs, sizes)
