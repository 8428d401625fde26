"""K1's forward (``warp_corr_q4_kernel`` in its launch configurations, its fp16 twin and the generic ``warp_corr_kernel`` of
csrc/warp_corr.hip) on the MI355X against the float64 restatement tests/warp_corr_ref.py, at tile, window and view edges.

Yardstick: the restatement in pixel coordinates (tied to cost_agg_f64 and the reference's recorded volume in
tests/test_warp_corr_cpu.py, where the case tables' conditions and the criterion's power to tell eight wrong kernels apart are
asserted too).  No test here reads the reference or the oracle.  Kernel and restatement get the SAME fp32 p12: the kernel's own,
``ops.relative_proj`` copied back, for camera cases (``dmvs_relative_proj`` answers to test_relative_proj), the literal one else.

  criterion  per case and kernel configuration e_max = max|a - f64| / max|f64| and e_mean = mean|a - f64| / max|f64| over ALL
             elements; each <= 8 e_ref with e_ref from the fp32 run of the restatement on stock ATen (CPU), and 16 * 2^-23 where
             e_ref < 4 * 2^-23 (the project's criterion).  Where the yardstick is identically zero the output is all zeros.
  op order   on the WINDOWS table alone the generic kernel gets ``warp_corr_ref.op_order_allowance`` added to its MAX bound: it follows
             the reference's op order (normalise to [-1, 1], un-normalise), whose four extra roundings move a sample by up to
             3.5 * 2^-24 * (W - 1) px, while the projections of that table are so simple that e_ref sits on the criterion's floor.
             The allowance is that displacement times the yardstick's own slope, derived in the function's docstring, not taken
             from a measurement; test_warp_corr_cpu.py asserts that the fp32 oracle, which has the same op order, exceeds the
             plain max bound there and obeys the plain bounds everywhere else.  The generic kernel's mean bound, its max bound on
             every other table, and all bounds of the q4 kernel and its fp16 twin are the plain criterion.
  guards     every launch writes into a NaN-filled buffer with guard elements on both sides: afterwards every element of
             [2,D,H,W] is finite and the guards are still NaN.
  exact      two launches of a SCATTER or WINDOWS case give the same bits (the forward has no atomics); an accumulating launch
             without source views changes nothing.
  edges      one-row and one-column maps: the q4 kernel works in pixel coordinates and obeys the criterion; the generic kernel
             follows the reference's op order, whose (n - 1) / 2 = 0 makes the coordinate NaN: it must return finite, fully written
             output (docs/kernels/K1_warp_corr.md says what that is).

Every parity test prints its figures before it asserts (K1 lines); docs/kernels/K1_warp_corr.md keeps the measured ones.  No test
provokes a fault: the refusals are host-side argument checks that launch nothing."""
import functools

import pytest
import torch

import warp_corr_ref as R

pytestmark = pytest.mark.gpu

F32, F16 = torch.float32, torch.float16
GUARD = 1024
CASES = R.all_cases()
BY_TABLE = {t: [n for n, c in CASES.items() if c["table"] == t] for t in
            ("SHAPES", "VIEWS", "EDGE_SHAPES", "AFFINE", "WINDOWS", "SCATTER", "SPECIAL")}
# (layout, variant): default; 4 planes per workgroup; 8 planes per workgroup (ignored for D <= 4); 53 / 80 / 160 KB windows; generic
CONFIGS = {"q4": ("q4", 0), "q4_dc4": ("q4", 8), "q4_dc8": ("q4", 16), "q4_win53": ("q4", 2), "q4_win80": ("q4", 3),
           "q4_win160": ("q4", 4), "hwc_generic": ("hwc", 0)}
FP16_VARIANTS = {"f16": 0, "f16_dc8": 16, "f16_win80": 3}
FP16_CASES = [n for n in BY_TABLE["SHAPES"] if CASES[n]["depth"].shape[2] % 2 == 0] + BY_TABLE["WINDOWS"] + BY_TABLE["SCATTER"]


@pytest.fixture(params=list(CONFIGS))
def k1(request):
    return request.param


# ------------------------------------------------------------------------------------------------ shared, computed once
@functools.lru_cache(maxsize=None)
def p12_of(name):
    """The fp32 p12 both sides get (CPU tensor)."""
    from dmvsnet_amd import ops
    c = CASES[name]
    return c["p12"].clone() if c["p12"] is not None else ops.relative_proj(c["cams"].cuda().contiguous()).cpu()


@functools.lru_cache(maxsize=None)
def ref_of(name, half=False):
    """(float64 yardstick, (e_max, e_mean) of the fp32 restatement); ``half``: on the fp16-rounded features.  Never modified."""
    c = CASES[name]
    return R.reference(dict(c, feats=R.as_fp16(c["feats"])) if half else c, p12_of(name))


@functools.lru_cache(maxsize=None)
def allowance_of(name, layout):
    """What the reference's op order may add to the max bound: the generic kernel on the WINDOWS table only (R.allowance)."""
    return R.allowance(CASES[name], p12_of(name)) if layout == "hwc" else 0.0


@functools.lru_cache(maxsize=None)
def dev_feats(name, layout, half=False):
    from dmvsnet_amd import ops
    hwc = [f.permute(1, 2, 0).contiguous().cuda() for f in CASES[name]["feats"]]
    if layout == "hwc":
        return hwc
    q4 = [ops.hwc_to_q4(f) for f in hwc]
    return [f.half() for f in q4] if half else q4


def guarded(D, H, W, fill=float("nan")):
    """A [2,D,H,W] view in the middle of a larger buffer."""
    n = 2 * D * H * W
    buf = torch.full((n + 2 * GUARD,), fill, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(2, D, H, W)


def check_guards(tag, buf, out):
    torch.cuda.synchronize()
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all(), f"{tag}: wrote outside [2,D,H,W]"
    assert torch.isfinite(out).all(), f"{tag}: elements not written (or not finite)"


def launch(name, layout, variant=0, half=False, **kw):
    """One guarded launch of a case -> sim [2,D,H,W] (device)."""
    from dmvsnet_amd import ops
    feats = dev_feats(name, layout, half)
    buf, out = guarded(*CASES[name]["depth"].shape)
    got = ops.warp_corr(feats[0], feats[1:], p12_of(name).cuda(), CASES[name]["depth"].cuda(), out=out, variant=variant, layout=layout, **kw)
    assert got is out
    check_guards(f"{name} {layout}/{variant}", buf, out)
    return out


def compare(tag, got, f64, e_ref, allowance=0.0):
    e, b = R.errors(got, f64), R.bounds(e_ref, allowance)
    print(f"K1 {tag}: e_hip max {e[0]:.3e} mean {e[1]:.3e}  e_ref max {e_ref[0]:.3e} mean {e_ref[1]:.3e}  "
          f"ratio max {e[0] / b[0]:.3f} mean {e[1] / b[1]:.3f}")
    assert got.dtype == F32 and tuple(got.shape) == tuple(f64.shape), tag
    if f64.abs().max().item() == 0.0:
        assert torch.equal(got.cpu(), torch.zeros_like(got, device="cpu")), f"{tag}: the yardstick is identically zero"
        return
    assert e[0] <= b[0], (tag, "max", e[0], e_ref[0])
    assert e[1] <= b[1], (tag, "mean", e[1], e_ref[1])


# ------------------------------------------------------------------------------------------------ parity with float64
@pytest.mark.parametrize("name", [n for n in CASES if CASES[n]["table"] != "EDGE_SHAPES"])
def test_parity(name, k1):
    layout, variant = CONFIGS[k1]
    got = launch(name, layout, variant)
    compare(f"{name} {k1}", got, *ref_of(name), allowance_of(name, layout))
    if CASES[name]["table"] in ("WINDOWS", "SCATTER"):
        assert torch.equal(launch(name, layout, variant), got), f"{name} {k1}: two launches differ"


@pytest.mark.parametrize("name", BY_TABLE["EDGE_SHAPES"])
def test_one_row_and_one_column_maps(name, k1):
    """q4: the criterion.  Generic kernel: finite and fully written (``launch`` checks both); what it returns is printed."""
    layout, variant = CONFIGS[k1]
    got = launch(name, layout, variant)
    if layout == "q4":
        compare(f"{name} {k1}", got, *ref_of(name))
    else:
        print(f"K1 {name} {k1}: max|sim| {got.abs().max().item():.3e} (float64 restatement in pixel coordinates: "
              f"{ref_of(name)[0].abs().max().item():.3e})")


@pytest.mark.parametrize("name", BY_TABLE["SHAPES"])
def test_generic_kernel_with_a_padded_pixel_stride(name):
    """pix_stride = 2 C: the features are the leading channels of a wider pixel-major tensor whose other channels are NaN."""
    from dmvsnet_amd import ops
    c = CASES[name]
    C = c["C"]
    wide = [torch.cat((f, torch.full_like(f, float("nan"))), dim=2).contiguous() for f in dev_feats(name, "hwc")]
    buf, out = guarded(*c["depth"].shape)
    ops.warp_corr(wide[0], wide[1:], p12_of(name).cuda(), c["depth"].cuda(), out=out, C=C, pix_stride=2 * C, layout="hwc")
    check_guards(name, buf, out)
    compare(f"{name} hwc_stride{2 * C}", out, *ref_of(name))


@pytest.mark.parametrize("variant", list(FP16_VARIANTS))
@pytest.mark.parametrize("name", FP16_CASES)
def test_parity_fp16_features(name, variant):
    """The fp16 twin on the features rounded to fp16; yardstick and e_ref on the same rounded values cast up (products and sums are
    fp32 in the kernel: v_dot2_f32_f16)."""
    got = launch(name, "q4", FP16_VARIANTS[variant], half=True)
    compare(f"{name} {variant}", got, *ref_of(name, True))
    if CASES[name]["table"] in ("WINDOWS", "SCATTER"):
        assert torch.equal(launch(name, "q4", FP16_VARIANTS[variant], half=True), got), f"{name} {variant}: two launches differ"


# ------------------------------------------------------------------------------------------------ accumulate
@pytest.mark.parametrize("layout", ["q4", "hwc"])
@pytest.mark.parametrize("name", ["views-c8-n9", "views-c32-n9"])
def test_accumulate_over_two_launches(name, layout):
    """Views 0 .. 7, then an accumulating launch with view 8: the same criterion against the float64 sum over all nine.  An
    accumulating launch without source views leaves the volume bit-unchanged."""
    from dmvsnet_amd import ops
    c = CASES[name]
    feats, p12, depth = dev_feats(name, layout), p12_of(name).cuda(), c["depth"].cuda()
    buf, out = guarded(*c["depth"].shape)
    ops.warp_corr(feats[0], feats[1:9], p12[:8].contiguous(), depth, out=out, layout=layout)
    check_guards(name, buf, out)
    ops.warp_corr(feats[0], feats[9:], p12[8:].contiguous(), depth, out=out, accumulate=True, layout=layout)
    check_guards(name, buf, out)
    compare(f"{name} {layout}_8+1_views", out, *ref_of(name))
    before = out.clone()
    ops.warp_corr(feats[0], [], p12[:0].contiguous(), depth, out=out, accumulate=True, layout=layout)
    check_guards(name, buf, out)
    assert torch.equal(out, before)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_output_alone():
    """nsrc = 17, C = 12, fp16 with odd W, a pixel stride that is no multiple of 4 or below C: DmvsError from the host-side checks of
    the C entries; a p12 with the wrong row count: the wrapper's assertion.  Nothing is launched, ``out`` keeps its bits."""
    from dmvsnet_amd import ops
    from dmvsnet_amd._lib import DmvsError
    D, H, W = 2, 9, 33
    g = torch.Generator().manual_seed(5)
    depth = (500.0 + torch.rand((D, H, W), generator=g)).cuda()
    out = torch.full((2, D, H, W), 7.0, device="cuda")

    def hwc(C, w=W):
        return torch.randn((H, w, C), generator=g).cuda()

    def p12(n):
        return R.affine_p12(1.0, 0.25, 1.0, 0.25).repeat(n, 1).cuda()

    f8, q8 = hwc(8), ops.hwc_to_q4(hwc(8))
    with pytest.raises(DmvsError):
        ops.warp_corr(q8, [q8] * 17, p12(17), depth, out=out, layout="q4")
    with pytest.raises(DmvsError):
        ops.warp_corr(f8, [f8] * 17, p12(17), depth, out=out, layout="hwc")
    f12 = hwc(12)
    with pytest.raises(DmvsError):
        ops.warp_corr(ops.hwc_to_q4(f12), [ops.hwc_to_q4(f12)], p12(1), depth, out=out, layout="q4")
    with pytest.raises(DmvsError):
        ops.warp_corr(f12, [f12], p12(1), depth, out=out, layout="hwc")
    with pytest.raises(DmvsError):   # fp16 windows are staged in pixel pairs: W = 33
        ops.warp_corr(q8.half(), [q8.half()], p12(1), depth, out=out, layout="q4")
    f10 = hwc(10)
    with pytest.raises(DmvsError):
        ops.warp_corr(f10, [f10], p12(1), depth, out=out, C=8, pix_stride=10, layout="hwc")
    with pytest.raises(DmvsError):
        ops.warp_corr(f8, [f8], p12(1), depth, out=out, C=8, pix_stride=4, layout="hwc")
    for layout, f in (("q4", q8), ("hwc", f8)):
        with pytest.raises(AssertionError):
            ops.warp_corr(f, [f], p12(2), depth, out=out, layout=layout)
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 7.0))
    # the same inputs are accepted once the argument is legal
    ops.warp_corr(q8, [q8] * 16, p12(16), depth, out=out, layout="q4")
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and not torch.equal(out, torch.full_like(out, 7.0))
