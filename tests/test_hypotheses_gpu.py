"""N2 (the hypothesis-plane kernels ``hyp_first_kernel`` / ``hyp_next_kernel``), their affine consumers in K1 / K4 and the layout
glue of csrc/layout.hip on the MI355X.

Yardstick: the float64 restatement tests/hypotheses_ref.py (checked against the oracle and the reference's recorded planes in
tests/test_hypotheses_cpu.py, where the case tables' conditions and their power to tell mutations apart are asserted too).  No test
here reads the reference or the oracle.

  criterion  per output tensor (and for the interval scalar): e = max-abs distance to the float64 restatement over the tensor's
             max-abs; e_hip <= 8 e_ref with e_ref from the fp32 run of the restatement on stock ATen (CPU), and 16 * 2^-23 where
             e_ref < 4 * 2^-23 (the project's criterion).  One first-stage case has an end of its inverse-depth range at exactly 0
             (hypotheses_ref.first_cases): there the non-finite planes must coincide and the rest obeys the criterion.
  exact      K1 / K4 fed ``AffinePlanes`` against the same kernel fed ``planes.volume()``, and the layout kernels against ``permute``
             on integer-valued inputs: torch.equal.
  guards     the C entries write every element of their output and nothing on either side of it.

Every parity test prints its figures before it asserts (HYP lines); docs/kernels/N2_hypotheses.md keeps the measured ones.  No test
provokes a fault: the refusals are host-side argument checks that launch nothing."""
import ctypes
import functools
import gc

import pytest
import torch

import hypotheses_ref as R

pytestmark = pytest.mark.gpu

F32 = torch.float32
FIRST, LATER = R.first_cases(), R.later_cases()
GUARD = 1024


@pytest.fixture(autouse=True)
def free_gpu_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def compare(tag, got, f64, f32):
    a, b, same = R.finite_part(got, f64)
    r, _, same_ref = R.finite_part(f32, f64)
    e_hip, e_ref = R.rel_dist(a, b), R.rel_dist(r, b)
    bound = R.bound_of(e_ref)
    print(f"HYP {tag}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {bound:.3e}  ratio {e_hip / bound:.3f}")
    assert got.dtype == F32 and tuple(got.shape) == tuple(f64.shape), tag
    assert same and same_ref, f"{tag}: non-finite elements differ from the float64 restatement's"
    assert e_hip <= bound, (tag, e_hip, e_ref)


@functools.lru_cache(maxsize=None)
def ref_first(name, inverse):
    """(float64 planes, interval, fp32 planes, interval) of one first-stage case: computed once, never modified."""
    c = FIRST[name]
    return R.first(c["dv"], c["D"], c["H"], c["W"], inverse) + R.first(c["dv"], c["D"], c["H"], c["W"], inverse, F32)


@functools.lru_cache(maxsize=None)
def ref_later(name, inverse):
    c = LATER[name]
    args = (c["last"], c["dv"], c["ratio"], c["D"], inverse, c["up"])
    return R.later(*args) + R.later(*args, F32)


# ------------------------------------------------------------------------------------------------ parity with float64
@pytest.mark.parametrize("name", list(FIRST))
def test_first_stage(name):
    from dmvsnet_amd import ops
    c = FIRST[name]
    D, H, W, dv = c["D"], c["H"], c["W"], c["dv"].cuda()
    for inverse in (False, True):
        f64, i64, f32, i32 = ref_first(name, inverse)
        got, itv = ops.hypotheses_first(dv, D, H, W, inverse)
        compare(f"first {name} inv={int(inverse)} planes", got, f64, f32)
        compare(f"first {name} inv={int(inverse)} interval", itv, i64, i32)
    f64, i64, f32, i32 = ref_first(name, False)
    planes, itv = ops.hypotheses_first(dv, D, H, W, False, affine=True)
    assert isinstance(planes, ops.AffinePlanes) and planes.shape == (D, H, W) and planes.step is itv
    compare(f"first {name} base", planes.base, f64[0], f32[0])
    compare(f"first {name} base interval", itv, i64, i32)
    compare(f"first {name} affine volume", planes.volume(), f64, R.affine_volume(f32[0], i32, D))


@pytest.mark.parametrize("name", list(LATER))
def test_later_stages(name):
    from dmvsnet_amd import ops
    c = LATER[name]
    D, up, dv, last = c["D"], c["up"], c["dv"].cuda(), c["last"].cuda()
    for inverse in (False, True):
        f64, i64, f32, i32 = ref_later(name, inverse)
        got, itv = ops.hypotheses_next(last, dv, c["ratio"], D, inverse, up=up)
        compare(f"later {name} inv={int(inverse)} planes", got, f64, f32)
        compare(f"later {name} inv={int(inverse)} interval", itv, i64, i32)
    f64, i64, f32, i32 = ref_later(name, False)
    planes, itv = ops.hypotheses_next(last, dv, c["ratio"], D, False, affine=True, up=up)
    assert isinstance(planes, ops.AffinePlanes) and planes.shape == (D, up * c["h"], up * c["w"]) and planes.step is itv
    compare(f"later {name} base", planes.base, f64[0], f32[0])
    compare(f"later {name} base interval", itv, i64, i32)
    compare(f"later {name} affine volume", planes.volume(), f64, R.affine_volume(f32[0], i32, D))
    # inverse-depth sampling is not affine in d: the volume comes back whatever ``affine`` says
    vol, _ = ops.hypotheses_next(last, dv, c["ratio"], D, True, affine=True, up=up)
    assert torch.is_tensor(vol) and tuple(vol.shape) == (D, up * c["h"], up * c["w"])


# ------------------------------------------------------------------------------------------------ guards and refusals
def _p(t, offset_floats=0):
    return ctypes.c_void_p(t.data_ptr() + 4 * offset_floats)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(n):
    return torch.full((n + 2 * GUARD,), float("nan"), device="cuda")


def _check_guarded(tag, buf, n, itv):
    torch.cuda.synchronize()
    assert torch.isfinite(buf[GUARD:GUARD + n]).all(), f"{tag}: output not fully written"
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all(), f"{tag}: wrote outside the output"
    assert torch.isfinite(itv).all(), f"{tag}: interval not written"


@pytest.mark.parametrize("D,H,W", [(5, 3, 257), (48, 2, 300), (8, 6, 258)])
def test_first_stage_writes_its_output_and_nothing_else(D, H, W):
    from dmvsnet_amd import _lib
    lib, dv = _lib.load(), R.depth_values("synth192").cuda()
    for inverse in (0, 1):
        buf, itv = _guarded(D * H * W), torch.full((1,), float("nan"), device="cuda")
        assert lib.dmvs_hypotheses_first(_p(dv), dv.numel(), D, H, W, inverse, _p(buf, GUARD), _p(itv), _stream()) == 0
        _check_guarded(f"first {D}x{H}x{W} inv={inverse}", buf, D * H * W, itv)
    buf, itv = _guarded(H * W), torch.full((1,), float("nan"), device="cuda")   # one plane, not D
    assert lib.dmvs_hypothesis_base_first(_p(dv), dv.numel(), D, H, W, _p(buf, GUARD), _p(itv), _stream()) == 0
    _check_guarded(f"base_first {D}x{H}x{W}", buf, H * W, itv)


@pytest.mark.parametrize("h,w,up,D", [(3, 129, 2, 8), (2, 150, 2, 5), (3, 257, 1, 8), (2, 300, 1, 24)])
def test_later_stages_write_their_output_and_nothing_else(h, w, up, D):
    from dmvsnet_amd import _lib
    lib, dv = _lib.load(), R.depth_values("synth192").cuda()
    last = R.make_last(h, w, dv, 2.0, *R.LAST_RANGE["synth192"], 7).cuda()
    H, W = up * h, up * w
    for inverse, base_only in ((0, 0), (1, 0), (0, 1)):
        n = H * W * (1 if base_only else D)
        buf, itv = _guarded(n), torch.full((1,), float("nan"), device="cuda")
        code = lib.dmvs_hypotheses_next_up(_p(last), h, w, up, _p(dv), dv.numel(), 2.0, D, inverse, base_only, _p(buf, GUARD), _p(itv),
                                           _stream())
        assert code == 0
        _check_guarded(f"next_up {h}x{w} up={up} D={D} inv={inverse} base_only={base_only}", buf, n, itv)


def test_host_side_refusals():
    """Argument checks of the C entries: DMVS_EINVAL before any launch."""
    from dmvsnet_amd import _lib, ops
    from dmvsnet_amd._lib import DmvsError
    dv = R.depth_values("synth192").cuda()
    last = torch.full((4, 6), 600.0, device="cuda")
    for affine in (False, True):
        with pytest.raises(DmvsError):
            ops.hypotheses_first(dv[:1].contiguous(), 8, 4, 6, False, affine=affine)   # n < 2
        with pytest.raises(DmvsError):
            ops.hypotheses_first(dv, 1, 4, 6, False, affine=affine)                     # D < 2
        with pytest.raises(DmvsError):
            ops.hypotheses_next(last, dv[:1].contiguous(), 2.0, 8, False, affine=affine)
        with pytest.raises(DmvsError):
            ops.hypotheses_next(last, dv, 2.0, 1, False, affine=affine)
        with pytest.raises(DmvsError):
            ops.hypotheses_next(last, dv, 2.0, 8, False, affine=affine, up=3)
    out, itv = torch.zeros(8 * 8 * 12, device="cuda"), torch.zeros(1, device="cuda")
    code = _lib.load().dmvs_hypotheses_next_up(_p(last), 4, 6, 2, _p(dv), dv.numel(), 2.0, 8, 1, 1, _p(out), _p(itv), _stream())
    assert code == _lib.EINVAL   # base_only with inverse sampling
    with pytest.raises(DmvsError):
        _lib.check(code, "dmvs_hypotheses_next_up")
    torch.cuda.synchronize()
    assert not out.any() and not itv.any()


# ------------------------------------------------------------------------------------------------ affine consumers: exact
def _affine_planes(H, W, D, ratio, lo, width, seed):
    """AffinePlanes [D,H,W] as a stage makes them: the x2 transition of a random (never smooth) coarse map, cut to H rows."""
    from dmvsnet_amd import ops
    g = torch.Generator().manual_seed(seed)
    last = (lo + width * torch.rand(((H + 1) // 2, W // 2), generator=g)).cuda()
    planes, _ = ops.hypotheses_next(last, R.depth_values("synth192").cuda(), ratio, D, False, affine=True)
    return planes.rows(0, H)


@pytest.mark.parametrize("H,W", [(5, 70), (3, 260)])
@pytest.mark.parametrize("D", [4, 5, 8, 16, 32, 48, 64])
def test_k4_on_affine_planes_equals_k4_on_their_volume(D, H, W):
    """``ops.depth_regress``: the ``base ?`` branch of every kernel form (registers D = 4 / 8, split D = 32 / 64, three-sweep otherwise
    and whenever ``prob`` is written) forms base + d * interval with the roundings of ``AffinePlanes.volume`` -- multiply, then
    add, no contraction -- so every output is bit-identical.  W = 70 and 260 give the 64-pixel split form and the 256-pixel forms
    more than one block in x with a ragged last one."""
    from dmvsnet_amd import ops
    planes = _affine_planes(H, W, D, 1.0, 560.0, 160.0, 10 * D + H)
    vol = planes.volume()
    assert tuple(vol.shape) == (D, H, W) and torch.isfinite(vol).all()
    logits = 2.0 * torch.randn((4, D, H, W), generator=torch.Generator().manual_seed(D + W)).cuda()
    for mode, alpha in ((0, 1.0), (1, 5.0)):
        for want_prob in (False, True):
            ra = ops.depth_regress(logits, planes, planes.step, alpha, mode, want_prob)
            rv = ops.depth_regress(logits, vol, planes.step, alpha, mode, want_prob)
            for k, (a, v) in enumerate(zip(ra, rv)):
                if k == 3 and not want_prob:
                    assert a is None and v is None
                    continue
                assert torch.isfinite(v).all() and torch.equal(a, v), (D, H, W, mode, want_prob, ("dsp", "sel", "conf", "prob")[k])


K1_CONFIGS = [("q4", 0), ("q4", 8), ("q4", 16), ("q4", 2), ("q4", 3), ("hwc", 0)]
K1_IDS = ["q4", "q4_dc4", "q4_dc8", "q4_win53", "q4_win80", "hwc_generic"]


def _k1_inputs(C, H, W, V, half=False):
    from dmvsnet_amd import ops, synth
    g = torch.Generator().manual_seed(31 * C + W)
    hwc = [torch.randn((H, W, C), generator=g).cuda() for _ in range(V)]
    if half:
        hwc = [f.half() for f in hwc]
    cams = synth.synth_cameras(2 * H, 2 * W, V)["stage2"]
    return hwc, ops.relative_proj(cams[0].cuda().contiguous())


@pytest.mark.parametrize("C", [8, 16, 32])
@pytest.mark.parametrize("layout,variant", K1_CONFIGS, ids=K1_IDS)
def test_k1_on_affine_planes_equals_k1_on_their_volume(layout, variant, C):
    """``ops.warp_corr``: ``hyp_plane`` of warp_corr.hip.  D = 3 (D <= 4), 5 and 11 (no multiple of the 4 or 8 planes of a
    workgroup: the ``min(d0 + j, D - 1)`` tail); three views at once, and two single-view launches with ``accumulate``."""
    from dmvsnet_amd import ops
    H, W, V = 19, 70, 3
    hwc, p12 = _k1_inputs(C, H, W, V)
    fs = [ops.hwc_to_q4(f) if layout == "q4" else f for f in hwc]
    for D in (3, 5, 11):
        planes = _affine_planes(H, W, D, 2.0, 600.0, 40.0, D)
        vol = planes.volume()
        s_a = ops.warp_corr(fs[0], fs[1:], p12, planes, variant=variant, layout=layout)
        s_v = ops.warp_corr(fs[0], fs[1:], p12, vol, variant=variant, layout=layout)
        assert tuple(s_v.shape) == (2, D, H, W) and torch.isfinite(s_v).all() and s_v.abs().max() > 0
        assert torch.equal(s_a, s_v), (layout, variant, C, D)
        acc = []
        for depth in (planes, vol):
            out = torch.full((2, D, H, W), float("nan"), device="cuda")
            ops.warp_corr(fs[0], fs[1:2], p12[0:1].contiguous(), depth, out=out, variant=variant, layout=layout)
            ops.warp_corr(fs[0], fs[2:3], p12[1:2].contiguous(), depth, out=out, accumulate=True, variant=variant, layout=layout)
            acc.append(out)
        assert torch.isfinite(acc[1]).all() and torch.equal(acc[0], acc[1]), (layout, variant, C, D, "accumulate")


def test_k1_fp16_features_on_affine_planes_equals_their_volume():
    from dmvsnet_amd import ops
    C, D, H, W = 16, 5, 19, 70
    hwc, p12 = _k1_inputs(C, H, W, 3, half=True)
    fs = [ops.hwc_to_q4(f) for f in hwc]
    planes = _affine_planes(H, W, D, 2.0, 600.0, 40.0, 77)
    s_a = ops.warp_corr(fs[0], fs[1:], p12, planes)
    s_v = ops.warp_corr(fs[0], fs[1:], p12, planes.volume())
    assert torch.isfinite(s_v).all() and s_v.abs().max() > 0 and torch.equal(s_a, s_v)


# ------------------------------------------------------------------------------------------------ layout glue: exact
LAYOUT_SIZES = {1: (1, 1), 255: (15, 17), 256: (16, 16), 257: (1, 257), 513: (27, 19)}   # H * W -> (H, W)


def _arange(*shape):
    n = 1
    for s in shape:
        n *= s
    assert n < 2 ** 24   # exact in fp32
    return torch.arange(n, dtype=F32).reshape(shape)


@pytest.mark.parametrize("HW", list(LAYOUT_SIZES))
@pytest.mark.parametrize("C", [8, 16, 32])
def test_nchw_and_planar_to_hwc(C, HW):
    from dmvsnet_amd import ops
    H, W = LAYOUT_SIZES[HW]
    x = _arange(2 * C, H, W)
    stack = _arange(2 * C, 3, H, W)   # read at view 1: channel stride 3 * H * W
    for c0 in (0, C):
        got = ops.nchw_to_hwc(x.cuda(), c0, C)
        assert torch.equal(got.cpu(), x[c0:c0 + C].permute(1, 2, 0).contiguous()), ("nchw_to_hwc", C, HW, c0)
        got = ops.planar_to_hwc(stack.cuda(), 1, c0, C)
        assert torch.equal(got.cpu(), stack[c0:c0 + C, 1].permute(1, 2, 0).contiguous()), ("planar_to_hwc", C, HW, c0)


@pytest.mark.parametrize("HW", list(LAYOUT_SIZES))
@pytest.mark.parametrize("C", [8, 16, 32])
def test_nchw_to_q4(C, HW):
    from dmvsnet_amd import ops
    H, W = LAYOUT_SIZES[HW]

    def want(t):   # [C,H,W] -> [C/4,H,W,4]
        return t.reshape(C // 4, 4, H, W).permute(0, 2, 3, 1).contiguous()

    x = _arange(C, H, W)
    assert torch.equal(ops.nchw_to_q4(x.cuda()).cpu(), want(x)), ("contiguous", C, HW)
    parent = _arange(1, 2 * C, H, W).cuda()
    half = parent.split(C, 1)[1][0]   # second half of a [1,2C,H,W] map: a view into the parent
    assert half.data_ptr() != parent.data_ptr()
    assert torch.equal(ops.nchw_to_q4(half).cpu(), want(parent.cpu()[0, C:])), ("split half", C, HW)
    stack = _arange(2 * C, 3, H, W).cuda()
    view = stack.split(C, 0)[1][:, 1]   # ... and of a [2C,3,H,W] stack at view 1: channel stride 3 * H * W from the parent
    assert view.stride(0) == 3 * H * W
    assert torch.equal(ops.nchw_to_q4(view).cpu(), want(stack.cpu()[C:, 1])), ("strided half", C, HW)
    out = torch.full((C // 4, H, W, 4), float("nan"), device="cuda")
    assert ops.nchw_to_q4(view, out=out) is out and torch.equal(out.cpu(), want(stack.cpu()[C:, 1])), ("out=", C, HW)


def test_layout_kernels_refuse_other_channel_counts():
    from dmvsnet_amd import ops
    from dmvsnet_amd._lib import DmvsError
    with pytest.raises(DmvsError):
        ops.nchw_to_hwc(_arange(24, 3, 5).cuda(), 0, 12)
    with pytest.raises(DmvsError):
        ops.planar_to_hwc(_arange(24, 3, 3, 5).cuda(), 1, 0, 12)
    with pytest.raises(DmvsError):
        ops.nchw_to_q4(_arange(12, 3, 5).cuda())
