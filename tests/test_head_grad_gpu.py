"""K4b (backward of the dual-depth regression), N6b (backward of the dual-depth loss) and ``DiffDepthNet`` / ``diff_mvs_loss`` on
the MI355X.

Yardsticks, none of which is the code under test: the float64 restatement with its closed-form backward (tests/head_grad_ref.py;
checked against autograd and the reference's recorded gradients in tests/test_head_grad_cpu.py) and the reference's recorded fp32
gradients (tests/golden/op_head_grad.npz).  No test reads the reference or the oracle.

  parity     per golden case and gradient tensor: e_ref = max-abs distance of the reference's fp32 gradient to the float64
             restatement over the tensor's max-abs, e_hip the same for the kernels; e_hip <= 8 e_ref (K1b's criterion: another
             association of the D-term sums).  Where e_ref is below 4 fp32 eps (routing-only gradients) e_hip <= 16 eps.
  shapes     at the config-2 stage-pass shapes the kernels against the float64 restatement on the same fp32 inputs (run in
             float64 on the GPU with stock ATen ops); the bounds are derived from the fp32 formats in each test's docstring.

Every test prints its figures before it asserts (PARITY / ROUTES / EDGE / SHAPE / FD / STAGE lines);
docs/kernels/K4b_depth_regress_backward.md is where the measured ones are kept -- none so far: this file has not run on an
MI355X yet (the document says so).  No test provokes a fault."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import head_grad_ref as R

pytestmark = pytest.mark.gpu

FACTOR = 8.0
EPS32 = 2.0 ** -23


@pytest.fixture(autouse=True)
def free_gpu_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def g(golden):
    return golden("op_head_grad.npz")


def to_cuda(case):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in case.items()}


def run_hip(case, edge=True, refine_alone=False, prob_volume=False):
    """The stage on the product's kernels.  -> (stage dict, loss, g_logits, g_rlogits), or the gradient on depth_values_c."""
    from dmvsnet_amd import DiffDepthNet, diff_mvs_loss
    c = to_cuda(case)
    net = DiffDepthNet("regression", prob_volume=prob_volume)
    L, Lr = c["logits"].clone().requires_grad_(True), c["rlogits"].clone().requires_grad_(True)
    main = net(L, c["hyp"], L.shape[2], c["interval"])
    hyps = main["depth_values_c"]
    if refine_alone:
        hyps = hyps.detach().requires_grad_(True)
    elif not edge:
        hyps = hyps.detach()
    refine = net.refine(Lr, hyps, 4, c["interval"])
    stage = {**refine, **main}
    loss = diff_mvs_loss({"stage1": stage}, {"stage1": c["gt"]}, {"stage1": c["mask"]}, "regression", dlossw=[case["weight"]])
    if refine_alone:
        return torch.autograd.grad(loss, hyps)[0]
    loss.backward()
    return stage, loss.detach(), L.grad, Lr.grad


def bound_of(e_ref):
    return FACTOR * e_ref if e_ref > 4 * EPS32 else 16 * EPS32


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_gradient_parity_golden_cases(g, name):
    case = R.golden_case(g, name)
    assert R.condition_violations(case) == []
    f64 = R.chain_f64(case)
    stage, loss, g_L, g_Lr = run_hip(case)
    g_c = run_hip(case, refine_alone=True)
    assert g_L.is_cuda and g_L.dtype == torch.float32 and g_L.shape == case["logits"].shape and g_Lr.shape == case["rlogits"].shape
    print(f"PARITY {name} loss: hip {loss.item():.7f}  reference {float(g[f'{name}.loss']):.7f}  float64 {f64['loss'].item():.7f}")
    assert abs(loss.item() - f64["loss"].item()) <= 1e-4 * f64["loss"].item()
    rows = []
    for k, got in (("g_logits", g_L), ("g_rlogits", g_Lr), ("g_c", g_c)):
        e_ref, e_hip = R.rel_dist(torch.from_numpy(g[f"{name}.{k}"]), f64[k]), R.rel_dist(got, f64[k])
        rows.append((k, e_hip, e_ref))
        print(f"PARITY {name} {k}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  ratio {e_hip / max(e_ref, 1e-30):.2f}  "
              f"(|grad| max {f64[k].abs().max().item():.3e})")
    for k, e_hip, e_ref in rows:
        assert e_hip <= bound_of(e_ref), (name, k, e_hip, e_ref)
    # masked pixels: exactly zero in every gradient of the refine pass (its only upstream is the loss)
    dead = ~(case["mask"] > 0.5)
    assert not g_Lr.cpu()[dead[:, None, None].expand_as(g_Lr)].any() and not g_c.cpu()[dead[:, None].expand_as(g_c)].any()


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_backward_routes_equal_the_forward_selection(g, name):
    """The channel that receives the gradient of a min / max is the channel whose expectation the forward wrote into the selection:
    mode 1 sends d depth to one channel per pixel; mode 0 is probed with a one-hot gradient on the stack entry that IS lo (then hi)
    in the rows y % 4 < 2.  (pixel, channel) sets compared exactly."""
    from dmvsnet_amd import ops
    case = to_cuda(R.golden_case(g, name))
    itv = torch.tensor([case["interval"]], device="cuda")
    total = 0
    for b in range(case["logits"].shape[0]):
        # mode 1 on the refine pass
        lg, hyp = case["rlogits"][b].contiguous(), case["hyp"][b, :4].contiguous()
        dsp, depth, _, _ = ops.depth_regress(lg, hyp, itv, 5.0, 1, False)
        gl, _ = ops.depth_regress_backward(lg, hyp, 5.0, 1, dsp, None, torch.ones_like(depth), False)
        took = (gl != 0).any(1)
        want = dsp == depth[None]
        assert int(want.sum()) == depth.numel() and torch.equal(took, want)
        total += int(want.sum())
        # mode 0 on the main pass
        lg, hyp = case["logits"][b].contiguous(), case["hyp"][b].contiguous()
        dsp, sel, _, _ = ops.depth_regress(lg, hyp, itv, 1.0, 0, False)
        H, W = dsp.shape[1:]
        yy, xx = R._yx(H, W, "cuda")
        rows = (yy % 4) < 2
        for t in (2, 3):   # stack entry 2 is lo, entry 3 is hi; plane k shows entry k + off
            k = t - ((yy + xx) % 2) * 2
            g_sel = torch.zeros_like(sel)
            for kk in range(4):
                g_sel[kk][(k == kk) & rows] = 1.0
            gl, _ = ops.depth_regress_backward(lg, hyp, 1.0, 0, dsp, None, g_sel, False)
            took = (gl != 0).any(1)
            shown = torch.stack([torch.where(k == kk, sel[kk], torch.zeros_like(sel[kk])) for kk in range(4)]).sum(0)
            pair = ((yy % 4) % 2)[None] == torch.tensor([0, 0, 1, 1], device="cuda")[:, None, None]
            want = (dsp == shown[None]) & rows[None] & pair
            assert int(want.sum()) == int(rows.sum()) and torch.equal(took, want)
            total += int(want.sum())
    print(f"ROUTES {name}: {total} (pixel, channel) routes, all equal to the forward's selection")


@pytest.mark.parametrize("name", ["d8_b2_11x9_w05", "d64_5x6_w05"])
def test_the_hypotheses_edge(g, name):
    case = R.golden_case(g, name)
    f64 = R.chain_f64(case)
    golden = torch.from_numpy(g[f"{name}.g_logits"])
    with_edge, without = run_hip(case)[2], run_hip(case, edge=False)[2]
    e_ref = R.rel_dist(golden, f64["g_logits"])
    e_with, e_without = R.rel_dist(with_edge, f64["g_logits"]), R.rel_dist(without, f64["g_logits"])
    e_no64 = R.rel_dist(without, R.chain_f64(case, edge=False)["g_logits"])
    print(f"EDGE {name}: with the edge {e_with:.3e} (e_ref {e_ref:.3e}); without it {e_without:.3e} from the golden's chain, "
          f"{e_no64:.3e} from the float64 chain without the edge")
    assert not torch.equal(with_edge, without)
    assert e_with <= bound_of(e_ref) < e_without


# ------------------------------------------------------------------------------------------------ forward identity
def test_forward_is_the_eval_kernel_bit_for_bit(g):
    from dmvsnet_amd import DiffDepthNet, ops
    for name in ("d8_b2_11x9_w05", "d48_6x9_full", "d64_5x6_w05"):
        case = to_cuda(R.golden_case(g, name))
        itv = torch.tensor([case["interval"]], device="cuda")
        for prob_volume in (True, False):
            net = DiffDepthNet(prob_volume=prob_volume)
            main = net(case["logits"].requires_grad_(True), case["hyp"], case["logits"].shape[2], case["interval"])
            refine = net.refine(case["rlogits"].requires_grad_(True), main["depth_values_c"], 4, case["interval"])
            assert ("prob_volume" in main) == prob_volume
            assert set(main) - {"prob_volume"} == {"photometric_confidence", "depth_sub_plus", "depth_values_c", "depth_values", "interval"}
            assert set(refine) == {"depth", "photometric_confidence_refine", "depth_sub_plus_refine"}
            for k in ("depth_sub_plus", "depth_values_c"):
                assert main[k].requires_grad
            for k in ("depth", "depth_sub_plus_refine"):
                assert refine[k].requires_grad
            assert not main["photometric_confidence"].requires_grad and not refine["photometric_confidence_refine"].requires_grad
            assert not prob_volume or not main["prob_volume"].requires_grad
            for b in range(case["logits"].shape[0]):
                dsp, sel, conf, prob = ops.depth_regress(case["logits"][b].detach().contiguous(), case["hyp"][b].contiguous(), itv, 1.0, 0,
                                                         prob_volume)
                assert torch.equal(main["depth_sub_plus"][b], dsp) and torch.equal(main["depth_values_c"][b], sel)
                assert torch.equal(main["photometric_confidence"][b], conf)
                assert not prob_volume or torch.equal(main["prob_volume"][b], prob)
                dsp_r, depth, conf_r, _ = ops.depth_regress(case["rlogits"][b].detach().contiguous(), sel, itv, 5.0, 1, False)
                assert torch.equal(refine["depth_sub_plus_refine"][b], dsp_r) and torch.equal(refine["depth"][b], depth)
                assert torch.equal(refine["photometric_confidence_refine"][b], conf_r)


def test_loss_is_validate_mvs_loss_bit_for_bit(g):
    from dmvsnet_amd import diff_mvs_loss, validate
    names = ("d8_9x10_w2", "d32_7x9_w2", "d8_b2_11x9_w05")   # three "stages" of different sizes and batch sizes
    inputs, gts, masks = {}, {}, {}
    for s, name in enumerate(names):
        key = f"stage{s + 1}"
        inputs[key] = {"depth_sub_plus": torch.from_numpy(g[f"{name}.depth_sub_plus"]).cuda().requires_grad_(True),
                       "depth_sub_plus_refine": torch.from_numpy(g[f"{name}.depth_sub_plus_refine"]).cuda().requires_grad_(True)}
        gts[key], masks[key] = torch.from_numpy(g[f"{name}.gt"]).cuda(), torch.from_numpy(g[f"{name}.mask"]).cuda()
    for kw in ({}, {"dlossw": [0.5, 1.0, 2.0]}):
        want = validate.mvs_loss(inputs, gts, masks, "regression", **kw)
        got = diff_mvs_loss(inputs, gts, masks, "regression", **kw)
        assert got.requires_grad and got.dim() == 0 and torch.equal(got.detach(), want)
        # ... and its gradient is the sum over the stages of the closed form, stage weights applied
        grads = torch.autograd.grad(got, [inputs[k][n] for k in inputs for n in ("depth_sub_plus", "depth_sub_plus_refine")])
        i = 0
        for s, key in enumerate(inputs):
            w = kw.get("dlossw", [1.0] * 3)[s]
            for n in ("depth_sub_plus", "depth_sub_plus_refine"):
                f64 = R.loss_set_backward(inputs[key][n].detach().double(), gts[key].double(), masks[key].double(), w)
                # N6b against float64 on the same fp32 planes: the bound of test_config2_stage_pass_shapes_against_float64
                assert R.rel_dist(grads[i], f64) <= 8 * EPS32 * gts[key].abs().max().item() + 16 * EPS32, (key, n)
                i += 1


# ------------------------------------------------------------------------------------------------ reproducibility, NaN, poison
def test_two_backward_runs_are_bit_equal():
    case = R.make_case(D=32, H=61, W=83, B=2, seed=41)
    a, b = run_hip(case), run_hip(case)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    case = R.make_case(D=8, H=70, W=131, seed=42)
    a, b = run_hip(case), run_hip(case)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_nan_under_the_mask_does_not_leak():
    from dmvsnet_amd import diff_mvs_loss
    case = R.make_case(D=8, H=37, W=70, B=2, seed=43)
    out = R.chain_f64(case)
    gt, mask = case["gt"].clone(), case["mask"]
    main, refine = out["depth_sub_plus"].float(), out["depth_sub_plus_refine"].float()

    def grads(main, refine, gt):
        leaves = [main.cuda().requires_grad_(True), refine.cuda().requires_grad_(True)]
        loss = diff_mvs_loss({"stage1": {"depth_sub_plus": leaves[0], "depth_sub_plus_refine": leaves[1]}}, {"stage1": gt.cuda()},
                             {"stage1": mask.cuda()}, "regression", dlossw=[0.5])
        loss.backward()
        return loss.detach(), leaves[0].grad, leaves[1].grad

    clean = grads(main, refine, gt)
    dead = ~(mask > 0.5)
    assert dead.any()
    pm, pr, pg = main.clone(), refine.clone(), gt.clone()
    pg[dead] = float("nan")
    pm[dead[:, None].expand_as(pm)] = float("nan")
    pr[:, 0::2][dead[:, None].expand(-1, 2, -1, -1)] = float("inf")
    pr[:, 1::2][dead[:, None].expand(-1, 2, -1, -1)] = float("-inf")
    got = grads(pm, pr, pg)
    assert torch.isfinite(got[0]) and torch.equal(got[0], clean[0])
    for a, b in zip(got[1:], clean[1:]):
        assert torch.isfinite(a).all() and torch.equal(a, b)
        assert not a.cpu()[dead[:, None].expand_as(a)].any()
    # an empty mask: the loss is NaN (as the forward always was), the gradient all zeros
    leaves = [main.cuda().requires_grad_(True), refine.cuda().requires_grad_(True)]
    loss = diff_mvs_loss({"stage1": {"depth_sub_plus": leaves[0], "depth_sub_plus_refine": leaves[1]}}, {"stage1": gt.cuda()},
                         {"stage1": torch.zeros_like(mask).cuda()}, "regression")
    loss.backward()
    assert torch.isnan(loss) and not leaves[0].grad.any() and not leaves[1].grad.any()


@pytest.mark.parametrize("D,mode,want_hyp", [(4, 1, True), (8, 0, False), (8, 0, True), (5, 0, True), (32, 0, False), (48, 0, False),
                                             (64, 0, False), (64, 1, True), (1, 0, True)])
def test_poisoned_outputs_are_fully_overwritten(D, mode, want_hyp):
    from dmvsnet_amd import _lib, ops
    H, W = 19, 131   # ragged against the 64- and 256-pixel tiles
    case = to_cuda(R.make_case(D=D, H=H, W=W, seed=50 + D))
    lg, hyp = case["logits"][0].contiguous(), case["hyp"][0].contiguous()
    itv = torch.tensor([case["interval"]], device="cuda")
    alpha = 5.0 if mode == 1 else 1.0
    dsp, sel, _, _ = ops.depth_regress(lg, hyp, itv, alpha, mode, False)
    gen = torch.Generator(device="cuda").manual_seed(D)
    g_dsp = torch.randn(dsp.shape, device="cuda", generator=gen)
    g_sel = torch.randn(sel.shape, device="cuda", generator=gen)
    g_logits = torch.full_like(lg, float("nan"))
    g_hyp = torch.full_like(hyp, float("nan")) if want_hyp else None
    ops.depth_regress_backward(lg, hyp, alpha, mode, dsp, g_dsp, g_sel, want_hyp, g_logits, g_hyp)
    assert torch.isfinite(g_logits).all() and (g_hyp is None or torch.isfinite(g_hyp).all())
    # ... with the right values
    if D == 1:   # one plane: p = 1, E = hyp exactly, every logit gradient is a zero; g_hyp = sum of G
        assert not g_logits.any()
        return
    _, e_h = check_regress(f"D={D} mode={mode} {H}x{W}", lg, hyp, alpha, mode, dsp, g_dsp, g_sel, g_logits, g_hyp)
    assert (e_h is not None) == want_hyp
    if D == 4 and mode == 1:   # N6b through the raw entry point, into poisoned buffers
        gt, mask = case["gt"].contiguous(), case["mask"].contiguous()
        main = dsp[None].contiguous()
        counts = torch.tensor([int((mask > 0.5).sum()), int(R._valid_cells(mask)[1].sum())], dtype=torch.int64, device="cuda")
        one = torch.ones(1, device="cuda")
        outs = [torch.full_like(main, float("nan")) for _ in range(2)]
        p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
        code = _lib.load().dmvs_dual_depth_loss_backward(p(main), p(main), p(gt), p(mask), 1, H, W, 1.0, p(counts), p(one), p(outs[0]),
                                                         p(outs[1]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert code == 0
        torch.cuda.synchronize()
        assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


def check_regress(tag, lg, hyp, alpha, mode, dsp, g_dsp, g_sel, g_logits, g_hyp):
    """K4b against float64 on the same fp32 inputs ([4,D,H,W] / [D,H,W] / planes of one sample), relative to the largest element.
    g = alpha p (hyp - E) G, and E is an INPUT of the backward: the forward's fp32 depth_sub_plus.  So the comparison has two parts,
    each with its own bound:

      the kernel  against the float64 closed form evaluated with the same E (and the same routing): what differs is the recomputed
                  softmax (an argument alpha l rounded once, expf to 2 ulp, a D-term sum, a division), one subtraction and three
                  products: (2 D + 16) eps32 max(1, alpha);
      the forward's E against the float64 expectation, in units of u = 2^-24 = eps32 / 2: a sequential fp32 sum of D products of
                  magnitude <= max|hyp| (D u for the products, D u for the partial sums), of softmax values that are themselves
                  rounded -- the D-term sum s, the division and expf to 2 ulp: (D + 8) u relative, common to all planes, so it
                  scales E; and the arguments alpha l, rounded once and once more in v - m: 2 u max|alpha l| relative per plane,
                  which moves E by at most that times max|hyp - E|:
                  |E - E64| <= (3 D + 8) u max|hyp| + 2 u max|alpha l| max|hyp - E|.

    (An earlier form of this check folded the second part into the first as D eps32 max|hyp| / max|hyp - E|.  That division was
    wrong: the tensor is normalised by max |p (hyp - E) G|, which is not max(p G) max|hyp - E| -- the element with the largest
    p G dE need not be the one with the largest |hyp - E|.)
    g_hyp does not depend on E: a 4-term sum of products of a softmax value (relative error (D + 4) eps32) with G: (D + 8) eps32.
    -> (e_logits, e_hyp | None)."""
    D = lg.shape[1]
    up = lambda t: None if t is None else t[None].double()   # noqa: E731
    _, E64 = R.softmax_expect(up(lg), up(hyp), alpha)
    u = EPS32 / 2
    span = (hyp[None] - dsp[:, None]).abs().max().item()
    d_E = (up(dsp) - E64).abs().max().item()
    b_E = (3 * D + 8) * u * hyp.abs().max().item() + 2 * u * alpha * lg.abs().max().item() * span
    w_l, w_h = R.regress_backward(up(lg), up(hyp), alpha, mode, up(g_dsp), up(g_sel), route_dsp=up(dsp), expect=up(dsp))
    e_l, b_l = R.rel_dist(g_logits[None], w_l), (2 * D + 16) * EPS32 * max(1.0, alpha)
    e_h = None if g_hyp is None else R.rel_dist(g_hyp[None], w_h)
    print(f"SHAPE K4b {tag}: g_logits {e_l:.3e} (bound {b_l:.3e})  forward's |E - E64| {d_E:.3e} mm (bound {b_E:.3e})"
          + ("" if e_h is None else f"  g_hyp {e_h:.3e} (bound {(D + 8) * EPS32:.3e})"))
    assert e_l <= b_l and d_E <= b_E
    assert e_h is None or e_h <= (D + 8) * EPS32
    return e_l, e_h


# ------------------------------------------------------------------------------------------------ config-2 shapes
@pytest.mark.parametrize("D,RD,h,w", R.CONFIG2_STAGES)
def test_config2_stage_pass_shapes_against_float64(D, RD, h, w):
    """Both passes and the loss at the shapes of a config-2 stage; the float64 restatement runs on the GPU (stock ATen, float64) on
    the kernels' own fp32 inputs -- the forward's dsp decides the routing on both sides, so no near-tie can flip.  Bounds:
    ``check_regress`` for K4b; N6b: every term is a short fp32 expression of exactly representable differences except the cell centres, sums of
    four depths of magnitude <= max|gt| rounded three times (3 eps32 max, and the same for the ground truth) and entering the
    derivative with slope 1 per mm in the quadratic branch: 8 eps32 max|gt| / (1 mm) relative to the per-pixel scale w / n that the
    largest element exceeds, plus 16 eps32 for the products."""
    from dmvsnet_amd import ops
    case = to_cuda(R.make_case(D=D, H=h, W=w, seed=60 + D, refine_D=RD))
    itv = torch.tensor([case["interval"]], device="cuda")
    gt, mask, weight = case["gt"], case["mask"], 2.0
    lg, hyp, rl = case["logits"][0], case["hyp"][0], case["rlogits"][0]
    dsp, hyps, _, _ = ops.depth_regress(lg, hyp, itv, 1.0, 0, False)
    dsp_r, depth, _, _ = ops.depth_regress(rl, hyps, itv, 5.0, 1, False)
    # N6b
    counts = torch.tensor([int((mask > 0.5).sum()), int(R._valid_cells(mask)[1].sum())], dtype=torch.int64, device="cuda")
    one = torch.ones(1, device="cuda")
    g_main, g_ref = ops.dual_depth_loss_backward(dsp[None].contiguous(), dsp_r[None].contiguous(), gt, mask, weight, counts, one)
    bound_l = 8 * EPS32 * gt.abs().max().item() + 16 * EPS32
    for name, got, src in (("main", g_main, dsp), ("refine", g_ref, dsp_r)):
        want = R.loss_set_backward(src[None].double(), gt.double(), mask.double(), weight)
        e = R.rel_dist(got, want)
        print(f"SHAPE N6b {name} {h}x{w}: {e:.3e} (bound {bound_l:.3e})")
        assert e <= bound_l
        assert not got[0][:, ~(mask[0] > 0.5)].any()
    # K4b, refine pass (mode 1, g_hyp wanted), then the main pass with the refine pass's g_hyp as g_sel
    g_rl, g_hyps = ops.depth_regress_backward(rl, hyps, 5.0, 1, dsp_r, g_ref[0], None, True)
    check_regress(f"refine D={RD} {h}x{w}", rl, hyps, 5.0, 1, dsp_r, g_ref[0], None, g_rl, g_hyps)
    g_lg, none = ops.depth_regress_backward(lg, hyp, 1.0, 0, dsp, g_main[0], g_hyps, False)
    assert none is None
    check_regress(f"main D={D} {h}x{w}", lg, hyp, 1.0, 0, dsp, g_main[0], g_hyps, g_lg, None)


def test_directional_finite_difference_at_a_ragged_shape():
    """(L(x + h v) - L(x - h v)) / 2h of the fp32 forward (the kernels' own loss) against <grad, v>, v a random direction in both
    logit volumes.  Bound: the two loss values are fp32 totals of 16 means, each rounded to fp32 once and added in fp32 -- up to
    16 eps32 |L| each side, divided by 2h; plus the truncation / kink error of the central difference itself, measured on the
    float64 restatement with the same x, v, h (|FD64 - <g64, v>|), which no rounding is part of."""
    from dmvsnet_amd import DiffDepthNet, diff_mvs_loss
    D, H, W, h = 8, 61, 83, 2.0 ** -8   # where the two parts of the bound balance on the float64 restatement (kinks against rounding)
    case = R.make_case(D=D, H=H, W=W, seed=71)
    c = to_cuda(case)
    gen = torch.Generator().manual_seed(7)
    v, vr = torch.randn(case["logits"].shape, generator=gen), torch.randn(case["rlogits"].shape, generator=gen)

    def forward32(s):
        net = DiffDepthNet(prob_volume=False)
        with torch.no_grad():
            main = net(c["logits"] + s * v.cuda(), c["hyp"], D, c["interval"])
            refine = net.refine(c["rlogits"] + s * vr.cuda(), main["depth_values_c"], 4, c["interval"])
            return diff_mvs_loss({"stage1": {**refine, **main}}, {"stage1": c["gt"]}, {"stage1": c["mask"]}, "regression",
                                 dlossw=[case["weight"]]).item()

    def forward64(s):
        with torch.no_grad():
            return R.head_loss(case["logits"].double() + s * v.double(), case["hyp"].double(), case["rlogits"].double() + s * vr.double(),
                               case["gt"].double(), case["mask"].double(), case["weight"])[0].item()

    _, loss, g_L, g_Lr = run_hip(case)
    dd = (g_L.double().cpu() * v.double()).sum().item() + (g_Lr.double().cpu() * vr.double()).sum().item()
    fd32 = (forward32(h) - forward32(-h)) / (2 * h)
    f64 = R.chain_f64(case)
    dd64 = (f64["g_logits"] * v.double()).sum().item() + (f64["g_rlogits"] * vr.double()).sum().item()
    trunc = abs((forward64(h) - forward64(-h)) / (2 * h) - dd64)
    bound = 2 * 16 * EPS32 * abs(loss.item()) / (2 * h) + trunc
    print(f"FD {H}x{W} D={D} h={h}: <grad, v> {dd:.6f}  fd32 {fd32:.6f}  |diff| {abs(fd32 - dd):.3e}  bound {bound:.3e} "
          f"(truncation on float64 {trunc:.3e}; float64 <grad, v> {dd64:.6f}; loss {loss.item():.5f})")
    assert abs(fd32 - dd) <= bound


# ------------------------------------------------------------------------------------------------ chained stage
def test_chained_stage_through_autograd():
    """features -> DiffCostAgg -> two-layer Conv3d stand-in -> DiffDepthNet.forward -> DiffCostAgg -> stand-in -> .refine ->
    diff_mvs_loss -> backward(), against the same chain with head and loss replaced by the ATen restatement: in fp32 (the
    "reference" of the parity criterion) and in float64 (the yardstick; the convolutions and the head in float64 on the CPU, the cost
    aggregation is the same fp32 kernel in all three).  Per parameter / feature gradient: e_hip <= 8 e_ref.  The stand-in's last
    layer has no bias: a per-channel constant shifts every logit of a softmax alike, so its gradient is identically zero (sum_d
    g_logits[c, d] = 0) and a relative comparison of two roundings of zero says nothing."""
    import costagg_grad_ref as CR
    from dmvsnet_amd import DiffCostAgg, DiffDepthNet, diff_mvs_loss
    H, W, V, D = 12, 16, 3, 8
    feats, cams, depth, _ = CR.make_case(C=8, V=V, D=D, H=H, W=W, seed=5)
    gen = np.random.Generator(np.random.PCG64(17))
    gt = (620.0 + 25.0 * torch.from_numpy(gen.standard_normal((1, H, W), dtype=np.float32))).cuda()
    mask = torch.from_numpy((gen.random((1, H, W), dtype=np.float32) > 0.15).astype(np.float32)).cuda()
    torch.manual_seed(3)
    nets0 = [torch.nn.Sequential(torch.nn.Conv3d(2, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv3d(8, 4, 3, padding=1, bias=False)) for _ in range(2)]
    agg = DiffCostAgg("variance")
    weight, itv = 0.5, 30.0

    def chain(kind):
        # the float64 yardstick's convolutions, head and loss run on the CPU (float64 convolutions are not a GPU library's business);
        # the copies are differentiable, the cost aggregation stays the same GPU kernel
        dt, dev = (torch.float64, "cpu") if kind == "f64" else (torch.float32, "cuda")
        nets = [torch.nn.Sequential(torch.nn.Conv3d(2, 8, 3, padding=1), torch.nn.ReLU(), torch.nn.Conv3d(8, 4, 3, padding=1, bias=False)).to(dev, dt)
                for _ in range(2)]
        for n, n0 in zip(nets, nets0):
            n.load_state_dict(n0.state_dict())
        leaves = [f.cuda().requires_grad_(True) for f in feats]
        hyp = depth.cuda()
        sim = agg(leaves, cams.cuda(), hyp)
        logits = nets[0](sim.to(dev, dt))
        if kind == "hip":
            head = DiffDepthNet(prob_volume=False)
            main = head(logits, hyp, D, itv)
            sim_c = agg(leaves, cams.cuda(), main["depth_values_c"])
            refine = head.refine(nets[1](sim_c), main["depth_values_c"], 4, itv)
            loss = diff_mvs_loss({"stage1": {**refine, **main}}, {"stage1": gt}, {"stage1": mask}, "regression", dlossw=[weight])
        else:
            dsp, hyps = R.regress_forward(logits, hyp.to(dev, dt), 1.0, 0)
            sim_c = agg(leaves, cams.cuda(), hyps.float().cuda())
            dsp_r, _ = R.regress_forward(nets[1](sim_c.to(dev, dt)), hyps, R.REFINE_ALPHA, 1)
            loss = R.loss_set(dsp, gt.to(dev, dt), mask.to(dev, dt), weight) + R.loss_set(dsp_r, gt.to(dev, dt), mask.to(dev, dt), weight)
        params = [p for n in nets for p in n.parameters()]
        grads = torch.autograd.grad(loss, params + leaves)
        names = [f"net{i}.{k}" for i, n in enumerate(nets) for k, _ in n.named_parameters()] + [f"feature{v}" for v in range(V)]
        return loss.item(), dict(zip(names, [x.detach().double().cpu() for x in grads]))

    l64, g64 = chain("f64")
    l32, g32 = chain("aten")
    lhip, ghip = chain("hip")
    print(f"STAGE loss: float64 {l64:.6f}  aten fp32 {l32:.6f}  hip {lhip:.6f}")
    bad = []
    for k in g64:
        assert g64[k].abs().max() > 0, k
        e_ref, e_hip = R.rel_dist(g32[k], g64[k]), R.rel_dist(ghip[k], g64[k])
        print(f"STAGE {k}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  ratio {e_hip / max(e_ref, 1e-30):.2f}")
        if e_hip > bound_of(e_ref):
            bad.append((k, e_hip, e_ref))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ plumbing, refusals
def test_frozen_inputs_skip_their_kernel():
    from dmvsnet_amd import DiffDepthNet, diff_mvs_loss, head
    c = to_cuda(R.make_case(D=8, H=9, W=10, B=2, seed=81))
    net = DiffDepthNet(prob_volume=False)

    def run(main_live, refine_live, edge=True):
        L, Lr = c["logits"].clone().requires_grad_(main_live), c["rlogits"].clone().requires_grad_(refine_live)
        before = dict(head.launch_counts)
        main = net(L, c["hyp"], 8, c["interval"])
        hyps = main["depth_values_c"] if edge else main["depth_values_c"].detach()
        refine = net.refine(Lr, hyps, 4, c["interval"])
        loss = diff_mvs_loss({"stage1": {**refine, **main}}, {"stage1": c["gt"]}, {"stage1": c["mask"]}, "regression")
        if loss.requires_grad:
            loss.backward()
        return L.grad, Lr.grad, {k: head.launch_counts[k] - before[k] for k in before}

    gl, glr, delta = run(True, True)
    assert gl is not None and glr is not None and delta == {"regress_bwd": 4, "loss_bwd": 1}   # two passes x B = 2
    gl2, glr2, delta = run(True, False)                  # frozen refine logits: the refine kernel still carries the hypotheses edge
    assert glr2 is None and delta == {"regress_bwd": 4, "loss_bwd": 1} and torch.equal(gl2, gl)
    gl3, glr3, delta = run(True, False, edge=False)      # ... and without the edge it is skipped
    assert glr3 is None and delta == {"regress_bwd": 2, "loss_bwd": 1} and not torch.equal(gl3, gl)
    gl4, glr4, delta = run(False, True)                  # frozen main logits: the main kernel is skipped
    assert gl4 is None and delta == {"regress_bwd": 2, "loss_bwd": 1} and torch.equal(glr4, glr)
    gl5, glr5, delta = run(False, False)                 # nothing requires grad: no graph, no kernel
    assert gl5 is None and glr5 is None and delta == {"regress_bwd": 0, "loss_bwd": 0}


def test_refusals_on_the_gpu():
    from dmvsnet_amd import DiffDepthNet, diff_mvs_loss
    from dmvsnet_amd._lib import DmvsError
    c = to_cuda(R.make_case(D=8, H=6, W=9, seed=82))
    net = DiffDepthNet()
    with pytest.raises(DmvsError):
        net(c["logits"].cpu(), c["hyp"], 8, c["interval"])
    with pytest.raises(DmvsError):
        net(c["logits"], c["hyp"].cpu(), 8, c["interval"])
    with pytest.raises(DmvsError):
        net(c["logits"].half(), c["hyp"].half(), 8, c["interval"])
    with pytest.raises(DmvsError):
        net.refine(c["rlogits"].half(), c["hyp"][:, :4], 4, c["interval"])
    with pytest.raises(DmvsError):
        net(c["logits"], c["hyp"][:, :4], 8, c["interval"])        # shapes disagree
    big = torch.zeros(1, 4, 65, 6, 9, device="cuda")
    with pytest.raises(DmvsError):
        net(big, torch.zeros(1, 65, 6, 9, device="cuda"), 65, c["interval"])
    with pytest.raises(NotImplementedError):
        DiffDepthNet("classification")
    main = net(c["logits"].requires_grad_(True), c["hyp"], 8, c["interval"])
    refine = net.refine(c["rlogits"], main["depth_values_c"], 4, c["interval"])
    stage = {**refine, **main}
    with pytest.raises(NotImplementedError):
        diff_mvs_loss({"stage1": stage}, {"stage1": c["gt"]}, {"stage1": c["mask"]}, "classification")
    with pytest.raises(DmvsError):
        diff_mvs_loss({"stage1": {k: v.half() if torch.is_tensor(v) else v for k, v in stage.items()}}, {"stage1": c["gt"]},
                      {"stage1": c["mask"]}, "regression")
    with pytest.raises(DmvsError):
        diff_mvs_loss({"stage1": stage}, {"stage1": c["gt"].cpu()}, {"stage1": c["mask"].cpu()}, "regression")
    loss = diff_mvs_loss({"stage1": stage}, {"stage1": c["gt"]}, {"stage1": c["mask"]}, "regression")
    gl, = torch.autograd.grad(loss, c["logits"], create_graph=True)
    with pytest.raises(RuntimeError):   # once_differentiable: a double backward is refused, not silently wrong
        gl.sum().backward()
