"""CPU: the differentiable dual-depth head (K4b, N6b; dmvsnet_amd/head.py) -- the float64 restatement against the reference's
recorded gradients, its closed-form backward against autograd / gradcheck of its own forward, and the errors that need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import head_grad_ref as R

EPS32 = 2.0 ** -23


@pytest.fixture(scope="module")
def g(golden):
    return golden("op_head_grad.npz")


def test_fixture_is_no_larger_than_the_costagg_one():
    import os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert os.path.getsize(os.path.join(here, "op_head_grad.npz")) <= os.path.getsize(os.path.join(here, "op_costagg_grad.npz"))


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_golden_inputs_are_the_seeded_ones_and_satisfy_the_conditions(g, name):
    case = R.golden_case(g, name)
    fresh = R.make_case(**R.GOLDEN_CASES[name])
    for k in ("logits", "hyp", "rlogits", "gt", "mask"):
        assert torch.equal(case[k], fresh[k]), k
    assert case["weight"] == fresh["weight"] and case["interval"] == pytest.approx(fresh["interval"])
    assert R.condition_violations(case) == []


def test_cases_cover_what_the_issue_lists():
    kws = list(R.GOLDEN_CASES.values())
    assert {k["D"] for k in kws} == {8, 32, 48, 64}
    assert any(k["H"] % 2 and k["W"] % 2 for k in kws) and any(k["H"] % 4 and k["W"] % 4 for k in kws)
    assert any(k["holes"] for k in kws) and any(k["weight"] != 1.0 for k in kws) and any(k["B"] == 2 for k in kws)
    assert all(k["H"] >= 4 for k in kws)   # every row class y % 4 of the checkerboard


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_restatement_against_the_reference(g, name):
    """Outputs: fp32 sums of D terms of magnitude |hyp| against float64, D * eps32 relative; the checkerboard stack of the rows
    y % 4 >= 2 reaches 8 hi - 7 lo (3 hi' - 2 lo' of hi' = 2 hi - lo, lo' = 2 lo - hi), 15 x the error of its operands, and the
    refine pass's outputs are expectations over those hypotheses: 16 x for everything behind depth_sub_plus.  Gradients: in the quadratic branch
    of the smooth-L1 (slope 1 per mm) the gradient IS est - gt, so the reference's fp32 rounding of a D-term expectation
    (<= D * eps32 / 2 * max|hyp| mm) appears in it undamped, relative to a largest gradient element of the same scale; the
    checkerboard stack (3 lo - 2 hi) and the refine softmax (alpha 5) amplify by a small factor: 8 x."""
    case = R.golden_case(g, name)
    D = case["logits"].shape[2]
    f64 = R.chain_f64(case)
    for k in ("depth_sub_plus", "depth_values_c", "depth_sub_plus_refine", "depth"):
        amp = 1 if k == "depth_sub_plus" else 16
        assert R.rel_dist(torch.from_numpy(g[f"{name}.{k}"]), f64[k]) <= amp * D * EPS32, k
    assert abs(float(g[f"{name}.loss"]) - f64["loss"].item()) <= 1e-4 * f64["loss"].item()
    bound = 8 * D * EPS32 / 2 * case["hyp"].abs().max().item()
    for k in ("g_logits", "g_rlogits", "g_c"):
        e_ref = R.rel_dist(torch.from_numpy(g[f"{name}.{k}"]), f64[k])
        print(f"RESTATEMENT {name} {k}: e_ref {e_ref:.3e} (bound {bound:.3e})")
        assert e_ref <= bound, (k, e_ref, bound)
    # the edge through depth_values_c is in the reference's gradient: without it the restatement is far off
    assert R.rel_dist(torch.from_numpy(g[f"{name}.g_logits"]), R.chain_f64(case, edge=False)["g_logits"]) > 0.05


@pytest.mark.parametrize("name", ["d8_b2_11x9_w05", "d48_6x9_full"])
def test_closed_form_chain_equals_autograd_of_the_forward(g, name):
    case = R.golden_case(g, name)
    L = case["logits"].double().requires_grad_(True)
    Lr = case["rlogits"].double().requires_grad_(True)
    loss, out = R.head_loss(L, case["hyp"].double(), Lr, case["gt"].double(), case["mask"].double(), case["weight"])
    g_L, g_Lr = torch.autograd.grad(loss, [L, Lr])
    f64 = R.chain_f64(case)
    assert R.rel_dist(f64["g_logits"], g_L) <= 1e-12 and R.rel_dist(f64["g_rlogits"], g_Lr) <= 1e-12
    assert abs(f64["loss"].item() - loss.item()) <= 1e-12 * loss.item()


class _Regress(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, hyp, alpha, mode):
        ctx.save_for_backward(logits, hyp)
        ctx.alpha, ctx.mode = alpha, mode
        return R.regress_forward(logits, hyp, alpha, mode)

    @staticmethod
    def backward(ctx, g_dsp, g_sel):
        logits, hyp = ctx.saved_tensors
        return (*R.regress_backward(logits, hyp, ctx.alpha, ctx.mode, g_dsp, g_sel), None, None)


class _LossSet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dsp, gt, mask, weight):
        ctx.save_for_backward(dsp, gt, mask)
        ctx.weight = weight
        return R.loss_set(dsp, gt, mask, weight)

    @staticmethod
    def backward(ctx, g):
        dsp, gt, mask = ctx.saved_tensors
        return R.loss_set_backward(dsp, gt, mask, ctx.weight) * g, None, None, None


@pytest.mark.parametrize("mode,alpha,D", [(0, 1.0, 5), (1, 5.0, 4)])
def test_gradcheck_of_the_regression_backward(mode, alpha, D):
    case = R.make_case(D=D, H=5, W=3, B=2, seed=3 + mode)
    L = (case["logits"].double() / 3).requires_grad_(True)
    hyp = case["hyp"].double().requires_grad_(True)
    dsp = R.regress_forward(L, hyp, alpha, mode)[0]
    assert ((dsp[:, 0] - dsp[:, 1]).abs() > 1e-3).all() and ((dsp[:, 2] - dsp[:, 3]).abs() > 1e-3).all()   # away from the min / max kink
    # the outputs are depths of ~600 mm (up to 15 x that inside the checkerboard stack): their float64 rounding, ~1e-12, over the
    # central-difference step 2e-6 is an absolute noise of ~1e-6 on a Jacobian with entries of order 1..20
    assert torch.autograd.gradcheck(lambda a, b: _Regress.apply(a, b, alpha, mode), (L, hyp), eps=1e-6, atol=1e-5, rtol=1e-5)


def test_gradcheck_of_the_loss_backward():
    for name in ("d8_9x10_w2", "d48_6x9_full"):   # with holes and full; conditions (a), (b) hold: every kink is >= 1e-3 away
        case = R.make_case(**R.GOLDEN_CASES[name])
        out = R.chain_f64(case)
        gt, mask = case["gt"].double(), case["mask"].double()
        for k in ("depth_sub_plus", "depth_sub_plus_refine"):
            dsp = out[k].clone().requires_grad_(True)
            # a loss of ~100 summed from hundreds of float64 terms carries ~1e-13 of rounding: ~1e-7 over the step 2e-6
            assert torch.autograd.gradcheck(lambda d: _LossSet.apply(d, gt, mask, case["weight"]), (dsp,), eps=1e-6, atol=1e-6, rtol=1e-5)


def test_empty_mask_and_no_cell():
    case = R.make_case(D=4, H=4, W=5, seed=1)
    dsp = R.chain_f64(case)["depth_sub_plus"]
    assert not R.loss_set_backward(dsp, case["gt"].double(), torch.zeros_like(case["mask"]).double(), 1.0).any()
    lone = torch.zeros_like(case["mask"])
    lone[0, 1, 1] = 1.0   # one valid pixel, no valid cell: the cell means are 0 / 0, the pixel's own terms still have a gradient
    g_ = R.loss_set_backward(dsp, case["gt"].double(), lone.double(), 1.0)
    assert torch.isfinite(g_).all() and g_[0, :, 1, 1].abs().min() > 0 and int((g_ != 0).sum()) == 4


# ------------------------------------------------------------------------------------------------ binding, refusals
def test_entry_points_check_their_arguments_without_a_gpu():
    from dmvsnet_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)   # never dereferenced: every call below returns before a launch
    assert lib.dmvs_depth_regress_backward(None, p, 1.0, 0, 8, 4, 4, p, p, None, p, None, None) == _lib.EINVAL
    assert lib.dmvs_depth_regress_backward(p, p, 1.0, 0, 8, 4, 4, p, None, None, p, None, None) == _lib.EINVAL   # no upstream gradient
    assert lib.dmvs_depth_regress_backward(p, p, 1.0, 2, 8, 4, 4, p, p, None, p, None, None) == _lib.EINVAL      # mode
    assert lib.dmvs_depth_regress_backward(p, p, 1.0, 0, 0, 4, 4, p, p, None, p, None, None) == _lib.EINVAL
    assert lib.dmvs_depth_regress_backward(p, p, 1.0, 0, 65, 4, 4, p, p, None, p, None, None) == _lib.EUNSUPPORTED
    assert lib.dmvs_dual_depth_loss_backward(p, p, p, p, 1, 4, 4, 1.0, None, p, p, p, None) == _lib.EINVAL       # counts
    assert lib.dmvs_dual_depth_loss_backward(p, p, p, p, 1, 4, 4, 1.0, p, p, None, None, None) == _lib.EINVAL    # no output
    assert lib.dmvs_dual_depth_loss_backward(p, p, p, p, 1, 1, 4, 1.0, p, p, p, p, None) == _lib.EINVAL          # h < 2
    assert lib.dmvs_version() == 140


def test_refusals_without_a_gpu():
    import dmvsnet_amd
    from dmvsnet_amd import DiffDepthNet, diff_mvs_loss, head
    from dmvsnet_amd._lib import DmvsError
    assert dmvsnet_amd.head is head and "DiffDepthNet" in dmvsnet_amd.__all__ and "diff_mvs_loss" in dmvsnet_amd.__all__
    with pytest.raises(NotImplementedError):
        DiffDepthNet("classification")
    net = DiffDepthNet()
    assert len(list(net.parameters())) == 0
    case = R.make_case(D=8, H=4, W=6, seed=0)
    before = dict(head.launch_counts)
    with pytest.raises(DmvsError):
        net(case["logits"], case["hyp"], 8, case["interval"])
    with pytest.raises(DmvsError):
        net.refine(case["rlogits"], case["hyp"][:, :4], 4, case["interval"])
    with pytest.raises(DmvsError):
        head.depth_regress("logits", case["hyp"], 1.0)
    out = R.chain_f64(case)
    stage = {"depth_sub_plus": out["depth_sub_plus"].float(), "depth_sub_plus_refine": out["depth_sub_plus_refine"].float()}
    with pytest.raises(DmvsError):
        diff_mvs_loss({"stage1": stage}, {"stage1": case["gt"]}, {"stage1": case["mask"]}, "regression")
    for mode in ("classification", "gfocal", "unification"):
        with pytest.raises(NotImplementedError):
            diff_mvs_loss({"stage1": stage}, {"stage1": case["gt"]}, {"stage1": case["mask"]}, mode)
    assert head.launch_counts == before
    # MVSNet.train() keeps raising
    with pytest.raises(NotImplementedError):
        dmvsnet_amd.MVSNet([8], [4], verbose=False).train()


def test_autograd_plumbing_with_stand_in_kernels(monkeypatch):
    """The kernels need a GPU; what is under test here is the graph ``head.py`` builds around them (as test_boundary.py does for
    DepthNet's dict): the four launches are replaced by the float64 restatement rounded to fp32.  Checked: which outputs are
    differentiable, the edge through depth_values_c, frozen inputs and the launch counters, and the gradients (bound: the
    restatement-against-reference bound above, the stand-ins round depth_sub_plus to fp32 just as the reference does)."""
    import contextlib
    from dmvsnet_amd import head, ops, validate

    def depth_regress(lg, hyp, itv, alpha, mode, want_prob):
        dsp, sel = R.regress_forward(lg[None].double(), hyp[None].double(), alpha, mode)
        prob = torch.softmax(lg * alpha, 1) if want_prob else None
        return dsp[0].float(), sel[0].float(), torch.zeros(lg.shape[2:]), prob

    def depth_regress_backward(lg, hyp, alpha, mode, dsp, g_dsp, g_sel, want_hyp, g_logits=None, g_hyp=None):
        up = lambda t: None if t is None else t[None].double()   # noqa: E731
        gl, gh = R.regress_backward(up(lg), up(hyp), alpha, mode, up(g_dsp), up(g_sel), route_dsp=up(dsp))
        g_logits.copy_(gl[0])
        if want_hyp:
            g_hyp.copy_(gh[0])
        return g_logits, (g_hyp if want_hyp else None)

    def launch(main, refine, gt, mask, depth, weight, thres, total, terms, counts, image_sums, metrics4):
        valid, cells = R._valid_cells(mask)
        counts[0], counts[1] = int(valid.sum()), int(cells.sum())
        total += sum(R.loss_set(t.double(), gt.double(), mask.double(), weight) for t in (main, refine)).float()

    def loss_backward(main, refine, gt, mask, weight, counts, g_total, want_main=True, want_refine=True):
        return tuple(R.loss_set_backward(t.double(), gt.double(), mask.double(), weight, g_total.item()).float() if w else None
                     for t, w in ((main, want_main), (refine, want_refine)))

    monkeypatch.setattr(ops, "depth_regress", depth_regress)
    monkeypatch.setattr(ops, "depth_regress_backward", depth_regress_backward)
    monkeypatch.setattr(ops, "dual_depth_loss_backward", loss_backward)
    monkeypatch.setattr(validate, "_launch", launch)
    monkeypatch.setattr(validate, "_plane", lambda t, what, shape=None: t.to(torch.float32).contiguous())
    monkeypatch.setattr(head, "_check", lambda *a: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())

    case = R.make_case(**R.GOLDEN_CASES["d8_b2_11x9_w05"])
    f64 = R.chain_f64(case)
    bound = 8 * 8 * EPS32 / 2 * case["hyp"].abs().max().item()

    def run(main_live, refine_live, edge=True, prob_volume=False):
        net = head.DiffDepthNet(prob_volume=prob_volume)
        L, Lr = case["logits"].clone().requires_grad_(main_live), case["rlogits"].clone().requires_grad_(refine_live)
        before = dict(head.launch_counts)
        main = net(L, case["hyp"], 8, case["interval"])
        hyps = main["depth_values_c"] if edge else main["depth_values_c"].detach()
        refine = net.refine(Lr, hyps, 4, case["interval"])
        loss = head.diff_mvs_loss({"stage1": {**refine, **main}}, {"stage1": case["gt"]}, {"stage1": case["mask"]}, "regression",
                                  dlossw=[case["weight"]])
        if loss.requires_grad:
            loss.backward()
        return main, refine, L.grad, Lr.grad, {k: head.launch_counts[k] - before[k] for k in before}

    for prob_volume in (True, False):
        main, refine, gl, glr, delta = run(True, True, prob_volume=prob_volume)
        assert ("prob_volume" in main) == prob_volume and (not prob_volume or not main["prob_volume"].requires_grad)
        assert not main["photometric_confidence"].requires_grad and not refine["photometric_confidence_refine"].requires_grad
        assert all(t.requires_grad for t in (main["depth_sub_plus"], main["depth_values_c"], refine["depth_sub_plus_refine"], refine["depth"]))
        assert delta == {"regress_bwd": 4, "loss_bwd": 1}   # two passes x B = 2, one stage
        assert R.rel_dist(gl, f64["g_logits"]) <= bound and R.rel_dist(glr, f64["g_rlogits"]) <= bound
    _, _, gl2, glr2, delta = run(True, False)             # frozen refine logits: the refine pass still carries the hypotheses edge
    assert glr2 is None and delta == {"regress_bwd": 4, "loss_bwd": 1} and torch.equal(gl2, gl)
    _, _, gl3, _, delta = run(True, False, edge=False)    # no edge: the refine pass has nothing to differentiate
    assert delta == {"regress_bwd": 2, "loss_bwd": 1}
    assert R.rel_dist(gl3, R.chain_f64(case, edge=False)["g_logits"]) <= bound < R.rel_dist(gl3, f64["g_logits"])
    _, _, gl4, glr4, delta = run(False, True)
    assert gl4 is None and delta == {"regress_bwd": 2, "loss_bwd": 1} and torch.equal(glr4, glr)
    assert run(False, False)[4] == {"regress_bwd": 0, "loss_bwd": 0}
