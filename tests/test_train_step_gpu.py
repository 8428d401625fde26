"""GPU (-m gpu): ``dmvsnet_amd.DiffMVSNet`` and ``train_step`` against ``StockMVSNet`` (tests/train_step_ref.py: the same wiring function
over stock ATen parts on the CPU, certified against the reference in float64 by tests/test_train_step_cpu.py).  Criterion, unless
stated: ``e_hip <= bound_of(e_ref)`` with both distances taken to ``StockMVSNet(float64)``, ``e_ref`` that of ``StockMVSNet(float32)``,
``bound_of`` = ``regnet_grad_ref.bound_of`` (factor 8, floor 16 * 2^-23).  Figures are printed before they are asserted.

T3  train-mode forward: every stage output and every BatchNorm running buffer, ``num_batches_tracked`` exactly, and the value of
    ``diff_mvs_loss`` on the outputs against ``validate_ref.mvs_loss_ref`` on the yardstick's; at 32 x 64, B = 2, (8, 8, 8) and at
    64 x 96, B = 1, (48, 32, 8).
T4  parameter gradients of a linear functional on FORCED decisions: the ReLU masks and min / max routings of the HIP run are replayed
    in both stock runs; per tensor ``e_hip <= 8 * max(e_ref, median of e_ref over the tensor's group)``, no tensor skipped.
T5  the graph's edges, exactly (the assertions of test_train_step_cpu.graph_edges, which also run on the stock model there).
T6  ``deterministic=True``: two steps from one state are the same bits; three ``train_step``s equal three steps on models rebuilt
    from the state dict before each step (a packed-weight cache that survived an in-place update would show); the loss falls by
    half of what the golden script measured on ``StockMVSNet(float32)``.
T7  eval mode under ``no_grad`` against ``dmvsnet_amd.MVSNet`` on the same state dict: depth rel-L1 <= 1e-3.

T3, T4, T6's first assertion and T7 also run on the axes of the reference's training recipe (scripts/train.sh: ``--inverse_depth``,
``--ndepths 48 32 8``, ``--num_view 5``, ``--batch_size 2``): ``b2_32x64_inv`` (inverse-depth sampling), ``b2_64x96_recipe`` (all four
flags; T4 there asserts through the wrappers' arguments that K4b ran in its channel-per-wave form at D = 48 and D = 32 and K1b with four
source views) and ``b2_32x64_unlike`` (every sample its own reference camera and depth range: the one documented deviation from the
reference, dmvsnet_amd/train.py).  T8: in eval mode every sample of the unlike batch is its own single-sample run, bit for bit.

Shapes are the smallest the parts accept (stage-1 volumes 8 x 8 x 16, the refine pass D = 4); ragged and edge shapes are the parts' own
tests' business.  D = 48 / 32 need ``ndepths``, not image size; 64 x 96 at B = 2 keeps the BatchNorm populations of the coarsest level
(D = 48 -> 6) large enough for ``e_ref`` to be roundoff and not the statistics' own noise (at 64 x 64 an fp32 and a float64 stock run
differ by up to 3.7e-2 in a gradient; at 64 x 96 by 1.5e-4, as the first case).
"""
import numpy as np
import pytest
import torch

import train_step_ref as T
import validate_ref as VR
from test_train_step_cpu import graph_edges

pytestmark = pytest.mark.gpu
FIRST, SECOND = "b2_32x64", "b1_64x96"
INV, RECIPE, UNLIKE = "b2_32x64_inv", "b2_64x96_recipe", "b2_32x64_unlike"


def _cuda(inputs):
    imgs, proj, dv = inputs
    return imgs.cuda(), {k: v.cuda() for k, v in proj.items()}, dv.cuda()


def _diff_model(sd, ndepths=T.NDEPTHS, **kw):
    import dmvsnet_amd as da
    net = da.DiffMVSNet(list(ndepths), list(T.RATIOS), **kw)
    net.load_state_dict(sd, strict=True)
    return net.cuda().train()


def _diff_of(name, sd, **kw):
    """``DiffMVSNet`` of a case of the table: its ``ndepths`` and ``inverse``."""
    return _diff_model(sd, T.CASES[name]["ndepths"], inverse_depth=T.CASES[name].get("inverse", False), **kw)


def _sample(kw):
    gt, mask = T.make_ground_truth(**kw)
    imgs, proj, dv = _cuda(T.make_inputs(**kw))
    return {"imgs": imgs, "proj_matrices": proj, "depth_values": dv, "depth": {k: v.cuda() for k, v in gt.items()},
            "mask": {k: v.cuda() for k, v in mask.items()}}


@pytest.fixture(scope="module")
def sd():
    return T.make_state_dict(0)


@pytest.fixture(scope="module")
def stock(sd):
    """Per case and mode, computed once and left unchanged: the unforced forward of StockMVSNet in float64 and fp32 (outputs, buffers
    after the step, the float64 run's decisions), in train mode unless asked."""
    cache = {}

    def get(name, train_mode=True):
        if (name, train_mode) not in cache:
            inputs = T.make_inputs(**T.CASES[name])
            res = {}
            for dtype in (torch.float64, torch.float32):
                net = T.stock_of(name, sd, dtype, train_mode)
                rec = T.ForcedDecisions()
                with torch.no_grad(), rec.record(net):
                    outs = net(*inputs)
                res[dtype] = dict(out=outs, buf=T.bn_buffers(net), decisions=rec)
            cache[(name, train_mode)] = res
        return cache[(name, train_mode)]
    return get


# ------------------------------------------------------------------------------------------------ T3
@pytest.mark.parametrize("name", [FIRST, SECOND, INV, RECIPE, UNLIKE])
def test_forward_against_float64(name, sd, stock):
    import dmvsnet_amd as da
    kw = T.CASES[name]
    ref = stock(name)
    f64, f32 = ref[torch.float64], ref[torch.float32]
    net = _diff_of(name, sd)
    with torch.no_grad():
        outs = net(*_cuda(T.make_inputs(**kw)))
    assert [k for k in outs if "stage" in k] == ["stage1", "stage2", "stage3"] and "prob_volume" not in outs
    assert all(torch.equal(outs[k], outs["stage3"][k]) for k in T.STAGE_OUTPUTS)
    rows = [(f"stage{s + 1}.{k}", outs[f"stage{s + 1}"][k], f32["out"][f"stage{s + 1}"][k], f64["out"][f"stage{s + 1}"][k])
            for s in range(3) for k in T.STAGE_OUTPUTS]
    buf = T.bn_buffers(net)
    assert set(buf) == set(f64["buf"])
    for k, b in buf.items():
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(f64["buf"][k]) == (kw["V"] if k.startswith("feature.") else 1), k
        else:
            rows.append((k, b, f32["buf"][k], f64["buf"][k]))
    gt, mask = T.make_ground_truth(**kw)
    loss = da.diff_mvs_loss(outs, {k: v.cuda() for k, v in gt.items()}, {k: v.cuda() for k, v in mask.items()}, "regression", dlossw=T.DLOSSW)
    as_fp32 = lambda o: {f"stage{s + 1}": {k: o[f"stage{s + 1}"][k].float() for k in ("depth_sub_plus", "depth_sub_plus_refine")} for s in range(3)}
    rows.append(("loss", loss.reshape(1), VR.mvs_loss_ref(as_fp32(f32["out"]), gt, mask, T.DLOSSW).reshape(1),
                 VR.mvs_loss_ref(as_fp32(f64["out"]), gt, mask, T.DLOSSW).double().reshape(1)))
    failed = []
    for key, hip, a32, a64 in rows:
        e_hip, e_ref = T.rel_dist(hip, a64), T.rel_dist(a32, a64)
        if "." not in key or key.startswith("stage") or not e_hip <= T.bound_of(e_ref):
            print(f"TRAINSTEP T3 {name} {key}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {T.bound_of(e_ref):.3e}")
        if not e_hip <= T.bound_of(e_ref):
            failed.append((key, e_hip, e_ref))
    print(f"TRAINSTEP T3 {name}: {len(rows)} tensors compared, {len(failed)} over the bound")
    assert not failed, failed


# ------------------------------------------------------------------------------------------------ T4
def _gradients_on_forced_decisions(name, sd, stock):
    kw = T.CASES[name]
    inputs, weights = T.make_inputs(**kw), T.functional_weights(**kw)
    loss_fn = lambda o: T.linear_functional(o, weights)
    net = _diff_of(name, sd)
    decisions = T.ForcedDecisions()
    _, g_hip, _ = T.run_step(net, _cuda(inputs), loss_fn, record=decisions)
    unforced = stock(name)[torch.float64]["decisions"]
    print(f"TRAINSTEP T4 {name}: {decisions.count()} ReLU decisions; the HIP run and an unforced float64 run differ in "
          f"{decisions.differing(unforced)} of them ({decisions.differing(unforced) / decisions.count():.2e})")
    grads = {}
    for dtype in (torch.float64, torch.float32):
        _, grads[dtype], _ = T.run_step(T.stock_of(name, sd, dtype), inputs, loss_fn, forced=decisions)
    g64, g32 = grads[torch.float64], grads[torch.float32]
    assert set(g_hip) == set(g64) and len(g64) == 403 and all(g is not None for g in g_hip.values())
    e_ref = {k: T.rel_dist(g32[k], g64[k]) for k in g64}
    e_hip = {k: T.rel_dist(g_hip[k], g64[k]) for k in g64}
    floor = {g: float(np.median([e for k, e in e_ref.items() if T.group_of(k) == g])) for g in T.GROUPS}
    failed = []
    for g in T.GROUPS:
        keys = [k for k in g64 if T.group_of(k) == g]
        ratio = {k: e_hip[k] / max(e_ref[k], floor[g]) for k in keys}
        worst = max(ratio, key=ratio.get)
        print(f"TRAINSTEP T4 {name} {g}: {len(keys)} tensors, e_ref median {floor[g]:.2e} max {max(e_ref[k] for k in keys):.2e}; e_hip median "
              f"{np.median([e_hip[k] for k in keys]):.2e} max {max(e_hip[k] for k in keys):.2e}; worst e_hip / max(e_ref, median) = "
              f"{ratio[worst]:.2f} ({worst})")
        failed += [(k, e_hip[k], e_ref[k], floor[g]) for k in keys if not e_hip[k] <= 8 * max(e_ref[k], floor[g])]
    assert sum(len([k for k in g64 if T.group_of(k) == g]) for g in T.GROUPS) == 403   # no tensor skipped
    assert not failed, failed


def test_gradients_on_forced_decisions(sd, stock):
    _gradients_on_forced_decisions(FIRST, sd, stock)


def test_gradients_on_forced_decisions_of_unlike_samples(sd, stock):
    _gradients_on_forced_decisions(UNLIKE, sd, stock)


def test_gradients_on_forced_decisions_at_the_recipe(sd, stock, monkeypatch):
    """T4 at the recipe's planes and views, and the kernel forms it is there for.  Which form of K4b runs is decided inside
    ``dmvs_depth_regress_backward`` from its arguments alone -- channel-per-wave for D in (32, 48, 64) without a hypothesis gradient, one
    thread per pixel otherwise (csrc/depth_regress_bwd.h) -- so the arguments of every call of the step are recorded and asserted; K1b
    likewise by its planes and the source views it is asked for, next to ``costagg.launch_counts``."""
    from dmvsnet_amd import costagg, head, ops
    kw = T.CASES[RECIPE]
    B, V = kw["B"], kw["V"]
    k4b, k1b = [], []
    real_k4b, real_k1b = ops.depth_regress_backward, ops.warp_corr_backward

    def spy_k4b(logits, hyp, alpha, mode, dsp, g_dsp, g_sel, want_hyp, *a, **k):
        k4b.append((int(logits.shape[1]), bool(want_hyp)))
        return real_k4b(logits, hyp, alpha, mode, dsp, g_dsp, g_sel, want_hyp, *a, **k)

    def spy_k1b(ref, srcs, proj12, depth, gsim, gref, gsrc):
        k1b.append((int(depth.shape[0]), gref is not None, sum(g is not None for g in gsrc)))
        return real_k1b(ref, srcs, proj12, depth, gsim, gref, gsrc)

    monkeypatch.setattr(ops, "depth_regress_backward", spy_k4b)
    monkeypatch.setattr(ops, "warp_corr_backward", spy_k1b)
    before = dict(costagg.launch_counts), dict(head.launch_counts)
    _gradients_on_forced_decisions(RECIPE, sd, stock)
    # per sample: the main pass of every stage without a hypothesis gradient (its planes are built under no_grad), the refine pass
    # (D = 4) with one (depth_values_c is live)
    assert sorted(k4b) == sorted([(D, False) for D in kw["ndepths"]] * B + [(4, True)] * (3 * B)), k4b
    assert {(48, False), (32, False)} <= set(k4b)   # the two channel-per-wave launches, B times each
    assert head.launch_counts["regress_bwd"] - before[1]["regress_bwd"] == 6 * B
    assert sorted(k1b) == sorted([(D, True, V - 1) for D in kw["ndepths"] + (4, 4, 4)] * B), k1b
    assert V - 1 == 4 and (48, True, 4) in k1b
    assert costagg.launch_counts["bwd_src_views"] - before[0]["bwd_src_views"] == 6 * B * (V - 1)
    assert costagg.launch_counts["bwd_ref"] - before[0]["bwd_ref"] == 6 * B


# ------------------------------------------------------------------------------------------------ T5
def test_graph_edges(sd):
    import dmvsnet_amd as da
    kw = T.CASES[FIRST]
    sample = _sample(kw)
    net = _diff_model(sd)
    graph_edges(net, (sample["imgs"], sample["proj_matrices"], sample["depth_values"]),
                lambda o: da.diff_mvs_loss(o, sample["depth"], sample["mask"], "regression", dlossw=T.DLOSSW))


# ------------------------------------------------------------------------------------------------ T6
def _deterministic_steps_are_the_same_bits(name, sd):
    import dmvsnet_amd as da
    sample = _sample(T.CASES[name])
    runs = []
    for _ in range(2):
        net = _diff_of(name, sd, deterministic=True)
        outs = net(sample["imgs"], sample["proj_matrices"], sample["depth_values"])
        loss = da.diff_mvs_loss(outs, sample["depth"], sample["mask"], "regression", dlossw=T.DLOSSW)
        loss.backward()
        runs.append((loss.detach(), {n: p.grad for n, p in net.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0]) and bool(torch.isfinite(runs[0][0]))
    assert [n for n in runs[0][1] if not torch.equal(runs[0][1][n], runs[1][1][n])] == []


def test_deterministic_steps_are_the_same_bits(sd):
    _deterministic_steps_are_the_same_bits(FIRST, sd)


def test_deterministic_steps_are_the_same_bits_at_the_recipe(sd):
    _deterministic_steps_are_the_same_bits(RECIPE, sd)


def test_three_steps_equal_three_steps_on_rebuilt_models(sd):
    import dmvsnet_amd as da
    sample = _sample(T.CASES[FIRST])
    keys = ("loss", "abs_depth_error", "thres2mm_error", "thres4mm_error", "thres8mm_error")
    net = _diff_model(sd, deterministic=True)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    kept = [da.train_step(net, opt, sample, T.DLOSSW) for _ in range(3)]
    assert all(tuple(r) == keys and all(v.dim() == 0 and bool(torch.isfinite(v)) for v in r.values()) for r in kept)
    state, opt_state, fresh = sd, None, []
    for _ in range(3):
        other = _diff_model(state, deterministic=True)
        other_opt = torch.optim.Adam(other.parameters(), lr=1e-3)
        if opt_state is not None:
            other_opt.load_state_dict(opt_state)
        fresh.append(da.train_step(other, other_opt, sample, T.DLOSSW))
        state, opt_state = {k: v.detach().clone() for k, v in other.state_dict().items()}, other_opt.state_dict()
    print("TRAINSTEP T6 losses:", [float(r["loss"]) for r in kept], "rebuilt:", [float(r["loss"]) for r in fresh])
    for a, b in zip(kept, fresh):
        assert all(torch.equal(a[k], b[k]) for k in keys)
    final = net.state_dict()
    assert [k for k in final if not torch.equal(final[k], state[k])] == []
    assert any(not torch.equal(final[k].cpu(), sd[k]) for k in final if k.endswith("prob.weight"))   # the steps did move the weights


def test_the_loss_falls(sd, golden):
    import dmvsnet_amd as da
    g = golden("op_train_step.npz")
    lr, steps, stored = float(g["descent.lr"]), int(g["descent.steps"]), g["descent.losses"]
    assert steps <= 10 and stored[-1] <= 0.9 * stored[0]
    sample = _sample(T.CASES[FIRST])
    net = _diff_model(sd)
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    losses = [float(da.train_step(net, opt, sample, T.DLOSSW)["loss"]) for _ in range(steps)]
    with torch.no_grad():
        outs = net(sample["imgs"], sample["proj_matrices"], sample["depth_values"])
        losses.append(float(da.diff_mvs_loss(outs, sample["depth"], sample["mask"], "regression", dlossw=T.DLOSSW)))
    fall, stored_fall = 1 - losses[-1] / losses[0], 1 - stored[-1] / stored[0]
    print(f"TRAINSTEP T6 lr {lr:g}, {steps} Adam steps: {losses[0]:.4f} -> {losses[-1]:.4f} ({fall:+.1%}); StockMVSNet(float32) on the CPU "
          f"{stored[0]:.4f} -> {stored[-1]:.4f} ({stored_fall:+.1%})")
    assert fall >= 0.5 * stored_fall


# ------------------------------------------------------------------------------------------------ T7
def _eval_mode_against_the_inference_model(name, sd):
    import dmvsnet_amd as da
    kw = T.CASES[name]
    inputs = _cuda(T.make_inputs(**kw))
    net = _diff_of(name, sd).eval()
    infer = da.MVSNet(list(kw["ndepths"]), list(T.RATIOS), inverse_depth=kw.get("inverse", False), verbose=False)
    infer.load_state_dict(net.state_dict(), strict=True)
    infer = infer.cuda()
    with torch.no_grad():
        got, want = net(*inputs)["depth"], infer(*inputs)["depth"]
    assert all(int(b) == 0 for k, b in net.state_dict().items() if k.endswith("num_batches_tracked"))   # eval mode updates nothing
    assert got.shape == want.shape == (kw["B"], kw["H"], kw["W"])
    rel = ((got - want).abs().mean() / want.abs().mean()).item()
    print(f"TRAINSTEP T7 {name} eval depth rel-L1 against dmvsnet_amd.MVSNet: {rel:.3e}")
    assert rel <= 1e-3


def test_eval_mode_against_the_inference_model(sd):
    _eval_mode_against_the_inference_model(FIRST, sd)


@pytest.mark.parametrize("name", [RECIPE, UNLIKE])
def test_eval_mode_against_the_inference_model_with_inverse_depth(name, sd):
    _eval_mode_against_the_inference_model(name, sd)   # (the inference model runs a batch as its samples, each on its own depth range)


# ------------------------------------------------------------------------------------------------ T8
def test_eval_mode_on_unlike_samples(sd, stock):
    """Eval mode (BatchNorm on running statistics: the samples are independent) on the unlike batch.  The outputs against
    ``StockMVSNet(float64)`` in eval mode under T3's bound; and every sample of the batch against ITS OWN single-sample run of
    ``DiffMVSNet``, bit for bit: every part launches its kernels per sample and eval-mode K5 is elementwise, so a sample cannot see its
    neighbours -- unless the wiring hands it their cameras or depth range.  Every stage output for sample 0; for the others every output
    but the two confidences, which read sample 0's ``interval`` in the batch (the documented rule) and their own alone."""
    kw = T.CASES[UNLIKE]
    ref = stock(UNLIKE, train_mode=False)
    f64, f32 = ref[torch.float64], ref[torch.float32]
    imgs, proj, dv = _cuda(T.make_inputs(**kw))
    net = _diff_of(UNLIKE, sd).eval()
    with torch.no_grad():
        outs = net(imgs, proj, dv)
        alone = [net(imgs[b:b + 1], {k: v[b:b + 1] for k, v in proj.items()}, dv[b:b + 1]) for b in range(kw["B"])]
    assert all(int(b) == 0 for k, b in net.state_dict().items() if k.endswith("num_batches_tracked"))   # eval mode updates nothing
    failed = []
    for s in range(3):
        key = f"stage{s + 1}"
        for k in T.STAGE_OUTPUTS:
            e_hip, e_ref = T.rel_dist(outs[key][k], f64["out"][key][k]), T.rel_dist(f32["out"][key][k], f64["out"][key][k])
            print(f"TRAINSTEP T8 {UNLIKE} eval {key}.{k}: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {T.bound_of(e_ref):.3e}")
            if not e_hip <= T.bound_of(e_ref):
                failed.append((key, k, e_hip, e_ref))
    assert not failed, failed
    differ = [(b, f"stage{s + 1}", k) for b in range(kw["B"]) for s in range(3) for k in T.STAGE_OUTPUTS
              if (b == 0 or "confidence" not in k) and not torch.equal(outs[f"stage{s + 1}"][k][b], alone[b][f"stage{s + 1}"][k][0])]
    print(f"TRAINSTEP T8 {UNLIKE}: samples of the batch that are not their own single-sample run, bit for bit: {differ}")
    assert differ == []
    # the rule itself: the batch reports sample 0's interval, and sample 1 alone another one
    assert all(float(outs[f"stage{s + 1}"]["interval"]) == float(alone[0][f"stage{s + 1}"]["interval"]) != float(alone[1][f"stage{s + 1}"]["interval"])
               for s in range(3))
