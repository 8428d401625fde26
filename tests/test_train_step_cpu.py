"""CPU (-m "not gpu"): the training model's wiring against the reference, and its refusals.

T1  ``StockMVSNet(float64)`` -- ``dmvsnet_amd.train.wire``, the function ``DiffMVSNet.forward`` runs, over stock ATen parts
    (tests/train_step_ref.py) -- reproduces a float64 run of the reference's own ``MVSNet`` in train mode, stored by
    tests/golden/make_golden_train_step.py in tests/golden/op_train_step.npz: every stage output, every BatchNorm running buffer and
    ``num_batches_tracked`` after the step, every BatchNorm weight / bias gradient, the weight gradients of every ``conv0`` and ``prob``
    and three digests of all 403 parameter gradients, to 1e-9 relative (max-abs over the tensor's max-abs).  Where the bound comes from:
    an fp32 and a float64 run of the reference agree to 2e-6 forward and 1e-4 backward on equal decisions, an amplification of 20 to
    2000 roundings, i.e. about 2e-13 in float64 (measured: 4.8e-13); 1e-9 is four decades above that and seven below what a wrong
    ``detach``, a FeatureNet run on the B * V batch or one flipped ReLU produces.  In float64 against float64 no decision flips.
    The mutation tests show that the comparison sees each of those.
    The same on the axes of the reference's training recipe (scripts/train.sh: ``--inverse_depth``, ``--ndepths 48 32 8``,
    ``--num_view 5``, ``--batch_size 2``), one fixture per case of ``train_step_ref.FIXTURES``: ``b2_32x32_inv`` (inverse-depth sampling)
    and ``b2_32x32_recipe`` (all four flags) in train mode as above; ``b2_32x32_unlike`` -- every sample its own reference camera and
    depth range -- in EVAL mode against the reference run once per sample with B = 1: with such a batch the reference takes sample 0's
    intervals for every sample's planes and ``wire`` does not (dmvsnet_amd/train.py, "One deviation"), so in train mode the two differ
    by 0.28 in a stage-1 output; on running statistics the samples are independent and every sample of the batch must be its own run.
    There the comparison is per sample: the differentiable outputs and the hypothesis volume of every sample, the two confidences of
    sample 0, and those of sample b > 0 against the reference's lines on its own ``depth_sub_plus`` with sample 0's ``interval`` (the
    documented rule); the gradients against the sum of the per-sample runs'.  Five more mutations -- ``inverse`` dropped in either
    hypothesis builder, planes or projections of sample 0 for every sample, the interval of another sample -- are seen by these cases
    and by no other.
T2 every rule of ``DiffMVSNet`` raises a ``DmvsError`` that names it, on CPU tensors included; the state-dict keys are the stock
    model's and ``dmvsnet_amd.MVSNet``'s; T5's graph-edge assertions on the stock model (the GPU test runs the same function on
    ``DiffMVSNet``).
"""
import numpy as np
import pytest
import torch

import costagg_grad_ref as CG
import train_step_ref as T
import dmvsnet_amd as da
from dmvsnet_amd import head, train
from dmvsnet_amd._lib import DmvsError

TOL = 1e-9
CASE = "b2_32x32"


@pytest.fixture(scope="module")
def fixtures(golden):
    cache = {}
    return lambda name: cache[name] if name in cache else cache.setdefault(name, golden(T.FIXTURES[name]))


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(name):
        if name not in cache:
            kw = T.CASES[name]
            cache[name] = dict(name=name, kw=kw, inputs=T.make_inputs(**kw), weights=T.functional_weights(**kw),
                               sd=T.make_state_dict(kw["seed"]))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def fixture(fixtures):
    return fixtures(CASE)


@pytest.fixture(scope="module")
def case(cases):
    return cases(CASE)


def _step(case, mutate=None):
    """One forward + backward of the case's stock float64 model: train mode, the unlike case in eval mode (as its fixture)."""
    net = T.stock_of(case["name"], case["sd"], torch.float64, train_mode=not case["kw"].get("unlike", False))
    if mutate is not None:
        mutate(net)
    outs, grads, _ = T.run_step(net, case["inputs"], lambda o: T.linear_functional(o, case["weights"]))
    return net, outs, grads


def _distances(fixture, net, outs, grads):
    """{stored key: distance to the stored array}, normalised by the stored tensor's max-abs (digests: see below).  A fixture of
    per-sample runs (it stores ``itv.*``) is compared per sample: the key gets the sample's index."""
    dist = {}
    buffers = T.bn_buffers(net)
    per_sample = any(k.startswith("itv.") for k in fixture)
    for key in fixture:
        kind, _, name = key.partition(".")
        want = torch.from_numpy(np.asarray(fixture[key]))
        if kind == "out" and per_sample:
            stage, _, what = name.partition(".")
            for b in range(want.shape[0]):
                w = want[b]
                if "confidence" in what and b > 0:   # the documented rule: sample 0's interval on the sample's own depth_sub_plus
                    dsp = fixture[f"out.{stage}." + ("depth_sub_plus_refine" if what.endswith("refine") else "depth_sub_plus")]
                    w = T.confidence(torch.from_numpy(dsp[b:b + 1]), torch.tensor(fixture[f"itv.{stage}"][0], dtype=torch.float64))[0]
                dist[f"{key}[{b}]"] = T.rel_dist(outs[stage][what][b], w)
        elif kind == "itv":   # what the reference's own run of sample 0 reports, and another number for every other sample
            dist[key] = abs(float(outs[name]["interval"]) - float(want[0])) / float(want[0])
            assert all(float(w) != float(want[0]) for w in want[1:])
        elif kind == "out":
            stage, _, what = name.partition(".")
            dist[key] = T.rel_dist(outs[stage][what], want)
        elif kind == "buf":
            if name.endswith("num_batches_tracked"):
                dist[key] = 0.0 if int(buffers[name]) == int(want) else float("inf")
            else:
                dist[key] = T.rel_dist(buffers[name], want)
        elif kind == "grad":
            dist[key] = T.rel_dist(grads[name], want)
        elif kind == "digest":
            # |sum|, |dot| <= sqrt(n) * norm (the dot's vector is standard normal): the three digests on that one scale
            scale = float(want[1]) * grads[name].numel() ** 0.5
            dist[key] = float(np.abs(T.digests(grads[name], name) - want.numpy()).max()) / scale
    return dist


def test_fixture_holds_what_the_test_needs(fixtures, case):
    params = [n for n, _ in T.stock_model(case["sd"], torch.float64).named_parameters()]
    assert len(params) == 403
    for name in T.FIXTURES:
        fixture, kw = fixtures(name), T.CASES[name]
        assert {k[7:] for k in fixture if k.startswith("digest.")} == set(params), name
        assert all(np.asarray(fixture[k]).dtype == np.float64 for k in fixture if k.startswith(("out.", "grad.", "digest.", "itv."))), name
        assert ("descent.losses" in fixture) == (name == CASE)
        if kw.get("unlike"):   # per-sample runs in eval mode: every stage output of every sample, the intervals, the digests
            assert {k.partition(".")[0] for k in fixture} == {"out", "itv", "digest", "fp32"}
            assert sum(k.startswith("out.") for k in fixture) == 3 * len(T.STAGE_OUTPUTS)
            assert all(fixture[k].shape[0] == kw["B"] for k in fixture if k.startswith(("out.", "itv.")))
            continue
        assert sum(k.startswith("buf.") and k.endswith("num_batches_tracked") for k in fixture) == 8 + 12 * 10, name
        assert sum(k.startswith("grad.") and ".bn." in k for k in fixture) == 2 * (8 + 12 * 10), name
        assert sum(k.startswith("grad.") and k.endswith("prob.weight") for k in fixture) == 12, name
        assert sum(k.startswith("out.") for k in fixture) == 3 * (len(T.STAGE_OUTPUTS) - 1), name


def test_unlike_inputs_are_unlike():
    """What the unlike cases are made of: sample 1 is sample 0's image set no more, its reference camera is camera 1 with its image,
    and its depth range has another start and another step, the ground truth's surface inside both."""
    kw = T.CASES["b2_32x32_unlike"]
    like, unlike = T.make_inputs(**{**kw, "unlike": False}), T.make_inputs(**kw)
    assert all(torch.equal(a[0], b[0]) for a, b in zip(like[:1] + like[2:], unlike[:1] + unlike[2:]))   # sample 0 as it was
    order = T.view_order(1, kw["V"])
    assert order[0] == 1 and sorted(order) == list(range(kw["V"]))
    assert torch.equal(unlike[0][1], like[0][1, order]) and not torch.equal(unlike[0][1], like[0][1])
    for key in like[1]:
        assert torch.equal(unlike[1][key][0], like[1][key][0]) and torch.equal(unlike[1][key][1], like[1][key][1, order])
        assert not torch.equal(unlike[1][key][1, 0, 0], unlike[1][key][0, 0, 0])   # another reference camera
    dv = unlike[2]
    assert float(dv[1, 0]) != float(dv[0, 0]) and abs(float(dv[1, 1] - dv[1, 0]) / float(dv[0, 1] - dv[0, 0]) - 1) > 0.1
    gt, _ = T.make_ground_truth(**kw)
    assert all(float(dv[b, 0]) < float(g[b].min()) and float(g[b].max()) < float(dv[b, -1]) for g in gt.values() for b in range(kw["B"]))


def test_wiring_reproduces_the_reference_in_float64(fixtures, cases):
    bad = {}
    for name in T.FIXTURES:
        fixture, case = fixtures(name), cases(name)
        net, outs, grads = _step(case)
        dist = _distances(fixture, net, outs, grads)
        B = case["kw"]["B"] if case["kw"].get("unlike") else 1   # a fixture of per-sample runs: every output once per sample
        assert len(dist) == sum((B if k.startswith("out.") else 1) for k in fixture if not k.startswith(("fp32.", "descent.")))
        worst = max(dist, key=dist.get)
        print(f"TRAINSTEP T1 {name}: {len(dist)} stored quantities, largest distance {dist[worst]:.2e} ({worst}); the reference's own fp32 "
              f"run: outputs {fixture['fp32.out'].max():.2e}, gradients median {np.median(fixture['fp32.grad']):.2e} max "
              f"{fixture['fp32.grad'].max():.2e}")
        bad.update({(name, k): v for k, v in dist.items() if not v <= TOL})
        tracked = {k: int(v) for k, v in T.bn_buffers(net).items() if k.endswith("num_batches_tracked")}
        if case["kw"].get("unlike"):   # eval mode updates nothing
            assert all(v == 0 for v in tracked.values())
        else:   # FeatureNet ran once per view: V updates of its BatchNorms, one of every other
            assert all(v == (case["kw"]["V"] if k.startswith("feature.") else 1) for k, v in tracked.items())
    assert not bad, bad


def _other_sample(parts, mutation):
    """The mutations that only a batch of unlike samples can see, on the namespace ``wire`` is about to run."""
    first, later, agg = parts.hypotheses_first, parts.hypotheses_next, parts.cost_agg
    if mutation == "planes_of_sample_0":
        parts.hypotheses_first = lambda dv, *a: first(dv[:1].expand_as(dv), *a)
        parts.hypotheses_next = lambda last, dv, *a: later(last, dv[:1].expand_as(dv), *a)
    elif mutation == "projections_of_sample_0":
        parts.cost_agg = lambda feats, proj, hyp: agg(feats, proj[:1].expand_as(proj).contiguous(), hyp)
    elif mutation == "interval_of_last_sample":
        parts.hypotheses_first = lambda dv, *a: (first(dv, *a)[0], first(dv.flip(0), *a)[1])
        parts.hypotheses_next = lambda last, dv, *a: (later(last, dv, *a)[0], later(last.flip(0), dv.flip(0), *a)[1])


MUTATIONS = {"detach_depth_values_c": CASE, "flip_one_relu": CASE, "batched_featurenet": CASE,
             "inverse_dropped_next": "b2_32x32_inv", "inverse_dropped_first": "b2_32x32_inv",
             "planes_of_sample_0": "b2_32x32_unlike", "projections_of_sample_0": "b2_32x32_unlike",
             "interval_of_last_sample": "b2_32x32_unlike"}


@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_the_comparison_sees_a_wrong_graph(fixtures, cases, mutation, monkeypatch):
    """What 1e-9 is seven decades below: each mutation of the wiring moves a stored quantity by far more than the bound.  The last
    five are seen by the inverse-depth and unlike cases only: on the first case (linear sampling, like samples) each of them computes
    the same bits as the unmutated wiring, which the test shows too."""
    fixture, case = fixtures(MUTATIONS[mutation]), cases(MUTATIONS[mutation])
    real_wire = train.wire

    def wire(parts, imgs, *args, **kw):
        if mutation == "inverse_dropped_next":
            real_next = parts.hypotheses_next
            parts.hypotheses_next = lambda last, dv, ratio, D, inverse: real_next(last, dv, ratio, D, False)
        elif mutation == "inverse_dropped_first":
            real_first = parts.hypotheses_first
            parts.hypotheses_first = lambda dv, D, h, w, inverse: real_first(dv, D, h, w, False)
        elif mutation in ("planes_of_sample_0", "projections_of_sample_0", "interval_of_last_sample"):
            _other_sample(parts, mutation)
        elif mutation == "detach_depth_values_c":
            real_head = parts.head
            parts.head = lambda *a: {k: (v.detach() if k == "depth_values_c" else v) for k, v in real_head(*a).items()}
        elif mutation == "batched_featurenet":
            B, V = imgs.shape[:2]
            real_feature, done = parts.feature, {}

            def feature(img):
                if "all" not in done:
                    done["all"], done["v"] = real_feature(imgs.transpose(0, 1).reshape(B * V, *imgs.shape[2:])), 0
                v = done["v"]
                done["v"] += 1
                return {k: t[v * B:(v + 1) * B] for k, t in done["all"].items()}
            parts.feature = feature
        return real_wire(parts, imgs, *args, **kw)

    monkeypatch.setattr(train, "wire", wire)
    mutate = None
    if mutation == "flip_one_relu":
        def mutate(net):   # one decision of 3.5 million: the largest stage-1 conv0 BatchNorm output goes to the other side
            def hook(mod, inp, out):
                flat = out.reshape(-1).clone()
                flat[out.detach().reshape(-1).argmax()] = -1.0
                return flat.view_as(out)
            net.cost_regularization[0].cosR_small.conv0.bn.register_forward_hook(hook)
    net, outs, grads = _step(case, mutate)
    dist = _distances(fixture, net, outs, grads)
    worst = max(dist, key=dist.get)
    print(f"TRAINSTEP T1 mutation {mutation} on {case['name']}: largest distance {dist[worst]:.2e} ({worst}), {dist[worst] / TOL:.1e} "
          f"times the bound; largest over the stage outputs alone {max(v for k, v in dist.items() if k.startswith('out.')):.2e}")
    assert dist[worst] > 1e4 * TOL
    if MUTATIONS[mutation] != CASE:   # ... and the first case cannot see it: the same bits with and without
        first = cases(CASE)
        with torch.no_grad():
            mutated = T.stock_of(CASE, first["sd"], torch.float64)(*first["inputs"])
            monkeypatch.setattr(train, "wire", real_wire)
            plain = T.stock_of(CASE, first["sd"], torch.float64)(*first["inputs"])
        assert all(torch.equal(mutated[f"stage{s + 1}"][k], plain[f"stage{s + 1}"][k]) for s in range(3) for k in T.STAGE_OUTPUTS + ("interval",))


def test_fp32_cost_aggregation_is_the_float64_helper_with_a_dtype():
    feats, cams, depth, _ = CG.make_case(C=8, V=3, D=4, H=8, W=12, seed=3, B=2)
    assert torch.equal(T.cost_agg(feats, cams, depth, torch.float64), CG.cost_agg_f64(feats, cams, depth))


# ------------------------------------------------------------------------------------------------ T5 on the stock model
def graph_edges(model, inputs, loss_of_outputs):
    """T5's assertions on ``model`` (train mode): shared by the CPU test (StockMVSNet) and the GPU test (DiffMVSNet).
    ``loss_of_outputs(outputs)`` -> the training loss."""
    params = dict(model.named_parameters())

    def backward_from(select):
        for p in params.values():
            p.grad = None
        outputs = model(*inputs)
        select(outputs).backward()
        return {n: p.grad for n, p in params.items()}

    def nothing(grads, prefix):
        got = [g for n, g in grads.items() if n.startswith(prefix)]
        return len(got) > 0 and all(g is None or not bool(g.any()) for g in got)

    def something(grads, prefix):
        got = [g for n, g in grads.items() if n.startswith(prefix)]
        return len(got) > 0 and all(g is not None and bool(g.any()) for g in got)

    # (a) the loss reaches every one of the 403 parameters
    grads = backward_from(loss_of_outputs)
    assert len(grads) == 403
    assert [n for n, g in grads.items() if g is None or not bool(g.any())] == []
    for s in range(3):
        key = f"stage{s + 1}"
        # (b) from stage s's refine outputs alone: last_depth is detached, depth_values_c is live
        grads = backward_from(lambda o: o[key]["depth_sub_plus_refine"].sum())
        for other in range(3):
            if other != s:
                assert nothing(grads, f"cost_regularization.{other}.") and nothing(grads, f"cost_regularization_refine.{other}."), (s, other)
        assert something(grads, f"cost_regularization.{s}.") and something(grads, f"cost_regularization_refine.{s}."), s
        # (c) from stage s's main outputs alone: the refine network of the stage gets nothing
        grads = backward_from(lambda o: o[key]["depth_sub_plus"].sum())
        assert nothing(grads, f"cost_regularization_refine.{s}.") and something(grads, f"cost_regularization.{s}."), s
        if s == 0:   # (d) stage 1 reads FeatureNet's coarsest level only
            for name in ("out2", "out3", "inner1", "inner2"):
                assert nothing(grads, f"feature.{name}."), name
            assert something(grads, "feature.out1.") and something(grads, "feature.conv0.")


def test_graph_edges_of_the_stock_model(cases):
    for name in (CASE, "b2_32x32_inv"):   # linear and inverse-depth sampling
        case = cases(name)
        gt, mask = T.make_ground_truth(**case["kw"])
        graph_edges(T.stock_of(name, case["sd"], torch.float64), case["inputs"], lambda o: T.stock_loss(o, gt, mask))


# ------------------------------------------------------------------------------------------------ T2
def test_state_dict_keys():
    diff = da.DiffMVSNet(T.NDEPTHS, T.RATIOS)
    keys = list(diff.state_dict())
    assert keys == list(da.MVSNet(list(T.NDEPTHS), list(T.RATIOS), verbose=False).state_dict())
    stock = T.StockMVSNet()
    assert sorted(keys) == sorted(stock.state_dict()) and len(keys) == 787
    assert {k: tuple(v.shape) for k, v in diff.state_dict().items()} == {k: tuple(v.shape) for k, v in stock.state_dict().items()}
    assert [n for n, _ in diff.named_children()] == ["feature", "cost_aggregation", "cost_regularization", "cost_regularization_refine", "DepthNet"]
    sd = T.make_state_dict(1)
    sd["feature.attn_mask"] = torch.zeros(1)   # model.py:65-70 drops such keys of a checkpoint before the strict load
    diff.load_state_dict(sd, strict=True)
    infer = da.MVSNet(list(T.NDEPTHS), list(T.RATIOS), verbose=False)
    infer.load_state_dict(diff.state_dict(), strict=True)
    back = da.DiffMVSNet(T.NDEPTHS, T.RATIOS)
    back.load_state_dict(infer.state_dict(), strict=True)
    assert all(torch.equal(v, back.state_dict()[k]) for k, v in diff.state_dict().items())
    assert da.train_step is train.train_step and da.DiffMVSNet is train.DiffMVSNet


@pytest.mark.parametrize("kwargs, rule", [
    (dict(ndepths=[8, 8], depth_interval_ratio=[2, 1]), "three stages"),
    (dict(ndepths=[8, 8, 8, 8], depth_interval_ratio=[4, 3, 2, 1]), "three stages"),
    (dict(cr_base_chs=[8, 8, 16]), "cr_base_chs"),
    (dict(ndepths=[48, 12, 8]), "multiple of 8"),
    (dict(ndepths=[head.MAX_D + 8, 32, 8]), "head.MAX_D"),
    (dict(fea_mode="unet"), "fea_mode"),
    (dict(agg_mode="adaptive"), "agg_mode"),
    (dict(depth_mode="classification"), "depth_mode"),
])
def test_constructor_refusals(kwargs, rule):
    kw = dict(ndepths=list(T.NDEPTHS), depth_interval_ratio=list(T.RATIOS))
    kw.update(kwargs)
    with pytest.raises(DmvsError, match=rule):
        da.DiffMVSNet(**kw)


def _cpu_inputs(B=1, V=3, H=32, W=32):
    return T.make_inputs(B, V, H, W)


@pytest.mark.parametrize("change, rule", [
    (lambda i, p, d: (i[..., :24, :], p, d), "multiples of 32"),
    (lambda i, p, d: (i[..., :, :16], p, d), "multiples of 32"),
    (lambda i, p, d: (i[:, :1], {k: v[:, :1] for k, v in p.items()}, d), "views"),
    (lambda i, p, d: (i.repeat(1, 6, 1, 1, 1), {k: v.repeat(1, 6, 1, 1, 1) for k, v in p.items()}, d), "views"),
    (lambda i, p, d: (i[0], p, d), r"\[B,V,3,H,W\]"),
    (lambda i, p, d: (i, {k: v for k, v in p.items() if k != "stage2"}, d), "proj_matrices"),
    (lambda i, p, d: (i, p, d[0]), "depth_values"),
    (lambda i, p, d: (i, p, d), "HIP device"),                       # well-formed, but on the CPU
    (lambda i, p, d: (i.double(), p, d), "fp32"),
])
def test_forward_refusals_on_cpu_tensors(change, rule):
    net = da.DiffMVSNet(T.NDEPTHS, T.RATIOS)
    with pytest.raises(DmvsError, match=rule):
        net(*change(*_cpu_inputs()))


def test_inference_model_still_refuses_train_mode():
    with pytest.raises(NotImplementedError):
        da.MVSNet(list(T.NDEPTHS), list(T.RATIOS), verbose=False).train()
