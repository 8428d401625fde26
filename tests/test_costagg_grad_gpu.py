"""K1b (backward of the fused warp + correlation) and ``cost_agg`` / ``DiffCostAgg`` on the MI355X.

Yardsticks, none of which is the code under test: the float64 restatement (tests/costagg_grad_ref.py), the fp32 oracle under
autograd (equal to the reference's gradients, tests/test_costagg_grad_cpu.py) and the reference's recorded gradients
(tests/golden/op_costagg_grad.npz).  Every bound is a multiple of the ORACLE's own distance to the float64 restatement,
measured in the same process:

  parity          e_hip <= 8 * e_oracle per gradient tensor -- the factor covers another summation order (the atomics' arrival
                  order included), fmaf against separate multiply / add, and the product's projection (fp64 inverse rounded
                  once, against the reference's fp32 LU);
  adjoint         <G, sim(dref, src)> == <dRef, dref> and <G, sim(ref, dsrc)> == <dSrc, dsrc> with the GENERIC forward kernel
                  (same coordinate routine as the backward), defect relative to sum |G * sim|, bound 8 x the oracle's defect
                  of the same identity at a small size (the largest of 8 draws: one draw of a zero-mean rounding sum can come
                  out arbitrarily close to zero and is no scale);
  stage pass      FeatureNet parameter gradients through cost_agg against the same chain through the oracle, bound 4 x the
                  distance between the oracle chain on the CPU and on the GPU with stock ATen kernels.

Every test prints its figures before it asserts (PARITY / ADJOINT / REPRO / STAGE lines); docs/kernels/K1b_warp_corr_backward.md
is where the measured ones are kept.
No test provokes a fault: taps outside the image and samples behind a camera are legal inputs."""
import gc

import numpy as np
import pytest
import torch

import costagg_grad_ref as R
from oracle import dmvs_oracle as O

pytestmark = pytest.mark.gpu

FACTOR = 8.0   # K1b per case table, guarded, with one-hot probes and 16 views: tests/test_warp_corr_grad_gpu.py


@pytest.fixture(autouse=True)
def free_gpu_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def cuda_case(feats, cams, depth, gsim):
    return [f.cuda() for f in feats], cams.cuda(), depth.cuda(), gsim.cuda()


def dist(a, b):
    return (a.detach().double().cpu() - b.detach().double().cpu()).abs().max().item()


def parity(name, feats, cams, depth, gsim, reference_grads=None):
    """e_hip and e_oracle per gradient tensor, both against the float64 restatement (CPU); asserts e_hip <= 8 e_oracle."""
    from dmvsnet_amd import cost_agg
    _, g64 = R.grads_f64(feats, cams, depth, gsim)
    _, g_or = R.grads_of(O.warp_corr, feats, cams, depth, gsim)
    if reference_grads is not None:   # the oracle IS the reference here too (other CPU: a few ulp)
        for a, b in zip(g_or, reference_grads):
            assert dist(a, torch.from_numpy(b)) <= 1e-6 * max(1.0, float(np.abs(b).max()))
    sim_hip, g_hip = R.grads_of(cost_agg, *cuda_case(feats, cams, depth, gsim))
    assert sim_hip.is_cuda and all(g.is_cuda and g.dtype == torch.float32 and g.shape == f.shape for g, f in zip(g_hip, feats))
    rows = []
    for v in range(len(feats)):
        e_or, e_hip = dist(g_or[v], g64[v]), dist(g_hip[v], g64[v])
        rows.append((v, e_hip, e_or))
        print(f"PARITY {name} grad{v}: e_hip {e_hip:.3e}  e_oracle {e_or:.3e}  ratio {e_hip / e_or:.2f}  "
              f"(|grad| max {g64[v].abs().max().item():.2f})")
    for v, e_hip, e_or in rows:
        assert e_hip <= FACTOR * e_or, (name, v, e_hip, e_or)


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_gradient_parity_golden_cases(golden, name):
    g = golden("op_costagg_grad.npz")
    V = R.GOLDEN_CASES[name]["V"]
    feats = [torch.from_numpy(g[f"{name}.feat{v}"]) for v in range(V)]
    case = (feats, torch.from_numpy(g[f"{name}.proj"]), torch.from_numpy(g[f"{name}.depth"]), torch.from_numpy(g[f"{name}.gsim"]))
    parity(name, *case, reference_grads=[g[f"{name}.grad{v}"] for v in range(V)])


@pytest.mark.parametrize("name", list(R.LARGE_CASES))
def test_gradient_parity_larger_cases(name):
    parity(name, *R.make_case(**R.LARGE_CASES[name]))


# ------------------------------------------------------------------------------------------------ forward, layout, masks
@pytest.mark.parametrize("name", ["c8_v3_d4", "c16_v7_d4", "c32_v3_d4", "c16_v3_d8_b2_61x83"])
def test_forward_is_the_product_kernel_bit_for_bit(name):
    from dmvsnet_amd import cost_agg, ops
    kw = R.GOLDEN_CASES.get(name) or R.LARGE_CASES[name]
    feats, cams, depth, _ = cuda_case(*R.make_case(**kw))
    sim = cost_agg(feats, cams, depth)
    assert tuple(sim.shape) == (depth.shape[0], 2) + tuple(depth.shape[1:])
    for b in range(depth.shape[0]):
        q4 = [ops.hwc_to_q4(f[b].permute(1, 2, 0).contiguous()) for f in feats]
        want = ops.warp_corr(q4[0], q4[1:], ops.relative_proj(cams[b].contiguous()), depth[b].contiguous(), layout="q4")
        assert torch.equal(sim[b], want)


def test_nchw_to_q4_equals_the_permute():
    from dmvsnet_amd import ops
    g = torch.Generator().manual_seed(5)
    for C, H, W in ((8, 5, 7), (16, 33, 65), (32, 16, 20)):
        x = torch.randn(2, 2 * C, H, W, generator=g).cuda()

        def want(t):
            return t.permute(1, 2, 0).reshape(H, W, C // 4, 4).permute(2, 0, 1, 3).contiguous()
        for half in x.split(C, 1):                 # the reference's stageK / stageK_c halves: channel-slice views
            for b in range(2):                     # a batch sample is a pointer offset
                assert not half.is_contiguous()
                assert torch.equal(ops.nchw_to_q4(half[b]), want(half[b]))
        strided = x[1, ::2]                        # a channel stride of two planes
        assert torch.equal(ops.nchw_to_q4(strided), want(strided))
        flipped = x[0, :C].transpose(1, 2).contiguous().transpose(1, 2)   # rows not contiguous: copied first
        assert torch.equal(ops.nchw_to_q4(flipped), want(flipped))


def test_needs_input_grad_masks_and_no_gradient_to_cameras_or_hypotheses():
    import dmvsnet_amd.costagg as ca
    feats, cams, depth, gsim = cuda_case(*R.make_case(**R.GOLDEN_CASES["c8_v7_d8"]))
    V = len(feats)
    full = R.grads_of(ca.cost_agg, feats, cams, depth, gsim)[1]

    def run(mask, depth_grad=False):
        leaves = [f.clone().requires_grad_(m) for f, m in zip(feats, mask)]
        d = depth.clone().requires_grad_(depth_grad)
        p = cams.clone().requires_grad_(depth_grad)
        before = dict(ca.launch_counts)
        sim = ca.cost_agg(leaves, p, d)
        sim.backward(gsim)
        delta = {k: ca.launch_counts[k] - before[k] for k in before}
        return leaves, d, p, delta

    # frozen reference: its kernel is skipped, the source gradients are unchanged (to the atomics' rounding)
    leaves, _, _, delta = run([False] + [True] * (V - 1))
    assert leaves[0].grad is None and delta == {"bwd_ref": 0, "bwd_src_views": V - 1}
    assert all(l.grad is not None for l in leaves[1:])
    # only the reference: the scatter kernel is skipped, and dRef is the same bits
    leaves, _, _, delta = run([True] + [False] * (V - 1))
    assert delta == {"bwd_ref": 1, "bwd_src_views": 0} and all(l.grad is None for l in leaves[1:])
    assert torch.equal(leaves[0].grad, full[0])
    # two frozen source views among six
    mask = [True, True, False, True, False, True, True]
    leaves, _, _, delta = run(mask)
    assert delta == {"bwd_ref": 1, "bwd_src_views": 4}
    for l, m, f in zip(leaves, mask, full):
        assert (l.grad is not None) == m
        if m:
            assert dist(l.grad, f) <= 1e-5 * f.abs().max().item()   # the same sums in another arrival order
    # cameras and hypotheses: no gradient, even when they ask for one (the reference's grid is built under no_grad)
    leaves, d, p, delta = run([True] * V, depth_grad=True)
    assert d.grad is None and p.grad is None and all(l.grad is not None for l in leaves)
    # nothing requires grad: no graph, no kernel
    before = dict(ca.launch_counts)
    sim = ca.cost_agg(feats, cams, depth)
    assert not sim.requires_grad and ca.launch_counts == before


def test_refusals_on_the_gpu():
    from dmvsnet_amd import cost_agg
    from dmvsnet_amd._lib import DmvsError
    feats, cams, depth, _ = cuda_case(*R.make_case(**R.GOLDEN_CASES["c8_v3_d4"]))
    with pytest.raises(DmvsError):
        cost_agg([f.half() for f in feats], cams, depth)
    with pytest.raises(DmvsError):
        cost_agg([f[:, :4] for f in feats], cams, depth)          # C = 4 is not built
    with pytest.raises(DmvsError):
        cost_agg(feats, cams.cpu(), depth)
    with torch.autocast("cuda", dtype=torch.float16):
        with pytest.raises(DmvsError):
            cost_agg([torch.nn.functional.conv2d(f, torch.ones(8, 8, 1, 1, device="cuda")) for f in feats], cams, depth)
    sim = cost_agg([f.requires_grad_(True) for f in feats], cams, depth)
    g, = torch.autograd.grad(sim.sum(), feats[0], create_graph=True)
    with pytest.raises(RuntimeError):   # once_differentiable: a double backward is refused, not silently wrong
        g.sum().backward()


# ------------------------------------------------------------------------------------------------ adjoint identity
def _adjoint_defects_oracle(seed):
    """Both identities on the fp32 oracle (CPU) at a small size; defect relative to sum |G * sim|."""
    feats, cams, depth, gsim = R.make_case(C=8, V=3, D=4, H=8, W=12, seed=seed)
    delta = R.make_case(C=8, V=3, D=4, H=8, W=12, seed=seed + 1000)[0]
    _, grads = R.grads_of(O.warp_corr, feats, cams, depth, gsim)
    out = []
    sim = O.warp_corr([delta[0]] + feats[1:], cams, depth).double()
    lhs, scale = (gsim.double() * sim).sum().item(), (gsim.double() * sim).abs().sum().item()
    out.append(abs(lhs - (grads[0].double() * delta[0].double()).sum().item()) / scale)
    sim = O.warp_corr([feats[0]] + delta[1:], cams, depth).double()
    lhs, scale = (gsim.double() * sim).sum().item(), (gsim.double() * sim).abs().sum().item()
    out.append(abs(lhs - sum((g.double() * d.double()).sum().item() for g, d in zip(grads[1:], delta[1:]))) / scale)
    return out


@pytest.mark.parametrize("stage,C,D,H,W", [("s1", 32, 48, 128, 160), ("s2", 16, 32, 256, 320), ("s3", 8, 8, 512, 640)])
def test_adjoint_identity_at_training_size(stage, C, D, H, W):
    from dmvsnet_amd import ops
    oracle_defect = max(x for s in range(8) for x in _adjoint_defects_oracle(100 + s))
    V = 5
    feats, cams, depth, gsim = cuda_case(*R.make_case(C=C, V=V, D=D, H=H, W=W, seed=31))
    delta = [f.cuda() for f in R.make_case(C=C, V=V, D=D, H=H, W=W, seed=32)[0]]
    proj12 = ops.relative_proj(cams[0].contiguous())
    hwc = lambda t: t[0].permute(1, 2, 0).contiguous()            # noqa: E731
    q4 = lambda t: ops.nchw_to_q4(t[0])                            # noqa: E731
    gref = torch.empty((C, H, W), device="cuda")
    gsrc = [torch.zeros((C, H, W), device="cuda") for _ in range(V - 1)]
    ops.warp_corr_backward(q4(feats[0]), [q4(f) for f in feats[1:]], proj12, depth[0], gsim[0], gref, gsrc)
    G = gsim[0].double()
    # <G, sim(dref, src)> == <dRef, dref>: the forward from the GENERIC kernel (layout="hwc")
    sim = ops.warp_corr(hwc(delta[0]), [hwc(f) for f in feats[1:]], proj12, depth[0], layout="hwc").double()
    lhs, scale = (G * sim).sum().item(), (G * sim).abs().sum().item()
    d_ref = abs(lhs - (gref.double() * delta[0][0].double()).sum().item()) / scale
    # <G, sim(ref, dsrc)> == sum_v <dSrc_v, dsrc_v>
    sim = ops.warp_corr(hwc(feats[0]), [hwc(f) for f in delta[1:]], proj12, depth[0], layout="hwc").double()
    lhs, scale = (G * sim).sum().item(), (G * sim).abs().sum().item()
    d_src = abs(lhs - sum((g.double() * d[0].double()).sum().item() for g, d in zip(gsrc, delta[1:]))) / scale
    print(f"ADJOINT {stage} C={C} D={D} {H}x{W} V={V}: defect dRef {d_ref:.3e}  dSrc {d_src:.3e}  "
          f"oracle (8x12, max of 16) {oracle_defect:.3e}")
    assert d_ref <= FACTOR * oracle_defect and d_src <= FACTOR * oracle_defect


# ------------------------------------------------------------------------------------------------ reproducibility
def test_dref_is_bitwise_reproducible_dsrc_to_rounding():
    from dmvsnet_amd import cost_agg
    case = R.make_case(**R.LARGE_CASES["c8_v7_d8_256x320"])
    _, g64 = R.grads_f64(*case)
    _, g_or = R.grads_of(O.warp_corr, *case)
    dev = cuda_case(*case)
    a = R.grads_of(cost_agg, *dev)[1]
    b = R.grads_of(cost_agg, *dev)[1]
    assert torch.equal(a[0], b[0])
    for v in range(1, len(a)):
        e_or, d = dist(g_or[v], g64[v]), dist(a[v], b[v])
        print(f"REPRO dSrc{v}: run-to-run {d:.3e}  e_oracle {e_or:.3e}  bitwise {torch.equal(a[v], b[v])}")
        assert d <= FACTOR * e_or


# ------------------------------------------------------------------------------------------------ one stage pass
def test_stage_pass_through_autograd():
    """oracle.feature_net (state dict requiring grad) -> cost aggregation -> oracle.cost_reg -> scalar.  Three chains: the
    oracle on the CPU, the oracle on the GPU (stock ATen kernels), cost_agg on the GPU.  Per FeatureNet parameter, relative
    L2: |cost_agg chain - oracle GPU chain| <= 4 x |oracle CPU chain - oracle GPU chain|."""
    from dmvsnet_amd import MVSNet, cost_agg, synth
    H, W, V, D = 64, 96, 3, 8
    net = MVSNet([D], [4], verbose=False)
    sd0 = synth.synth_state_dict(net.state_dict(), seed=3)
    imgs, proj, dv = synth.synth_inputs(H, W, V, seed=3)
    hyp, _ = O.depth_hypotheses(dv, D, None, (H // 4, W // 4))
    wsum = torch.from_numpy(np.random.Generator(np.random.PCG64(9)).standard_normal((1, 4, D, H // 4, W // 4), dtype=np.float32))

    def chain(agg, dev):
        sd = {k: v.detach().to(dev).clone() for k, v in sd0.items()}
        params = {k: v.requires_grad_(True) for k, v in sd.items() if k.startswith("feature.") and v.is_floating_point()
                  and "running_" not in k}
        feats = [O.feature_net(sd, imgs[:, v].to(dev))["stage1"] for v in range(V)]
        sim = agg(feats, proj["stage1"].to(dev), hyp.to(dev))
        loss = (O.cost_reg(sd, "cost_regularization.0", sim) * wsum.to(dev)).sum()
        names = list(params)
        grads = torch.autograd.grad(loss, [params[k] for k in names], allow_unused=True)
        return {k: g.detach().double().cpu() for k, g in zip(names, grads) if g is not None}, loss.item()

    g_cpu, l_cpu = chain(O.warp_corr, "cpu")
    g_gpu, l_gpu = chain(O.warp_corr, "cuda")
    g_hip, l_hip = chain(cost_agg, "cuda")
    assert set(g_cpu) == set(g_gpu) == set(g_hip) and len(g_hip) >= 20
    print(f"STAGE loss: oracle cpu {l_cpu:.6f}  oracle gpu {l_gpu:.6f}  cost_agg {l_hip:.6f}")
    bad = []
    for k in g_gpu:
        n = g_gpu[k].norm().item()
        assert n > 0, k
        base = (g_cpu[k] - g_gpu[k]).norm().item() / n
        got = (g_hip[k] - g_gpu[k]).norm().item() / n
        print(f"STAGE {k}: cost_agg vs oracle-gpu {got:.3e}  oracle cpu vs gpu {base:.3e}  ratio {got / base:.2f}")
        if got > 4.0 * base:
            bad.append((k, got, base))
    assert not bad, bad
