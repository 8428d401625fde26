"""K1b's deterministic mode (max pre-pass, ``warp_corr_bwd_src_kernel`` on csrc/warp_corr_bwd_det.h's ``FixedSink``, finalize) on the
MI355X, through ``ops.warp_corr_backward_det`` and ``cost_agg(..., deterministic=...)``.

  bits       on the cases where fp32 forms the tap weights exactly (``costagg_det_ref.exact_names``: CONTENTION and the half-pixel AFFINE
             offsets; tests/test_costagg_det_cpu.py asserts the exactness on every one) each dSrc_v equals the CPU emulation of the
             contract under ``torch.equal``.  On these i.i.d. normal inputs nearly every addend sits on the grid 2^-k, so the CONTENTION
             cases run a second time with ``costagg_det_ref.wide_gsim``, where the rounding to the grid decides bits (the CPU file shows
             that truncation is told apart there and not on the plain cases).
  order      SHAPES, VIEWS, SCATTER, SPECIAL, CONTENTION: two launches of variant 0 and one of variant 1 (planes in reverse, chunks of 4,
             workgroups in reverse) give the same bits; dRef equals ``ops.warp_corr_backward``'s bit for bit.
  parity     every table under ``warp_corr_grad_ref.reference`` / ``bounds_of`` through tests/k1b_gpu_harness.py's ``compare`` (the
             harness both K1b files import, with its cached references, which are computed once for both): WINDOWS the mean bound
             only, CONTENTION the PLAIN bound -- allowance 0, which the atomic path cannot promise.  EDGE_SHAPES: exact zeros.
  guards     every gsrc is a NaN-filled view between 1024 sentinel elements (``launch``): afterwards the guards hold their bits, every
             wanted element is finite (so: written), a view not asked for is still all NaN.  Views 0, 7, 15 of 16 alone equal the
             all-views run bit for bit; a workspace one element short is refused with DMVS_EINVAL before anything is launched.
  rules      one inf (or NaN) in gsim or in the reference features: every wanted dSrc all NaN, guards intact; gsim = 0: all zeros.
  autograd   ``deterministic=True`` on a batch of two: each sample's dSrc equals its single-sample run bit for bit; None follows
             ``torch.use_deterministic_algorithms``; False and the default take the atomic path; ``DiffCostAgg`` the same; told apart by
             ``costagg.det_launch_counts`` / ``launch_counts``.

No test provokes a fault: the inputs are the forward suite's legal ones, and inf / NaN values are data to these kernels (they are
compared as bit patterns and never used as an address)."""
import functools

import pytest
import torch

import costagg_det_ref as DR
import k1b_gpu_harness as T   # the harness and the cached float64 references, computed once for both K1b files
from k1b_gpu_harness import BY_TABLE, CASES

pytestmark = pytest.mark.gpu

ORDER = [n for t in ("SHAPES", "VIEWS", "SCATTER", "SPECIAL", "CONTENTION") for n in BY_TABLE[t]]
EXACT = DR.exact_names()
launch = functools.partial(T.launch, mode="det")   # every gsrc starts as NaN inside SENTINEL guards


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    T.print_worst("det", "det cost_agg")


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def launched(name):
    """The default launch of a case (all views, variant 0), shared by the tests that compare against it.  Never modified."""
    return launch(name)


# ------------------------------------------------------------------------------------------------ bit equality to the emulation
def assert_equals_emulation(name, gsim):
    c = CASES[name]
    want = DR.emulate(c["feats"], c["p12"], c["depth"], gsim)
    _, gsrc = launch(name, gsim=gsim, want_ref=False)
    for v, (g, w) in enumerate(zip(gsrc, want)):
        diff = bits(g.cpu()) != bits(w)
        print(f"K1BDET {name} dSrc{v}: {int(diff.sum())} of {diff.numel()} elements differ from the emulation")
        assert not diff.any(), f"{name} dSrc{v}: differs at {diff.nonzero()[:8].tolist()}"


@pytest.mark.parametrize("name", EXACT)
def test_bit_equal_to_the_emulation(name):
    assert_equals_emulation(name, CASES[name]["gsim"])


@pytest.mark.parametrize("name", BY_TABLE["CONTENTION"])
def test_bit_equal_to_the_emulation_with_a_wide_dynamic_range(name):
    assert_equals_emulation(name, DR.wide_gsim(CASES[name]["gsim"]))


# ------------------------------------------------------------------------------------------------ order freedom
@pytest.mark.parametrize("name", ORDER)
def test_runs_and_decompositions_give_the_same_bits(name):
    from dmvsnet_amd import ops
    c = CASES[name]
    a_ref, a_src = launched(name)
    b_ref, b_src = launch(name)
    r_ref, r_src = launch(name, variant=1)
    for v, (a, b, r) in enumerate(zip(a_src, b_src, r_src)):
        assert same_bits(a, b), f"{name} dSrc{v}: two launches differ"
        assert same_bits(a, r), f"{name} dSrc{v}: variant 1 differs at {(bits(a) != bits(r)).nonzero()[:8].tolist()}"
    assert same_bits(a_ref, b_ref) and same_bits(a_ref, r_ref)
    gref = torch.full_like(a_ref, float("nan"))
    ops.warp_corr_backward(T.dev_feats(name)[0], T.dev_feats(name)[1:], T.p12_of(name).cuda(), c["depth"].cuda(), c["gsim"].cuda(), gref,
                           [None] * len(a_src))
    assert same_bits(a_ref, gref), f"{name}: dRef differs from dmvs_warp_corr_backward's"


# ------------------------------------------------------------------------------------------------ parity with float64
@pytest.mark.parametrize("name", [n for n in CASES if CASES[n]["table"] != "EDGE_SHAPES"])
def test_parity(name):
    gref, gsrc = launched(name)
    g64, e_ref, _ = T.ref_of(name)
    table = CASES[name]["table"]
    for k, g in enumerate([gref] + gsrc):   # allowance 0 on every table: CONTENTION under the plain bound
        T.compare(f"{name} det {'dRef' if k == 0 else f'dSrc{k - 1}'}", table, g, g64[k], e_ref[k], 0.0, route="det")


@pytest.mark.parametrize("name", BY_TABLE["EDGE_SHAPES"])
def test_one_row_and_one_column_maps(name):
    gref, gsrc = launched(name)
    for k, g in enumerate([gref] + gsrc):
        assert torch.equal(g.cpu(), torch.zeros(g.shape)), (name, k)


# ------------------------------------------------------------------------------------------------ masks and the workspace
@pytest.mark.parametrize("name", ["views-c8-n16", "views-c32-n16"])
def test_three_of_sixteen_views_equal_the_all_views_run(name):
    some = (0, 7, 15)
    full_ref, full = launched(name)
    gref, gsrc = launch(name, want=some)
    assert same_bits(gref, full_ref)
    assert [v for v, g in enumerate(gsrc) if g is not None] == list(some)
    for v in some:
        assert same_bits(gsrc[v], full[v]), f"{name}: dSrc{v} depends on which other views are asked for"
    gref, gsrc = launch(name, want_ref=False, want=(15,), variant=1)
    assert gref is None and same_bits(gsrc[15], full[15])
    gref, gsrc = launch(name, want=())
    assert same_bits(gref, full_ref) and all(g is None for g in gsrc)


def test_a_short_workspace_is_refused_and_a_given_one_is_used():
    from dmvsnet_amd import ops
    from dmvsnet_amd._lib import DmvsError
    name = "views-c8-n6"
    c = CASES[name]
    C, (_, H, W) = c["C"], c["depth"].shape
    need = ops.warp_corr_backward_det_workspace(C, H, W, 6)
    assert need == 8 * 6 * C * H * W
    with pytest.raises(DmvsError, match=r"code -1"):
        launch(name, workspace=torch.empty((need // 8 - 1,), dtype=torch.int64, device="cuda"))
    with pytest.raises(DmvsError, match="int64"):
        launch(name, workspace=torch.empty((need // 4,), dtype=torch.int32, device="cuda"))
    # three views need half of it; a dirty workspace is cleared by the entry
    ws = torch.full((need // 8,), 0x0123456789ABCDEF, dtype=torch.int64, device="cuda")
    _, gsrc = launch(name, want=(1, 2, 4), workspace=ws[:need // 16])
    for v in (1, 2, 4):
        assert same_bits(gsrc[v], launched(name)[1][v])
    assert (ws[need // 16:] == 0x0123456789ABCDEF).all(), "wrote past the workspace it was given"


# ------------------------------------------------------------------------------------------------ the zero and non-finite rules
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_a_non_finite_maximum_makes_every_wanted_gradient_nan(bad):
    from dmvsnet_amd import ops
    name = "views-c8-n6"
    c = CASES[name]
    g = c["gsim"].clone()
    g[1, 2, 5, 40] = bad
    launch(name, gsim=g, want_ref=False, want=(0, 3, 5), expect="nan")
    launch(name, gsim=g, want_ref=False, want=(2,), variant=1, expect="nan")
    ref = c["feats"][0].clone()
    ref[3, 7, 9] = bad
    feats = [ops.hwc_to_q4(ref.permute(1, 2, 0).contiguous().cuda())] + T.dev_feats(name)[1:]
    launch(name, feats=feats, want_ref=False, want=(1, 4), expect="nan")


def test_a_zero_maximum_gives_zeros():
    name = "views-c8-n6"
    _, gsrc = launch(name, gsim=torch.zeros_like(CASES[name]["gsim"]), want_ref=False)
    for g in gsrc:
        assert torch.equal(bits(g), torch.zeros_like(bits(g)))


# ------------------------------------------------------------------------------------------------ through autograd
def grads_through(feats, cams, depth, gsim, module=False, **kw):
    """feats V x [B,C,H,W], cams [B,V,2,4,4], depth [B,D,H,W], gsim [B,2,D,H,W] (CPU) -> V gradients [B,C,H,W] (device)."""
    from dmvsnet_amd import DiffCostAgg, cost_agg
    leaves = [f.cuda().requires_grad_(True) for f in feats]
    if module:
        sim = DiffCostAgg("variance", leaves[0].shape[1], **kw)(leaves, cams.cuda(), depth.cuda(), stage_idx=0)
    else:
        sim = cost_agg(leaves, cams.cuda(), depth.cuda(), **kw)
    grads = torch.autograd.grad(sim, leaves, gsim.cuda())
    torch.cuda.synchronize()
    return list(grads)


def counts():
    import dmvsnet_amd.costagg as ca
    return dict(ca.launch_counts), dict(ca.det_launch_counts)


def moved(before):
    after = counts()
    return tuple({k: a[k] - b[k] for k in a} for a, b in zip(after, before))


NAMES2 = ("scatter-outlier-c8", "scatter-checker-c8")
NONE = {"bwd_ref": 0, "bwd_src_views": 0}


def single(name, **kw):
    c = CASES[name]
    return grads_through([f[None] for f in c["feats"]], c["cams"][None], c["depth"][None], c["gsim"][None], **kw)


def batch_of_two(**kw):
    cs = [CASES[n] for n in NAMES2]
    return grads_through([torch.stack(fs) for fs in zip(cs[0]["feats"], cs[1]["feats"])], torch.stack([c["cams"] for c in cs]),
                         torch.stack([c["depth"] for c in cs]), torch.stack([c["gsim"] for c in cs]), **kw)


@pytest.mark.parametrize("module", [False, True])
def test_each_sample_of_a_batch_equals_its_single_sample_run(module):
    before = counts()
    singles = [single(n, module=module, deterministic=True) for n in NAMES2]
    assert moved(before) == (NONE, {"bwd_ref": 2, "bwd_src_views": 4})
    before = counts()
    batch = batch_of_two(module=module, deterministic=True)
    assert moved(before) == (NONE, {"bwd_ref": 2, "bwd_src_views": 4})
    for b, name in enumerate(NAMES2):
        for v, (g, s) in enumerate(zip(batch, singles[b])):
            assert same_bits(g[b], s[0]), f"{name}: gradient of view {v} in the batch differs from its single-sample run"
        T.compare_all(name, [g[b] for g in batch], route="det cost_agg")
        # and from the direct launch of the same sample with the kernel's own p12
        for v, g in enumerate(launched(name)[1]):
            assert same_bits(batch[1 + v][b], g), (name, v)


def test_none_follows_the_torch_flag():
    name = NAMES2[0]
    want = single(name, deterministic=True)
    was = torch.are_deterministic_algorithms_enabled()
    warn = torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        before = counts()
        got = single(name)
        assert moved(before) == (NONE, {"bwd_ref": 1, "bwd_src_views": 2})
        before = counts()
        single(name, deterministic=False)   # False forces the atomics under the flag too
        assert moved(before) == ({"bwd_ref": 1, "bwd_src_views": 2}, NONE)
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)
    assert torch.are_deterministic_algorithms_enabled() == was
    for g, w in zip(got, want):
        assert same_bits(g, w)


@pytest.mark.parametrize("kw", [{}, {"deterministic": False}, {"deterministic": None}])
def test_the_default_and_false_take_the_atomic_path(kw):
    assert not torch.are_deterministic_algorithms_enabled()
    name = NAMES2[1]
    for module in (False, True):
        before = counts()
        grads = single(name, module=module, **kw)
        assert moved(before) == ({"bwd_ref": 1, "bwd_src_views": 2}, NONE)
        T.compare_all(name, [g[0] for g in grads], route="cost_agg")
    assert same_bits(grads[0][0], launched(name)[0])   # dRef: the same kernel either way
