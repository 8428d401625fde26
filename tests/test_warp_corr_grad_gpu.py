"""K1b (``warp_corr_bwd_ref_kernel`` / ``warp_corr_bwd_src_kernel`` of csrc/warp_corr_bwd.h) on the MI355X against the float64
restatement tests/warp_corr_grad_ref.py, on the forward's case tables: tile seams, partial plane chunks, 1 to 16 source views, exact
integer and half-pixel samples, samples on -1 / W / H, a zero denominator, cameras behind or inside the volume, scattered
hypotheses, many-to-one projections.

Yardstick: the restatement in pixel coordinates (tied to float64 autograd and to the reference's recorded gradients in
tests/test_warp_corr_grad_cpu.py, where the tables' conditions, the op-order exclusion and the criterion's power to tell nine wrong
kernels apart are asserted too).  No test here reads the reference or the oracle.  Kernel and restatement get the SAME fp32 p12: the
kernel's own, ``ops.relative_proj`` copied back, for camera cases, the literal one else.  All direct launches go through
``ops.warp_corr_backward`` on quad-planar features (``ops.hwc_to_q4``), with the harness tests/k1b_gpu_harness.py shares with the
deterministic mode's file.

  criterion  per gradient tensor (dRef and each dSrc_v on its own) e_max and e_mean relative to the tensor's max-abs, each
             <= 8 e_ref (16 * 2^-23 where e_ref < 4 * 2^-23); bit-for-bit zero where the yardstick is identically zero.  WINDOWS:
             the mean bound only; CONTENTION: max(plain, any-order summation allowance) on the max -- both derived in
             warp_corr_grad_ref's docstring.  EDGE_SHAPES: every tensor exactly zero.
  guards     gref is a NaN-filled view, each gsrc[v] a zero-filled one, in the middle of a larger buffer with 1024 guard elements
             of a FINITE sentinel on both sides (an atomic add into NaN leaves NaN and would not show): afterwards every guard
             holds the sentinel's bits, gref is finite everywhere, and the buffer of a view that was not asked for is untouched.
  exact      one-hot gsim probes, ``torch.equal`` against the fp32 restatement (test_warp_corr_grad_cpu.py asserts that fp32 is
             exact there): a swapped tap, a wrong channel group or a wrong divisor is named without a tolerance.
  masks      16 views with three asked for, the reference alone, no reference; the same through ``cost_agg`` with
             ``costagg.launch_counts``.
  cost_agg   the camera tables and a batch of two through ``dmvsnet_amd.cost_agg`` under autograd (``nchw_to_q4``,
             ``relative_proj``, the batch loop), same yardstick and bounds.

Every comparison prints its figures before it asserts (K1B lines), the worst ratio per table is printed at the end of the module;
docs/kernels/K1b_warp_corr_backward.md keeps the measured ones.  No test provokes a fault: behind-camera, zero-denominator and
1e9-pixel samples are legal inputs which the forward suite launches through the same coordinate routine."""
import pytest
import torch

import warp_corr_grad_ref as GR
from k1b_gpu_harness import BY_TABLE, CASES, F32, PROBES, compare_all, launch, print_worst

pytestmark = pytest.mark.gpu

CAMERA = [n for n, c in CASES.items() if c["cams"] is not None and c["table"] != "EDGE_SHAPES"]


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    print_worst("direct", "cost_agg")


# ------------------------------------------------------------------------------------------------ parity with float64
@pytest.mark.parametrize("name", [n for n in CASES if CASES[n]["table"] != "EDGE_SHAPES"])
def test_parity(name):
    gref, gsrc = launch(name)
    compare_all(name, [gref] + gsrc)


@pytest.mark.parametrize("name", BY_TABLE["EDGE_SHAPES"])
def test_one_row_and_one_column_maps(name):
    """The reference's (n - 1) / 2 = 0 puts every tap outside: every gradient exactly zero, dRef fully written (``launch``)."""
    gref, gsrc = launch(name)
    for k, g in enumerate([gref] + gsrc):
        print(f"K1B {name} tensor {k}: max|grad| {g.abs().max().item():.3e}")
        assert torch.equal(g.cpu(), torch.zeros(g.shape)), (name, k)


@pytest.mark.parametrize("name", ["scatter-outlier-c16", "scatter-checker-c32"])
def test_dref_is_bitwise_reproducible_and_both_dsrc_obey_the_criterion(name):
    a_ref, a_src = launch(name)
    b_ref, b_src = launch(name)
    assert torch.equal(a_ref, b_ref), f"{name}: dRef differs between two launches"
    compare_all(name, [a_ref] + a_src)
    compare_all(name, [b_ref] + b_src)
    print(f"K1B {name}: dSrc bitwise equal between two launches: {[torch.equal(x, y) for x, y in zip(a_src, b_src)]}")


# ------------------------------------------------------------------------------------------------ one-hot probes
@pytest.mark.parametrize("name", list(PROBES))
def test_one_hot_probes_are_exact(name):
    """dSrc == the fp32 restatement bit for bit: at most four taps per channel of the probe's group, exact zeros in the other group
    and everywhere else; dRef likewise on the integer offsets."""
    c, src_exact, ref_exact = PROBES[name]
    D, H, W = c["depth"].shape
    n = 0
    for d, y, x in GR.probe_voxels(D, H, W):
        for g in (0, 1):
            gs = GR.one_hot(D, H, W, g, d, y, x)
            want = GR.grads_ref(c["feats"], c["p12"], c["depth"], gs, F32)
            gref, gsrc = launch(name, gsim=gs)
            tag = f"{name} probe g{g} d{d} y{y} x{x}"
            assert src_exact and torch.equal(gsrc[0].cpu(), want[1]), \
                f"{tag}: dSrc differs at {(gsrc[0].cpu() != want[1]).nonzero()[:8].tolist()}"
            assert not gsrc[0][1 - g::2].any() and (gsrc[0][g::2] != 0).sum((1, 2)).max().item() <= 4, tag
            if ref_exact:
                assert torch.equal(gref.cpu(), want[0]), f"{tag}: dRef differs at {(gref.cpu() != want[0]).nonzero()[:8].tolist()}"
            n += 1
    print(f"K1B {name}: {n} one-hot probes exact (dSrc{' and dRef' if ref_exact else ''})")


# ------------------------------------------------------------------------------------------------ sixteen views and masks
@pytest.mark.parametrize("name", ["views-c8-n16", "views-c32-n16"])
def test_sixteen_views_with_masks(name):
    import dmvsnet_amd.costagg as ca
    some = (0, 7, 15)
    full_ref, _ = launch(name)
    # three views and the reference
    gref, gsrc = launch(name, want=some)
    assert torch.equal(gref, full_ref)
    compare_all(name, [gref] + gsrc)
    assert [v for v, g in enumerate(gsrc) if g is not None] == list(some)
    # the reference alone; then the three views without it (``launch`` checks that what was not asked for stays untouched)
    gref, gsrc = launch(name, want=())
    assert torch.equal(gref, full_ref) and all(g is None for g in gsrc)
    gref, gsrc = launch(name, want_ref=False, want=some)
    assert gref is None
    compare_all(name, [None] + gsrc)
    # the same masks through cost_agg
    c = CASES[name]
    V = len(c["feats"])
    cams, depth, gsim = c["cams"][None].cuda(), c["depth"][None].cuda(), c["gsim"][None].cuda()
    for mask, counts in (([True] + [v - 1 in some for v in range(1, V)], {"bwd_ref": 1, "bwd_src_views": 3}),
                         ([True] + [False] * (V - 1), {"bwd_ref": 1, "bwd_src_views": 0}),
                         ([False] + [v - 1 in some for v in range(1, V)], {"bwd_ref": 0, "bwd_src_views": 3})):
        leaves = [f[None].cuda().requires_grad_(m) for f, m in zip(c["feats"], mask)]
        before = dict(ca.launch_counts)
        ca.cost_agg(leaves, cams, depth).backward(gsim)
        assert {k: ca.launch_counts[k] - before[k] for k in before} == counts, mask
        assert [l.grad is not None for l in leaves] == mask
        if mask[0]:
            assert torch.equal(leaves[0].grad[0], full_ref)
        compare_all(name, [None if l.grad is None else l.grad[0] for l in leaves], route="cost_agg")


# ------------------------------------------------------------------------------------------------ through cost_agg
def grads_through_cost_agg(feats, cams, depth, gsim):
    """feats V x [B,C,H,W], cams [B,V,2,4,4], depth [B,D,H,W], gsim [B,2,D,H,W] (CPU) -> V gradients [B,C,H,W] (device)."""
    from dmvsnet_amd import cost_agg
    leaves = [f.cuda().requires_grad_(True) for f in feats]
    sim = cost_agg(leaves, cams.cuda(), depth.cuda())
    grads = torch.autograd.grad(sim, leaves, gsim.cuda())
    torch.cuda.synchronize()
    return list(grads)


@pytest.mark.parametrize("name", CAMERA)
def test_parity_through_cost_agg(name):
    c = CASES[name]
    assert c["table"] in ("SHAPES", "VIEWS", "SCATTER", "SPECIAL")
    grads = grads_through_cost_agg([f[None] for f in c["feats"]], c["cams"][None], c["depth"][None], c["gsim"][None])
    compare_all(name, [g[0] for g in grads], route="cost_agg")


def test_batch_of_two_through_cost_agg():
    names = ("scatter-outlier-c8", "scatter-checker-c8")
    cs = [CASES[n] for n in names]
    assert cs[0]["depth"].shape == cs[1]["depth"].shape and len(cs[0]["feats"]) == len(cs[1]["feats"])
    single = [grads_through_cost_agg([f[None] for f in c["feats"]], c["cams"][None], c["depth"][None], c["gsim"][None]) for c in cs]
    batch = grads_through_cost_agg([torch.stack(fs) for fs in zip(cs[0]["feats"], cs[1]["feats"])], torch.stack([c["cams"] for c in cs]),
                                   torch.stack([c["depth"] for c in cs]), torch.stack([c["gsim"] for c in cs]))
    for b, name in enumerate(names):
        assert torch.equal(batch[0][b], single[b][0][0]), f"{name}: dRef of sample {b} differs from its single-sample run"
        compare_all(name, [g[b] for g in batch], route="cost_agg")
