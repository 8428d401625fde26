"""K1b's pre-summed scatter (``warp_corr_bwd_src_presum_kernel`` of csrc/warp_corr_bwd_presum.h: bounding box of a workgroup's taps, sums
in an LDS window, one global add per window element; a box above the capacity falls back to adds per tap) on the MI355X, through
``ops.warp_corr_backward_presum``, ``cost_agg(..., presum=True)`` and ``DiffMVSNet(..., presum=True)``.

  bits      deterministic sink: a sum of integers does not depend on grouping, so on every case of every table, on the ten wide-range
            ``gsim`` cases of test_costagg_det_gpu.py, on the SEAMS and CAPACITY tables of tests/costagg_presum_ref.py, under variants
            0 - 3, every wanted dSrc is ``torch.equal`` to what ``ops.warp_corr_backward_det`` writes.  No tolerance.  The non-finite and
            zero-maximum rules are that mode's: all NaN, fully written; all zero.
  parity    atomic sink: the same addends in another order of the fp32 sum.  Every gradient tensor under ``k1b_gpu_harness.compare_all``
            with its table's own bounds (plain 8 e_ref; the any-order allowance on CONTENTION; WINDOWS the mean only), variants 0 and 2,
            worst ratios printed under the route "presum".  The one-hot probes at exact offsets stay ``torch.equal``.
  paths     ``path_counts`` (workgroups windowed, direct, empty) against ``costagg_presum_ref.predict`` on the exact-coordinate tables
            (AFFINE, CONTENTION, SEAMS) and on CAPACITY, whose two maps hold a box of exactly ``cap`` (windowed) and ``cap + 1`` texels
            (direct): a kernel that always fell back would pass every value test.
  seams     SEAMS: overlapping windows of neighbouring workgroups and of the two chunks, partial tiles with lanes outside the map at
            the barriers; both sinks, guards intact, 3 of 16 views, views not asked for untouched; EDGE_SHAPES exact zeros.  At W = 130 the
            reference's coordinate round trip is inexact, so against float64 the table takes the WINDOWS rule (see ``test_seams_atomic``)
            and the max is held to the fp32 op-order restatement within the any-order allowance instead.
  autograd  ``cost_agg(..., presum=True)`` on a batch of two in both modes (``presum_launch_counts`` moves, the other dicts do not;
            deterministic: every gradient equal to ``presum=False``'s; atomic: dRef equal), and one whole ``train_step`` of the smallest
            ``DiffMVSNet`` with ``deterministic=True``: every parameter gradient and every parameter equal to ``presum=False``'s.

Every output is a view between 1024 sentinel elements.  No test provokes a fault: the inputs are the forward suite's legal ones; NaN,
behind-camera and 1e9-offset samples are outside the image and never enter a box or a window."""
import functools

import pytest
import torch

import costagg_det_ref as DR
import costagg_presum_ref as PR
import k1b_gpu_harness as T
import warp_corr_grad_ref as GR
from k1b_gpu_harness import BY_TABLE, CASES

pytestmark = pytest.mark.gpu

SEAMS = PR.seam_cases()
EXACT_TABLES = ("AFFINE", "CONTENTION")          # fp32 forms the coordinates exactly: the box restatement is the kernel's
NOT_EDGE = [n for n in CASES if CASES[n]["table"] != "EDGE_SHAPES"]


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    T.print_worst("presum", "presum seams AFFINE", "presum seams WINDOWS", "presum cost_agg")


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def cap_of(C, det, variant):
    from dmvsnet_amd import ops
    return ops.warp_corr_backward_presum_cap(C, det, variant)


@functools.lru_cache(maxsize=None)
def capacity_cases():
    return {c["name"]: c for c in PR.capacity_cases(cap_of(8, True, 2))}


def case_of(name):
    if name in SEAMS:
        return SEAMS[name]
    if name.startswith("capacity-"):
        return capacity_cases()[name]
    return T.case_of(name)


@functools.lru_cache(maxsize=None)
def p12_of(name):
    return case_of(name)["p12"].clone() if name in SEAMS or name.startswith("capacity-") else T.p12_of(name)


@functools.lru_cache(maxsize=None)
def dev_feats(name):
    from dmvsnet_amd import ops
    if name in SEAMS or name.startswith("capacity-"):
        return [ops.hwc_to_q4(f.permute(1, 2, 0).contiguous().cuda()) for f in case_of(name)["feats"]]
    return T.dev_feats(name)


@functools.lru_cache(maxsize=None)
def own_ref(name):
    """The float64 yardstick of a SEAMS / CAPACITY case, as ``k1b_gpu_harness.ref_of``.  Never modified."""
    c = case_of(name)
    return GR.reference(c, p12_of(name)) + (GR.allowances(c, p12_of(name)),)


def launch(name, det, variant=0, gsim=None, feats=None, want_ref=False, want=None, presum=True, counts=False, expect="finite"):
    """One guarded launch of a case through ``ops.warp_corr_backward_presum`` (``presum=False``: through the existing entry of the same
    mode, variant bit 0 only) -> (gref or None, [gsrc_v or None], [windowed, direct, empty] or None).  gref starts as NaN; gsrc start
    as zeros (atomic: added into) or NaN (deterministic: written).  Afterwards the guards hold their bits, every wanted gsrc is
    ``expect`` ("finite", so: written, or "nan"), a view not asked for is untouched."""
    from dmvsnet_amd import ops
    c = case_of(name)
    C, (D, H, W) = c["C"], c["depth"].shape
    feats = dev_feats(name) if feats is None else feats
    nsrc = len(feats) - 1
    want = set(range(nsrc)) if want is None else set(want)
    gsim = c["gsim"] if gsim is None else gsim
    rbuf, gref = T.guarded(C, H, W, float("nan"))
    sbufs = [T.guarded(C, H, W, float("nan") if det else 0.0) for _ in range(nsrc)]
    args = (feats[0], feats[1:], p12_of(name).cuda(), c["depth"].cuda(), gsim.cuda(), gref if want_ref else None,
            [g if v in want else None for v, (_, g) in enumerate(sbufs)])
    pc = torch.zeros((3,), dtype=torch.int32, device="cuda") if counts else None
    if presum:
        ops.warp_corr_backward_presum(*args, deterministic=det, variant=variant, path_counts=pc)
    elif det:
        ops.warp_corr_backward_det(*args, variant=variant & 1)
    else:
        ops.warp_corr_backward(*args)
    torch.cuda.synchronize()
    assert T.guards_intact(rbuf), f"{name}: wrote outside gref"
    if not want_ref:
        assert torch.isnan(gref).all(), f"{name}: gref touched though not asked for"
    else:
        assert torch.isfinite(gref).all(), f"{name}: gref elements not written (or not finite)"
    for v, (buf, g) in enumerate(sbufs):
        assert T.guards_intact(buf), f"{name}: wrote outside gsrc[{v}]"
        if v not in want:
            assert torch.isnan(g).all() if det else not g.any(), f"{name}: gsrc[{v}] touched though not asked for"
        elif expect == "finite":
            assert torch.isfinite(g).all(), f"{name}: gsrc[{v}] has elements that were not written (or are not finite)"
        else:
            assert torch.isnan(g).all(), f"{name}: gsrc[{v}] is not all NaN"
    return (gref if want_ref else None), [g if v in want else None for v, (_, g) in enumerate(sbufs)], (pc.tolist() if counts else None)


@functools.lru_cache(maxsize=None)
def plain(name, det):
    """The existing entry's dSrc of a case in one mode (all views), shared by the tests that compare against it.  Never modified."""
    return launch(name, det, presum=False)[1]


def assert_equals_det_entry(name, variant, gsim=None):
    want = plain(name, True) if gsim is None else launch(name, True, gsim=gsim, presum=False)[1]
    _, got, _ = launch(name, True, variant, gsim=gsim)
    for v, (g, w) in enumerate(zip(got, want)):
        diff = bits(g) != bits(w)
        assert not diff.any(), f"{name} variant {variant} dSrc{v}: {int(diff.sum())} elements differ, first {diff.nonzero()[:8].tolist()}"


# ------------------------------------------------------------------------------------------------ deterministic sink: the same bits
@pytest.mark.parametrize("name", list(CASES))
def test_deterministic_bits_equal_the_existing_entry(name):
    for variant in range(4):
        assert_equals_det_entry(name, variant)


@pytest.mark.parametrize("name", BY_TABLE["CONTENTION"])
def test_deterministic_bits_with_a_wide_dynamic_range(name):
    gsim = DR.wide_gsim(CASES[name]["gsim"])
    for variant in range(4):
        assert_equals_det_entry(name, variant, gsim=gsim)


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_a_non_finite_maximum_makes_every_wanted_gradient_nan(bad):
    from dmvsnet_amd import ops
    name = "views-c8-n6"
    c = CASES[name]
    g = c["gsim"].clone()
    g[1, 2, 5, 40] = bad
    launch(name, True, gsim=g, want=(0, 3, 5), expect="nan")
    launch(name, True, 3, gsim=g, want=(2,), expect="nan")
    ref = c["feats"][0].clone()
    ref[3, 7, 9] = bad
    feats = [ops.hwc_to_q4(ref.permute(1, 2, 0).contiguous().cuda())] + T.dev_feats(name)[1:]
    launch(name, True, 2, feats=feats, want=(1, 4), expect="nan")


def test_a_zero_maximum_gives_zeros():
    name = "views-c8-n6"
    for variant in (0, 2):
        _, gsrc, _ = launch(name, True, variant, gsim=torch.zeros_like(CASES[name]["gsim"]))
        for g in gsrc:
            assert torch.equal(bits(g), torch.zeros_like(bits(g)))


# ------------------------------------------------------------------------------------------------ atomic sink: the existing criterion
@pytest.mark.parametrize("variant", (0, 2))
@pytest.mark.parametrize("name", NOT_EDGE)
def test_atomic_parity(name, variant):
    gref, gsrc, _ = launch(name, False, variant, want_ref=True)
    T.compare_all(name, [gref] + gsrc, route="presum")


@pytest.mark.parametrize("name", BY_TABLE["EDGE_SHAPES"])
def test_one_pixel_one_row_and_one_column_maps_return_exact_zeros(name):
    for det in (False, True):
        for variant in (0, 3) if det else (0, 2):
            gref, gsrc, counts = launch(name, det, variant, want_ref=True, counts=True)
            for k, g in enumerate([gref] + gsrc):
                assert torch.equal(g.cpu(), torch.zeros(g.shape)), (name, det, variant, k)
            assert counts[0] == counts[1] == 0 and counts[2] > 0   # every tap is outside: nothing but empty boxes


@pytest.mark.parametrize("name", [n for n, (_, src_exact, _) in T.PROBES.items() if src_exact])
def test_one_hot_probes_stay_exact(name):
    """A single addend per texel is exact in any grouping: the probes of test_warp_corr_grad_gpu.py through the window."""
    c = T.case_of(name)
    D, H, W = c["depth"].shape
    for k, (d, y, x) in enumerate(GR.probe_voxels(D, H, W)):
        gsim = GR.one_hot(D, H, W, k % 2, d, y, x)
        want = GR.grads_ref(c["feats"], T.p12_of(name), c["depth"], gsim, GR.F32)
        _, gsrc, _ = launch(name, False, 2 * (k % 2), gsim=gsim)
        assert torch.equal(gsrc[0].cpu(), want[1]), (name, d, y, x)


# ------------------------------------------------------------------------------------------------ both paths ran
def counted(name, det, variant, want=None):
    c = case_of(name)
    _, _, counts = launch(name, det, variant, counts=True, want=want)
    pred = PR.predict(p12_of(name), c["depth"], c["C"], cap_of(c["C"], det, variant), variant, views=want)
    print(f"K1BPRESUM {name} det {int(det)} variant {variant}: windowed / direct / empty {counts}, predicted {pred}")
    return counts, pred


def test_the_identity_is_windowed_and_far_offsets_are_empty():
    for det in (False, True):
        for variant in (2, 3):
            counts, pred = counted(GR.affine_name(8, 0, 0), det, variant)
            assert counts == pred and counts[0] > 0 and counts[1] == 0
            counts, pred = counted(GR.affine_name(32, 1e9, -1e9), det, variant)
            assert counts == pred and counts[0] == counts[1] == 0 and counts[2] > 0


@pytest.mark.parametrize("name", [n for t in EXACT_TABLES for n in BY_TABLE[t]])
def test_path_counts_equal_the_prediction_on_exact_coordinates(name):
    for det, variant in ((False, 0), (False, 2), (True, 1), (True, 2), (True, 3)):
        counts, pred = counted(name, det, variant)
        assert counts == pred, (name, det, variant)


def test_a_box_of_exactly_the_capacity_is_windowed_and_one_more_texel_is_direct():
    at, over = capacity_cases()
    for det in (False, True):
        cap = cap_of(8, det, 2)
        for variant in (2, 3):
            for name, path in ((at, 0), (over, 1)):
                c = case_of(name)
                box = PR.boxes(c["p12"][0], c["depth"], 8)[(0, 0, 0)]
                assert PR.texels(box) == cap + path   # constructed on the CPU first
                counts, pred = counted(name, det, variant)
                assert counts == pred and counts[path] == 2 and counts[1 - path] == 0 and counts[2] > 0, (name, det, variant)
        counts, pred = counted(over, det, 0)   # the full capacity holds it
        assert counts == pred and counts[0] == 2 and counts[1] == 0


@pytest.mark.parametrize("side", (0, 1))
def test_values_on_both_sides_of_the_capacity(side):
    name = list(capacity_cases())[side]
    g64, e_ref, allow = own_ref(name)
    for variant in (0, 2):
        _, gsrc, _ = launch(name, False, variant)
        T.compare(f"{name} presum v{variant} dSrc0", "CONTENTION", gsrc[0], g64[1], e_ref[1], allow[1], route="presum")
    for variant in range(4):
        assert_equals_det_entry(name, variant)


def test_a_scatter_case_with_an_outlier_takes_the_direct_path():
    for det in (False, True):
        _, _, counts = launch("scatter-outlier-c8", det, 2, counts=True)
        print(f"K1BPRESUM scatter-outlier-c8 det {int(det)} variant 2: windowed / direct / empty {counts}")
        assert counts[1] > 0 and sum(counts) == 2 * 16   # two views; 32 x 128 is 8 x 2 tiles; one chunk, one quad group
        _, _, full = launch("scatter-outlier-c8", det, 0, counts=True)
        print(f"K1BPRESUM scatter-outlier-c8 det {int(det)} variant 0: windowed / direct / empty {full}")
        assert full[0] > 0 and sum(full) == 2 * 16


# ------------------------------------------------------------------------------------------------ seams of the new decomposition
@functools.lru_cache(maxsize=None)
def seam_op_order(name):
    """The fp32 restatement of a SEAMS case WITH the reference's normalise / un-normalise round trip -- the kernels' op order, the
    kernels' fp32 addends, summed sequentially on the CPU -- and the any-order allowance A per tensor.  Never modified."""
    c = SEAMS[name]
    g32 = GR.grads_ref(c["feats"], c["p12"], c["depth"], c["gsim"], GR.F32, ref_order=True)
    return g32, [a for a, _ in GR.summation_allowance(c["feats"], c["p12"], c["depth"], c["gsim"])]


@pytest.mark.parametrize("name", list(SEAMS))
def test_seams_atomic(name):
    """A deviation from the plain 8 e_ref rule, for the WINDOWS reason.  Against float64 SEAMS takes the WINDOWS rule -- the mean bound, the
    max printed -- on dRef and on the dSrc of the offset cases, and the plain rule on the dSrc of the identity cases: (W - 1) / 2 = 64.5 is no
    power of two, the reference's round trip moves a sample by ulps and the fp32 op-order restatement itself exceeds the plain max
    bound (test_costagg_presum_cpu.py asserts it; dRef, the unchanged kernel, sits at the same 2.1 x).  The max is held instead to
    that restatement: the same fp32 addends, summed in another order on either side, so at most 2 A apart (A the any-order allowance
    of ``warp_corr_grad_ref.summation_allowance``) plus one fp32 rounding of the result."""
    c = SEAMS[name]
    g64, e_ref, _ = own_ref(name)
    g32, allow = seam_op_order(name)
    full_ref = None
    for variant in (0, 2):
        gref, gsrc, counts = launch(name, False, variant, want_ref=True, counts=True)
        for k, g in enumerate([gref] + gsrc):
            tag = f"{name} presum v{variant} {'dRef' if k == 0 else f'dSrc{k - 1}'}"
            # the plain max bound where the op-order restatement itself obeys it: dSrc of the identity cases (0.73 / 0.77 of it on the CPU)
            table = "AFFINE" if k > 0 and name.endswith("-0_0") else "WINDOWS"
            T.compare(tag, table, g, g64[k], e_ref[k], 0.0, route="presum seams " + table)
            e, bound = GR.errors(g, g32[k].double())[0], 2.0 * allow[k] * 1.01 + 2.0 ** -23
            print(f"K1BPRESUM {tag}: to the fp32 op-order restatement {e:.3e}, bound 2 A + 2^-23 = {bound:.3e}")
            assert e <= bound, (tag, e, bound)
        assert counts == PR.predict(c["p12"], c["depth"], c["C"], cap_of(c["C"], False, variant), variant), (name, variant)
        if variant == 2:
            assert counts[0] > 0 and counts[1] > 0
        full_ref = gref if full_ref is None else full_ref
        assert same_bits(gref, full_ref)
    # dRef is the existing kernel: the existing entry's bits
    from dmvsnet_amd import ops
    plain_ref = torch.full_like(full_ref, float("nan"))
    ops.warp_corr_backward(dev_feats(name)[0], dev_feats(name)[1:], p12_of(name).cuda(), c["depth"].cuda(), c["gsim"].cuda(), plain_ref, [None])
    assert same_bits(full_ref, plain_ref)


@pytest.mark.parametrize("name", list(SEAMS))
def test_seams_deterministic(name):
    g32, allow = seam_op_order(name)
    for variant in range(4):
        assert_equals_det_entry(name, variant)
        counts, pred = counted(name, True, variant)
        assert counts == pred
    e, bound = GR.errors(plain(name, True)[0], g32[1].double())[0], allow[1] * 1.01 + 2.0 ** -23
    assert e <= bound, (name, e, bound)   # an exactly rounded sum against a sequential one: A


@pytest.mark.parametrize("name", ["views-c8-n16", "views-c32-n16"])
def test_three_of_sixteen_views(name):
    some = (0, 7, 15)
    for det, variants in ((True, (0, 3)), (False, (0, 2))):
        for variant in variants:
            gref, gsrc, _ = launch(name, det, variant, want=some, want_ref=True)   # launch asserts: the other thirteen untouched
            assert [v for v, g in enumerate(gsrc) if g is not None] == list(some)
            if det:
                for v in some:
                    assert same_bits(gsrc[v], plain(name, True)[v]), f"{name}: dSrc{v} depends on which other views are asked for"
            else:
                T.compare_all(name, [gref] + gsrc, route="presum")
    gref, gsrc, _ = launch(name, True, 1, want=(), want_ref=True)
    assert all(g is None for g in gsrc)


# ------------------------------------------------------------------------------------------------ through autograd
def grads_through(feats, cams, depth, gsim, **kw):
    from dmvsnet_amd import cost_agg
    leaves = [f.cuda().requires_grad_(True) for f in feats]
    sim = cost_agg(leaves, cams.cuda(), depth.cuda(), **kw)
    grads = torch.autograd.grad(sim, leaves, gsim.cuda())
    torch.cuda.synchronize()
    return list(grads)


def all_counts():
    import dmvsnet_amd.costagg as ca
    return dict(ca.launch_counts), dict(ca.det_launch_counts), dict(ca.presum_launch_counts)


NAMES2 = ("scatter-outlier-c8", "scatter-checker-c8")
NONE = {"bwd_ref": 0, "bwd_src_views": 0}


def batch_of_two(**kw):
    cs = [CASES[n] for n in NAMES2]
    return grads_through([torch.stack(fs) for fs in zip(cs[0]["feats"], cs[1]["feats"])], torch.stack([c["cams"] for c in cs]),
                         torch.stack([c["depth"] for c in cs]), torch.stack([c["gsim"] for c in cs]), **kw)


@pytest.mark.parametrize("det", (False, True))
def test_cost_agg_with_presum_on_a_batch_of_two(det):
    before = all_counts()
    got = batch_of_two(deterministic=det, presum=True)
    moved = tuple({k: a[k] - b[k] for k in a} for a, b in zip(all_counts(), before))
    assert moved == (NONE, NONE, {"bwd_ref": 2, "bwd_src_views": 4})
    before = all_counts()
    want = batch_of_two(deterministic=det)
    moved = tuple({k: a[k] - b[k] for k in a} for a, b in zip(all_counts(), before))
    assert moved == ((NONE, {"bwd_ref": 2, "bwd_src_views": 4}, NONE) if det else ({"bwd_ref": 2, "bwd_src_views": 4}, NONE, NONE))
    assert same_bits(got[0], want[0])   # dRef: the same kernel
    for b, name in enumerate(NAMES2):
        T.compare_all(name, [g[b] for g in got], route="presum cost_agg")
    if det:
        for v, (g, w) in enumerate(zip(got, want)):
            assert same_bits(g, w), f"gradient of view {v} differs from presum=False"


def test_diffcostagg_hands_the_keyword_on():
    from dmvsnet_amd import DiffCostAgg
    c = CASES[NAMES2[0]]
    leaves = [f[None].cuda().requires_grad_(True) for f in c["feats"]]
    before = all_counts()
    sim = DiffCostAgg("variance", 8, deterministic=True, presum=True)(leaves, c["cams"][None].cuda(), c["depth"][None].cuda(), stage_idx=0)
    grads = torch.autograd.grad(sim, leaves, c["gsim"][None].cuda())
    moved = tuple({k: a[k] - b[k] for k in a} for a, b in zip(all_counts(), before))
    assert moved == (NONE, NONE, {"bwd_ref": 1, "bwd_src_views": 2})
    for v, g in enumerate(plain(NAMES2[0], True)):
        assert same_bits(grads[1 + v][0], g), v


# ------------------------------------------------------------------------------------------------ a whole step
def test_a_whole_deterministic_step_is_the_same_bits_with_presum():
    import dmvsnet_amd as da
    import dmvsnet_amd.costagg as ca
    import train_step_ref as TS
    kw = dict(B=1, V=3, H=32, W=64, ndepths=TS.NDEPTHS, seed=0)   # the smallest configuration DiffMVSNet accepts
    gt, mask = TS.make_ground_truth(**kw)
    imgs, proj, dv = TS.make_inputs(**kw)
    sample = {"imgs": imgs.cuda(), "proj_matrices": {k: v.cuda() for k, v in proj.items()}, "depth_values": dv.cuda(),
              "depth": {k: v.cuda() for k, v in gt.items()}, "mask": {k: v.cuda() for k, v in mask.items()}}
    sd = TS.make_state_dict(0)
    runs = []
    for presum in (False, True):
        net = da.DiffMVSNet(list(TS.NDEPTHS), list(TS.RATIOS), deterministic=True, presum=presum)
        net.load_state_dict(sd, strict=True)
        net = net.cuda().train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        before = dict(ca.presum_launch_counts)
        res = da.train_step(net, opt, sample, TS.DLOSSW)
        torch.cuda.synchronize()
        assert (ca.presum_launch_counts["bwd_src_views"] > before["bwd_src_views"]) == presum
        runs.append((res, {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None},
                     {n: p.detach().clone() for n, p in net.named_parameters()}))
    (ra, ga, pa), (rb, gb, pb) = runs
    assert bool(torch.isfinite(ra["loss"])) and torch.equal(ra["loss"], rb["loss"])
    assert len(ga) > 0 and set(ga) == set(gb) and [n for n in ga if not torch.equal(ga[n], gb[n])] == []
    assert [n for n in pa if not torch.equal(pa[n], pb[n])] == []
    assert any(not torch.equal(pa[n].cpu(), sd[n]) for n in pa if n.endswith("prob.weight"))   # the step did move the weights
