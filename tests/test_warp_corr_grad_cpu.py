"""The float64 restatement of K1b's gradients (tests/warp_corr_grad_ref.py) against everything else that states them, the conditions
its case tables have to meet, and its power to tell a wrong backward kernel from a right one.  CPU only; no kernel runs here.

  tie        with a float64 p12 the restatement equals float64 autograd through costagg_grad_ref.cost_agg_f64 (grid_sample,
             normalised coordinates) on every camera case with H, W > 1, to a bound derived from float64 rounding on both sides
             (``_tie_bound``); its fp32 run and the reference's recorded gradients (tests/golden/op_costagg_grad.npz) are within
             the project's criterion of each other against the float64 run.
  edges      on one-row and one-column maps costagg_grad_ref.grads_f64 -- the reference's form -- gives exactly zero source gradients
             and a NaN dRef (ATen's NaN * 0); with zero padding applied tap by tap, as K1b applies it, every tensor is exactly zero.
  tables     exact coordinates on AFFINE and CONTENTION (with the reference's round trip in fp32), e_ref non-zero where the table
             says so, zero source gradients at the far AFFINE offsets, a partial last chunk, 16 views.
  op order   the fp32 restatement with the reference's normalise / un-normalise round trip -- K1b's op order -- obeys the plain
             bounds on every table but WINDOWS; there it obeys the mean bound and EXCEEDS the max bound: the ground for asserting
             the mean bound only on that table.
  mutations  nine wrong backward kernels, each over a bound of the criterion on a named case.
  exact      with a one-hot gsim the fp32 and the float64 restatement agree bit for bit where the GPU file's probes rely on it.

Every check prints its figures."""
import functools

import numpy as np
import pytest
import torch

import costagg_grad_ref as G
import warp_corr_grad_ref as GR
import warp_corr_ref as R

F64, F32 = torch.float64, torch.float32
CASES = GR.all_cases()
BY_TABLE = {t: [n for n, c in CASES.items() if c["table"] == t] for t in GR.TABLES}
CAMERA = [n for n, c in CASES.items() if c["cams"] is not None and c["table"] != "EDGE_SHAPES"]


def p12_of(case, dtype=F32):
    return case["p12"].to(dtype) if case["p12"] is not None else R.p12_of_cams(case["cams"], dtype)


@functools.lru_cache(maxsize=None)
def ref_of(name):
    """([float64 gradients], [(e_max, e_mean) of the fp32 restatement]): computed once, never modified."""
    return GR.reference(CASES[name], p12_of(CASES[name]))


@functools.lru_cache(maxsize=None)
def allowances_of(name):
    return GR.allowances(CASES[name], p12_of(CASES[name]))


def ratios(table, got, f64, e_ref, allowance):
    """(e_max / max bound, e_mean / mean bound) of one tensor with the PLAIN max bound on WINDOWS too (which the table does not
    assert); (0, 0) for an all-zero output of an identically zero yardstick, inf for any other."""
    e = GR.errors(got, f64)
    if f64.abs().max().item() == 0.0:
        return e
    b = GR.bounds_of("SHAPES" if table == "WINDOWS" else table, e_ref, allowance)
    return e[0] / b[0], e[1] / b[1]


def test_the_tables_hold_what_the_issue_lists():
    assert len(CASES) == 85 + 10 and len(BY_TABLE["CONTENTION"]) == 2 * len(GR.CONTENTION) == 10
    assert sum(len(v) for v in BY_TABLE.values()) == len(CASES)
    assert len(GR.MUTATIONS) == 9
    for name in BY_TABLE["CONTENTION"]:
        c = CASES[name]
        assert tuple(c["depth"].shape) == R.AFFINE_SHAPE and c["C"] in (8, 32) and len(c["feats"]) == 2
        assert set(c["depth"].reshape(-1).tolist()) == {256.0, 512.0, 1024.0}
    for name, c in CASES.items():
        assert c["gsim"].dtype == F32 and tuple(c["gsim"].shape) == (2,) + tuple(c["depth"].shape), name
        assert not torch.equal(c["gsim"], GR.gsim_of(name + "x", *c["depth"].shape)) and torch.equal(c["gsim"], GR.gsim_of(name, *c["depth"].shape))
    # a partial last chunk beside a full one (D = 9 and 13), 16 source views
    assert {tuple(CASES[n]["depth"].shape)[0] for n in BY_TABLE["SHAPES"]} >= {9, 13} and GR.DCH == 8
    assert {len(CASES[n]["feats"]) - 1 for n in BY_TABLE["VIEWS"]} >= {1, 16}
    s = GR.seam_case()
    assert tuple(s["depth"].shape) == (2, 9, 65) and s["p12"][0].tolist() == [1, 0, 1, 0, 1, 1, 0, 0, 1, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ ties
def _tie_bound(c, p12):
    """What two float64 statements of one gradient may differ by, per tensor, relative to its max-abs.  The two compute a sample's
    position by different routes of at most 16 rounded operations each on numbers no larger than the coordinate itself (projection,
    divide; here nothing more, there normalise and ATen's un-normalise), so for a sample that has a tap inside the image
    (|i| <= max(H, W)) the positions differ by at most delta = 2 * 16 * 2^-53 * max(H, W) px; a bilinear weight moves by at most
    2 delta (|dw / dtx|, |dw / dty| <= 1), an element by 2 delta * ``slope`` (sum |t_i / w_i| over its addends, from
    warp_corr_grad_ref.summation_allowance).  Summing the n <= 4 (V - 1) D H W addends in either order adds n * 2^-53 * slope at
    most.  Of the order of 1e-12."""
    D, H, W = c["depth"].shape
    delta = 2 * 16 * 2.0 ** -53 * max(H, W)
    n = 4 * p12.shape[0] * D * H * W
    return [(2 * delta + n * 2.0 ** -53) * slope for _, slope in GR.summation_allowance(c["feats"], p12, c["depth"], c["gsim"])]


@pytest.mark.parametrize("name", CAMERA)
def test_restatement_equals_float64_autograd(name):
    c = CASES[name]
    p12 = p12_of(c, F64)
    _, want = G.grads_f64([f[None] for f in c["feats"]], c["cams"][None], c["depth"][None], c["gsim"][None])
    got = GR.grads_ref(c["feats"], p12, c["depth"], c["gsim"], F64)
    assert len(got) == len(want) == len(c["feats"])
    for v, (a, b, bound) in enumerate(zip(got, want, _tie_bound(c, p12))):
        e = (a - b[0]).abs().max().item() / b.abs().max().item()
        print(f"TIE {name} grad{v}: |restatement - autograd| / max|grad| = {e:.3e}  bound {bound:.3e}")
        assert a.dtype == F64 and a.shape == b[0].shape and b.abs().max().item() > 0 and bound < 1e-9
        assert e <= bound, (name, v, e, bound)


@pytest.mark.parametrize("name", list(G.GOLDEN_CASES))
def test_fp32_restatement_and_recorded_gradients_agree(golden, name):
    """Against the float64 restatement (fp32 p12 from ``p12_of_cams``, the same for both runs): the reference's recorded gradients
    are within the criterion whose e_ref is the fp32 restatement's, and the fp32 restatement within the one whose e_ref is theirs."""
    g = golden("op_costagg_grad.npz")
    V = G.GOLDEN_CASES[name]["V"]
    feats = [torch.from_numpy(g[f"{name}.feat{v}"])[0] for v in range(V)]
    p12 = R.p12_of_cams(torch.from_numpy(g[f"{name}.proj"])[0], F32)
    depth, gsim = torch.from_numpy(g[f"{name}.depth"])[0], torch.from_numpy(g[f"{name}.gsim"])[0]
    g64 = GR.grads_ref(feats, p12, depth, gsim, F64)
    g32 = GR.grads_ref(feats, p12, depth, gsim, F32)
    for v in range(V):
        e32, eg = GR.errors(g32[v], g64[v]), GR.errors(torch.from_numpy(g[f"{name}.grad{v}"])[0], g64[v])
        print(f"GOLDEN {name} grad{v}: fp32 restatement max {e32[0]:.3e} mean {e32[1]:.3e}   recorded max {eg[0]:.3e} mean {eg[1]:.3e}")
        for a, b in ((eg, GR.bounds(e32)), (e32, GR.bounds(eg))):
            assert a[0] <= b[0] and a[1] <= b[1], (name, v, e32, eg)


@pytest.mark.parametrize("name", BY_TABLE["EDGE_SHAPES"])
def test_one_row_and_one_column_maps_have_zero_gradients(name):
    """The reference's form: (n - 1) / 2 = 0 makes the un-normalised coordinate NaN, every tap lies outside, nothing is sampled and
    nothing scattered.  costagg_grad_ref.grads_f64 -- float64 autograd through grid_sample -- says so for every SOURCE gradient:
    exactly zero.  For the REFERENCE view it cannot: stock ATen's CPU grid_sample forms weight * masked value = NaN * 0 in its
    forward, so the warped volume, sim and with them dRef = gsim * warped come out all NaN (asserted: NaN everywhere, no finite
    non-zero element), where zero padding -- a tap outside counts zero on its own -- gives 0.  The restatement with the reference's
    round trip, which applies exactly that rule, is exactly zero in every tensor and both precisions: that is what K1b is held to in
    the GPU file.  The pixel-coordinate restatement itself is not zero there (printed)."""
    c = CASES[name]
    sim, grads = G.grads_f64([f[None] for f in c["feats"]], c["cams"][None], c["depth"][None], c["gsim"][None])
    for v, g in enumerate(grads[1:], 1):
        assert torch.isfinite(g).all() and torch.equal(g, torch.zeros_like(g)), (name, v)
    assert torch.isnan(sim).all() and torch.isnan(grads[0]).all(), name
    for dt in (F64, F32):
        for g in GR.grads_ref(c["feats"], p12_of(c), c["depth"], c["gsim"], dt, ref_order=True):
            assert torch.equal(g, torch.zeros_like(g)), name
    pix = GR.grads_ref(c["feats"], p12_of(c), c["depth"], c["gsim"], F64)
    print(f"EDGE {name}: grads_f64 dSrc all zero, dRef all NaN (ATen's NaN * 0); round-trip restatement all zero; pixel-coordinate restatement max|grad| {max(g.abs().max().item() for g in pix):.3e}")


# ------------------------------------------------------------------------------------------------ table conditions
def _round_trip(i, n):
    return ((i / ((n - 1) / 2) - 1.0) + 1.0) / 2.0 * (n - 1)


def test_affine_and_contention_coordinates_are_exact():
    """fp32 with the reference's round trip == float64 without it, bit for bit after the clamp to [-1, W] x [-1, H]."""
    for name in BY_TABLE["AFFINE"] + BY_TABLE["CONTENTION"] + [GR.SEAM_NAME]:
        c = CASES.get(name) or GR.seam_case()
        D, H, W = c["depth"].shape
        x32, y32 = R.coordinates(c["p12"][0], c["depth"])
        x64, y64 = R.coordinates(c["p12"][0].double(), c["depth"].double())
        assert x32.dtype == F32 and x64.dtype == F64
        for a32, a64, n in ((x32, x64, W), (y32, y64, H)):
            assert torch.equal(a32.clamp(-1, n).double(), a64.clamp(-1, n)), name
            assert torch.equal(_round_trip(a32, n).clamp(-1, n).double(), a64.clamp(-1, n)), name


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n]["table"] != "EDGE_SHAPES"])
def test_e_ref_per_gradient_tensor(name):
    c = CASES[name]
    g64, e_ref = ref_of(name)
    for v, (g, e) in enumerate(zip(g64, e_ref)):
        print(f"E_REF {name} grad{v}: e_ref max {e[0]:.3e} mean {e[1]:.3e}   max|f64| {g.abs().max().item():.3f}")
        assert torch.isfinite(g).all() and np.isfinite(e).all()
        if c["nonzero_e_ref"]:
            assert e[0] > 0 and e[1] > 0 and g.abs().max().item() > 0.1
        if c["table"] in ("AFFINE", "WINDOWS"):
            assert e[0] < 4 * 2.0 ** -23 and e[1] < 4 * 2.0 ** -23   # below the criterion's floor
        if c["table"] == "CONTENTION":
            assert e[0] < 1e-6 and e[1] < 4 * 2.0 ** -23             # near it, with up to 891 addends per element
    if c["table"] == "AFFINE":
        far = (c["p12"][0, 2].item(), c["p12"][0, 5].item()) in ((33, 0), (0, 9), (1e9, -1e9))
        assert far == (c["p12"][0, 2].item() >= R.AFFINE_SHAPE[2] or c["p12"][0, 5].item() >= R.AFFINE_SHAPE[1])
        assert all((g.abs().max().item() == 0.0) == far for g in g64), name   # every sample outside: both gradients identically zero
    if c["table"] == "CONTENTION":
        a = allowances_of(name)
        print(f"E_REF {name}: summation allowance dRef {a[0]:.3e} dSrc {a[1]:.3e}")
        if name.split("-")[2] == "0_16_0_4":   # 891 addends per element
            assert 2e-4 <= a[1] <= 2e-3
        assert all(0 < x <= 2e-3 for x in a)


# ------------------------------------------------------------------------------------------------ op order
@functools.lru_cache(maxsize=None)
def _ref_order_ratios(name):
    c = CASES[name]
    g64, e_ref = ref_of(name)
    got = GR.grads_ref(c["feats"], p12_of(c), c["depth"], c["gsim"], F32, ref_order=True)
    return [ratios(c["table"], a, b, e, al) for a, b, e, al in zip(got, g64, e_ref, allowances_of(name))]


@pytest.mark.parametrize("table", [t for t in GR.TABLES if t not in ("EDGE_SHAPES", "WINDOWS")])
def test_reference_op_order_obeys_the_plain_bounds(table):
    worst = [0.0, 0.0]
    for name in BY_TABLE[table]:
        for v, r in enumerate(_ref_order_ratios(name)):
            assert r[0] <= 1.0 and r[1] <= 1.0, (name, v, r)
            worst = [max(worst[0], r[0]), max(worst[1], r[1])]
    print(f"OP ORDER {table}: worst e / bound of the fp32 restatement with the round trip: max {worst[0]:.3f} mean {worst[1]:.3f}")


def test_reference_op_order_exceeds_the_plain_max_bound_on_windows():
    """The ground for warp_corr_grad_ref.bounds_of leaving the max bound out on WINDOWS, and only there.  Were this to stop being
    true, the exclusion would have lost its ground and this test says so."""
    over, worst_mean = {}, 0.0
    for name in BY_TABLE["WINDOWS"]:
        rs = _ref_order_ratios(name)
        over[name] = max(r[0] for r in rs)
        worst_mean = max(worst_mean, max(r[1] for r in rs))
    n = sum(v > 1.0 for v in over.values())
    print(f"OP ORDER WINDOWS: over the plain max bound on {n} of {len(over)} cases, worst {max(over.values()):.2f} x; "
          f"worst mean / bound {worst_mean:.3f}")
    assert worst_mean <= 1.0
    assert n >= 1 and n >= len(over) // 2 and max(over.values()) >= 2.0, over


# ------------------------------------------------------------------------------------------------ sensitivity
@functools.lru_cache(maxsize=None)
def _excess(mutation, name):
    """max over the tensors of max(e_max / bound, e_mean / bound) of the mutated fp32 restatement, under the bounds the GPU file
    asserts for the case's table (no max bound on WINDOWS)."""
    c = CASES[name]
    g64, e_ref = ref_of(name)
    got = GR.grads_ref(c["feats"], p12_of(c), c["depth"], c["gsim"], F32, mutation)
    worst = 0.0
    for a, b, e, al in zip(got, g64, e_ref, allowances_of(name)):
        r = ratios(c["table"], a, b, e, al)
        worst = max(worst, r[1] if c["table"] == "WINDOWS" and b.abs().max().item() > 0 else max(r))
    return worst


# mutation -> cases on which it has to show (all of them checked; the best one printed)
SHOWS_ON = {
    "w01_w10_swapped": ("shape-c16-v3-d3-9x33", "scatter-checker-c8", "affine-c8-0.25_8.75", "window0-c8-9x36"),
    "border_clamp": ("shape-c8-v3-d5-17x70", "affine-c8--0.5_0.5", "special-behind-c8"),
    "x1in_wm1": ("affine-c8-0.25_8.75", "affine-c32-0.5_-0.5"),
    "groups_swapped": ("shape-c8-v2-d1-2x2", "views-c32-n16", "contention-c8-0_16_0_4"),
    "divisor_c": ("shape-c32-v2-d4-7x31", "affine-c8-0_0", "window3-c16-16x68"),
    "chunk_tail_dropped": ("shape-c8-v3-d9-10x40", "shape-c32-v3-d13-9x65", "shape-c16-v3-d3-9x33"),
    "last_view_dropped_dref": ("views-c8-n16", "views-c32-n9", "shape-c8-v3-d8-8x64"),
    "dsrc_view_shifted": ("views-c8-n16", "scatter-outlier-c8", "special-turned"),
    "align_corners_false": ("shape-c8-v3-d8-8x64", "window5-c32-20x92", "contention-c32-0_16.5_0_3.25"),
}


@pytest.mark.parametrize("mutation", GR.MUTATIONS)
def test_mutations_exceed_the_bound(mutation):
    """Each wrong backward kernel -- w01 and w10 swapped in the scatter, an outside tap clamped to the border and added, x1in tested
    against W - 1, the correlation groups swapped, divisor C, the last plane of a partial 8-plane chunk dropped from dSrc, the last
    source view dropped from dRef, dSrc of view v written into view v - 1, align_corners=False coordinates -- is at least 20 x over
    the max or the mean bound on every case named for it."""
    assert set(SHOWS_ON) == set(GR.MUTATIONS)
    per_case = {n: _excess(mutation, n) for n in SHOWS_ON[mutation]}
    best = max(per_case, key=per_case.get)
    print(f"MUTATION {mutation}: {per_case[best]:.1f} x a bound on {best}; " + "  ".join(f"{n} {v:.1f}" for n, v in per_case.items()))
    assert min(per_case.values()) >= 20.0, (mutation, per_case)


def test_the_unmutated_restatement_is_not_caught():
    """The other half of sensitivity: the fp32 restatement itself is at 1/8 of the bound (or below the floor) everywhere."""
    for name in ("shape-c8-v3-d9-10x40", "views-c8-n16", "affine-c8-0.25_8.75", "contention-c8-0_16_0_4"):
        c = CASES[name]
        g64, e_ref = ref_of(name)
        got = GR.grads_ref(c["feats"], p12_of(c), c["depth"], c["gsim"], F32)
        for a, b, e, al in zip(got, g64, e_ref, allowances_of(name)):
            assert max(ratios(c["table"], a, b, e, al)) <= 0.25, name


# ------------------------------------------------------------------------------------------------ exactness of the probes
def test_one_hot_gradients_are_exact_in_fp32():
    """dSrc on the AFFINE offsets that are multiples of 0.5 (weights 0, 1/4, 1/2, 1; 2 / C a power of two), dRef on the integer ones
    (one tap of weight 1): fp32 == float64 bit for bit, at most four non-zero taps per channel of the probe's group, zeros elsewhere."""
    assert set(GR.INT_OFFSETS) < set(GR.HALF_OFFSETS) < set(R.AFFINE_OFFSETS) and len(GR.HALF_OFFSETS) == 8
    n = 0
    for name, c, src_exact, ref_exact in GR.probe_cases():
        D, H, W = c["depth"].shape
        for d, y, x in GR.probe_voxels(D, H, W):
            for g in (0, 1):
                gs = GR.one_hot(D, H, W, g, d, y, x)
                a = GR.grads_ref(c["feats"], c["p12"], c["depth"], gs, F32)
                b = GR.grads_ref(c["feats"], c["p12"], c["depth"], gs, F64)
                assert src_exact and torch.equal(a[1].double(), b[1]), (name, d, y, x, g)
                assert (a[1][g::2] != 0).sum((1, 2)).max().item() <= 4 and not a[1][1 - g::2].any(), (name, d, y, x, g)
                if ref_exact:
                    assert torch.equal(a[0].double(), b[0]) and (a[0] != 0).sum().item() <= c["C"] // 2, (name, d, y, x, g)
                    elsewhere = a[0].clone()
                    elsewhere[g::2, y, x] = 0.0
                    assert not elsewhere.any(), (name, d, y, x, g)
                n += 1
    print(f"PROBES: {n} one-hot gradients exact in fp32")
