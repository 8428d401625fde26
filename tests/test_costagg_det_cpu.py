"""CPU: the contract of K1b's deterministic mode, on its emulation tests/costagg_det_ref.py (no product code runs here).

  order      the emulation gives the same bits under random permutations of the addends; a sequential fp32 sum of the same addends
             under the same permutations does not, on CONTENTION -- the table can tell an order-dependent sum from an order-free one
  exact      on the cases tests/test_costagg_det_gpu.py compares bit for bit (``costagg_det_ref.exact_names``) fp32 forms the tap
             weights, the tap positions and the in-image tests exactly as float64 does, on EVERY such case
  parity     on every table but WINDOWS (its documented op-order exclusion) and EDGE_SHAPES (all zeros) each dSrc_v meets
             ``warp_corr_grad_ref.bounds_of`` against the float64 yardstick with allowance 0: on CONTENTION the plain bound, without
             the any-order summation allowance the atomic path needs
  derived    against the float64 sum of the same fp32 addends, per element: |err| <= n * 2^-(k+1) + 2^-24 * |sum| -- n roundings to
             the grid 2^-k of at most half a step each, and the one rounding of the result to fp32
  headroom   |q| <= 2^50 and |sum * 2^k| < 2^62 on every case; the zero-maximum and non-finite rules
  mutations  k without its headroom for the addend count (k = 62 - E) passes 2^62 on the all-collide CONTENTION cases; quantising by
             truncation changes the bits on every CONTENTION case once its gsim has the dynamic range of ``costagg_det_ref.wide_gsim``
             (on the plain cases nearly every addend sits on the grid and the rounding mode cannot show: printed, not asserted)."""
import functools

import pytest
import torch

import costagg_det_ref as DR
import warp_corr_grad_ref as GR
import warp_corr_ref as R
from warp_corr_grad_ref import F32, F64

CASES = GR.all_cases()
PARITY = [n for n, c in CASES.items() if c["table"] in GR.PLAIN_TABLES + ("CONTENTION",)]
CONTENTION = [n for n, c in CASES.items() if c["table"] == "CONTENTION"]
ALL_COLLIDE = [n for n in CONTENTION if n.endswith("-0_16_0_4")]


@functools.lru_cache(maxsize=None)
def p12_of(name):
    c = CASES[name]
    return c["p12"].clone() if c["p12"] is not None else R.p12_of_cams(c["cams"], F32)


def args_of(name):
    c = CASES[name]
    return c["feats"], p12_of(name), c["depth"], c["gsim"]


@functools.lru_cache(maxsize=None)
def emulated(name):
    return DR.emulate(*args_of(name))


def k_of(name):
    c = CASES[name]
    return DR.exponent_of(c["feats"][0], c["gsim"], *c["depth"].shape)


# ------------------------------------------------------------------------------------------------ order
@pytest.mark.parametrize("name", CONTENTION)
def test_emulation_is_order_free(name):
    base = emulated(name)
    for seed in (11, 22, 33):
        got = DR.emulate(*args_of(name), perm_seed=seed)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(base, got)), (name, seed)


def test_a_sequential_fp32_sum_is_not():
    differing = []
    for name in CONTENTION:
        base = DR.sequential_fp32(*args_of(name))
        if any(not torch.equal(a, b) for seed in (11, 22, 33) for a, b in zip(base, DR.sequential_fp32(*args_of(name), perm_seed=seed))):
            differing.append(name)
    print(f"K1BDET fp32 sums that depend on the order: {len(differing)} of {len(CONTENTION)} CONTENTION cases")
    assert differing, "the CONTENTION table cannot tell an order-dependent sum from an order-free one"


# ------------------------------------------------------------------------------------------------ exact cases
def test_exact_cases_are_the_stated_ones():
    names = DR.exact_names()
    assert set(CONTENTION) <= set(names) and len(set(names)) == len(names) == 26
    assert all(CASES[n]["p12"] is not None for n in names)   # literal projections: kernel and emulation get the same fp32 numbers


@pytest.mark.parametrize("name", DR.exact_names())
def test_fp32_forms_the_weights_exactly(name):
    c = CASES[name]
    for v in range(c["p12"].shape[0]):
        t32 = GR._taps(c["p12"][v].to(F32), c["depth"].to(F32), None, True)     # what the emulation (and the kernel) forms
        t64 = GR._taps(c["p12"][v].to(F64), c["depth"].to(F64), None, False)    # the yardstick's
        for (w32, in32, i32), (w64, in64, i64) in zip(t32, t64):
            assert torch.equal(in32, in64), name
            live = in64.reshape(-1)
            assert torch.equal(i32[live], i64[live]), name
            assert torch.equal(torch.where(in32, w32, torch.zeros(())).to(F64), torch.where(in64, w64, torch.zeros((), dtype=F64))), name


# ------------------------------------------------------------------------------------------------ parity and the derived bound
@functools.lru_cache(maxsize=None)
def ref_of(name):
    return GR.reference(CASES[name], p12_of(name))


@pytest.mark.parametrize("name", PARITY)
def test_parity_with_float64_without_allowance(name):
    g64, e_ref = ref_of(name)
    table = CASES[name]["table"]
    for v, got in enumerate(emulated(name)):
        f64, er = g64[1 + v], e_ref[1 + v]
        e = GR.errors(got, f64)
        bmax, bmean = GR.bounds_of(table, er, 0.0)
        print(f"K1BDET {name} emulation dSrc{v}: e max {e[0]:.3e} mean {e[1]:.3e}  e_ref max {er[0]:.3e} mean {er[1]:.3e}  "
              f"ratio max {e[0] / bmax:.3f} mean {e[1] / bmean:.3f}")
        assert torch.isfinite(got).all()
        if f64.abs().max().item() == 0.0:
            assert torch.equal(got, torch.zeros(got.shape)), (name, v)
            continue
        assert e[0] <= bmax and e[1] <= bmean, (name, v, e, er)


@pytest.mark.parametrize("name", PARITY)
def test_derived_bound_against_the_float64_sum_of_the_addends(name):
    k, state = k_of(name)
    assert state == "ok"
    for v, ((s, n), got) in enumerate(zip(DR.float64_sums(*args_of(name)), emulated(name))):
        err = (got.to(F64) - s).abs()
        bound = n * 2.0 ** -(k + 1) + 2.0 ** -24 * s.abs()
        worst = (err / bound.clamp(min=1e-300)).max().item()
        print(f"K1BDET {name} dSrc{v}: k {k}  max addends per element {int(n.max())}  worst err / bound {worst:.3f}")
        assert (err <= bound).all(), (name, v, worst)


# ------------------------------------------------------------------------------------------------ headroom and the special rules
@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c["table"] != "EDGE_SHAPES"])
def test_no_sum_reaches_2_62(name):
    k, state = k_of(name)
    assert state == "ok"
    C, H, W = CASES[name]["feats"][0].shape
    for idx, t, _ in DR.addends(*args_of(name)):
        q = DR.quantise(t, k)
        assert q.abs().max().item() <= 2 ** 50, name
        acc = torch.zeros((C, H * W), dtype=F64).index_add_(1, idx, q.to(F64))   # |q| <= 2^50: float64 sums them to 2^-2 of a unit
        assert acc.abs().max().item() < 2.0 ** 62, name


def test_zero_and_non_finite_rules():
    name = "contention-c8-0.5_0_0.5_0"
    feats, p12, depth, gsim = args_of(name)
    C, H, W = feats[0].shape
    zeros = [torch.zeros((C, H, W))] * p12.shape[0]
    assert DR.exponent_of(feats[0], torch.zeros_like(gsim), *depth.shape) == (0, "zero")
    assert DR.exponent_of(torch.zeros_like(feats[0]), gsim, *depth.shape) == (0, "zero")
    for a, b in zip(DR.emulate(feats, p12, depth, torch.zeros_like(gsim)), zeros):
        assert torch.equal(a, b)
    for a, b in zip(DR.emulate([torch.zeros_like(feats[0])] + list(feats[1:]), p12, depth, gsim), zeros):
        assert torch.equal(a, b)
    for bad in (float("inf"), float("-inf"), float("nan")):
        g = gsim.clone()
        g[1, 2, 3, 4] = bad
        assert all(torch.isnan(t).all() for t in DR.emulate(feats, p12, depth, g)), bad
        r = feats[0].clone()
        r[3, 2, 1] = bad
        assert all(torch.isnan(t).all() for t in DR.emulate([r] + list(feats[1:]), p12, depth, gsim)), bad
    # addends that may overflow fp32 count as non-finite
    assert DR.exponent_of(feats[0] * 2.0 ** 70, gsim * 2.0 ** 60, *depth.shape) == (0, "nan")
    # subnormal maxima are ordinary numbers
    k, state = DR.exponent_of(torch.full_like(feats[0], 2.0 ** -149), torch.full_like(gsim, 2.0 ** -140), *depth.shape)
    assert state == "ok" and k == 50 - (-149 - 140 + 2 - 2)


# ------------------------------------------------------------------------------------------------ mutations
def test_k_without_headroom_overflows_where_every_sample_collides():
    """L dropped from k, read as k = 62 - E (dropped from min(62 - L, 50) alone it would leave the cap of 50, which has headroom
    for 2^12 addends by itself and is no wrong kernel on these shapes).  Every all-collide case passes the 2^62 that
    ``test_no_sum_reaches_2_62`` holds the contract to -- the guarantee is gone; whether an int64 sum then wraps at 2^63 depends on the
    draw (these two reach 2^62.2 and 2^62.8 and do not: printed)."""
    assert len(ALL_COLLIDE) == 2
    for name in ALL_COLLIDE:
        k, _ = DR.exponent_of(CASES[name]["feats"][0], CASES[name]["gsim"], *CASES[name]["depth"].shape, mutation="no_headroom")
        C, H, W = CASES[name]["feats"][0].shape
        worst = 0.0
        for idx, t, _ in DR.addends(*args_of(name)):
            acc = torch.zeros((C, H * W), dtype=F64).index_add_(1, idx, DR.quantise(t, k).to(F64))
            worst = max(worst, acc.abs().max().item())
        g64 = GR.grads_ref(*args_of(name), F64)
        e = max(GR.errors(a, b)[0] for a, b in zip(DR.emulate(*args_of(name), mutation="no_headroom"), g64[1:]))
        print(f"K1BDET {name} no_headroom: max |sum * 2^k| = 2^{torch.log2(torch.tensor(worst)).item():.2f}  e_max of its int64 sum {e:.3e}")
        assert worst >= 2.0 ** 62, name


@pytest.mark.parametrize("name", CONTENTION)
def test_truncation_is_caught_by_the_bit_comparison(name):
    feats, p12, depth, gsim = args_of(name)
    plain = any(not torch.equal(a, b) for a, b in zip(DR.emulate(feats, p12, depth, gsim, mutation="truncate"), emulated(name)))
    print(f"K1BDET {name}: truncation changes the bits of the plain case: {plain}")
    wide = DR.wide_gsim(gsim)
    good = DR.emulate(feats, p12, depth, wide)
    assert all(torch.equal(a, b) for a, b in zip(good, DR.emulate(feats, p12, depth, wide, perm_seed=7))), name
    assert any(not torch.equal(a, b) for a, b in zip(DR.emulate(feats, p12, depth, wide, mutation="truncate"), good)), name
