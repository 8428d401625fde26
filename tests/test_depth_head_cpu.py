"""The yardstick of the depth head's forward (tests/depth_head_ref.py) held to the recorded reference outputs, to the oracle and to
ATen; the conditions its case tables claim; and the mistakes the criterion tells apart.  CPU only: no kernel runs here.

  restatement  float64 ``head`` against tests/golden/op_depthnet.npz (the reference's own fp32 outputs: they must obey the criterion
               with e_ref from the fp32 oracle), against the oracle run in float64 (1e-12) and ``prob_conv`` against F.conv3d in
               float64 (1e-12).
  tables       widths / heights / depths per kernel form, the tile, block and plane residues they are there for, row classes and
               parities, the share of mid-range confidences, the bit-equal expectations of SPECIAL (c) / (d), disjoint impulses.
  mutations    each mistake of the issue's list built into the fp32 restatement on table cases: its distance to the yardstick is
               at least 20 times bound_of(e_ref).  The smallest ratio is printed."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import depth_head_ref as R
import head_grad_ref as G

F64, F32 = R.F64, R.F32


def _close64(a, b, tol=1e-12):
    return (a - b).abs().max().item() <= tol * max(b.abs().max().item(), 1e-300)


# ------------------------------------------------------------------------------------------------ restatement
def test_head_against_the_recorded_reference_outputs(golden):
    """Stored: what the reference computed in fp32.  The float64 restatement on the same inputs is its exact-arithmetic value, so
    each stored tensor lies within the criterion of it, e_ref taken from the fp32 oracle (the stored outputs ARE an fp32 run of the
    reference: they must not need more room than any other fp32 implementation gets)."""
    g = {k: torch.from_numpy(v) for k, v in golden("op_depthnet.npz").items()}
    itv = g["interval"]
    runs = ((g["logits"][0], g["depth_values"][0], 1.0, 0, {"dsp": "dsp", "sel": "hyps", "conf": "conf", "prob": "prob"}),
            (g["logits_c"][0], g["hyps"][0], 5.0, 1, {"dsp": "dsp_refine", "sel": "depth", "conf": "conf_refine"}))
    for logits, hyp, alpha, mode, names in runs:
        y = R.head(logits.double(), hyp.double(), itv.double(), alpha, mode)
        o = R.oracle_head(logits, hyp, itv, alpha, mode)
        for k, stored in names.items():
            e, b = R.errors(g[stored][0], y[k]), R.bounds(R.errors(o[k], y[k]))
            print(f"HEAD recorded {stored}: e {e[0]:.3e} / {e[1]:.3e}  bound {b[0]:.3e} / {b[1]:.3e}")
            assert e[0] <= b[0] and e[1] <= b[1], (stored, e, b)


@pytest.mark.parametrize("D,H,W", [(4, 7, 9), (8, 5, 12), (5, 6, 7), (32, 3, 5)])
def test_head_against_the_oracle_in_float64(D, H, W):
    for kind in R.DEPTHS:
        c = R.k4_case(D, H, W, kind)
        L, hyp, itv = c["logits"].double(), R.yardstick_planes(c), c["interval"].double()
        for mode, alpha in R.K4_RUNS:
            y, o = R.head(L, hyp, itv, alpha, mode), R.oracle_head(L, hyp, itv, alpha, mode)
            m = R.head_mutated(L, hyp, itv, alpha, mode, None)
            for k in y:
                assert y[k].dtype == F64 and o[k].dtype == F64
                assert _close64(y[k], o[k]), (kind, mode, alpha, k)
                assert _close64(m[k], y[k]), ("head_mutated(None)", kind, mode, alpha, k)
            sel, conf = R.tail(y["dsp"], itv, mode)
            assert torch.equal(sel, y["sel"]) and torch.equal(conf, y["conf"])


@pytest.mark.parametrize("Cin,D,H,W", [(8, 5, 17, 36), (2, 3, 4, 5), (16, 1, 1, 1), (8, 9, 6, 33)])
def test_prob_conv_against_aten_in_float64(Cin, D, H, W):
    x, w = R.prob_case(Cin, D, H, W)
    want = F.conv3d(x.double().unsqueeze(0), w.double(), padding=1)[0]
    assert _close64(R.prob_conv(x, w), want)


def test_affine_planes_are_the_kernels_roundings_in_fp32():
    c = R.k4_case(8, 5, 12, "affine")
    d = torch.arange(8, dtype=F32).view(-1, 1, 1)
    assert torch.equal(c["hyp"], c["base"][None] + d * c["interval"])
    assert R.errors(c["hyp"], R.yardstick_planes(c))[0] <= R.EPS32


# ------------------------------------------------------------------------------------------------ table conditions
def _v4_owned(W):
    """Columns owned by each tile column of the V4 form: tile bx owns x in 32 bx - 31 .. 32 bx, cut to the map."""
    nx = (W - 1 + 31) // 32 + 1
    return [len(range(max(32 * bx - 31, 0), min(32 * bx, W - 1) + 1)) for bx in range(nx)]


def test_prob_table_hits_what_it_claims():
    plain = [s for s in R.PROB_SHAPES if s[0] == 8 and not s[4]]
    assert 14 <= len(plain) <= 18
    assert {s[3] for s in plain if s[3] % 4 == 0} == set(R.PROB_W_V4) and {s[3] for s in plain if s[3] % 4} == set(R.PROB_W_DWORD)
    assert {s[2] for s in plain} == set(R.PROB_H) and {s[1] for s in plain} == set(R.PROB_D)
    for need in ((1, 1, 1), (1, 1, 4), (5, 17, 36), (9, 33, 68)):
        assert (8,) + need + (False,) in R.PROB_SHAPES
    # each loader form sees every height and every depth class: below / at / above the 16-row tile, the 4-plane block
    for form in (0, 1):
        mine = [s for s in plain if (s[3] % 4 == 0) == bool(form)]
        assert {min(s[2], 18) // 16 + (s[2] > 16) for s in mine} >= {0, 1, 2}
        assert {s[1] % 4 for s in mine} >= {0, 1, 2} and any(s[1] > 4 for s in mine) and any(s[1] > 8 for s in mine)
    # V4 tiles: at W = 4 tile 0 owns x = 0 alone and tile 1 the other three; at 32 / 64 the last tile is one column short of a full
    # one (the issue's "owns one column" holds for the FIRST tile, at every width); at 36 / 68 it owns three
    assert _v4_owned(4) == [1, 3] and _v4_owned(32) == [1, 31] and _v4_owned(64) == [1, 32, 31]
    assert _v4_owned(36) == [1, 32, 3] and _v4_owned(68) == [1, 32, 32, 3]
    assert all(sum(_v4_owned(W)) == W for W in R.PROB_W_V4)
    assert sorted(s[0] for s in R.PROB_SHAPES if s[0] != 8) == [2, 16]
    mis = [s for s in R.PROB_SHAPES if s[4]]
    assert len(mis) == 1 and mis[0][3] % 4 == 0 and mis[0][0] == 8


def test_fused_table_hits_what_it_claims():
    assert 8 <= len(R.FUSED_SHAPES) <= 12
    assert {s[0] for s in R.FUSED_SHAPES} == set(R.FUSED_D) and {s[2] for s in R.FUSED_SHAPES} == set(R.FUSED_W)
    assert {s[1] for s in R.FUSED_SHAPES} == set(R.FUSED_H)
    for D in R.FUSED_D:    # both z-block counts meet one-tile, ragged and multi-tile maps in both directions
        mine = [s for s in R.FUSED_SHAPES if s[0] == D]
        assert {s[2] for s in mine} == set(R.FUSED_W) and {s[1] for s in mine} == set(R.FUSED_H)
    # the exchange pairs rows r and r + 8 of a tile: maps with the second row dead (H - 16 by <= 8) and live
    assert any(s[1] % 16 in range(1, 9) for s in R.FUSED_SHAPES) and any(s[1] % 16 in (0, 15) for s in R.FUSED_SHAPES)
    reasons = [(c, d, w, m) for c, d, _, w, m in R.FUSED_DECLINED]
    assert sum(d not in (4, 8) for _, d, _, _ in reasons) == 2 and sum(w % 4 != 0 for _, _, w, _ in reasons) == 1
    assert sum(c % 2 for c, _, _, _ in reasons) == 1 and sum(m for _, _, _, m in reasons) == 1
    for c, d, w, m in reasons:   # one reason each
        assert (d not in (4, 8)) + (w % 4 != 0) + (c % 2) + m == 1


def test_k4_table_hits_what_it_claims():
    assert {R.K4_FORM[s[0]] for s in R.K4_SHAPES} == {"reg4", "reg8", "split", "generic"}
    assert {s[0] for s in R.K4_SHAPES} == set(R.K4_FORM)
    thread = [s for s in R.K4_SHAPES if R.K4_FORM[s[0]] != "split"]
    split = [s for s in R.K4_SHAPES if R.K4_FORM[s[0]] == "split"]
    assert {s[2] for s in thread} == set(R.K4_W_THREAD) and {s[2] for s in split} == set(R.K4_W_SPLIT)
    assert {s[1] for s in R.K4_SHAPES} == set(R.K4_H)
    for group, block in ((thread, 256), (split, 64)):
        res = {s[2] % block for s in group}
        assert {1, block - 1, 0} <= res                      # one pixel, one short of a block, exactly a block ...
        assert any(s[2] > block and s[2] % block for s in group)   # ... and more than one block with a ragged last one
        assert {s[1] for s in group} == set(R.K4_H)
    for form in ("reg4", "reg8", "split", "generic"):
        mine = [s for s in R.K4_SHAPES if R.K4_FORM[s[0]] == form]
        classes = [{y & 3 for y in range(s[1])} for s in mine]
        assert any(c == {0, 1, 2, 3} for c in classes), form          # every row class y & 3 (hence both parities) ...
        assert any(c != {0, 1, 2, 3} for c in classes), form          # ... and an entry that lacks some, on purpose
        assert any(s[2] >= 2 for s in mine)                           # both column parities
    assert {y & 3 for y in range(1)} == {0}


@pytest.mark.parametrize("D,H,W", R.K4_SHAPES)
def test_confidence_is_mid_range_on_a_quarter_of_each_map(D, H, W):
    """Otherwise a wrong confidence formula could hide in the saturated tail.  Exception, stated: affine planes at D = 1 are the
    base plane itself, the four expectations coincide (std == 0) and interval / 1e-5 saturates the sigmoid: conf == 1 there."""
    low = 1.0
    for kind in R.DEPTHS:
        for mode, alpha in R.K4_RUNS[:2]:
            y, _ = R.k4_reference(D, H, W, kind, mode, alpha)
            if kind == "affine" and D == 1:
                assert torch.equal(y["conf"], torch.ones_like(y["conf"]))
                continue
            share = R.mid_share(y["conf"])
            low = min(low, share)
            assert share >= 0.25, (D, H, W, kind, alpha, share)
    print(f"HEAD mid-range confidence share D={D} {H}x{W}: >= {low:.2f}")


@pytest.mark.parametrize("D,H,W", R.FUSED_SHAPES)
def test_fused_confidence_is_mid_range_on_a_quarter_of_each_map(D, H, W):
    for kind in ("synth", "affine"):
        y, e_ref = R.fused_reference(D, H, W, kind, 0, 1.0)
        assert R.mid_share(y["conf"]) >= 0.25, (D, H, W, kind, R.mid_share(y["conf"]))
        assert torch.isfinite(y["dsp"]).all() and all(e == e for pair in e_ref.values() for e in pair)


def test_special_identical_channels_give_bit_equal_expectations_in_fp32():
    """SPECIAL (c), (d): with four identical channels the four fp32 expectations are the same bits, the spread is 0 and the
    confidence 2 (sigmoid(2) - 0.5) at interval 2e-5 and exactly 1 at 2.65.  True of the fp32 restatement at every pixel.  Of the
    ATen oracle it is true at all but a few pixels per map (measured 0 .. 0.3 %): its softmax takes the vector body or the scalar
    tail of exp depending on where a channel starts in memory, and the two differ in the last bit.  So the premise is asserted for
    the restatement everywhere and for the oracle on at least 99 % of each map, the consequence wherever the premise holds; the
    GPU file asserts the premise on the kernels' own output (they run the same instructions for every channel)."""
    for D, H, W in ((4, 7, 255), (32, 7, 63), (5, 7, 255)):
        c = R.k4_case(D, H, W, "synth")
        L = R.special_identical(c)
        for mode, alpha in R.K4_RUNS[:2]:
            m = R.head_mutated(L, c["hyp"], torch.tensor(2e-5), alpha, mode, None)
            assert all(torch.equal(m["dsp"][k], m["dsp"][0]) for k in range(1, 4))
            assert (m["conf"].double() - R.CONF_AT_Z2).abs().max().item() <= 4 * R.EPS32
            o = R.oracle_head(L, c["hyp"], torch.tensor(2e-5), alpha, mode)
            same = (o["dsp"] == o["dsp"][0]).all(0)
            assert same.double().mean().item() >= 0.99
            assert (o["conf"][same].double() - R.CONF_AT_Z2).abs().max().item() <= 4 * R.EPS32
            o = R.oracle_head(L, c["hyp"], torch.tensor(2.65), alpha, mode)
            assert torch.equal(o["conf"][same], torch.ones_like(o["conf"][same]))
            y = R.head(L.double(), c["hyp"].double(), torch.tensor(2.65, dtype=F64), alpha, mode)
            stack = y["sel"] if mode == 1 else y["sel"][0]
            assert _close64(stack, y["dsp"][0])     # every six-stack entry, every checkerboard pick: the expectation itself


def test_special_one_hot_and_equal_logits():
    D, H, W = 8, 5, 256
    c = R.k4_case(D, H, W, "synth")
    L, hot = R.special_one_hot(D, H, W)
    y = R.head(L.double(), c["hyp"].double(), c["interval"].double(), 5.0, 1)
    assert torch.isfinite(y["prob"]).all() and torch.equal(y["dsp"], c["hyp"].double()[None].expand(4, -1, -1, -1).gather(1, hot[:, None])[:, 0])
    y = R.head(R.special_equal(D, H, W).double(), c["hyp"].double(), c["interval"].double(), 1.0, 0)
    assert _close64(y["prob"], torch.full_like(y["prob"], 1.0 / D))


def test_impulses_have_disjoint_supports_and_sit_on_every_edge():
    sites = R.impulse_sites()
    D, H, W = R.IMPULSE_VOLUME
    for (_, *p), (_, *q) in itertools.combinations(sites, 2):
        assert max(abs(a - b) for a, b in zip(p, q)) >= 3, (p, q)    # 3 x 3 x 3 supports share no voxel, whatever the channels
    assert {s[1] for s in sites} == set(R.IMPULSE_Z) and {s[2] for s in sites} == set(R.IMPULSE_Y) and {s[3] for s in sites} == set(R.IMPULSE_X)
    assert {s[0] for s in sites} == set(range(8)) and len(sites) >= 16
    assert R.IMPULSE_Z[-1] == D - 1 and R.IMPULSE_Y[-1] == H - 1 and R.IMPULSE_X[-1] == W - 1
    # the response of the yardstick: every output voxel is one weight (exactly representable) or 0
    x, w = R.impulse_case()
    y = R.prob_conv(x, w)
    assert torch.equal(y.float().double(), y) and int((y != 0).sum()) > 0
    assert set(y.unique().tolist()) <= set(w.double().unique().tolist()) | {0.0}


# ------------------------------------------------------------------------------------------------ mutations
def _ratio(mut, f64, e_ref):
    return R.errors(mut, f64)[0] / R.bound_of(e_ref[0])


@pytest.mark.parametrize("mutation", R.PROB_MUTATIONS)
def test_prob_mutations_are_caught(mutation):
    low = float("inf")
    for Cin, D, H, W, _ in ((8, 5, 17, 36, False), (8, 9, 33, 68, False), (8, 9, 17, 65, False)):
        x, w = R.prob_case(Cin, D, H, W)
        f64 = R.prob_conv(x, w)
        e_ref = R.errors(R.oracle_conv(x, w), f64)
        assert R.errors(R.prob_conv(x, w, F32), f64)[0] <= R.bound_of(e_ref[0])     # the unmutated fp32 restatement passes
        low = min(low, _ratio(R.prob_conv(x, w, F32, mutation), f64, e_ref))
    print(f"HEAD mutation {mutation}: smallest ratio to the bound {low:.3g}")
    assert low >= R.MUTATION_RATIO


MUTATION_CASES = ((4, 7, 255), (8, 5, 256), (32, 7, 63), (32, 2, 130), (5, 7, 255))


def _applies(mutation, D, H, W, mode, alpha):
    """Where the mistake changes anything at all."""
    return {"alpha_dropped": alpha != 1.0, "last_block_w1": W % 64 > 1, "q2_plain": mode == 0 and H >= 3, "window_parity": mode == 0,
            "mode1_swap": mode == 1 and H >= 2}.get(mutation, True)


@pytest.mark.parametrize("mutation", [m for m in R.HEAD_MUTATIONS if m != "no_eps"])
def test_head_mutations_are_caught(mutation):
    """The largest ratio over the output tensors of a run (one failing tensor fails the test), the smallest over the runs."""
    low, runs = float("inf"), 0
    for (D, H, W), kind in itertools.product(MUTATION_CASES, ("synth", "unit")):
        c = R.k4_case(D, H, W, kind)
        for mode, alpha in R.K4_RUNS:
            if not _applies(mutation, D, H, W, mode, alpha):
                continue
            y, e_ref = R.k4_reference(D, H, W, kind, mode, alpha)
            plain = R.head_mutated(c["logits"], c["hyp"], c["interval"], alpha, mode, None)
            assert all(R.errors(plain[k], y[k])[0] <= R.bound_of(e_ref[k][0]) for k in y), "the unmutated fp32 restatement passes"
            m = R.head_mutated(c["logits"], c["hyp"], c["interval"], alpha, mode, mutation)
            low = min(low, max(_ratio(m[k], y[k], e_ref[k]) for k in y))
            runs += 1
    print(f"HEAD mutation {mutation}: smallest ratio to the bound {low:.3g} over {runs} runs")
    assert runs >= 4 and low >= R.MUTATION_RATIO


def test_missing_1e5_is_caught_on_special_c_alone():
    """Elsewhere std >> 1e-5 and the term is invisible: on the mutation cases the mistake stays under the bound.  With four identical
    channels and interval 2e-5 it turns 2 (sigmoid(2) - 0.5) into 1."""
    c = R.k4_case(8, 5, 256, "synth")
    itv = torch.tensor(2e-5)
    L = R.special_identical(c)
    y = R.head(L.double(), c["hyp"].double(), itv.double(), 1.0, 0)
    e_ref = R.errors(R.oracle_head(L, c["hyp"], itv, 1.0, 0)["conf"], y["conf"])
    m = R.head_mutated(L, c["hyp"], itv, 1.0, 0, "no_eps")
    ratio = _ratio(m["conf"], y["conf"], e_ref)
    print(f"HEAD mutation no_eps on SPECIAL (c): ratio to the bound {ratio:.3g}")
    assert ratio >= R.MUTATION_RATIO
    y, e_ref = R.k4_reference(8, 5, 256, "synth", 0, 1.0)
    m = R.head_mutated(c["logits"], c["hyp"], c["interval"], 1.0, 0, "no_eps")
    assert _ratio(m["conf"], y["conf"], e_ref["conf"]) < 1.0


def test_caps_hold_for_the_fp32_oracle():
    """The conditional caps are derived, not fitted: the fp32 oracle's own tail, fed its own expectations, stays under them."""
    for (D, H, W), kind in itertools.product(MUTATION_CASES, R.DEPTHS):
        c = R.k4_case(D, H, W, kind)
        for mode, alpha in R.K4_RUNS:
            o = R.oracle_head(c["logits"], c["hyp"], c["interval"], alpha, mode)
            sel, conf = R.tail(o["dsp"].double(), c["interval"].double(), mode)
            if mode == 1:
                assert torch.equal(o["sel"].double(), sel)
            else:
                assert ((o["sel"].double() - sel).abs() <= R.sel_cap(o["dsp"], sel)).all(), (D, H, W, kind)
            assert ((o["conf"].double() - conf).abs() <= R.conf_cap(o["dsp"], c["interval"])).all(), (D, H, W, kind, alpha)


def test_criterion_constants():
    assert R.FACTOR == 8 and R.EPS32 == 2.0 ** -23 and R.bound_of(0.0) == 16 * R.EPS32 and R.bound_of(5 * R.EPS32) == 40 * R.EPS32
    assert G.select is R.select and G.softmax_expect is R.softmax_expect
    z = torch.linspace(0.01, 40, 40000, dtype=F64)
    assert (z ** 2 / 2 / torch.cosh(z / 2) ** 2).max().item() < R.CONF_SLOPE
