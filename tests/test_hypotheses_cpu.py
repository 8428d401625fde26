"""The float64 restatement of the hypothesis planes (tests/hypotheses_ref.py) against everything else that states them, and the
conditions its case tables have to meet.  CPU only; no kernel runs here.

  golden     the restatement in fp32 against tests/golden/op_hypotheses.npz (recorded from the reference), with the tolerances
             tests/test_gpu_parity.py uses for the same arrays.
  oracle     the restatement in float64 against oracle.depth_hypotheses + F.interpolate(scale_factor=2, mode="bilinear") in float64,
             over the whole case tables: linear sampling to 1e-12 relative; inverse sampling to fp32 rounding, because the oracle
             casts its inverse-depth planes to fp32 (and builds the first stage's linspace in fp32).
  table      every float64 plane of a later-stage case is positive and at least 0.25 x the smallest ``last`` of the case, and
             ``last`` spreads over at least 20 plane spacings.
  mutations  align_corners=True, nearest upsample, parity from the fine pixel, n - 1 in depth_interval, interval = pix, spans swapped
             between the parities, the linspace's upper half off by one: each moves the float64 result by more than the GPU
             criterion's bound of the case, on every case where it can differ.  See ``test_mutations_exceed_the_bound``."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hypotheses_ref as R
from oracle import dmvs_oracle as O

F64, F32 = torch.float64, torch.float32
FIRST, LATER = R.first_cases(), R.later_cases()
UP2 = [k for k, c in LATER.items() if c["up"] == 2]


def close(got, want, atol, what):
    np.testing.assert_allclose(got.numpy(), want, atol=atol, rtol=0.0, err_msg=what)


@pytest.mark.parametrize("inv", [0, 1])
def test_fp32_restatement_reproduces_the_golden(golden, inv):
    g = golden("op_hypotheses.npz")
    dv = R.depth_values("synth192")
    s, i = R.first(dv, 8, 6, 8, bool(inv), F32)
    close(s, g[f"first_inv{inv}"][0], 2e-4, "first")
    close(i, g[f"first_inv{inv}_itv"], 1e-5, "first interval")
    last = torch.from_numpy(g["last"][0])
    s, i = R.later(last, dv, 2.0, 8, bool(inv), 2, F32)
    close(s, g[f"later_inv{inv}_up"][0], 3e-4, "later")
    close(i, g[f"later_inv{inv}_itv"], 1e-5, "later interval")
    if not inv:   # the affine form: plane 0 is the base, base + d * interval the volume
        b, i = R.first(dv, 8, 6, 8, False, F32)
        close(b[0], g["first_inv0"][0][0], 2e-4, "first base")
        close(R.affine_volume(b[0], i, 8), g["first_inv0"][0], 3e-4, "first affine volume")
        close(s[0], g["later_inv0_up"][0][0], 3e-4, "later base")
        close(R.affine_volume(s[0], torch.from_numpy(g["later_inv0_itv"]), 8), g["later_inv0_up"][0], 4e-4, "later affine volume")


def test_depth_values_match_synth():
    from dmvsnet_amd import synth
    assert torch.equal(R.depth_values("synth192"), synth.synth_depth_values()[0])
    assert R.depth_values("synth2").tolist() == [R.depth_values("synth192")[0].item(), R.depth_values("synth192")[-1].item()]
    small = R.depth_values("small48")
    assert small.numel() == 48 and small[0].item() == 2.0 and small[-1].item() == 10.0


@pytest.mark.parametrize("name", list(FIRST))
def test_first_stage_equals_the_oracle_in_float64(name):
    c = FIRST[name]
    for inverse in (False, True):
        want, want_i = O.depth_hypotheses(c["dv"].double()[None], c["D"], None, (c["H"], c["W"]), inverse)
        got, got_i = R.first(c["dv"], c["D"], c["H"], c["W"], inverse)
        a, b, same = R.finite_part(want[0], got)
        # inverse: the oracle's torch.linspace runs in fp32 (a few roundings of 1 / lo, the step and the sum), then one cast
        tol = 8 * R.EPS32 if inverse else 1e-12
        e, e_i = R.rel_dist(a, b), R.rel_dist(want_i, got_i)
        print(f"ORACLE first {name} inv={int(inverse)}: planes {e:.3e}  interval {e_i:.3e}  (tolerance {tol:.3e})")
        assert same and got.shape == (c["D"], c["H"], c["W"]) and e <= tol and e_i <= (R.EPS32 if inverse else 1e-12)
        # the one case with an end at 0 (first_cases) is the only one with a non-finite plane, and only in inverse depth
        assert bool(torch.isfinite(got).all()) == (not (inverse and name == "5-3x257-small48")), name


@pytest.mark.parametrize("name", list(LATER))
def test_later_stages_equal_the_oracle_in_float64(name):
    c = LATER[name]
    last, pix = c["last"].double(), R.pix_interval(c["dv"], c["ratio"])
    for inverse in (False, True):
        want, want_i = O.depth_hypotheses(last[None], c["D"], pix, None, inverse)
        want = want.double()   # (inverse: fp32-rounded values; the resize itself runs in float64)
        if c["up"] == 2:
            want = F.interpolate(want, scale_factor=2, mode="bilinear")
        got, got_i = R.later(c["last"], c["dv"], c["ratio"], c["D"], inverse, c["up"])
        tol = R.EPS32 if inverse else 1e-12   # one rounding to fp32 is 2^-24 relative per plane; the taps' weights sum to 1
        e, e_i = R.rel_dist(want[0], got), R.rel_dist(want_i, got_i)
        print(f"ORACLE later {name} inv={int(inverse)}: planes {e:.3e}  interval {e_i:.3e}  (tolerance {tol:.3e})")
        assert got.shape == (c["D"], c["up"] * c["h"], c["up"] * c["w"]) and e <= tol and e_i <= tol


@pytest.mark.parametrize("name", list(LATER))
def test_table_conditions(name):
    """Far from the pole of 1 / lo (so the fp32 run is a fair yardstick) and never smooth."""
    c = LATER[name]
    pix = R.pix_interval(c["dv"], c["ratio"]).item()
    lo, hi = c["last"].min().item(), c["last"].max().item()
    lo_t, w_t = R.LAST_RANGE["small48" if name.endswith("small48") else "synth192"]
    width = max(w_t, R.MIN_SPACINGS * pix)
    assert lo_t <= lo and hi <= lo_t + width * (1 + 1e-6)
    if c["h"] * c["w"] >= 64:   # the draws do fill the width
        assert hi - lo >= 0.9 * width
    for inverse in (False, True):
        vol, _ = R.later(c["last"], c["dv"], c["ratio"], c["D"], inverse, c["up"])
        floor = vol.min().item()
        print(f"TABLE {name} inv={int(inverse)}: pix {pix:.4f}  last {lo:.3f} .. {hi:.3f} ({(hi - lo) / pix:.1f} spacings)  "
              f"min plane {floor:.3f}  (0.25 min last {0.25 * lo:.3f})")
        assert torch.isfinite(vol).all() and floor > 0 and floor >= 0.25 * lo


def test_fp32_restatement_is_a_fair_yardstick():
    """e_ref of every compared tensor, printed; nothing is required of it beyond being finite and small against a plane spacing
    (a table whose fp32 run were off by a spacing would make 8 e_ref meaningless)."""
    worst = 0.0
    for name, c in LATER.items():
        for inverse in (False, True):
            f64, _ = R.later(c["last"], c["dv"], c["ratio"], c["D"], inverse, c["up"])
            f32, _ = R.later(c["last"], c["dv"], c["ratio"], c["D"], inverse, c["up"], F32)
            e = R.rel_dist(f32, f64)
            worst = max(worst, e)
            spacing = R.pix_interval(c["dv"], c["ratio"]).item() / f64.abs().max().item()
            assert f32.dtype == F32 and e < 1e-3 * spacing, (name, inverse, e, spacing)
    for name, c in FIRST.items():
        for inverse in (False, True):
            a, b, same = R.finite_part(R.first(c["dv"], c["D"], c["H"], c["W"], inverse, F32)[0],
                                       R.first(c["dv"], c["D"], c["H"], c["W"], inverse)[0])
            assert same, name
            worst = max(worst, R.rel_dist(a, b))
    print(f"YARDSTICK worst e_ref {worst:.3e}")
    assert worst < 1e-5


# ------------------------------------------------------------------------------------------------ mutations
def corner_taps(n_out, n_in, dtype):
    """align_corners=True."""
    s = torch.arange(n_out, dtype=dtype) * ((n_in - 1) / (n_out - 1))
    i0 = s.floor().long().clamp(max=n_in - 1)
    return i0, (i0 + 1).clamp(max=n_in - 1), s - i0.to(dtype)


def nearest2(vol):
    return vol.repeat_interleave(2, 1).repeat_interleave(2, 2)


def mutated_later(c, inverse, what):
    """(planes, interval, affine volume or None) of one mutation of ``R.later`` in float64; ``what`` None: the restatement."""
    last = c["last"].double()
    D, up = c["D"], c["up"]
    pix = R.pix_interval(c["dv"], c["ratio"], n=c["dv"].numel() - 1 if what == "n-1" else None)
    vn, vp = R.spans(last, pix, D, inverse)
    itv = pix if what == "itv=pix" else (D * pix) / (D - 1)
    if what == "swapped":
        vn, vp = vp, vn
    resize = {"corners": lambda v: R.upsample2(v, corner_taps), "nearest": nearest2}.get(what, R.upsample2) if up == 2 else (lambda v: v)
    if what == "fine-parity":
        vol = torch.where(R.parity(up * c["h"], up * c["w"]), resize(vn), resize(vp))
    else:
        vol = resize(torch.where(R.parity(c["h"], c["w"]), vn, vp))
    return vol, itv, (None if inverse else R.affine_volume(vol[0], itv, D))


def can_differ(what, c):
    """From the formulas alone, never from the results."""
    if what in ("corners", "nearest"):   # a resize of one pixel is that pixel whatever the taps
        return c["up"] == 2 and c["h"] * c["w"] > 1
    if what == "fine-parity":            # at up == 1 the fine pixel is the coarse one
        return c["up"] == 2
    return True


def test_mutations_exceed_the_bound():
    """Each mutation against the unmutated float64 restatement, relative distance over the bound the GPU test grants that case
    (bound_of(e_ref), e_ref from the fp32 run).  Compared tensors: the planes; for "itv=pix" the interval and the affine volume
    (the planes do not read the interval).

    Skipped, from the formulas: the two resize mutations on the one-pixel map (up2-1x1, both depth ranges) and on the 12 up == 1
    cases, "fine-parity" on the 12 up == 1 cases.  D == 2 is NOT skipped for "swapped": its spans are last - 2 pix .. last and last ..
    last + 2 pix, which differ.

    The linspace split.  Moving the split n // 2 of the first stage's inverse-depth linspace by one (odd D: the middle element counted
    from the other end) is an identity in exact arithmetic -- a + step * i == b - step * (n - 1 - i) -- so it moves the float64 result
    by a rounding (asserted: <= 1e-14) and no criterion can see it: either split is right.  What CAN be wrong there is the upper
    half counted back from the wrong index, b - step * (n - i): one whole step; that is the mutation asserted above the bound, on
    every first-stage case (D == 2 included: its upper half is the far end itself)."""
    skipped, worst = [], {}
    for what in ("corners", "nearest", "fine-parity", "n-1", "itv=pix", "swapped"):
        for name, c in LATER.items():
            if not can_differ(what, c):
                skipped.append((what, name))
                continue
            for inverse in (False, True):
                f64 = mutated_later(c, inverse, None)
                mut = mutated_later(c, inverse, what)
                f32, f32_i = R.later(c["last"], c["dv"], c["ratio"], c["D"], inverse, c["up"], F32)
                if what == "itv=pix":
                    pairs = [(mut[1], f64[1], R.bound_of(R.rel_dist(f32_i, f64[1])))]
                    if not inverse:
                        e_ref = R.rel_dist(R.affine_volume(f32[0], f32_i, c["D"]), f64[2])
                        pairs.append((mut[2], f64[2], R.bound_of(e_ref)))
                else:
                    pairs = [(mut[0], f64[0], R.bound_of(R.rel_dist(f32, f64[0])))]
                for m, f, bound in pairs:
                    ratio = R.rel_dist(m, f) / bound
                    worst[what] = min(worst.get(what, float("inf")), ratio)
                    assert ratio > 1.0, (what, name, inverse, R.rel_dist(m, f), bound)
    for name, c in FIRST.items():
        D = c["D"]
        f64 = R.first(c["dv"], D, c["H"], c["W"], True)[0]
        f32 = R.first(c["dv"], D, c["H"], c["W"], True, F32)[0]
        a, b, _ = R.finite_part(f32, f64)
        bound = R.bound_of(R.rel_dist(a, b))
        if D % 2:
            moved = R.first(c["dv"], D, c["H"], c["W"], True, mid=D // 2 + 1)[0]
            ok = torch.isfinite(moved) & torch.isfinite(f64)   # (the case with an end at 0: inf - inf on one side of the split only)
            assert R.rel_dist(moved[ok], f64[ok]) <= 1e-14, (name, R.rel_dist(moved[ok], f64[ok]))
        off = one_off_first(c)
        a, b, same = R.finite_part(off, f64)
        ratio = R.rel_dist(a, b) / bound
        worst["upper-half"] = min(worst.get("upper-half", float("inf")), ratio)
        assert ratio > 1.0, ("upper-half", name, R.rel_dist(a, b), bound)
    for what, ratio in worst.items():
        print(f"MUTATION {what}: smallest distance / bound over the cases {ratio:.3e}")
    print(f"MUTATION skipped ({len(skipped)}): " + ", ".join(f"{w}:{n}" for w, n in skipped))
    assert len(skipped) == 14 + 14 + 12 and set(worst) == {"corners", "nearest", "fine-parity", "n-1", "itv=pix", "swapped", "upper-half"}


def one_off_first(c):
    """First stage, inverse depth, with the linspace's upper half counted back from b one index too far."""
    def lin(a, b, n):
        i = torch.arange(n, dtype=a.dtype)
        step = (b - a) / (n - 1)
        return torch.where(i < n // 2, a + step * i, b - step * (n - i))

    dv, D = c["dv"].double(), c["D"]
    itv = (dv[-1] - dv[0]) / (D - 1)
    vn = 1 / lin(1 / (dv[0] - itv), 1 / (dv[-1] - itv), D)
    vp = 1 / lin(1 / (dv[0] + itv), 1 / (dv[-1] + itv), D)   # (the recomputed interval equals itv in exact arithmetic)
    return torch.where(R.parity(c["H"], c["W"]), vn.view(D, 1, 1), vp.view(D, 1, 1)).expand(D, c["H"], c["W"])
