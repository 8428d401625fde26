"""The yardstick of the regularisation networks (tests/costreg_ref.py) held to the oracle in float64; what its case tables and its
launch table claim; and the mistakes of the chaining code the criterion tells apart.  CPU only: no kernel runs here.

  restatement  ``net_f64`` against oracle.cost_reg on float64 tensors, logits and the six intermediates of either branch (1e-12 of
               max-abs: the same arithmetic up to association); ``heads_f64`` against oracle._expectation in float64.
  tables       every claim a shape is in FULL_SHAPES / REFINE_SHAPES for, from the restated geometry (regconv_ref.geometry,
               winoconv_ref's tile and unit functions): level shapes, the levels with W % 4 != 0, the level that reaches depth 8,
               the layers that run through @d1, the fusable heads.
  launches     ``expected_launches`` has 1 + 2 x 10 entries plus declines, and every layer the entry its claim names.
  e_ref        finite, non-zero, below 16 eps on every shape (a condition on the recipe's inputs); all values printed.
  mutations    every mistake of costreg_ref.MUTATIONS sits above the bound the GPU file uses; the smallest ratio is printed."""
import pytest
import torch

import costreg_ref as C
import regconv_ref as RC
import winoconv_ref as W

F64, F32 = C.F64, C.F32
EPS = 2.0 ** -23
ALL = [(r, s) for r in (False, True) for s in C.shapes_of(r)]
IDS = [("refine" if r else "full") + "-" + "x".join(map(str, s)) for r, s in ALL]


def _close64(a, b, tol=1e-12):
    assert a.dtype == F64 and b.dtype == F64 and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return (a - b).abs().max().item() <= tol * max(b.abs().max().item(), 1e-300)


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("refine,shape", ALL, ids=IDS)
def test_net_against_the_oracle_in_float64(refine, shape):
    sd = C.state_dict()
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    x = C.sim_volume(refine, *shape)
    want, wlev = C.oracle_net(sd64, C.PREFIX[refine], x.double(), refine, keys=True)
    r = C.reference(refine, *shape)
    assert tuple(r["f64"].shape) == (4,) + shape
    assert _close64(r["f64"], want)
    assert set(r["levels"]) == {f"{b}.{k}" for b in C.BRANCHES for k in C.LEVEL_KEYS} == set(wlev)
    lv = C.levels(refine, *shape)
    for b in C.BRANCHES:
        for k, l, ch in zip(C.LEVEL_KEYS, (0, 1, 2, 2, 1, 0), (8, 16, 32, 32, 16, 8)):
            assert tuple(r["levels"][f"{b}.{k}"].shape) == (ch,) + lv[l], (b, k)
            assert _close64(r["levels"][f"{b}.{k}"], wlev[f"{b}.{k}"]), (b, k)
    # the stepwise oracle chain of costreg_ref IS oracle.cost_reg
    o32, _ = C.oracle_net(sd, C.PREFIX[refine], x, refine, keys=True)
    assert torch.equal(o32, r["oracle32"])
    # the branches are not interchangeable and the concatenation is small, huge
    assert not _close64(r["f64"][:2], r["f64"][2:], 1e-3)
    twin = dict(sd)
    twin.update({k.replace("cosR_huge", "cosR_small"): v for k, v in sd.items() if "cosR_huge" in k})     # huge's weights in both
    both = C.net_f64(twin, C.PREFIX[refine], x, refine)
    assert torch.equal(both[:2], r["f64"][2:]) and torch.equal(both[2:], r["f64"][2:])


def test_heads_against_the_oracle_in_float64():
    from oracle import dmvs_oracle as O
    for refine, shape in C.fused_cases():
        D, H, Wd = shape
        r = C.reference(refine, *shape)
        base, step, vol = C.planes(*shape)
        alpha = C.ALPHA[refine]
        want = O._expectation(r["f64"][None], vol.double()[None], alpha)[1][0]
        got = C.heads_f64(r["f64"], vol, alpha)
        assert tuple(got.shape) == (4, H, Wd) and _close64(got, want), shape
        # the affine form: the same planes (d * interval is exact in fp32 for d < 8, so the fp32 volume IS base + d * interval)
        assert torch.equal(vol.double(), base.double()[None] + torch.arange(D, dtype=F64).view(-1, 1, 1) * step.double())
        assert torch.equal(C.heads_f64(r["f64"], (base, step), alpha), got)
        assert got.min().item() >= C.DEPTH_MIN - 1e-9 and got.max().item() <= vol.max().item() + 1e-9     # a convex combination
        f64, e_ref = C.heads_reference(refine, *shape)
        assert torch.equal(f64, got)
        print(f"COSTREG heads {'refine' if refine else 'full'} {shape}: e_ref max {e_ref[0] / EPS:.2f} eps mean {e_ref[1] / EPS:.2f} eps")
        assert 0 < e_ref[0] < 16 * EPS and 0 < e_ref[1] <= e_ref[0]
    assert [s for r, s in C.fused_cases() if not r] == [(8, 8, 8), (8, 24, 40), (8, 40, 136)]
    assert [s for r, s in C.fused_cases() if r] == list(C.REFINE_SHAPES)


# ------------------------------------------------------------------------------------------------ tables
def test_level_shapes():
    assert all(n % 8 == 0 for s in C.FULL_SHAPES for n in s)
    assert all(s[0] == 4 and s[1] % 8 == 0 and s[2] % 8 == 0 for s in C.REFINE_SHAPES)
    for refine, (D, H, Wd) in ALL:
        lv = C.levels(refine, D, H, Wd)
        assert lv[0] == (D, H, Wd) and lv[1] == (D // 2, H // 2, Wd // 2) and lv[2] == (D // 4, H // 4, Wd // 4)
        assert lv[3] == (1 if refine else D // 8, H // 8, Wd // 8)
        # the product's own out_shape rules (regconv_ref restates them per row)
        assert RC.out_shape("conv1", *lv[0]) == lv[1] and RC.out_shape("conv3", *lv[1]) == lv[2]
        assert RC.out_shape("conv5_2d" if refine else "conv5", *lv[2]) == lv[3]
        assert RC.out_shape("conv7_2d" if refine else "conv7", *lv[3]) == lv[2]
        assert RC.out_shape("conv9", *lv[2]) == lv[1] and RC.out_shape("conv11", *lv[1]) == lv[0]


def test_which_levels_have_unaligned_widths_and_reach_depth_8():
    ragged = {(r, s): tuple(l for l in range(4) if C.levels(r, *s)[l][2] % 4) for r, s in ALL}
    assert ragged == {
        (False, (8, 8, 8)): (2, 3), (False, (8, 24, 40)): (2, 3), (False, (16, 16, 48)): (3,), (False, (32, 8, 72)): (2, 3),
        (False, (8, 40, 136)): (2, 3), (True, (4, 8, 8)): (2, 3), (True, (4, 24, 40)): (2, 3), (True, (4, 16, 136)): (2, 3),
        (True, (4, 40, 72)): (2, 3)}
    # levels 0 and 1 are never ragged (W % 8 == 0): K3w's conv0 form and K3z / K3w on conv2 never decline on the tables' shapes
    assert all(0 not in v and 1 not in v for v in ragged.values())
    deep = [(r, s) for r, s in ALL if C.levels(r, *s)[1][0] >= C.ZMARCH_MIN_DEPTH]
    assert deep == [(False, (16, 16, 48)), (False, (32, 8, 72))]
    assert C.ZMARCH_MIN_DEPTH == W.ZMARCH_MIN_DEPTH == 8
    assert {s: C.d1_layers(False, *s) for s in C.FULL_SHAPES} == {
        (8, 8, 8): ["conv6"], (8, 24, 40): ["conv6"], (16, 16, 48): [], (32, 8, 72): [], (8, 40, 136): ["conv6"]}
    assert all(C.d1_layers(True, *s) == ["conv4"] for s in C.REFINE_SHAPES)


def _entries(refine, shape, setting, fused=False):
    """{layer: entry} of the small branch (the huge one is asserted to be its copy) and conv0."""
    L = C.expected_launches(refine, *shape, setting, fused)
    assert all(code == 0 for _, _, code in L) and len(L) == 21
    assert L[1:11] == L[11:]
    names = ("conv0", "conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "conv7", "conv9", "conv11", "prob")
    return {n: e for n, (e, _, _) in zip(names, L[:11])}, {n: d for n, (_, d, _) in zip(names, L[:11])}


def test_claims_of_the_full_table():
    # (8, 8, 8): one tile column and row per level in the Winograd forms and K3r, one tile column in K3; conv6 on one voxel via @d1
    lv = C.levels(False, 8, 8, 8)
    assert lv == ((8, 8, 8), (4, 4, 4), (2, 2, 2), (1, 1, 1))
    assert W.wino_counts("conv0", *lv[0])[:2] == (1, 1) and W.wino_counts("conv2", *lv[1])[:2] == (1, 1)
    assert all(len({u[:2] for u in us}) <= 1 for us in W.coarse_units("conv4", *lv[2]).values())
    for name, l in (("conv1", 0), ("conv3", 1), ("conv5", 2), ("conv7", 3), ("conv9", 2), ("conv11", 1)):
        for form in RC.forms_of(name):
            assert RC.geometry(name, form, *lv[l])["nx"] == 1
    e, d = _entries(False, (8, 8, 8), "auto")
    assert e["conv6"] == "conv3d_coarse" and d["conv6"] == (64, 64, 1, 1, 1, 1)
    assert d["conv4"] == (32, 32, 2, 2, 2, 3) and d["conv7"] == (64, 32, 1, 1, 1, 3)
    assert C.fusable(8, 8)
    # (8, 24, 40): K3r with the dword loader and the dword store at both of its levels, odd extents at the bottom
    lv = C.levels(False, 8, 24, 40)
    assert lv[2] == (2, 6, 10) and lv[3] == (1, 3, 5)
    assert W.coarse_v4_st4(lv[2][2]) == (False, False) and W.coarse_v4_st4(lv[3][2]) == (False, False)
    assert lv[3][1] % 2 == 1 and lv[3][2] % 2 == 1
    e, d = _entries(False, (8, 24, 40), "auto")
    assert e["conv4"] == e["conv6"] == "conv3d_coarse" and d["conv4"][-1] == 3 and d["conv6"][2:] == (1, 3, 5, 1)
    assert C.fusable(8, 40)
    # (16, 16, 48): conv2 on depth 8 -> K3z; conv6 on two planes, each with one dead depth tap; head not fusable
    lv = C.levels(False, 16, 16, 48)
    assert lv[1] == (8, 8, 24) and lv[3] == (2, 2, 6)
    e, d = _entries(False, (16, 16, 48), "auto")
    assert e["conv2"] == "conv3d_zmarch" and d["conv2"] == (16, 16, 8, 8, 24, 3)
    assert e["conv6"] == "conv3d_coarse" and d["conv6"] == (64, 64, 2, 2, 6, 3)
    assert W.coarse_dead("conv6", 2, 0) == 1 and W.coarse_dead("conv6", 2, 1) == 2
    assert not C.fusable(16, 48) and (False, (16, 16, 48)) not in C.fused_cases()
    assert _entries(False, (16, 16, 48), "no_zmarch")[0]["conv2"] == "conv3d_wino"
    # the one place of the tables where conv4 reaches K3w (W/4 = 12); conv6 has no level with W % 4 == 0 anywhere
    assert _entries(False, (16, 16, 48), "no_coarse")[0]["conv4"] == "conv3d_wino"
    assert all(_entries(r, s, "no_coarse")[0]["conv6"] == "conv3d_mfma" for r, s in ALL)
    # (32, 8, 72): conv2 on depth 16; H/8 = 1, W/8 = 9
    lv = C.levels(False, 32, 8, 72)
    assert lv[1][0] == 16 and lv[3] == (4, 1, 9)
    assert _entries(False, (32, 8, 72), "auto")[0]["conv2"] == "conv3d_zmarch"
    assert len({(s[0], s[1]) for segs in W.zmarch_plan(*lv[1]).values() for s in segs}) == -(-lv[1][2] // 8) * -(-lv[1][1] // 8)
    # (8, 40, 136): several tiles per row at full resolution, ragged against 32, 64 and 128; 68, 34, 17 below
    lv = C.levels(False, 8, 40, 136)
    assert [l[2] for l in lv] == [136, 68, 34, 17]
    assert all(136 % t not in (0,) and 136 > t for t in (32, 64, 128))
    assert W.wino_counts("conv0", *lv[0])[:2] == (5, 5) and W.wino_counts("conv2", *lv[1])[0] == 3
    assert RC.geometry("conv1", "small", *lv[0])["nx"] == 3 and RC.geometry("conv11", "only", *lv[1])["x_last"] == 4
    assert C.fusable(8, 136)


def test_claims_of_the_refine_table():
    assert C.levels(True, 4, 8, 8) == ((4, 8, 8), (2, 4, 4), (1, 2, 2), (1, 1, 1))
    for s in C.REFINE_SHAPES:
        e, d = _entries(True, s, "auto")
        lv = C.levels(True, *s)
        assert lv[2][0] == lv[3][0] == 1
        assert e["conv2"] == "conv3d_wino" and d["conv2"][-1] == 3          # depth 2: below ZMARCH_MIN_DEPTH
        assert e["conv4"] == "conv3d_coarse" and d["conv4"] == (32, 32) + lv[2] + (1,)      # @d1
        assert d["conv5"][-1] == d["conv6"][-1] == d["conv7"][-1] == 1 and d["conv9"][-1] == d["conv11"][-1] == 3
        assert C.fusable(s[0], s[2])
        # K3w's conv2 row on a two-plane volume takes its ZSKIP instantiation
        assert W.wino_zskip("conv2", lv[1][0])
    lv = C.levels(True, 4, 24, 40)
    assert lv[2][1:] == (6, 10) and lv[3][1:] == (3, 5) and lv[2][2] % 4 and lv[3][2] % 4
    lv = C.levels(True, 4, 16, 136)
    assert W.wino_counts("conv0", *lv[0])[0] == 5 and 136 % 32 and W.wino_counts("conv2", *lv[1])[0] == 3
    lv = C.levels(True, 4, 40, 72)
    assert lv[3][2] == 9 and W.wino_counts("conv0", *lv[0])[1] == 5 and W.wino_counts("conv2", *lv[1])[1] > 1
    assert RC.geometry("conv1", "big", *lv[0])["ny"] > 1


# ------------------------------------------------------------------------------------------------ launches
@pytest.mark.parametrize("setting", C.SETTINGS)
def test_expected_launches(setting):
    s1 = {"auto": "conv3d_wino", "no_zmarch": "conv3d_wino", "no_coarse": "conv3d_wino", "no_wino": "conv3d_mfma",
          "mfma": "conv3d_mfma", "direct": "conv3d_direct"}[setting]
    k3 = "conv3d_direct" if setting == "direct" else "conv3d_mfma"
    for refine, shape in ALL:
        e, d = _entries(refine, shape, setting)
        lv = C.levels(refine, *shape)
        assert e["conv0"] == s1 and d["conv0"] == (2, 16) + shape + (3,)
        assert all(e[n] == k3 for n in ("conv1", "conv3", "conv5", "conv7", "conv9", "conv11"))
        assert e["prob"] == "conv3d_direct" and d["prob"] == (8, 2) + shape + (3,)
        for n, l in (("conv2", 1), ("conv4", 2), ("conv6", 3)):
            assert d[n][2:5] == lv[l]
            if setting in ("no_wino", "mfma", "direct"):
                assert e[n] == k3
            elif n == "conv2":
                zm = setting != "no_zmarch" and lv[1][0] >= 8
                assert e[n] == ("conv3d_zmarch" if zm else "conv3d_wino")
            elif setting == "no_coarse":
                assert e[n] == ("conv3d_wino" if lv[l][2] % 4 == 0 else "conv3d_mfma")
            else:
                assert e[n] == "conv3d_coarse"
        d1 = C.d1_layers(refine, *shape)
        for n in ("conv2", "conv4", "conv6"):
            kd = 1 if (n in d1 and setting != "direct") or (refine and n == "conv6") else 3
            assert d[n][-1] == kd, (refine, shape, n)
        fam = C.families(C.expected_launches(refine, *shape, setting, False))
        assert fam.count("prob_head") == 2 and fam[10] == fam[20] == "prob_head"
        assert set(fam[:10]) == {"conv3d_direct" if setting == "direct" else "conv3d_mfma"}
        if C.fusable(shape[0], shape[2], setting):
            ef, df = _entries(refine, shape, setting, fused=True)
            assert ef["prob"] == "prob_regress" and df == d and {k: v for k, v in ef.items() if k != "prob"} == \
                {k: v for k, v in e.items() if k != "prob"}
    assert not C.fusable(8, 8, "direct")


def test_expected_launches_lists_declined_calls():
    """No tensor of a run is misaligned and no width of levels 0 / 1 is ragged on the tables' shapes, so no run of the GPU file has a
    declined call; the rule is in the table all the same, as ops.conv3d walks it: K3z and K3w decline, K3 runs."""
    L = C.expected_launches(False, 16, 16, 48, "auto", False, aligned=False)
    assert len(L) == 21 + sum(code != 0 for _, _, code in L) == 21 + 1 + 2 * 2
    assert [(e, c) for e, _, c in L[:2]] == [("conv3d_wino", C.EUNSUPPORTED), ("conv3d_mfma", 0)]
    assert [(e, c) for e, _, c in L[3:6]] == [("conv3d_zmarch", C.EUNSUPPORTED), ("conv3d_wino", C.EUNSUPPORTED), ("conv3d_mfma", 0)]
    assert C.families(L) == C.families(C.expected_launches(False, 16, 16, 48, "mfma", False))
    # a ragged width on a deep level (not a table shape): K3z is asked and declines, `auto` reads K3w's plan and does not ask it
    L = C.expected_launches(False, 16, 16, 40, "auto", False)
    assert [(e, c) for e, _, c in L[2:4]] == [("conv3d_zmarch", 0), ("conv3d_mfma", 0)]
    L = C.expected_launches(False, 16, 16, 44, "auto", False)
    assert [(e, c) for e, _, c in L[2:5]] == [("conv3d_zmarch", C.EUNSUPPORTED), ("conv3d_mfma", 0), ("conv3d_mfma", 0)]


def test_cases_of_the_gpu_file():
    cases = C.cases()
    assert len(cases) == len(set(cases)) == 9 * 5 + 2 * 2
    assert [s for r, s, st in cases if st == "direct"] == [(8, 8, 8), (8, 24, 40), (4, 8, 8), (4, 24, 40)]
    assert {C.backend_of(st) for st in C.SETTINGS} == {"auto", "mfma", "direct"}
    assert C.switches_of("auto") == {"use_zmarch": True, "use_coarse": True, "use_wino": True}
    assert sum(not v for st in C.SETTINGS for v in C.switches_of(st).values()) == 3


# ------------------------------------------------------------------------------------------------ e_ref and mutations
def test_e_ref_of_every_shape():
    for refine, shape in ALL:
        r = C.reference(refine, *shape)
        e = r["e_ref"]
        print(f"COSTREG e_ref {'refine' if refine else 'full'} {shape}: max {e[0]:.3e} ({e[0] / EPS:.2f} eps)  mean {e[1]:.3e} "
              f"({e[1] / EPS:.2f} eps)  max|f64| {r['f64'].abs().max().item():.2f}")
        assert torch.isfinite(r["f64"]).all() and torch.isfinite(r["oracle32"]).all()
        assert 0 < e[1] <= e[0] < 16 * EPS, (refine, shape, e)
        for k, el in r["levels_e_ref"].items():
            assert 0 < el[1] <= el[0] < 16 * EPS, (refine, shape, k, el)
        x = C.sim_volume(refine, *shape)
        assert x.dtype == F32 and -0.5 <= x.min().item() and x.max().item() <= 1.5


def test_mutations_sit_above_the_bound():
    sd, worst = C.state_dict(), {}
    for m in C.MUTATIONS:
        hit = C.mutation_cases(m)
        assert hit, m
        for refine, shape in ALL:
            r = C.reference(refine, *shape)
            got = C.net_f64(sd, C.PREFIX[refine], C.sim_volume(refine, *shape), refine, mutation=m)
            if (refine, shape) not in hit:
                assert torch.equal(got, r["f64"]), (m, refine, shape)      # nothing to see at this shape
                continue
            e, b = C.errors(got, r["f64"]), C.bounds(r["e_ref"])
            ratio = (e[0] / b[0], e[1] / b[1])
            w = worst.setdefault(m, [float("inf"), None, float("inf"), None])
            if ratio[0] < w[0]:
                w[0], w[1] = ratio[0], (refine, shape)
            if ratio[1] < w[2]:
                w[2], w[3] = ratio[1], (refine, shape)
            assert ratio[0] > 1.0 and ratio[1] > 1.0, (m, refine, shape, ratio)
    for m, w in worst.items():
        print(f"COSTREG mutation {m}: smallest error / bound  max {w[0]:.1f} {w[1]}  mean {w[2]:.1f} {w[3]}")
    print(f"COSTREG smallest mutation ratio: max {min(w[0] for w in worst.values()):.1f}  mean {min(w[2] for w in worst.values()):.1f}")
    assert set(worst) == set(C.MUTATIONS)
