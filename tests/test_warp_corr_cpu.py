"""The float64 restatement of K1's forward (tests/warp_corr_ref.py) against everything else that states the operation, the conditions
its case tables have to meet, and its power to tell a wrong kernel from a right one.  CPU only; no kernel runs here.

  tie        in float64 with a float64 p12 the restatement equals costagg_grad_ref.cost_agg_f64 (grid_sample, normalised
             coordinates) to 1e-12 of max|sim| on every SHAPES and VIEWS case, and reproduces tests/golden/op_costagg.npz.
  e_ref      printed beside the fp32 oracle's distance for every case; non-zero wherever the table says so.
  tables     window-mode coverage, the hypothesis outlier's distance, exact coordinates, no fp16 subnormals, the share of samples
             with a tap outside the image.
  op order   the fp32 oracle (normalise, grid_sample, un-normalise: the generic kernel's op order) obeys the plain criterion, max and
             mean, on every table but WINDOWS; on WINDOWS, where e_ref is below the criterion's floor, it obeys the plain mean bound
             and EXCEEDS the plain max bound, and obeys the max bound with ``warp_corr_ref.op_order_allowance`` -- the ground for
             giving the generic kernel that allowance there, on the max, and nowhere else.  All of it asserted.
  mutations  eight wrong kernels, each at least 20 x over a bound of the criterion.  See ``test_mutations_exceed_the_bound``.

The p12 of a camera case is composed in float64 and rounded to fp32 here (the GPU file takes the kernel's own, from
``ops.relative_proj``): either way the restatement and the implementation under test get the same fp32 numbers."""
import functools

import numpy as np
import pytest
import torch

import costagg_grad_ref as G
import warp_corr_ref as R
from oracle import dmvs_oracle as O

F64, F32 = torch.float64, torch.float32
CASES = R.all_cases()
BY_TABLE = {t: [n for n, c in CASES.items() if c["table"] == t] for t in
            ("SHAPES", "VIEWS", "EDGE_SHAPES", "AFFINE", "WINDOWS", "SCATTER", "SPECIAL")}


def p12_of(case, dtype=F32):
    return case["p12"].to(dtype) if case["p12"] is not None else R.p12_of_cams(case["cams"], dtype)


@functools.lru_cache(maxsize=None)
def ref_of(name):
    """(float64 yardstick, (e_max, e_mean) of the fp32 restatement): computed once, never modified."""
    return R.reference(CASES[name], p12_of(CASES[name]))


def test_the_tables_hold_what_the_issue_lists():
    assert len(BY_TABLE["SHAPES"]) == 10 and len(BY_TABLE["VIEWS"]) == 9 and len(BY_TABLE["EDGE_SHAPES"]) == 3
    assert len(BY_TABLE["AFFINE"]) == 2 * 9 and len(BY_TABLE["WINDOWS"]) == 3 * len(R.WINDOWS)
    assert sum(len(v) for v in BY_TABLE.values()) == len(CASES)
    for name, c in CASES.items():
        D, H, W = c["depth"].shape
        assert H <= 72 and W <= 160 and D <= 48 and c["C"] in (8, 16, 32), name
        assert all(f.dtype == F32 and tuple(f.shape) == (c["C"], H, W) for f in c["feats"]), name
        assert (c["p12"] is None) != (c["cams"] is None) and len(c["feats"]) - 1 == p12_of(c).shape[0], name
        if c["table"] == "WINDOWS":
            assert D == R.WINDOWS_D


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("name", BY_TABLE["SHAPES"] + BY_TABLE["VIEWS"])
def test_restatement_equals_cost_agg_f64(name):
    c = CASES[name]
    want = G.cost_agg_f64([f[None] for f in c["feats"]], c["cams"][None], c["depth"][None])[0]
    got = R.warp_corr_ref(c["feats"], p12_of(c, F64), c["depth"], F64)
    e = (got - want).abs().max().item() / want.abs().max().item()
    print(f"TIE {name}: |restatement - cost_agg_f64| / max|sim| = {e:.3e}")
    assert got.dtype == F64 and got.shape == want.shape and e <= 1e-12


def test_restatement_reproduces_the_golden(golden):
    g = golden("op_costagg.npz")
    feats = [torch.from_numpy(g[f"feat{v}"])[0] for v in range(3)]
    cams, depth = torch.from_numpy(g["proj"])[0], torch.from_numpy(g["depth"])[0]
    for dtype in (F64, F32):   # 1e-5: the tolerance test_gpu_parity.py puts on the kernels for this file
        got = R.warp_corr_ref(feats, R.p12_of_cams(cams, dtype), depth, dtype)
        np.testing.assert_allclose(got.numpy(), g["sim"][0], atol=1e-5, rtol=0.0)


def _oracle(c, p12):
    """The fp32 oracle (normalise, grid_sample, un-normalise) fed the same fp32 p12."""
    total = 0
    ref = c["feats"][0]
    C, H, W = ref.shape
    D = c["depth"].shape[0]
    for v in range(p12.shape[0]):
        warped = O.warp_source(c["feats"][v + 1][None], p12[v, :9].view(1, 3, 3), p12[v, 9:].view(1, 3), c["depth"][None])
        total = total + (warped.view(1, C // 2, 2, D, H, W) * ref.view(1, C // 2, 2, 1, H, W)).mean(1)[0]
    return total


@pytest.mark.parametrize("name", list(CASES))
def test_e_ref_beside_the_oracle(name):
    """e_ref must not silently sit on the criterion's floor where the table expects rounding error; on the one-row / one-column
    maps the oracle divides by (n - 1) / 2 = 0 and returns NaN, which is printed and not compared."""
    c = CASES[name]
    f64, e_ref = ref_of(name)
    e_or = R.errors(_oracle(c, p12_of(c)), f64)
    print(f"E_REF {name}: e_ref max {e_ref[0]:.3e} mean {e_ref[1]:.3e}   oracle max {e_or[0]:.3e} mean {e_or[1]:.3e}   "
          f"max|f64| {f64.abs().max().item():.3f}")
    assert torch.isfinite(f64).all() and np.isfinite(e_ref).all()
    if c["nonzero_e_ref"]:
        assert e_ref[0] > 0 and e_ref[1] > 0 and f64.abs().max().item() > 0.1
    if c["table"] == "EDGE_SHAPES":
        assert not np.isfinite(e_or[0])
    else:
        # the oracle has the generic kernel's op order: the plain criterion everywhere, but for the max bound on WINDOWS, which
        # carries warp_corr_ref.allowance (0 on every other table); test_oracle_exceeds_the_plain_max_bound_on_windows is the other half
        allow = allowance_of(name)
        b, plain = R.bounds(e_ref, allow), R.bounds(e_ref)
        print(f"E_REF {name}: op-order allowance {allow:.3e}   oracle / bound {e_or[0] / b[0]:.3f} {e_or[1] / b[1]:.3f}"
              f"   oracle / plain bound {e_or[0] / plain[0]:.3f} {e_or[1] / plain[1]:.3f}")
        assert (allow > 0) == (c["table"] == "WINDOWS") and b[1] == plain[1]
        if f64.abs().max().item() > 0:
            assert e_or[0] <= b[0] and e_or[1] <= b[1]
    if c["table"] == "AFFINE":
        assert e_ref[0] <= 2.5e-7


def test_oracle_exceeds_the_plain_max_bound_on_windows():
    """Why the generic kernel's max bound is widened on WINDOWS: every case there has e_ref below the criterion's floor (the
    projections sx x + ox are nearly exact in fp32), and the reference's op order alone -- the fp32 oracle on stock ATen -- is over
    the plain max bound on most of them (1.1-4.8 x on 30 of 33 where this was written; the two smallest maps, W <= 36, stay under
    it).  Were this to stop being true, the allowance would have lost its ground and this test says so."""
    over = {}
    for name in BY_TABLE["WINDOWS"]:
        f64, e_ref = ref_of(name)
        assert e_ref[0] < 4 * 2.0 ** -23 and e_ref[1] < 4 * 2.0 ** -23, name
        over[name] = R.errors(_oracle(CASES[name], p12_of(CASES[name])), f64)[0] / R.bounds(e_ref)[0]
    n = sum(v > 1.0 for v in over.values())
    print(f"WINDOWS: oracle over the plain max bound on {n} of {len(over)} cases, worst {max(over.values()):.2f} x")
    assert n >= len(over) // 2 and max(over.values()) >= 2.0, over


# ------------------------------------------------------------------------------------------------ table conditions
def test_features_are_never_smooth_and_never_fp16_subnormal():
    """Normal draws of scale 1, neighbouring pixels uncorrelated; rounded to fp16 no value is subnormal (or zero, or infinite)."""
    for name, c in CASES.items():
        x = torch.stack(c["feats"])
        h = x.half()
        assert (h.float().abs() >= 2.0 ** -14).all() and torch.isfinite(h.float()).all(), name
        if x.numel() >= 4096:
            assert abs(x.std().item() - 1.0) < 0.05 and abs(x.mean().item()) < 0.05, name
            assert abs((x[..., 1:] * x[..., :-1]).mean().item()) < 0.05, name


@pytest.mark.parametrize("name", BY_TABLE["SHAPES"])
def test_outside_share_of_shapes(name):
    """5-60 % of the samples have a tap outside the image, so both the zero padding and the interior are exercised.  The 2 x 2
    map cannot meet the upper end -- all four taps are inside only for a sample within its single pixel cell -- and is held to
    'not every sample outside' instead."""
    c = CASES[name]
    share = R.outside_share(p12_of(c), c["depth"])
    print(f"TABLE {name}: outside share {share:.3f}")
    _, H, W = c["depth"].shape
    if (H, W) == (2, 2):
        assert 0.05 <= share < 1.0
    else:
        assert 0.05 <= share <= 0.60


def test_affine_coordinates_are_exact():
    """fp32 and float64 coordinates coincide after the clamp to [-1, W] x [-1, H] (x + 1e9 rounds in fp32, far outside), and the
    table holds integer, half-pixel and exactly -1 / W / H positions."""
    seen = set()
    for name in BY_TABLE["AFFINE"]:
        c = CASES[name]
        D, H, W = c["depth"].shape
        (x32, y32), (x64, y64) = R.coordinates(c["p12"][0], c["depth"]), R.coordinates(c["p12"][0].double(), c["depth"].double())
        assert torch.equal(x32.clamp(-1, W).double(), x64.clamp(-1, W)) and torch.equal(y32.clamp(-1, H).double(), y64.clamp(-1, H)), name
        seen.update(x64.clamp(-2, W + 1).reshape(-1).tolist())
        seen.update((1000 + y64.clamp(-2, H + 1)).reshape(-1).tolist())
        f64, _ = ref_of(name)
        ox, oy = c["p12"][0, 2].item(), c["p12"][0, 5].item()
        assert (f64.abs().max().item() == 0.0) == (ox >= W or oy >= H), name   # every sample outside: the yardstick is exactly zero
    D, H, W = R.AFFINE_SHAPE
    for v in (-1.0, 0.0, -0.5, float(W - 1), float(W), 0.25, 1000.0 - 1, 1000.0 + H - 1, 1000.0 + H, 1000.0 + 8.75):
        assert v in seen, v


def _tile_inside_share(sx, ox, sy, oy, H, W, tx, ty):
    x = torch.arange(tx, min(tx + R.TW, W), dtype=F64).view(1, -1)
    y = torch.arange(ty, min(ty + R.TH, H), dtype=F64).view(-1, 1)
    x0, y0 = torch.floor(sx * x + ox), torch.floor(sy * y + oy)
    return ((x0 >= 0) & (x0 + 1 <= W - 1) & (y0 >= 0) & (y0 + 1 <= H - 1)).double().mean().item()


def test_windows_reach_every_slab_mode():
    """For every C, window selector 1 .. 3 and every mode that C has, plus the global-tap path, some tile of WINDOWS takes it with at
    least half of its samples having all four taps inside the image; for selector 4 (160 KB) the slab modes only."""
    tiles = []   # (pieces, inside share, geometry index)
    for k, g in enumerate(R.WINDOWS):
        assert g[4] <= 72 and g[5] <= 160 and g[5] % 2 == 0   # even W: the fp16 twin runs them too
        for tx, ty, n in R.q4_tile_windows(*g):
            tiles.append((n, _tile_inside_share(*g, tx, ty), k))
    assert R._q4_window_pieces(*R.WINDOWS[0]) == {n for n, _, k in tiles if k == 0}
    for C in (8, 16, 32):
        for sel, winq in R.WINQ.items():
            want = list(R.q4_modes_of(C)) + (["global"] if sel < 4 else [])
            for mode in want:
                hit = [(n, k) for n, share, k in tiles if share >= 0.5 and R.q4_mode(n, C, winq) == mode]
                print(f"WINDOWS c{C} selector {sel} mode {mode}: {sorted(set(hit))}")
                assert hit, (C, sel, mode)


def test_q4_mode_restates_the_kernel_rule():
    assert R.q4_modes_of(8) == (0, 1) and R.q4_modes_of(16) == (0, 1, 2) and R.q4_modes_of(32) == (0, 1, 2, 3)
    # selector 1 (2552 quads): pitches 316 / 636 / 1276 / 2552 for C = 32 -- 317 .. 319 pieces do NOT fit mode 0 (2552 / 8 = 319)
    assert [R.q4_mode(n, 32, 2552) for n in (316, 317, 319, 636, 637, 1276, 1277, 2552, 2553)] == [0, 1, 1, 1, 2, 2, 3, 3, "global"]
    assert [R.q4_mode(n, 16, 2552) for n in (636, 637, 638, 1276, 1277, 2552, 2553)] == [0, 1, 1, 1, 2, 2, "global"]
    assert [R.q4_mode(n, 8, 2552) for n in (1276, 1277, 2552, 2553)] == [0, 1, 1, "global"]
    assert [R.q4_mode(n, 32, 3408) for n in (424, 425, 852, 853, 1704, 1705, 3408, 3409)] == [0, 1, 1, 2, 2, 3, 3, "global"]
    assert [R.q4_mode(n, 32, 5112) for n in (636, 637, 1276, 1277, 2556, 2557, 5112, 5113)] == [0, 1, 1, 2, 2, 3, 3, "global"]
    assert [R.q4_mode(n, 32, 10232) for n in (1276, 1277, 2556, 2557, 5116, 5117, 10232, 10233)] == [0, 1, 1, 2, 2, 3, 3, "global"]
    assert R.WINQ == {s: (((160 * 1024 // w) - 64) // 16) & ~7 for s, w in ((1, 4), (2, 3), (3, 2), (4, 1))}


def test_scatter_outlier_stands_clear_of_its_tile():
    """Over the 16 tiles the outlier sits in every wave's rows, on the tile's first and on its last pixel, and in both plane chunks of
    C = 16; in some view its float64 source position lies at least 2 px outside the bounding box of all other samples of its tile --
    a window sized without it cannot hold it -- and at least for the four tiles that do not touch the image's edge its four taps are
    inside the image there, so that a window missing it changes the result."""
    D, H, W = R.SCATTER_SHAPE
    pos = [R.outlier_position(k) for k in range(16)]
    assert {r // 2 for _, r, _ in pos} == {0, 1, 2, 3} and (0, 0) in {(r, c) for _, r, c in pos} and (R.TH - 1, R.TW - 1) in {(r, c) for _, r, c in pos}
    assert {d // 4 for d, _, _ in pos} == {0, 1} and {d for d, _, _ in pos} == set(range(8))
    for name in ("scatter-outlier-c8", "scatter-outlier-c16"):
        c = CASES[name]
        assert ((c["depth"] == 500.0).sum().item() == 16) and (c["depth"][c["depth"] != 500.0] - 740.0).abs().max().item() <= 2.0
        p12 = p12_of(c, F64)
        coords = [R.coordinates(p12[v], c["depth"].double()) for v in range(p12.shape[0])]
        inside = 0
        for k, (d, r, col) in enumerate(pos):
            ys, xs = slice((k // 4) * R.TH, (k // 4 + 1) * R.TH), slice((k % 4) * R.TW, (k % 4 + 1) * R.TW)
            best, best_in = 0.0, False
            for ix, iy in coords:
                tx, ty = ix[:, ys, xs].clone(), iy[:, ys, xs].clone()
                ox, oy = tx[d, r, col].item(), ty[d, r, col].item()
                tx[d, r, col], ty[d, r, col] = tx[0, 0, 0] if (d, r, col) != (0, 0, 0) else tx[0, 0, 1], ty[0, 0, 0] if (d, r, col) != (0, 0, 0) else ty[0, 0, 1]
                gap = max(tx.min().item() - ox, ox - tx.max().item(), ty.min().item() - oy, oy - ty.max().item())
                if gap > best:
                    best, best_in = gap, 0 <= ox < W - 1 and 0 <= oy < H - 1
            inside += best_in
            print(f"SCATTER {name} tile {k}: outlier at plane {d} row {r} col {col}, {best:.2f} px outside the others' box")
            assert best >= 2.0, (name, k, best)
        assert inside >= 4, (name, inside)


def test_special_projections_do_what_the_table_says():
    D, H, W = R.SPECIAL_SHAPE
    c = CASES["special-zero-denominator-c8"]
    P, d = c["p12"][0], c["depth"]
    for dt in (F32, F64):   # the denominator x * d is exactly 0 on the column x = 0 in either precision, and nowhere else
        x = torch.arange(W, dtype=dt).view(1, 1, W)
        pz = (P[6].to(dt) * x + P[8].to(dt)) * d.to(dt) + P[11].to(dt)
        assert (pz[:, :, 0] == 0).all() and (pz[:, :, 1:] > 0).all()
    ix, iy = R.coordinates(CASES["special-behind-c8"]["p12"][0].double(), d.double())
    assert torch.equal(ix, -torch.arange(W, dtype=F64).view(1, 1, W).expand(D, H, W))
    ix, iy = R.coordinates(CASES["special-behind-mirrored-c8"]["p12"][0].double(), CASES["special-behind-mirrored-c8"]["depth"].double())
    assert ix.min() == 0 and ix.max() == W - 1 and iy.min() == 0 and iy.max() == H - 1
    # turned camera: the denominator changes sign inside tiles of the last view
    c = CASES["special-turned"]
    P = p12_of(c, F64)[-1]
    Dt, Ht, Wt = c["depth"].shape
    x, y = torch.arange(Wt, dtype=F64).view(1, 1, Wt), torch.arange(Ht, dtype=F64).view(1, Ht, 1)
    pz = (P[6] * x + P[7] * y + P[8]) * c["depth"].double() + P[11]
    assert (pz[:, :8, :32] > 0).any() and (pz[:, :8, :32] < 0).any()


# ------------------------------------------------------------------------------------------------ sensitivity
# mutation -> tables on which it is the identity in exact arithmetic (or not defined) and therefore not required to show:
#   next_plane / window_from_dmax on WINDOWS: the projections there do not depend on the depth.
IDENTITY = {"next_plane": ("WINDOWS",), "window_from_dmax": ("WINDOWS",)}


@functools.lru_cache(maxsize=None)
def allowance_of(name):
    return R.allowance(CASES[name], p12_of(CASES[name]))


@functools.lru_cache(maxsize=None)
def _excess(mutation, name):
    """max(e_max / bound_max, e_mean / bound_mean) of the mutated fp32 restatement on one case: the plain criterion, but for the max
    bound on WINDOWS, which is taken with the generic kernel's allowance (the q4 kernel's plain bound there is tighter, so its
    excess is larger still)."""
    c = CASES[name]
    f64, e_ref = ref_of(name)
    e = R.errors(R.warp_corr_ref(c["feats"], p12_of(c), c["depth"], F32, mutation), f64)
    b = R.bounds(e_ref, allowance_of(name))
    assert c["table"] == "WINDOWS" or b == R.bounds(e_ref)
    return max(e[0] / b[0], e[1] / b[1])


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_mutations_exceed_the_bound(mutation):
    """Each wrong kernel -- coordinates shifted by 1/256 px, align_corners=False weights, border clamp instead of zero padding, the
    channel groups swapped, the last view dropped, plane min(d + 1, D - 1), divisor C, a window sized from dmax alone -- is at least
    20 x over the max or the mean bound on some SHAPES case, and on some WINDOWS and some SCATTER case unless it is an identity
    there (IDENTITY).  The bounds are the plain ones on SHAPES and SCATTER (``_excess``)."""
    for table in ("SHAPES", "WINDOWS", "SCATTER"):
        if table in IDENTITY.get(mutation, ()):
            worst = max(_excess(mutation, n) for n in BY_TABLE[table][:6])
            print(f"MUTATION {mutation} on {table}: identity, {worst:.2f} x the bound")
            assert worst <= 1.0
            continue
        per_case = {n: _excess(mutation, n) for n in BY_TABLE[table]}
        best = max(per_case, key=per_case.get)
        print(f"MUTATION {mutation} on {table}: {per_case[best]:.1f} x a bound on {best}; "
              f"{sum(v >= 20 for v in per_case.values())} of {len(per_case)} cases at 20 x or more")
        assert per_case[best] >= 20.0, (mutation, table, per_case)
