"""CPU: pins tests/fusion_ref.py -- the float64 restatement of the fusion filter N4 -- and proves what its case tables claim,
without a GPU.

* The restatement against oracle/fusion_oracle.py run with every tensor widened to float64 (pairs and whole views), and against
  the recorded reference outputs (tests/golden/fusion_geo.npz, fusion_scene.npz) under their existing tolerances.
* An fp32 emulation of ``geo_pair`` in the kernel's own operation order sits inside the criterion on every SCENES case
  (``EMUL`` lines print e_emul / bound); it sizes the criterion and is never a yardstick on the GPU.
* Every claim of the tables: ragged workgroups, scan carries, wave seams with final pixels, taps outside per side, ladder levels,
  and that every exact case is exact (float64 values representable in fp32, the emulation equal to them bit for bit).
* The undecided share of every SCENES / SOURCES case and gate is within its cap, from the restatement and the fp32 oracle alone.
"""
import numpy as np
import pytest
import torch

import fusion_ref as R
from dmvsnet_amd.fusion import fold_projection
from test_fusion import CONF, PAIRS, _same_mask, _scene

SCENE_IDS = [f"{s[0]}x{s[1]}" for s in R.SCENES]
GATE_EPS = 1e-9


def _bases(ladder):
    return R.LADDER_BASES if ladder else R.STATIC_GATE


def _close(a, b, floor):
    """1e-9 relative wherever both are finite; ``floor``: the magnitude below which the difference is taken absolutely (dist
    and rel are differences that cancel to ~0 at consistent pixels: the gate is their scale there)."""
    fin = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(np.isfinite(a), np.isfinite(b)) and np.array_equal(np.isnan(a), np.isnan(b))
    err = np.abs(a[fin] - b[fin]) / np.maximum(np.abs(b[fin]), floor)
    return float(err.max()) if err.size else 0.0


@pytest.fixture(scope="module")
def scenes():
    """Restatement, float64 and fp32 oracle and the emulation of every pair of every SCENES row, computed once."""
    out = {}
    for idx, (H, W, V, seed, _) in enumerate(R.SCENES):
        depths, confs, cam = R.scene(H, W, V, seed)
        for ladder in (False, True):
            rows = []
            for v in range(1, V):
                args = (depths[0], cam(0), depths[v], cam(v), ladder)
                rows.append({"f64": R.pair(depths[0], *cam(0), depths[v], *cam(v), ladder), "o64": R.oracle_pair(*args, double=True),
                             "o32": R.oracle_pair(*args),
                             "emul": R.emul_pair32(depths[0], depths[v], fold_projection(*cam(0), *cam(v)), ladder)})
            out[idx, ladder] = (depths, confs, cam, rows)
    return out


# ------------------------------------------------------------------------------------------------ restatement vs the oracle
@pytest.mark.parametrize("ladder", [False, True], ids=["static", "ladder"])
@pytest.mark.parametrize("idx", range(len(R.SCENES)), ids=SCENE_IDS)
def test_pair_matches_oracle_in_float64(scenes, idx, ladder):
    _, _, _, rows = scenes[idx, ladder]
    td0, tr0 = R.STATIC_GATE
    for v, row in enumerate(rows, 1):
        f, o = row["f64"], row["o64"]
        errs = (_close(f[0], o[0], 1e-300), _close(f[1], o[1], td0), _close(f[2], o[2], tr0))
        print(f"F64 {SCENE_IDS[idx]} {'ladder' if ladder else 'static'} src {v}: rz {errs[0]:.2e} dist {errs[1]:.2e} rel {errs[2]:.2e}")
        assert max(errs) < 1e-9
        for td, tr in R.gate_list(ladder, *_bases(ladder), fp32_args=False):
            near = (np.abs(o[1] - td) <= GATE_EPS * td) | (np.abs(o[2] - tr) <= GATE_EPS * tr)
            assert np.array_equal(R.verdict(f[1], f[2], td, tr)[~near], R.verdict(o[1], o[2], td, tr)[~near])


@pytest.mark.parametrize("dynamic", [False, True], ids=["static", "dynamic"])
def test_view_matches_filter_view_in_float64(dynamic):
    """oracle.filter_view on float64 maps and cameras against the restated view: masks, averaged depth, points."""
    from oracle import fusion_oracle as FO
    _, depths, confs, imgs, cam = _scene()
    D = lambda a: np.asarray(a, np.float32).astype(np.float64)   # noqa: E731
    for r, srcs in PAIRS:
        want = FO.filter_view(D(depths[r]), tuple(D(m) for m in cam(r)), confs[r], CONF, imgs[r], [D(depths[s]) for s in srcs],
                              [tuple(D(m) for m in cam(s)) for s in srcs], thres_view=2, dynamic=dynamic)
        got = R.view(depths[r], cam(r), (confs[r][2], confs[r][1], confs[r][0]), CONF, [depths[s] for s in srcs], [cam(s) for s in srcs],
                     2, dynamic, fp32_args=False)
        near = np.zeros(depths[r].shape, bool)
        for s in range(len(srcs)):
            for td, tr in got["gates"]:
                near |= (np.abs(got["dist"][s] - td) <= GATE_EPS * td) | (np.abs(got["rel"][s] - tr) <= GATE_EPS * tr)
        assert near.mean() < 1e-3
        for k in ("photo", "geo", "final"):
            assert np.array_equal(got[k][~near], want[k][~near]), (r, k)
        assert _close(got["depth_avg"][~near], want["depth_averaged"][~near], 1e-300) < 1e-9
        if not near.any():
            scale = np.abs(got["xyz"]).max()
            assert got["xyz"].shape == want["xyz"].shape and np.abs(got["xyz"] - want["xyz"]).max() <= 1e-6 * scale   # want is fp32
        print(f"F64 view {r} {'dynamic' if dynamic else 'static'}: final {int(got['final'].sum())} near a gate {int(near.sum())}")


def test_restatement_matches_recorded_pairs(golden):
    """tests/golden/fusion_geo.npz: masks under the slack test_fusion.py gives the oracle; the reprojected depth under the
    2e-5 test_fusion.py gives another arithmetic than the recording's (its 2e-6 is between two fp32 runs of the same ATen
    ops: the recording's own distance from float64 is up to 1.8e-5 on this scene, OPEN lines of test_fusion_ref_gpu.py)."""
    g = golden("fusion_geo.npz")
    _, depths, _, _, cam = _scene()
    for v in range(1, 5):
        rz, dist, rel = R.pair(depths[0], *cam(0), depths[v], *cam(v), False)
        m = R.verdict(dist, rel, 1.0, 0.01)
        for tag in ("torch", "np"):
            assert _same_mask(m, g[f"{tag}.mask.{v}"])
            ok = m & g[f"{tag}.mask.{v}"]
            np.testing.assert_allclose(rz[ok], g[f"{tag}.rep.{v}"][ok], rtol=2e-5)
        rz, dist, rel = R.pair(depths[0], *cam(0), depths[v], *cam(v), True)
        masks = np.stack([R.verdict(dist, rel, td, tr) for td, tr in R.gate_list(True, 1 / 4, 1 / 1300, fp32_args=False)])
        assert _same_mask(masks, g[f"dy.masks.{v}"], slack=9)
        ok = masks[-1] & g[f"dy.masks.{v}"][-1]
        np.testing.assert_allclose(rz[ok], g[f"dy.rep.{v}"][ok], rtol=2e-5)


@pytest.mark.parametrize("tag,dynamic", [("pcd", False), ("dy", True)])
def test_restatement_matches_recorded_scene(golden, tag, dynamic):
    """tests/golden/fusion_scene.npz: the masks of every reference view and the fused cloud."""
    g = golden("fusion_scene.npz")
    _, depths, confs, _, cam = _scene()
    xyz = []
    for r, srcs in PAIRS:
        out = R.view(depths[r], cam(r), (confs[r][2], confs[r][1], confs[r][0]), CONF, [depths[s] for s in srcs], [cam(s) for s in srcs],
                     2, dynamic, fp32_args=False)
        for kind in ("photo", "geo", "final"):
            assert _same_mask(out[kind], g[f"{tag}.mask.{r}.{kind}"], 0 if kind == "photo" else 3), (r, kind)
        xyz.append(out["xyz"])
    v, xyz = g[f"{tag}.vertex"], np.concatenate(xyz)
    assert abs(len(xyz) - len(v)) <= 9
    if len(xyz) == len(v):
        np.testing.assert_allclose(xyz, np.stack((v["x"], v["y"], v["z"]), 1), rtol=1e-5, atol=1e-3)


def test_literal_P_agrees_with_cameras():
    """pair_P on fold_projection's float64 products is the unfolded chain up to float64 rounding."""
    _, depths, _, _, cam = _scene()
    Kr, Er, Ks, Es = (np.asarray(m, np.float64) for m in (*cam(0), *cam(1)))
    rel, back = Es @ np.linalg.inv(Er), Er @ np.linalg.inv(Es)
    P64 = np.concatenate([(Ks @ rel[:3, :3] @ np.linalg.inv(Kr)).ravel(), Ks @ rel[:3, 3], (back[:3, :3] @ np.linalg.inv(Ks)).ravel(),
                          back[:3, 3], Kr.ravel()])
    orig = R.split_P
    try:
        R.split_P = lambda P: (P[0:9].reshape(3, 3), P[9:12], P[12:21].reshape(3, 3), P[21:24], P[24:33].reshape(3, 3))
        got = R.pair_P(depths[0], depths[1], P64, False)
    finally:
        R.split_P = orig
    want = R.pair(depths[0], *cam(0), depths[1], *cam(1), False)
    assert _close(got[0], want[0], 1e-300) < 1e-9 and _close(got[1], want[1], 1.0) < 1e-9 and _close(got[2], want[2], 0.01) < 1e-9


# ------------------------------------------------------------------------------------------------ the emulation inside the bound
@pytest.mark.parametrize("ladder", [False, True], ids=["static", "ladder"])
@pytest.mark.parametrize("idx", range(len(R.SCENES)), ids=SCENE_IDS)
def test_emulation_sits_inside_the_bound(scenes, idx, ladder):
    _, _, _, rows = scenes[idx, ladder]
    gates = R.gate_list(ladder, *_bases(ladder))
    for v, row in enumerate(rows, 1):
        f, o, e = row["f64"], row["o32"], row["emul"]
        fin = np.isfinite(f[1]) & np.isfinite(f[2]) & np.isfinite(o[1]) & np.isfinite(o[2])
        both = R.verdict(o[1], o[2], *gates[-1]) & R.emul_verdict32(e[1], e[2], *_bases(ladder), level=10 if ladder else None)
        for what, keep in (("open", fin), ("accepted", both)):
            e_em, e_ref = R.errors(e[0], f[0], keep), R.errors(o[0], f[0], keep)
            b = R.bounds(e_ref)
            print(f"EMUL {SCENE_IDS[idx]} {'ladder' if ladder else 'static'} src {v} {what} ({int(keep.sum())}): e_emul/bound "
                  f"{e_em[0] / b[0]:.3f}/{e_em[1] / b[1]:.3f} e_ref {e_ref[0]:.3g}/{e_ref[1]:.3g}")
            assert e_em[0] <= b[0] and e_em[1] <= b[1]
        # the emulation's verdicts obey the verdict rule too
        band = R.bands(o, f, gates)
        for i, (td, tr) in zip(R.LEVELS, gates):
            yes, no = R.decided(f[1], f[2], td, tr, band)
            got = R.emul_verdict32(e[1], e[2], *_bases(ladder), level=i if ladder else None)
            assert got[yes].all() and not got[no].any()


# ------------------------------------------------------------------------------------------------ undecided shares
@pytest.mark.parametrize("ladder", [False, True], ids=["static", "ladder"])
@pytest.mark.parametrize("idx", range(len(R.SCENES)), ids=SCENE_IDS)
def test_undecided_share_of_scenes(scenes, idx, ladder):
    _, _, _, rows = scenes[idx, ladder]
    gates, cap = R.gate_list(ladder, *_bases(ladder)), R.LADDER_CAP if ladder else R.STATIC_CAP
    for v, row in enumerate(rows, 1):
        band = R.bands(row["o32"], row["f64"], gates)
        shares = [R.undecided_share(row["f64"][1], row["f64"][2], td, tr, band) for td, tr in gates]
        # the oracle itself flips no decided pixel
        for td, tr in gates:
            yes, no = R.decided(row["f64"][1], row["f64"][2], td, tr, band)
            o = R.verdict(row["o32"][1], row["o32"][2], td, tr)
            assert o[yes].all() and not o[no].any()
        print(f"SHARE {SCENE_IDS[idx]} {'ladder' if ladder else 'static'} src {v}: band {band[0]:.3g}/{band[1]:.3g} worst undecided "
              f"{max(shares):.4f} cap {cap}")
        assert max(shares) <= cap


@pytest.mark.parametrize("dynamic,nsrc", R.SOURCES, ids=[f"{'dynamic' if d else 'static'}-{n}" for d, n in R.SOURCES])
def test_undecided_share_of_sources(dynamic, nsrc):
    depths, _, cam = R.scene(*R.SOURCES_HW, nsrc + 1, nsrc)
    depths[0][0, :] = 0.0
    gates, cap = R.gate_list(dynamic, *_bases(dynamic)), R.LADDER_CAP if dynamic else R.STATIC_CAP
    worst = 0.0
    for ref, srcs in ((0, range(1, nsrc + 1)),):
        for s in srcs:
            f = R.pair(depths[ref], *cam(ref), depths[s], *cam(s), dynamic)
            band = R.bands(R.oracle_pair(depths[ref], cam(ref), depths[s], cam(s), dynamic), f, gates)
            worst = max([worst] + [R.undecided_share(f[1], f[2], td, tr, band) for td, tr in gates])
    print(f"SHARE sources {'dynamic' if dynamic else 'static'} nsrc {nsrc}: worst undecided {worst:.4f} cap {cap}")
    assert worst <= cap


# ------------------------------------------------------------------------------------------------ the tables' claims: geometry
def test_scene_geometry_claims():
    claims = {(37, 53): dict(wgs=8, ragged=87, nx=1, idle=203), (3, 257): dict(wgs=4, ragged=253, nx=2, idle=255),
              (2, 513): dict(wgs=5, ragged=254, nx=3, idle=255), (1, 300): dict(wgs=2, ragged=212, nx=2, idle=212),
              (300, 1): dict(wgs=2, ragged=212, nx=1, idle=255), (96, 128): dict(wgs=48, ragged=0, nx=1, idle=128)}
    for H, W, _, _, why in R.SCENES:
        c, (nx, ny, idle) = claims[H, W], R.pair_grid(H, W)
        assert (R.workgroups(H, W), R.ragged_lanes(H, W), nx, idle, ny) == (c["wgs"], c["ragged"], c["nx"], c["idle"], H), (H, W, why)
        assert H * W <= R.MAX_PIXELS
    # per-pair blockIdx.x = 1 and 2 with one lane in use; one column: W - 1 = 0
    assert R.pair_grid(3, 257)[0] - 1 == 1 and 257 - 256 == 1 and R.pair_grid(2, 513)[0] - 1 == 2 and 513 - 512 == 1
    assert R.SOURCES_HW == (37, 53) and max(n for _, n in R.SOURCES) == 16 and max(n for d, n in R.SOURCES if d) == 10


def test_one_column_scene_has_every_x1_tap_outside(scenes):
    depths, _, cam, rows = scenes[4, False]
    assert depths[0].shape == (300, 1)
    for v in range(1, len(depths)):
        P = fold_projection(*cam(0), *cam(v))
        xs, ys = R.project_P(depths[0], P)
        fin = np.isfinite(xs) & np.isfinite(ys)
        t = R.taps(xs, ys, 300, 1)
        # x0 and x1 = x0 + 1 cannot both be column 0
        assert not (t[0][3] & t[1][3])[fin].any() and not (t[2][3] & t[3][3])[fin].any()
    assert any((row["f64"][0] != 0).any() for row in rows)          # and some pixels do sample the one column


def test_emit_geometry_claims():
    wgs = {(1, 1): 1, (1, 63): 1, (1, 64): 1, (1, 65): 1, (1, 255): 1, (1, 256): 1, (1, 257): 2, (257, 256): 257, (342, 384): 513,
           (343, 383): 514}
    carries = {(257, 256): 1, (342, 384): 2, (343, 383): 2}
    for H, W in R.EMIT_SIZES:
        n = R.workgroups(H, W)
        assert n == wgs[H, W] and R.scan_passes(n) - 1 == carries.get((H, W), 0)
        assert H * W <= R.MAX_PIXELS
        for name in R.EMIT_PATTERNS:
            final = R.emit_pattern(name, H, W)
            counts, waves = R.wg_counts(final), R.wave_counts(final)
            assert counts.sum() == final.sum() == waves.sum() and len(counts) == n
            off = R.scan_offsets(counts)
            assert off[0] == 0 and off[-1] == final.sum() and np.array_equal(np.diff(off), counts)
            if name == "none":
                assert not final.any()
            if name == "all":
                assert final.all() and counts[-1] == R.WG - R.ragged_lanes(H, W)
            if name == "last":
                assert final.sum() == 1 and counts[-1] == 1 and off[-2] == 0
            if name == "wave_edges":
                lanes = np.nonzero(final.reshape(-1))[0] % R.WG
                assert set(lanes.tolist()) == {l for l in R.WAVE_EDGE_LANES if l < H * W}
                if H * W >= R.WG:       # every wave of a full workgroup carries final pixels on its first and / or last lane
                    assert waves[0].tolist() == [1, 2, 2, 2]
            if name == "one_full_wg" and n >= 3:
                b = n // 2
                assert counts[b] == R.WG and counts.sum() == R.WG and counts[b - 1] == 0 and counts[b + 1] == 0
            if name == "half" and H * W >= 256:
                assert 0.4 < final.mean() < 0.6 and (waves[:-1] > 0).all()
    assert R.ragged_lanes(343, 383) == 215 and R.ragged_lanes(342, 384) == 0 and 343 * 383 == R.MAX_PIXELS
    d = R.emit_depths(343, 383)
    assert np.array_equal(d.astype(np.float32).astype(np.float64), d) and len(np.unique(d.reshape(-1)[:R.WG])) == R.WG


# ------------------------------------------------------------------------------------------------ the tables' claims: EXACT
def _exactly(f, e):
    """float64 values representable in fp32 and the emulation equal to them bit for bit (NaN to NaN) -- at the pixels that
    sample anything: where every tap is outside, sd = 0, kz is patched and dist = |(x, y)| is an irrational square root,
    rounded once in either precision (rz = 0 and rel = 1 are exact there too; test_exact_shift_rows, all-outside)."""
    sampled = e[3] != 0
    for a, b in zip(f, e[:3]):
        a, b = a[sampled], b[sampled]
        a32 = a.astype(np.float32)
        if not (np.array_equal(a32.astype(np.float64), a, equal_nan=True) and np.array_equal(a32, b, equal_nan=True)
                and np.array_equal(np.signbit(a32[a32 != 0]), np.signbit(b[a32 != 0]))):
            return False
    return True


@pytest.mark.parametrize("ladder", [False, True], ids=["static", "ladder"])
@pytest.mark.parametrize("row", R.EXACT_SHIFTS, ids=[r[0] for r in R.EXACT_SHIFTS])
def test_exact_shift_rows(row, ladder):
    name, sx, sy, L, Rt, T, B = row
    H, W = R.EXACT_HW
    for k in (8, 12):
        d_ref, d_src, P = R.exact_case(sx, sy, k)
        xs, ys = R.project_P(d_ref, P)
        x, y = R._grid(H, W)
        assert np.array_equal(xs, x + sx) and np.array_equal(ys, y + sy)
        want = tuple(tuple(sorted(i % n for i in t)) for t, n in zip((L, Rt, T, B), (W, W, H, H)))
        assert R.tap_sides(xs, ys, H, W) == want, (name, R.tap_sides(xs, ys, H, W))
        f, e = R.pair_P(d_ref, d_src, P, ladder), R.emul_pair32(d_ref, d_src, P, ladder)
        inner = R.interior(H, W, sx, sy)
        assert (f[0][inner] == d_src[0, 0]).all() and (f[1][inner] == np.hypot(sx, sy)).all() and (f[2][inner] == 2.0 ** -k).all()
        assert np.array_equal(f[0], e[0].astype(np.float64)) and np.array_equal(e[3] == 0, f[0] == 0)
        if name == "all-outside":            # sd = 0, kz == 0: patched, dist = |(x, y)| (an irrational square root, rounded once
            assert (e[3] == 0).all() and (f[0] == 0).all() and (f[2] == 1).all()      # in either precision) and rel = 1
            assert np.allclose(f[1], np.hypot(x, y), rtol=1e-15) and np.isfinite(e[1]).all()
        else:
            assert _exactly(f, e), name
    # the boundaries the name states
    if name.startswith("xs="):
        hit = {"xs=-1": (0, -1.0), "xs=-0.5|W-1.5": (0, -0.5), "xs=0|W-1": (W - 1, W - 1.0), "xs=W-0.5": (W - 1, W - 0.5), "xs=W": (W - 1, float(W))}
        col, val = hit[name]
        assert (xs[:, col] == val).all()
        if name == "xs=-0.5|W-1.5":
            assert (xs[:, W - 1] == W - 1.5).all()
        if name == "xs=0|W-1":
            assert (xs[:, 0] == 0).all()
    if name.startswith("ys="):
        hit = {"ys=-1": (0, -1.0), "ys=-0.5|H-1.5": (0, -0.5), "ys=H-0.5": (H - 1, H - 0.5), "ys=H": (H - 1, float(H))}
        r, val = hit[name]
        assert (ys[r] == val).all()


def test_exact_corner_rows_reach_the_four_corners():
    H, W = R.EXACT_HW
    corner = {"corners-": (0, 0), "corners+": (H - 1, W - 1), "corners-+": (H - 1, 0), "corners+-": (0, W - 1)}
    for name, sx, sy, *_ in R.EXACT_SHIFTS:
        if name in corner:
            d_ref, d_src, P = R.exact_case(sx, sy, 8)
            f = R.pair_P(d_ref, d_src, P)
            y, x = corner[name]
            assert f[0][y, x] == 0.625 * 0.5 * d_src[0, 0]        # one tap inside, under the weight 5/8 * 1/2
            assert np.hypot(sx, sy) == 0.625


def test_exact_gate_rows():
    for name, sx, sy, k, td, tr, verdict in R.EXACT_GATES:
        d_ref, d_src, P = R.exact_case(sx, sy, k)
        f, e = R.pair_P(d_ref, d_src, P), R.emul_pair32(d_ref, d_src, P)
        inner = R.interior(*R.EXACT_HW, sx, sy)
        assert inner.sum() >= 8 and (f[1][inner] == np.hypot(sx, sy)).all() and (f[2][inner] == 2.0 ** -k).all()
        assert np.float32(td) == td and np.float32(tr) == tr                      # the gate reaches the kernel as written
        assert (R.verdict(f[1], f[2], td, tr)[inner] == verdict).all(), name
        assert np.array_equal(R.emul_verdict32(e[1], e[2], td, tr), R.verdict(f[1], f[2], td, tr)) and _exactly(f, e), name
    on = [r for r in R.EXACT_GATES if " on the gate" in r[0]]
    assert len(on) == 3 and not any(r[6] for r in on)                              # the inequalities are strict
    assert R._step(0.5, True) > 0.5 > R._step(0.5, False) and R._step(0.5, True) - 0.5 == 2.0 ** -24


def test_exact_ladder_rows():
    bd, br = R.EXACT_LADDER_BASES
    assert np.float32(bd) == bd and np.float32(br) == br
    for name, sx, k, levels in R.EXACT_LADDER:
        d_ref, d_src, P = R.exact_case(sx, 0.0, k)
        f, e = R.pair_P(d_ref, d_src, P, True), R.emul_pair32(d_ref, d_src, P, True)
        inner = R.interior(*R.EXACT_HW, sx, 0.0)
        assert inner.sum() >= 8 and _exactly(f, e)
        for i, (td, tr) in zip(R.LEVELS, R.gate_list(True, bd, br)):
            assert (td, tr) == (i * bd, i * br)
            assert (R.verdict(f[1], f[2], td, tr)[inner] == (i in levels)).all(), (name, i)
            assert np.array_equal(R.emul_verdict32(e[1], e[2], bd, br, level=i), R.verdict(f[1], f[2], td, tr))
    assert dict((r[0], r[3]) for r in R.EXACT_LADDER)["shift 0.5"] == tuple(range(3, 11))
    assert dict((r[0], r[3]) for r in R.EXACT_LADDER)["rel 2^-8"] == tuple(range(5, 11))


def test_hostile_rows_are_exact_too():
    """The HOSTILE rows ride the exact scaffold: the emulation reproduces the restated rz and every verdict under IEEE rules."""
    H, W = R.EXACT_HW
    for _, value in R.HOSTILE_VALUES:
        for which in ("ref", "src"):
            for sx, sy in ((0.0, 0.0), (0.375, 0.5), (-0.5, 0.0)):
                for ladder in (False, True):
                    d_ref, d_src, P = R.exact_case(sx, sy, 8)
                    m = d_ref if which == "ref" else d_src
                    m[2, 3] = m[0, 0] = m[-1, -1] = m[3, 0] = value
                    f, e = R.pair_P(d_ref, d_src, P, ladder), R.emul_pair32(d_ref, d_src, P, ladder)
                    assert np.array_equal(f[0].astype(np.float32), e[0], equal_nan=True), (value, which, sx)
                    for td, tr in ((np.inf, np.inf), (4.0, 2.0 ** -6)):
                        assert np.array_equal(R.verdict(f[1], f[2], td, tr), R.emul_verdict32(e[1], e[2], td, tr))
    # a NaN source pixel reaches its left, upper and upper-left neighbours under zero weights at shift (0, 0)
    d_ref, d_src, P = R.exact_case(0.0, 0.0, 8)
    d_src[2, 3] = np.nan
    rz = R.pair_P(d_ref, d_src, P)[0]
    assert set(zip(*np.nonzero(np.isnan(rz)))) == {(2, 3), (2, 2), (1, 3), (1, 2)}
    t = torch.nn.functional.grid_sample(torch.from_numpy(d_src)[None, None].double(),
                                        torch.tensor([[[[2 / (W - 1) * 2 - 1, 2 / (H - 1) * 2 - 1]]]], dtype=torch.float64),
                                        mode="bilinear", padding_mode="zeros", align_corners=True)
    assert torch.isnan(t).all()                      # grid_sample at pixel (2, 2): the NaN tap under weight zero


def test_view_forms():
    """The geo forms on hand-made counts: static votes >= thres_view; dynamic any_i<=nsrc level[i-2] >= i, votes >= nsrc + 1 never."""
    votes = np.array([[0, 1, 2, 3]])
    assert R.geo_static(votes, 2).tolist() == [[False, False, True, True]]
    lv = np.zeros((9, 1, 4), np.int64)
    lv[0, 0, 1], lv[1, 0, 2], lv[2, 0, 3] = 2, 3, 4
    assert R.geo_dynamic(votes, lv, 3).tolist() == [[False, True, True, False]]       # level i = 4 is not read at nsrc = 3
    assert R.geo_dynamic(votes, lv, 4).tolist() == [[False, True, True, True]]
    assert not R.geo_dynamic(np.full((1, 4), 3), np.zeros((9, 1, 4), np.int64), 3).any()
    assert not R.geo_dynamic(np.minimum(votes, 1), lv, 1).any()                       # one source: no gate is read
