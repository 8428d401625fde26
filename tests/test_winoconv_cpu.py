"""What tests/winoconv_ref.py claims about the four Winograd kernels of conv0 / conv2 / conv4 / conv6 (K3w's 3D rows and conv0, K3r,
K3z), asserted from the launch geometry restated there; its fp32 emulation held to the plain criterion on every input the GPU file
reads; and the mistakes the criterion tells apart.  CPU only: no kernel runs here (the plan, the knobs and the packers are host
functions of the library).

  rows         the kernels' tables in the sources against the restated ones; the packers accept exactly the rows of ROWS.
  tables       every class the case tables name: SMALL, WALK (tile counts against dmvs_conv3d_wino_plan, more tiles than resident
               workgroups, ragged eighths, a workgroup that changes its ZSKIP case between consecutive tiles), the ZSKIP cases that
               are ever dispatched, COARSE (loaders, dead-tap sets, short and empty eighths at `k3r_grid` 32), ZMARCH (segment lengths,
               stage masks, ranges that start and end inside a column, empty workgroups).
  emulation    ``wino_emulate`` in fp32 inside the plain bound, BatchNorm + ReLU and raw; exact on the integer cases.
  mutations    each mistake at least MUTATION_RATIO times bound_of(e_ref) away at every shape that claims to expose it."""
import os

import pytest
import torch

import winoconv_ref as R

F64, F32 = R.F64, R.F32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dmvsnet_amd", "csrc")
EPS32 = 2.0 ** -23
IDS = lambda v: v if isinstance(v, str) else "x".join(map(str, v))  # noqa: E731


def _lib():
    from dmvsnet_amd import _lib
    return _lib, _lib.load()


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ rows
def test_restated_tables_are_the_sources():
    wino, coarse, zmarch = _src("conv3d_wino.hip"), _src("conv3d_coarse.hip"), _src("conv3d_zmarch.hip")
    for text in ("wino_row<3, 1, 1, 1, 2, 1>(16, 16, true, true)", "wino_row<3, 1, 1, 2, 1, 1>(16, 16, false, true)",
                 "wino_row<3, 2, 2, 1, 1, 1>(32, 32, false, true)", "wino_row<3, 4, 2, 1, 1, 1>(64, 64, false, true)",
                 "wino_row<1, 4, 2, 1, 1, 1>(64, 64, false, true)", "{2, 16, 3, false, 1, 0, 2, 8, false, {launch_conv0_wino, nullptr}}",
                 "if (KD == 3) { bz = r % a.nz; by = r / a.nz; } else { by = r % a.ny; bz = r / a.ny; }",
                 "t.ox0 = bx * 32; t.oz0 = (r % a.nz) * TZ; t.oy0 = (r / a.nz) * TY;",
                 "if constexpr (KD == 3 && TZ == 2 && !ZSKIP)", "(oz0 == 0 ? 1 : 0) | (min(a.D - oz0, TZ + 1) - 1) << 1",
                 "256u * (unsigned)std::max<size_t>(1, std::min<size_t>(2, (160 * 1024) / lds))"):
        assert text in wino, text
    for text in ("{32, 32, 3, 2},", "{64, 64, 3, 1},", "{32, 32, 1, 2},", "{64, 64, 1, 2},", "oz = r % a.D;", "oy0 = 8 * (r / a.D);",
                 "a.st4 = (W % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) ? 1 : 0;",
                 "const bool v4 = W % 4 == 0 && (reinterpret_cast<uintptr_t>(in) & 15) == 0;", "if constexpr (KD == 3 && V4)",
                 "static constexpr int CPS = KD == 3 ? 16 : 32;"):
        assert text in coarse, text
    for text in ("const int rounds = mine / nslots, tail_c = rounds * nslots;", "tail_planes * slot / nslots", "zse = min(lim, a.zs);",
                 "while (t < zse) stage(std::integral_constant<int, 7>{});", "a.zs = g_k3z_zs ? (int)g_k3z_zs : a.D;"):
        assert text in zmarch, text
    assert {n: (R.wino_geom(n, 3)["TZ"], R.wino_geom(n, 3)["TY"]) for n in R.WINO_ROWS} == {
        "conv0": (2, 8), "conv2": (2, 8), "conv4": (1, 8), "conv6": (1, 4), "conv6_2d": (1, 4)}
    assert (R.wino_geom("conv2", 1)["TZ"], R.wino_geom("conv2", 1)["TY"]) == (1, 16)
    # one stage fits the LDS twice on every row (resident 512); two stages fit twice on conv2 and the 2D row, once on the others
    assert {n: R.wino_resident(n, 3, 0) for n in R.WINO_ROWS if n != "conv0"} == {n: (512, 1) for n in R.WINO_ROWS if n != "conv0"}
    assert R.wino_resident("conv2", 1, 0) == (512, 1) and R.wino_resident("conv2", 3, 1) == (512, 1)
    assert {n: R.wino_resident(n, 3, 2)[0] for n in R.WINO_ROWS[1:]} == {"conv2": 512, "conv4": 256, "conv6": 256, "conv6_2d": 512}
    assert R.wino_resident("conv2", 1, 2) == (256, 2)
    for n in R.WINO_ROWS[1:]:
        res, st = R.wino_resident(n, 3, 2)
        assert st == 2 and res == 256 * max(1, min(2, R.LDS_BYTES // (2 * R.wino_geom(n, 3)["lds"]))) and 2 * R.wino_geom(n, 3)["lds"] <= R.LDS_BYTES
    assert R.zmarch_resident() == 512 and R.wino_geom("conv0", 5)["lds"] == 34304


def test_packers_accept_exactly_the_rows():
    """K3w's packer (with conv0's (channel, depth tap) order), K3r's and K3z's: a packed length for the rows of ROWS that list the
    form, none for any other shape -- K3w's three FeatureNet rows aside, which tests/featurenet_ref.py owns."""
    L, lib = _lib()
    feature = {(16, 16, 1), (32, 32, 1), (32, 16, 1)}
    for fn, form in (("dmvs_conv3d_wino_weight_floats", "wino"), ("dmvs_conv3d_coarse_weight_floats", "coarse"),
                     ("dmvs_conv3d_zmarch_weight_floats", "zmarch")):
        want = {r[:3] for r in R.ROWS.values() if form in r[3]}
        got = {(ci, co, kd) for ci in (2, 4, 8, 16, 32, 64) for co in (2, 8, 16, 32, 64) for kd in (1, 3) if getattr(lib, fn)(ci, co, kd) > 0}
        assert got - (feature if form == "wino" else set()) == want, (form, got)
    from dmvsnet_amd import ops
    for name, (cin, cout, kd, forms) in R.ROWS.items():
        w = R.make_weight(name)
        for form, pack in (("wino", ops.pack_wino), ("coarse", ops.pack_coarse), ("zmarch", ops.pack_zmarch)):
            p = pack(w, cin, cout, kd)
            assert (p is not None) == (form in forms or (form == "wino" and (cin, cout, kd) in feature)), (name, form)
            assert p is None or torch.isfinite(p).all()
    assert ops.pack_wino(R.make_weight("conv0"), 2, 16, 3).numel() == 2 * 4 * 256      # two k-steps: taps (0, 1), then tap 2 + zeros


# ------------------------------------------------------------------------------------------------ K3w tables
def test_wino_plans_match_the_library():
    L, lib = _lib()
    for name, s in R.wino_cases() + [v[:2] for v in R.WALK.values()] + [("conv2", t) for t in R.ZPAD_SHAPES]:
        cin, cout, kd = R.ROWS[name][:3]
        assert lib.dmvs_conv3d_wino_plan(cin, cout, *s, kd) == R.wino_tiles(name, *s), (name, s)
    for label, (name, s, tiles) in R.WALK.items():
        assert R.wino_tiles(name, *s) == tiles, label
    assert lib.dmvs_conv3d_wino_plan(16, 16, 3, 9, 34, 3) == L.EUNSUPPORTED


def test_small_reaches_what_it_names():
    last = lambda n, t: n - (-(-n // t) - 1) * t  # noqa: E731
    for name in R.WINO_ROWS:
        ty = {s: R.wino_geom(name, s[0])["TY"] for s in R.SMALL}
        assert R.wino_tiles(name, *R.SMALL[0]) == 1                                                         # a single tile
        assert any(-(-s[2] // 32) == 2 and last(s[2], 32) == 4 for s in R.SMALL)                             # a second x tile 4 wide
        assert any(s[1] == ty[s] + 1 for s in R.SMALL), name                                                # H = TY + 1
        if R.wino_geom(name, 3)["TZ"] == 2:                                                                  # odd D: a partial z tile
            assert any(s[0] % 2 == 1 and s[0] > 1 for s in R.SMALL)
    assert R.wino_cfg("conv2", 1) == (3, 1, 1, 1, 2, 1) and R.SMALL[0][0] == 1 and R.wino_cfg("conv2", 2)[3] == 2
    assert all(s[2] % 4 == 0 for s in R.SMALL) and {R.kind_of(*s) for s in R.SMALL} == set(R.KINDS)
    assert all(s in R.SMALL for s in R.Q4_SHAPES) and all(s[1] % 2 == 1 and s[2] % 32 == 4 for s in R.Q4_SHAPES)


def test_zskip_cases_that_are_dispatched():
    """conv2 on K3w: the skipping instantiation at D = 2, 3, 4 and the plain kernel at D = 1 (the flat row) and D = 5.  Of the six
    compiled tile cases zc = 3 (D = 2: the one tile is first and last), 5 and 0 (D = 3: first; the partial last tile), 5 and 2
    (D = 4) run -- zc = 1 (first tile of a depth-1 volume) and zc = 4 (neither first nor near the end: D >= 5) never do."""
    seen = {}
    for s in R.SMALL + tuple(t for t in R.ZPAD_SHAPES):
        D = s[0]
        if not R.wino_zskip("conv2", D):
            assert D in (1, 5)
            continue
        seen.setdefault(D, set()).update(R.wino_zcase(D, oz0) for oz0 in range(0, D, 2))
    assert seen == {2: {3}, 3: {5, 0}, 4: {5, 2}}
    assert not R.wino_zskip("conv2", 3, knob=0) and not any(R.wino_zskip(n, 3) for n in R.WINO_ROWS if n != "conv2")
    # the live pairs of each dispatched case are those of the tile itself
    for D, cases in seen.items():
        for oz0 in range(0, D, 2):
            assert R.wino_zcase_live(R.wino_zcase(D, oz0)) == R.live_mask(R.ZFORM_S1, D, oz0, 2), (D, oz0)
    assert R.wino_zcase_live(3) == 0b011110 and R.wino_zcase_live(0) == 0b000011 and R.wino_zcase_live(2) == 0b011111


def test_walk_reaches_what_it_names():
    last = lambda n, t: n - (-(-n // t) - 1) * t  # noqa: E731
    for label, (name, s, tiles) in R.WALK.items():
        D, H, W = s
        g = R.wino_geom(name, D)
        assert tiles % 8 != 0 and last(W, 32) == 4 and last(H, g["TY"]) == 2, label
        for stages in (0, 1, 2):
            grid = R.wino_grid(name, D, H, W, stages)
            assert tiles > grid and grid in (256, 512), (label, stages)
            walks = [R.xcd_walk(tiles, grid, b) for b in range(grid)]
            assert sorted(t for w in walks for t in w) == list(range(tiles))                # every tile once
            assert max(map(len, walks)) >= 2 and min(map(len, walks)) < max(map(len, walks))
        assert R.wino_grid(name, D, H, W, persistent=0) == 8 * (-(-tiles // 8)) > tiles      # one tile each, the last XCD's eighth short
        per = (tiles + 7) >> 3
        assert tiles - 7 * per < per                                                        # XCD 7 walks fewer tiles than the others
        if name != "conv0":
            assert 16 * D * H * W <= 3.8e6 * 16 / min(16, R.ROWS[name][0]) and R.ROWS[name][1] * D * H * W < 3.8e6
    assert R.wino_grid("conv0", 5, 194, 196, conv0_grid=8) == 8 and R.wino_grid("conv0", 5, 194, 196) == 512
    # conv0 at `wino_conv0_grid` 8: a workgroup walks several tiles at two SMALL shapes already, one of them with a partial z tile
    multi = [s for s in R.SMALL if max(len(R.xcd_walk(R.wino_tiles("conv0", *s), 8, b)) for b in range(8)) >= 2]
    assert multi == [(3, 9, 68), (5, 17, 100)] and all(R.wino_grid("conv0", *s, conv0_grid=8) == 8 for s in multi)
    assert any(s[0] % 2 == 1 and s[0] > 1 for s in R.SMALL)            # ... and its last k-step (tap 2) on a partial z tile
    # the skipping shape: some workgroup meets two different ZSKIP cases on consecutive tiles
    name, s, tiles = R.WALK["conv2.skip"]
    grid = R.wino_grid(name, *s)
    changes = 0
    for b in range(grid):
        zc = [R.wino_zcase(s[0], R.wino_tile_of(name, *s, t)[2]) for t in R.xcd_walk(tiles, grid, b)]
        changes += any(a != c for a, c in zip(zc, zc[1:]))
    assert R.wino_zskip(name, s[0]) and changes > 0
    # tile order: x, z, y on the 3D rows (the second list position row-wise is the next z tile), x, y, z on the 2D row
    assert R.wino_tile_of("conv6", 3, 98, 196, 7) == (0, 0, 1) and R.wino_tile_of("conv6_2d", 3, 98, 196, 7) == (0, 4, 0)
    assert R.wino_tile_of("conv2", 5, 194, 196, 7) == (0, 0, 2) and R.wino_tile_of("conv0", 5, 194, 196, 21) == (0, 8, 0)


# ------------------------------------------------------------------------------------------------ K3r table
def test_coarse_reaches_what_it_names():
    assert {R.coarse_v4_st4(s[2])[0] for s in R.COARSE} == {True, False}                      # both loaders
    assert any(s[1] < 8 and s[2] < 8 for s in R.COARSE)                                       # smaller than one 8 x 8 group
    assert any(s[1] % 8 and s[2] % 8 and s[1] > 8 and s[2] > 8 for s in R.COARSE)             # ragged right and bottom groups
    for name in ("conv4", "conv6"):
        dead = {R.coarse_dead(name, s[0], oz) for s in R.COARSE if R.coarse_skipping(name, s[0], s[2]) for oz in range(s[0])}
        assert dead == {0, 1, 2, 3}, (name, dead)                                              # every dead-tap copy runs
        assert not R.coarse_skipping(name, 5, 23) and not R.coarse_skipping(name, 8, 8)       # D = 5 and D = 8: the plain kernel
        assert any(s[0] == 5 and R.coarse_v4_st4(s[2])[0] for s in R.COARSE)                  # D = 5: the plain kernel on the 16-byte loader
        assert not R.coarse_skipping(name, 3, 12, in_off=1) and R.coarse_skipping(name, 3, 12)   # V4 false: no skipping form
        assert not R.coarse_skipping(name, 2, 7)                                               # the dword loader
    assert all(R.coarse_dead(n, 3, oz) == 0 for n in ("conv4_2d", "conv6_2d") for oz in range(3))
    assert {R.coarse_ncg(n) for n in R.COARSE_ROWS} == {1, 2, 4} and R.coarse_ncg("conv6") == 4
    # the four (V4, st4) combinations are independent at W % 4 == 0
    assert all(s[2] % 4 == 0 for s in R.ALIGNMENT_SHAPES) and all(s in R.COARSE for s in R.ALIGNMENT_SHAPES)
    assert {R.coarse_v4_st4(68, i, o) for i in (0, 1) for o in (0, 1)} == {(True, True), (False, True), (True, False), (False, False)}
    assert all(s[0] <= 4 for s in R.ALIGNMENT_SHAPES)
    # k3r_grid = 32: several units per workgroup with differing dead-tap sets; an XCD whose eighth ends early; an XCD with none
    mixed = short = none = 0
    for name in ("conv4", "conv6"):
        for s in R.COARSE:
            units = R.coarse_units(name, *s, grid=32)
            total = sorted(u for (xcd, cg, slot), us in units.items() if cg == 0 for u in us)
            want = sorted((8 * gx, 8 * gy, z) for gx in range(-(-s[2] // 8)) for gy in range(-(-s[1] // 8)) for z in range(s[0]))
            assert total == want, (name, s)                                                     # every unit once per cout group
            assert all(us == units[xcd, 0, slot] for (xcd, cg, slot), us in units.items())
            per_xcd = {x: sum(len(us) for (xcd, cg, slot), us in units.items() if xcd == x and cg == 0) for x in range(8)}
            short += 0 < min(v for v in per_xcd.values() if v) < max(per_xcd.values())
            none += min(per_xcd.values()) == 0 and max(per_xcd.values()) > 0
            if R.coarse_skipping(name, s[0], s[2]):
                for us in units.values():
                    d = [R.coarse_dead(name, s[0], u[2]) for u in us]
                    mixed += any(a != b for a, b in zip(d, d[1:]))
    assert mixed > 0 and short > 0 and none > 0
    u256 = R.coarse_units("conv6", 4, 10, 68, grid=256)
    assert len(u256) == 256 and sum(map(len, u256.values())) == 4 * 9 * 2 * 4
    assert {R.kind_of(*s) for s in R.COARSE} == set(R.KINDS)


# ------------------------------------------------------------------------------------------------ K3z table
def test_zmarch_reaches_what_it_names():
    lengths, masks = set(), set()
    inside = empty_xcd = empty_share = minus1 = plane_d = mid_start = mid_end = 0
    for s in R.ZMARCH:
        D, H, W = s
        for zs in R.ZMARCH_ZS:
            for grid in R.ZMARCH_GRIDS:
                plan = R.zmarch_plan(D, H, W, grid, zs)
                done = sorted((ox, oy, z) for segs in plan.values() for ox, oy, z0, n in segs for z in range(z0, z0 + n))
                assert done == sorted((8 * gx, 8 * gy, z) for gx in range(-(-W // 8)) for gy in range(-(-H // 8)) for z in range(D)), (s, zs, grid)
                ncols, per = -(-W // 8) * -(-H // 8), (-(-W // 8) * -(-H // 8) + 7) >> 3
                for b, segs in plan.items():
                    if not segs:
                        if ncols - (b & 7) * per <= 0:
                            empty_xcd += 1
                        else:
                            empty_share += 1
                    for ox, oy, z0, n in segs:
                        assert 1 <= n <= (zs or D) and z0 + n <= D
                        lengths.add(min(n, 3))
                        masks.update(R.zmarch_masks(n))
                        assert len(R.zmarch_masks(n)) == n + 2
                        minus1 += z0 == 0
                        plane_d += z0 + n == D
                        mid_start += z0 > 0
                        mid_end += z0 + n < D
                    if zs == 0 and segs:       # no cap: a segment is cut by the plane range alone
                        first, lastseg = segs[0], segs[-1]
                        inside += first[2] > 0 and lastseg[2] + lastseg[3] < D
    assert lengths == {1, 2, 3} and masks == {1, 2, 3, 4, 6, 7}
    assert inside > 0 and empty_xcd > 0 and empty_share > 0 and minus1 > 0 and plane_d > 0 and mid_start > 0 and mid_end > 0
    assert all(s[2] % 4 == 0 for s in R.ZMARCH) and any(s[0] >= R.ZMARCH_MIN_DEPTH for s in R.ZMARCH) and any(s[0] < R.ZMARCH_MIN_DEPTH for s in R.ZMARCH)
    assert R.zmarch_masks(1) == [1, 2, 4] and R.zmarch_masks(2) == [1, 3, 6, 4] and R.zmarch_masks(4) == [1, 3, 7, 7, 6, 4]
    assert R.zmarch_grid(1, 1, 4) == 8 and R.zmarch_grid(9, 10, 68, 64) == 64 and R.zmarch_grid(9, 10, 68) == 168


# ------------------------------------------------------------------------------------------------ knobs
def test_tune_ranges():
    L, lib = _lib()
    bad = {"wino_stages": (-1, 3), "wino_conv0_grid": (0, 4, 12), "k3r_grid": (0, 16, 48, 1056), "k3z_grid": (-8, 12, 4104), "k3z_zs": (-1, 65),
           "zpad_skip": (2,)}
    good = {"wino_stages": (0, 1, 2), "wino_conv0_grid": (8, 512), "k3r_grid": (32, 256, 1024), "k3z_grid": (0, 8, 16, 64, 4096),
            "k3z_zs": (0, 1, 2, 3, 5, 64), "zpad_skip": (0, 1), "wino_persistent": (0, 1), "k3r_counted_wait": (0, 1)}
    try:
        for k, vs in bad.items():
            for v in vs:
                assert lib.dmvs_tune(k.encode(), v) == L.EINVAL, (k, v)
        for k, vs in good.items():
            for v in vs:
                assert lib.dmvs_tune(k.encode(), v) == 0, (k, v)
        assert set(good) == set(R.KNOB_DEFAULTS)
        assert all(g in good["k3z_grid"] for g in R.ZMARCH_GRIDS) and all(z in good["k3z_zs"] for z in R.ZMARCH_ZS)
        assert all(g in good["k3r_grid"] for g in R.COARSE_GRIDS)
    finally:
        for k, v in R.KNOB_DEFAULTS.items():
            assert lib.dmvs_tune(k.encode(), v) == 0


# ------------------------------------------------------------------------------------------------ emulation
WORST = {"max": (0.0, ""), "mean": (0.0, ""), "e_ref_lo": (float("inf"), ""), "e_ref_hi": (0.0, "")}


@pytest.mark.parametrize("name,shape", R.gpu_cases(), ids=IDS)
def test_emulation_is_inside_the_plain_bound(name, shape):
    """fp32 Winograd with the longest serial accumulation chain against float64, on the GPU file's own inputs, BatchNorm + ReLU and
    raw: inside bounds(e_ref) on max and mean -- the kernels get the plain bound with no allowance."""
    x, w, scale, shift = R.case(name, *shape)
    raw = R.wino_emulate(name, x, w)
    for bn in (True, False):
        f64, e_ref = R.reference(name, *shape, bn)[:2]
        got = R._bn_relu_skip(raw, scale, shift, True, None, F32) if bn else raw
        e, b = R.errors(got, f64), R.bounds(e_ref)
        tag = f"{name} {IDS(shape)} {'bn' if bn else 'raw'}"
        print(f"WINOCONV emulation {tag}: e max {e[0] / EPS32:.2f} eps mean {e[1] / EPS32:.3f} eps  e_ref max {e_ref[0] / EPS32:.2f} eps  "
              f"ratio max {e[0] / b[0]:.3f} mean {e[1] / b[1]:.3f}")
        for key, v in (("max", e[0] / b[0]), ("mean", e[1] / b[1]), ("e_ref_hi", e_ref[0] / EPS32)):
            if v > WORST[key][0]:
                WORST[key] = (v, tag)
        if e_ref[0] / EPS32 < WORST["e_ref_lo"][0]:
            WORST["e_ref_lo"] = (e_ref[0] / EPS32, tag)
        assert got.dtype == F32 and e[0] <= b[0] and e[1] <= b[1], (tag, e, e_ref)
    # the float64 emulation is the yardstick itself: the Winograd form is restated correctly
    if shape[0] * shape[1] * shape[2] <= 20000:
        f64 = R.reference(name, *shape, False)[0]
        assert (R.wino_emulate(name, x, w, dtype=F64) - f64).abs().max().item() <= 1e-12 * f64.abs().max().item()


def test_emulation_summary():
    print(f"WINOCONV emulation worst distance / bound: max {WORST['max'][0]:.3f} ({WORST['max'][1]})  mean {WORST['mean'][0]:.3f} "
          f"({WORST['mean'][1]});  e_ref max from {WORST['e_ref_lo'][0]:.2f} eps ({WORST['e_ref_lo'][1]}) to {WORST['e_ref_hi'][0]:.2f} eps "
          f"({WORST['e_ref_hi'][1]})")
    assert WORST["max"][0] <= 1.0 and WORST["mean"][0] <= 1.0


@pytest.mark.parametrize("name,form,shape", [c for c in R.EXACT if c[2][1] * c[2][2] < 20000], ids=IDS)
def test_integer_cases_are_exact_in_fp32(name, form, shape):
    """Integer inputs and weights, and the impulse input: fp32 Winograd equals float64 to the last bit, so the GPU file may ask the
    kernels for torch.equal."""
    kd = R.ROWS[name][2]
    for x, w in (R.exact_case(name, *shape), R.impulse_case(name, *shape)):
        want = R.conv3d(x, w, 1, kd)
        assert torch.equal(want, want.round()) and want.abs().max().item() < 2 ** 22
        assert torch.equal(R.wino_emulate(name, x, w).double(), want)
        G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=F64)
        U = torch.einsum("ai,ockij,bj->ockab", G, w.double(), G)
        assert torch.equal(U * 4, (U * 4).round())
    x, w = R.impulse_case(name, *shape)
    assert w[0, 0].unique().numel() == 9 * kd and len(R.impulse_positions(name, *shape)) >= 2


def test_exact_table_covers_every_form():
    assert {(n, f) for n, f, _ in R.EXACT} == {(n, f) for n, r in R.ROWS.items() for f in r[3]}
    walk = {(v[0], v[1]) for v in R.WALK.values()}
    assert any((n, s) in walk and n == "conv0" for n, f, s in R.EXACT) and any((n, s) in walk and f == "wino" and n != "conv0" for n, f, s in R.EXACT)
    tables = {"wino": R.SMALL + tuple(v[1] for v in R.WALK.values()), "coarse": R.COARSE + ((3, 98, 196),), "zmarch": R.ZMARCH}
    assert all(s in tables[f] for n, f, s in R.EXACT)


# ------------------------------------------------------------------------------------------------ mutations
LOWEST = {}


@pytest.mark.parametrize("mutation", list(R.MUTATIONS))
def test_mutations_are_caught(mutation):
    low, runs = (float("inf"), None), 0
    for name, shapes, param in R.MUTATIONS[mutation]:
        assert shapes, (mutation, name)
        for D, H, W in shapes:
            x, w, scale, shift = R.case(name, D, H, W)
            f64, e_ref = R.reference(name, D, H, W, True)[:2]
            plain = R.wino_emulate(name, x, w, scale, shift, True)
            e, b = R.errors(plain, f64), R.bounds(e_ref)
            assert e[0] <= b[0] and e[1] <= b[1], "the unmutated emulation passes"
            m, p = R.mutation_args(mutation, name, (D, H, W), param)
            ratio = R.errors(R.mutate(name, m, p, x, w, scale, shift, True), f64)[0] / R.bound_of(e_ref[0])
            low = min(low, (ratio, f"{name} {D}x{H}x{W}"))
            runs += 1
    LOWEST[mutation] = low
    print(f"WINOCONV mutation {mutation}: smallest ratio to the bound {low[0]:.3g} ({low[1]}) over {runs} runs")
    assert runs >= 2 and low[0] >= R.MUTATION_RATIO


def test_mutation_list_covers_the_issue():
    assert len(R.MUTATIONS) == 11
    assert all(n in R.ROWS and shapes for v in R.MUTATIONS.values() for n, shapes, _ in v)
    if len(LOWEST) == len(R.MUTATIONS):
        m = min(LOWEST, key=lambda k: LOWEST[k][0])
        print(f"WINOCONV smallest mutation ratio: {LOWEST[m][0]:.3g} ({m}, {LOWEST[m][1]})")


def test_knobs_are_back_at_their_defaults():
    """Last in the file: the library has no getter, so the knobs are set once more."""
    L, lib = _lib()
    for k, v in R.KNOB_DEFAULTS.items():
        assert lib.dmvs_tune(k.encode(), v) == 0
