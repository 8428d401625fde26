"""The yardstick of the FeatureNet kernels (tests/featurenet_ref.py) held to ATen, to the oracle and to the recorded reference
outputs; what its case tables claim; and the mistakes the criterion tells apart.  CPU only: no kernel runs here (the plans and the
knobs are host functions of the library).

  restatement  float64 ``conv`` / ``up2_add`` / ``fpn_head`` against F.conv2d / F.interpolate and ``fpn`` against the oracle's
               feature_net, all in float64 (1e-12); the fp32 restatement against tests/golden/op_featurenet.npz within the criterion.
  tables       K3s seam classes per (c8_rows, H), strip seams, the launcher's own R; K3's tile form under each knob setting
               (dmvs_conv3d_mfma_plan) and the tile residues of each shape; K3w's and the level-3 kernel's tile counts against their
               persistent grids; which NET case takes the fused level 3.  Every class a table names has a case.
  knobs        dmvs_tune rejects out-of-range values and the defaults come back.
  mutations    each mistake of featurenet_ref.MUTATIONS built into the fp32 restatement, on the table meant to catch it: at least
               20 times bound_of(e_ref) away from the yardstick.  The smallest ratio is printed.
  Winograd     F(2x2, 3x3) in fp32 with the kernels' transforms obeys the PLAIN criterion on the WINO_2D and FPN inputs: the
               Winograd kernels get no allowance."""
import os

import pytest
import torch
import torch.nn.functional as F

import featurenet_ref as R

F64, F32 = R.F64, R.F32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dmvsnet_amd", "csrc")


def _close64(a, b, tol=1e-12):
    assert a.dtype == F64 and b.dtype == F64 and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return (a - b).abs().max().item() <= tol * max(b.abs().max().item(), 1e-300)


def _lib():
    from dmvsnet_amd import _lib
    return _lib, _lib.load()


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("name", list(R.K3_ROWS))
def test_conv_against_aten_in_float64(name):
    cin, cout, mode, k, _ = R.K3_ROWS[name]
    cin = 3 if name == "conv0.0" else cin
    stride = 2 if mode == R.CONV2D_K5S2 else 1
    for V, H, W in R.k3_shapes(name):
        x, w, scale, shift = R.conv_case(cin, cout, k, V, H, W)
        y = R.conv(x, w, stride, scale, shift, True)
        want = torch.relu(F.conv2d(x.double().permute(1, 0, 2, 3), w.double(), None, stride, k // 2) * scale.double().view(1, -1, 1, 1)
                          + shift.double().view(1, -1, 1, 1)).permute(1, 0, 2, 3)
        assert tuple(y.shape) == (cout, V, (H + 1) // 2 if stride == 2 else H, (W + 1) // 2 if stride == 2 else W)
        assert _close64(y, want), (name, V, H, W)
        assert _close64(R.aten_conv(x, w, stride, scale, shift, True, F64), want)
        assert R.conv(x, w, stride, scale, shift, True, F32).dtype == F32


def test_up2_fused_and_fpn_head_against_aten_in_float64():
    for name, (V, H, W) in R.k3_skip_cases():
        cin, cout = R.K3_ROWS[name][:2]
        x, w, scale, shift, sk = R.skip_case(cin, cout, V, H, W)
        up = F.interpolate(sk.double().permute(1, 0, 2, 3), scale_factor=2, mode="nearest").permute(1, 0, 2, 3)
        want = F.conv2d(x.double().permute(1, 0, 2, 3), w.double(), shift.double()).permute(1, 0, 2, 3) + up
        assert _close64(R.up2_add(R.conv(x, w, 1, scale, shift), sk), want), (name, V, H, W)
    for V, H, W in ((2, 5, 61), (1, 9, 62), (1, 1, 1)):
        x, l0, l1 = R.fused_case(V, H, W)
        assert _close64(R.fused_conv0(x, l0, l1), R.aten_fused_conv0(x, l0, l1, F64))
    for V, H, W in R.FPN_SHAPES[:4]:
        lat, td, w_lat, b_lat, w3 = R.fpn_case(V, H, W)
        intra = F.conv2d(lat.double().permute(1, 0, 2, 3), w_lat.double()[:, :, None, None], b_lat.double()) + \
            F.interpolate(td.double().permute(1, 0, 2, 3), scale_factor=2, mode="nearest")
        want = F.conv2d(intra, w3.double(), None, 1, 1).permute(1, 0, 2, 3)
        assert _close64(R.fpn_head(lat, td, w_lat, b_lat, w3), want), (V, H, W)
        assert _close64(R.wino_fpn_head(lat, td, w_lat, b_lat, w3, F64), want, 1e-11), (V, H, W)
    x, w, _, _ = R.conv_case(16, 16, 3, 2, 17, 36, False)
    assert _close64(R.wino_conv(x, w, F64), R.conv(x, w), 1e-11)


def test_q4_layout_both_ways():
    p = torch.arange(16 * 2 * 3 * 5, dtype=F32).view(16, 2, 3, 5)
    q = R.planar_to_q4(p)
    assert tuple(q.shape) == (2, 2, 2, 3, 5, 4)
    for c, v, y, x in ((0, 0, 0, 0), (5, 1, 2, 3), (9, 0, 1, 4), (15, 1, 2, 4)):
        assert q[c // 8, v, (c % 8) // 4, y, x, c % 4] == p[c, v, y, x]
    assert torch.equal(R.q4_halves_to_planar(q), p)
    assert not torch.equal(R.q4_halves_to_planar(q, "q4_halves_swapped"), p)
    assert not torch.equal(R.q4_halves_to_planar(q, "q4_perm"), p)


@pytest.mark.parametrize("V,H,W", [(2, 8, 12), (1, 20, 44)])
def test_fpn_against_the_oracle_in_float64(V, H, W):
    from oracle import dmvs_oracle as O
    sd, imgs = R.net_state_dict(), R.net_images(V, H, W)
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    o = O.feature_net(sd64, imgs.double())
    for k, y in zip((1, 2, 3), R.fpn(sd, imgs)):
        want = torch.cat((o[f"stage{k}"], o[f"stage{k}_c"]), 1).permute(1, 0, 2, 3)
        assert tuple(y.shape) == (64 >> (k - 1), V, H >> (3 - k), W >> (3 - k))
        assert _close64(y, want), k


def test_fpn_against_the_recorded_reference_outputs(golden):
    """Stored: what the reference computed in fp32 on its own weights.  The float64 restatement is its exact-arithmetic value; the
    stored tensors and the fp32 restatement lie within the criterion of it, e_ref from the fp32 oracle."""
    from dmvsnet_amd import MVSNet, synth
    g = golden("op_featurenet.npz")
    net = MVSNet([8], [4], verbose=False)
    sd = synth.synth_state_dict(net.state_dict(), int(g["seed"]))
    img = torch.from_numpy(g["img"])
    f64, f32, ora = R.fpn(sd, img), R.fpn(sd, img, F32), R.oracle_fpn(sd, img)
    for k in (1, 2, 3):
        stored = torch.cat((torch.from_numpy(g[f"stage{k}"]), torch.from_numpy(g[f"stage{k}_c"])), 1).permute(1, 0, 2, 3)
        b = R.bounds(R.errors(ora[k - 1], f64[k - 1]))
        for what, t in (("stored", stored), ("fp32 restatement", f32[k - 1])):
            e = R.errors(t, f64[k - 1])
            print(f"FEAT recorded stage{k} {what}: e {e[0]:.3e} / {e[1]:.3e}  bound {b[0]:.3e} / {b[1]:.3e}")
            assert e[0] <= b[0] and e[1] <= b[1], (k, what, e, b)


# ------------------------------------------------------------------------------------------------ tables
def test_c8_tables():
    Rs = []
    for value in R.C8_ROWS:
        for V, H, W in R.C8_SHAPES:
            r = R.c8_rows_of(value, V, H, W)
            assert r % R.C8_NS == 0 and r == (8 if value == 0 else -(-value // 4) * 4), (value, V, H, W, r)
            for Wf in R.FUSED_W:      # the fused kernel: the same R (rounded to 4 again), strips of 60
                assert R.c8_rows_of(value, V, H, Wf, R.STRIPF) == r
        Rs.append(r)
    assert sorted(Rs) == [4, 8, 12, 20, 32]
    # the product's own choice at config 2 (5 x 1184 x 1600) is none of the multiples of 8 below 24: what the knob is there for
    assert R.c8_rows_of(0, 5, 1184, 1600) == 20 and R.c8_rows_of(0, 5, 1184, 1600, R.STRIPF) == 20
    hs = sorted({H for _, H, _ in R.C8_SHAPES})
    assert hs == sorted(H for _, H in R.fused_vh())
    seen = set()
    for r in Rs:
        for H in hs:
            seen |= R.c8_seam_classes(r, H)
    assert seen == set(R.C8_SEAM_CLASSES), seen
    # without (1,22,3) no H of the issue's eight shapes is two rows into a last block at any R of C8_ROWS
    assert not any("last+2" in R.c8_seam_classes(r, H) for r in Rs for H in hs if H != 22)
    for r in Rs:     # every R has H < R, H = R + 1 and one row into the last block
        assert {"H<R", "H=R+1", "last+1"} <= set().union(*(R.c8_seam_classes(r, H) for H in hs)), r
    ws = {W for _, _, W in R.C8_SHAPES}
    assert {R.STRIP - 1, R.STRIP, R.STRIP + 1, 2 * R.STRIP, 2 * R.STRIP + 1, 3 * R.STRIP + 1} <= ws and {1, 2} <= ws
    assert any(V >= 3 for V, _, _ in R.C8_SHAPES) and any(V == 2 and W > R.STRIP for V, _, W in R.C8_SHAPES)
    assert {1, 2, 59, 60, 61, 62, 119, 120, 121, 181} == set(R.FUSED_W) and R.STRIPF == 60
    src = open(os.path.join(CSRC, "conv2d_c8.hip")).read()
    assert "constexpr int STRIP = 62;" in src and "constexpr int STRIPF = 60;" in src and "#define C8_NS 4" in src


@pytest.fixture
def knobs():
    """Sets dmvs_tune knobs and puts the defaults back."""
    L, lib = _lib()

    def put(**kw):
        for k, v in kw.items():
            if v is not None:
                L.check(lib.dmvs_tune(k.encode(), v), f"dmvs_tune({k})")
    yield put
    for k, v in {**R.K3_DEFAULTS, "c8_rows": 0, "wino_persistent": 1, "wino_stages": 0}.items():
        assert lib.dmvs_tune(k.encode(), v) == 0


def _plan(lib, name, V, H, W):
    cin, cout, mode, _, _ = R.K3_ROWS[name]
    return lib.dmvs_conv3d_mfma_plan(cin, cout, V, H, W, mode, 1)


def test_k3_2d_tables(knobs):
    L, lib = _lib()
    assert len(R.K3_ROWS) == 10
    src = open(os.path.join(CSRC, "conv3d_mfma.hip")).read()
    for name, (cin, cout, mode, k, MB) in R.K3_ROWS.items():
        tag = {R.CONV_S1: "DMVS_CONV_S1", R.CONV2D_K5S2: "DMVS_CONV2D_K5S2", R.CONV2D_K1: "DMVS_CONV2D_K1"}[mode]
        assert f"{{{cin}, {cout}, {tag}, 1, {32 if cout >= 32 else 16}, {MB}," in src, name     # the row of kCfgs
        assert lib.dmvs_conv3d_mfma_weight_floats(cin, cout, mode, 1) > 0
    forms_seen = set()
    for name, (V, H, W) in R.k3_2d_cases():
        for form in R.k3_forms(name):
            mb, sb = R.K3_KNOBS[form]
            knobs(**R.K3_DEFAULTS)
            knobs(k3_min_blocks=mb, k3_split_blocks=sb)
            plan = _plan(lib, name, V, H, W)
            tz, ty, split = R.k3_expected_plan(name, form)
            assert plan >= 0 and (plan & 0xffff) == tz * 256 + ty and bool(plan & R.PLAN_MBS) == bool(split), (name, form, V, H, W, hex(plan))
            assert bool(plan & R.PLAN_V4) == (W % 4 == 0)
            forms_seen.add((tz, ty, split))
    assert forms_seen == {(1, 16, 0), (1, 8, 0), (1, 4, 0), (1, 2, 1)}
    knobs(**R.K3_DEFAULTS)
    # out1's three forms are three different tiles; every other row's default is its plain small tile at these sizes
    assert len({R.k3_expected_plan("out1", f) for f in R.k3_forms("out1")}) == 3
    for name, (V, H, W) in R.k3_2d_cases():
        if name != "out1":
            assert (_plan(lib, name, V, H, W) & 0x2ffff) == 256 + 4
    # the product's level-3 shape of config 2 takes the big tile by itself: 18.5 tile rows x 12.5 tile columns
    assert (_plan(lib, "conv2.x", 5, 296, 400) & 0x2ffff) == 256 + 16 and 296 / 16 == 18.5 and 400 / 32 == 12.5
    # what each shape is there for
    s1 = R.K3_S1_SHAPES
    assert s1[0][2] == 32 + 4 and s1[0][1] == 16 + 1 == 4 * 4 + 1 and s1[0][0] > 1
    assert s1[1][2] % 4 == 1 and s1[2][2] % 4 == 2 and s1[2][1] == 2 * 16 + 1
    assert -(-s1[3][2] // 32) == 3 and s1[3][2] % 32 == 4 and s1[3][1] == 4 and s1[4] == (1, 1, 1)
    assert {W % 4 == 0 for _, _, W in s1} == {True, False}
    out = tuple(((H + 1) // 2, (W + 1) // 2) for _, H, W in R.K3_K5S2_SHAPES)
    assert out == R.K3_K5S2_OUT
    k5 = R.K3_K5S2_SHAPES
    assert k5[1][1] % 2 == 1 and k5[1][2] % 2 == 1 and out[1][1] % 4 != 0 and out[0][1] > 32
    assert -(-out[2][1] // 32) == 3 and out[2][1] % 32 == 1 and out[2][0] == 2 * 8 + 1 and out[2][0] % 4 == 1
    assert {W % 4 == 0 for _, _, W in k5} == {True, False}
    for _, H, W in R.K3_SKIP_SHAPES:
        assert H % 2 == 0 and W % 2 == 0
    assert any(W > 64 for _, _, W in R.K3_SKIP_SHAPES) and any(H > 32 for _, H, _ in R.K3_SKIP_SHAPES)
    assert [n for n, v in R.K3_ROWS.items() if v[1] % 8 == 0] == list(R.K3_ROWS)    # OUT_Q4 applies to every row


def test_wino_and_fpn_tables():
    L, lib = _lib()
    src = open(os.path.join(CSRC, "conv3d_wino.hip")).read()
    assert "const unsigned resident = 256u * (unsigned)std::max<size_t>(1, std::min<size_t>(2, (160 * 1024) / lds));" in src
    assert "std::min(xcd_grid(a.nx * a.ny * a.nz), g_wino_persistent ? resident : 0xffffffffu)" in src
    assert "const unsigned grid = std::min(xcd_grid(a.nx * a.ny * a.nz), 256u);" in src        # dmvs_conv3d_wino_fpn2
    multi = ragged_eighths = 0
    for name, (V, H, W) in R.wino_cases():
        cin, cout, ty = R.WINO_ROWS[name]
        plan = lib.dmvs_conv3d_wino_plan(cin, cout, V, H, W, 1)
        assert plan == R.wino_tiles(name, V, H, W) and W % 4 == 0, (name, V, H, W, plan)
        if (V, H, W) in R.WINO_MULTI[ty]:
            multi += 1
            assert plan in (8 * 7 * 11, 7 * 7 * 11) and plan > R.WINO_RESIDENT
            ragged_eighths += plan % 8 != 0         # (616 = 8 x 77 fills every XCD's eighth; 539 does not)
            assert H % ty == 2 and W % 32 == 4      # last tile: 2 rows x 4 columns
        else:
            assert plan <= R.WINO_RESIDENT
            assert H % ty != 0 or W % 32 != 0       # ragged
    assert multi == 6 and ragged_eighths == 3 and {ty for _, _, ty in R.WINO_ROWS.values()} == {16, 8}
    for V, H, W in R.FPN_SHAPES:
        assert H % 2 == 0 and W % 8 == 0
    tiles = [R.fpn_tiles(*s) for s in R.FPN_SHAPES]
    assert tiles[-1] == 6 * 6 * 9 == 324 and tiles[-1] > R.FPN_GRID and tiles[-1] % 8 != 0 and all(t <= R.FPN_GRID for t in tiles[:-1])
    V, H, W = R.FPN_SHAPES[-1]
    assert H % 16 == 2 and W % 32 == 8              # last tile: 2 rows x 8 columns
    assert any(H % 16 and W % 32 for _, H, W in R.FPN_SHAPES[:-1])
    kinds = {(H % 2 == 1, W % 8 == 4) for _, H, W in R.FPN_DECLINED}
    assert kinds == {(True, False), (False, True), (True, True)}


def test_net_table():
    fused = {s: R.net_level3_fused(s[1], s[2]) for s in R.NET_SHAPES}
    assert fused == {(2, 36, 72): True, (1, 20, 44): False, (3, 64, 136): True}
    assert R.NET_SHAPES[1][2] & 7 == 4
    for V, H, W in R.NET_SHAPES:
        assert H % 4 == 0 and W % 4 == 0
    assert (36 // 4, 72 // 4) == (9, 18) and 18 % 4 != 0 and (20 // 4, 44 // 4) == (5, 11)      # level 1: the dword loader
    assert any(V == 3 for V, _, _ in R.NET_SHAPES)


def test_tune_rejects_out_of_range_and_restores(knobs):
    L, lib = _lib()
    for name, bad in (("c8_rows", -1), ("c8_rows", 4097), ("k3_min_blocks", -1), ("k3_split_blocks", -1), ("wino_stages", -1),
                      ("wino_stages", 3)):
        assert lib.dmvs_tune(name.encode(), bad) == L.EINVAL, (name, bad)
    assert lib.dmvs_tune(b"c8_row", 8) == L.EUNSUPPORTED
    # a rejected value changes nothing, an accepted one does, and the defaults come back
    assert (_plan(lib, "out1", 2, 17, 36) & 0x2ffff) == (R.PLAN_MBS | 256 + 2)
    knobs(k3_min_blocks=0)
    assert lib.dmvs_tune(b"k3_min_blocks", -5) == L.EINVAL
    assert (_plan(lib, "out1", 2, 17, 36) & 0x2ffff) == 256 + 16
    knobs(**R.K3_DEFAULTS)
    assert (_plan(lib, "out1", 2, 17, 36) & 0x2ffff) == (R.PLAN_MBS | 256 + 2)
    for name, ok in (("c8_rows", 4096), ("c8_rows", 0), ("wino_stages", 2), ("wino_stages", 0), ("wino_persistent", 0), ("wino_persistent", 1)):
        assert lib.dmvs_tune(name.encode(), ok) == 0


# ------------------------------------------------------------------------------------------------ mutations
def _ratio(mut, f64, e_ref):
    return R.errors(mut, f64)[0] / R.bound_of(e_ref[0])


def _passes(a, f64, e_ref):
    e, b = R.errors(a, f64), R.bounds(e_ref)
    return e[0] <= b[0] and e[1] <= b[1]


def _c8_runs(mutation):
    """(mutated fp32, plain fp32, f64, e_ref) on the C8 cases the mistake shows on."""
    for cin in (3, 8):
        for V, H, W in R.C8_SHAPES:
            params = [None]
            if mutation == "strip_edge":
                params = [R.STRIP] if W > R.STRIP else []
            elif mutation == "halo_row_zero":
                params = [r for r in (4, 8, 12, 20, 32) if H > r]
            elif mutation == "view_bleed":
                params = [None] if V > 1 else []
            elif H * W < 64:
                params = []
            x, w, scale, shift = R.conv_case(cin, 8, 3, V, H, W)
            f64, e_ref = R.conv_reference(cin, 8, 3, 1, V, H, W)
            for prm in params:
                yield R.conv(x, w, 1, scale, shift, True, F32, mutation, prm), R.conv(x, w, 1, scale, shift, True, F32), f64, e_ref


def _fused_runs(mutation):
    inner = {"strip_edge_fused": "strip_edge", "halo_row_zero_fused": "halo_row_zero"}.get(mutation, mutation)
    for W in R.FUSED_W:
        for V, H in R.fused_vh():
            params = [None]
            if inner == "strip_edge":
                params = [R.STRIPF] if W > R.STRIPF else []
            elif inner == "halo_row_zero":
                params = [r for r in (4, 8, 12, 20, 32) if H > r]
            x, l0, l1 = R.fused_case(V, H, W)
            f64, e_ref = R.fused_reference(V, H, W)
            for prm in params:
                yield R.fused_conv0(x, l0, l1, F32, inner, prm), R.fused_conv0(x, l0, l1, F32), f64, e_ref


def _k3_runs(mutation):
    if mutation == "in_views_ch4":
        cases = [("conv0.0", s) for s in R.K3_S1_SHAPES if s[0] > 1]
    elif mutation.startswith("k5s2"):
        cases = [(n, s) for n in ("conv1.0", "conv2.0") for s in R.K3_K5S2_SHAPES if s[1] % 2 or s[2] % 2]
    else:
        cases = [(n, s) for n, s in R.k3_2d_cases() if s[1] * s[2] >= 64]
    for name, (V, H, W) in cases:
        cin, cout, mode, k, _ = R.K3_ROWS[name]
        cin = 3 if name == "conv0.0" else cin
        stride = 2 if mode == R.CONV2D_K5S2 else 1
        x, w, scale, shift = R.conv_case(cin, cout, k, V, H, W)
        f64, e_ref = R.conv_reference(cin, cout, k, stride, V, H, W)
        plain = R.conv(x, w, stride, scale, shift, True, F32)
        if mutation.startswith("q4"):
            yield R.q4_halves_to_planar(R.planar_to_q4(plain), mutation), R.q4_halves_to_planar(R.planar_to_q4(plain)), f64, e_ref
        else:
            yield R.conv(x, w, stride, scale, shift, True, F32, mutation), plain, f64, e_ref


def _skip_runs(mutation):
    for name, (V, H, W) in R.k3_skip_cases():
        cin, cout = R.K3_ROWS[name][:2]
        x, w, scale, shift, sk = R.skip_case(cin, cout, V, H, W)
        f64, e_ref = R.skip_reference(cin, cout, V, H, W)
        y = R.conv(x, w, 1, scale, shift, False, F32)
        yield R.up2_add(y, sk, mutation), R.up2_add(y, sk), f64, e_ref


def _fpn_runs(mutation):
    inner = "up2_round" if mutation == "up2_round_fpn" else mutation
    for V, H, W in R.FPN_SHAPES:
        c = R.fpn_case(V, H, W)
        f64, e_ref = R.fpn_reference(V, H, W)
        yield R.fpn_head(*c, dtype=F32, mutation=inner), R.fpn_head(*c, dtype=F32), f64, e_ref


RUNS = {"C8": _c8_runs, "FUSED": _fused_runs, "K3_2D": _k3_runs, "K3_SKIP": _skip_runs, "FPN": _fpn_runs}


@pytest.mark.parametrize("mutation", list(R.MUTATIONS))
def test_mutations_are_caught(mutation):
    low, runs = float("inf"), 0
    for mut, plain, f64, e_ref in RUNS[R.MUTATIONS[mutation]](mutation):
        assert _passes(plain, f64, e_ref), "the unmutated fp32 restatement passes"
        low = min(low, _ratio(mut, f64, e_ref))
        runs += 1
    print(f"FEAT mutation {mutation} ({R.MUTATIONS[mutation]}): smallest ratio to the bound {low:.3g} over {runs} runs")
    assert runs >= 2 and low >= R.MUTATION_RATIO


def test_mutation_list_covers_the_issue():
    assert set(R.MUTATIONS.values()) == set(RUNS)
    assert len(R.MUTATIONS) == 17


# ------------------------------------------------------------------------------------------------ Winograd in fp32
def test_winograd_fp32_obeys_the_plain_criterion():
    """The justification of the plain bound for K3w and fpn_wino_kernel: their arithmetic, emulated in fp32 on the CPU, stays under
    bounds(e_ref) on the very inputs the GPU file uses -- no allowance."""
    worst = [0.0, 0.0]
    for name, (V, H, W) in R.wino_cases():
        cin, cout, _ = R.WINO_ROWS[name]
        bn = R.WINO_BN[name]
        x, w, scale, shift = R.conv_case(cin, cout, 3, V, H, W, bn)
        f64, e_ref = R.conv_reference(cin, cout, 3, 1, V, H, W, bn)
        y = R.wino_conv(x, w)
        if bn:
            y = torch.relu(y * scale.view(-1, 1, 1, 1) + shift.view(-1, 1, 1, 1))
        e, b = R.errors(y, f64), R.bounds(e_ref)
        worst = [max(worst[0], e[0] / b[0]), max(worst[1], e[1] / b[1])]
        assert e[0] <= b[0] and e[1] <= b[1], (name, V, H, W, e, b)
    for V, H, W in R.FPN_SHAPES:
        c = R.fpn_case(V, H, W)
        f64, e_ref = R.fpn_reference(V, H, W)
        e, b = R.errors(R.wino_fpn_head(*c), f64), R.bounds(e_ref)
        worst = [max(worst[0], e[0] / b[0]), max(worst[1], e[1] / b[1])]
        assert e[0] <= b[0] and e[1] <= b[1], ("fpn", V, H, W, e, b)
    print(f"FEAT winograd fp32 emulation: worst e / bound  max {worst[0]:.3f}  mean {worst[1]:.3f}")
