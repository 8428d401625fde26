"""The yardstick of K3's regularisation convs (tests/regconv_ref.py) held to ATen in float64; what its case tables claim; the tile
form the library picks under each knob setting; and the mistakes the criterion tells apart.  CPU only: no kernel runs here (the plan,
the knobs, the packer and zpad_live_mask are host functions of the library).

  restatement  float64 ``conv3d`` / ``deconv3d`` against F.conv3d / F.conv_transpose3d in float64 (1e-12) on every row and shape.
  tables       every claim of the case tables from the restated tile geometry: x seams, partial y tiles at which TY, partial z
               tiles, the loader, the 16-byte stores; every (row, form, shape) plan against dmvs_conv3d_mfma_plan; the skipping
               condition against the marked shapes and against the library's dmvs_zpad_live_mask.
  e_ref        fp32 ATen against the yardstick, max and mean per row (printed).
  mutations    each mistake of regconv_ref.MUTATIONS built into the fp32 restatement: at least 20 times bound_of(e_ref) away from
               the yardstick on every row and shape it applies to.  The smallest ratio is printed.
  packing      ops.pack_mfma followed by the un-pack restated from the packer's three orders returns the weights."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import regconv_ref as R

F64, F32 = R.F64, R.F32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dmvsnet_amd", "csrc")
EPS32 = 2.0 ** -23
IDS = lambda v: v if isinstance(v, str) else "x".join(map(str, v))  # noqa: E731


def _close64(a, b, tol=1e-12):
    assert a.dtype == F64 and b.dtype == F64 and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return (a - b).abs().max().item() <= tol * max(b.abs().max().item(), 1e-300)


def _lib():
    from dmvsnet_amd import _lib
    return _lib, _lib.load()


@pytest.fixture
def knobs():
    """Sets dmvs_tune knobs and puts the defaults back."""
    L, lib = _lib()

    def put(**kw):
        for k, v in kw.items():
            if v is not None:
                L.check(lib.dmvs_tune(k.encode(), v), f"dmvs_tune({k})")
    yield put
    for k, v in R.KNOB_DEFAULTS.items():
        assert lib.dmvs_tune(k.encode(), v) == 0


# ------------------------------------------------------------------------------------------------ restatement
@pytest.mark.parametrize("name", list(R.ROWS))
def test_restatement_against_aten_in_float64(name):
    cin, cout, mode, kd = R.ROWS[name][:4]
    for D, H, W in R.shapes_of(name):
        x, w, scale, shift, skip = R.case(name, D, H, W)
        x5, w5 = x.double()[None], w.double()
        if mode == R.DECONV_S2:
            y = F.conv_transpose3d(x5, w5, None, 2, 1, 1) if kd == 3 else F.conv_transpose3d(x5, w5, None, (1, 2, 2), (0, 1, 1), (0, 1, 1))
        else:
            s = R.stride_of(name)
            y = F.conv3d(x5, w5, None, (s if kd == 3 else 1, s, s), (kd // 2, 1, 1))
        want = torch.relu(y[0] * scale.double().view(-1, 1, 1, 1) + shift.double().view(-1, 1, 1, 1)) + skip.double()
        got = R.run(name, x, w, scale, shift, True, skip)
        assert tuple(got.shape) == (cout,) + R.out_shape(name, D, H, W) == tuple(skip.shape), (name, D, H, W)
        assert _close64(got, want), (name, D, H, W)
        assert _close64(R.run(name, x, w, scale, shift, True, skip, F64, aten=True), want)
        assert _close64(R.reference(name, D, H, W, True)[0], want) and _close64(R.reference(name, D, H, W, False)[0], want - skip.double())
        assert R.run(name, x, w, scale, shift, True, skip, F32).dtype == F32
        xe, we, ske = R.exact_case(name, D, H, W) if (name, (D, H, W)) in R.EXACT_CASES else (None, None, None)
        if xe is not None:      # the exact case: fp32 ATen, the fp32 and the float64 restatement agree to the last bit
            e64 = R.run(name, xe, we, None, None, False, ske)
            assert torch.equal(R.run(name, xe, we, None, None, False, ske, F32).double(), e64)
            assert torch.equal(R.run(name, xe, we, None, None, False, ske, F32, aten=True).double(), e64)
            assert e64.abs().max().item() < 2 ** 24 and torch.equal(e64, e64.round())


def test_residual_goes_in_behind_the_relu():
    x, w, scale, shift, skip = R.case("conv2", 2, 5, 30)
    y = R.run("conv2", x, w, scale, shift, True)
    assert (y == 0).float().mean().item() > 0.2      # the ReLU cuts
    assert torch.equal(R.run("conv2", x, w, scale, shift, True, skip), y + skip.double())


# ------------------------------------------------------------------------------------------------ tables
def test_rows_are_the_rows_of_kcfgs():
    L, lib = _lib()
    src = open(os.path.join(CSRC, "conv3d_mfma.hip")).read()
    table = src[src.index("const Cfg kCfgs[] = {"):src.index("// FeatureNet (module.py:283-311)")]
    rows = [ln.split("}")[0].strip(" {") for ln in table.splitlines()[1:] if ln.strip().startswith("{")]
    assert len(rows) == len(R.ROWS) == 13
    consts = {"CI_CONV1": 1, "CI_CONV2": 4, "CI_CONV4": 2, "CI_CONV6": 4, "CI_CONV6_2D": 4, "DCI9": 4, "DCI11": 4}
    assert "constexpr int CI_CONV2 = 4, CI_CONV4 = 2, CI_CONV6 = 4, CI_CONV6_2D = 4;" in src and "constexpr int DCI11 = 4, DCI9 = 4;" in src
    assert "#define DMVS_CONV1_CI 1" in src
    for text, (name, (cin, cout, mode, kd, M, MB, ci_ch, pym, nmb)) in zip(rows, R.ROWS.items()):
        f = [t.strip() for t in text.split(",")]
        got = (int(f[0]), int(f[1]), f[2], int(f[3]), int(f[4]), int(f[5]), consts.get(f[6]) or int(f[6]), int(f[7]) if len(f) > 7 else 0)
        assert got == (cin, cout, R.MODE_TAG[mode], kd, M, MB, ci_ch, pym), (name, text)
        assert lib.dmvs_conv3d_mfma_weight_floats(cin, cout, mode, kd) == len(R.pack_sources(name))
    # conv7's two-row form: NMB = 2 in launch_deconv, both kdepths
    assert "launch_deconv<16, 3, 8, false, 2>(a, st) : launch_deconv<16, 1, 8, false, 2>(a, st)" in src
    assert [n for n, r in R.ROWS.items() if r[8] == 2] == ["conv7", "conv7_2d"] and [n for n, r in R.ROWS.items() if r[7]] == ["conv11"]
    assert {n: len(R.forms_of(n)) for n in R.ROWS} == {**{n: 2 for n in R.ROWS}, **{n: 3 for n in ("conv5", "conv6", "conv5_2d", "conv6_2d")},
                                                       **{n: 1 for n in ("conv7", "conv9", "conv11", "conv7_2d")}}
    assert len(R.cases()) == 5 * 6 + 4 * 7 + 4 * 6


def test_plans_match_the_library(knobs):
    L, lib = _lib()
    seen = set()
    for name, (D, H, W) in R.cases():
        cin, cout, mode, kd = R.ROWS[name][:4]
        for form in R.forms_of(name):
            mb, sb = R.K3_KNOBS[form]
            knobs(**R.K3_DEFAULTS)
            knobs(k3_min_blocks=mb, k3_split_blocks=sb)
            plan = lib.dmvs_conv3d_mfma_plan(cin, cout, D, H, W, mode, kd)
            assert plan == R.expected_plan(name, form, D, H, W), (name, form, D, H, W, hex(plan))
            seen.add((mode, form) + R.tile_of(name, form, D, H, W))
        knobs(**R.K3_DEFAULTS)
        default = lib.dmvs_conv3d_mfma_plan(cin, cout, D, H, W, mode, kd)     # what today's tests run: small, split or the one form
        assert default == R.expected_plan(name, R.forms_of(name)[-1], D, H, W)
    S1, S2, T2 = R.CONV_S1, R.CONV_S2, R.DECONV_S2
    assert seen == {(S1, "big", 2, 8, 0), (S1, "big", 1, 16, 0), (S1, "small", 2, 2, 0), (S1, "small", 1, 4, 0), (S1, "split", 2, 1, 1),
                    (S1, "split", 1, 2, 1), (S2, "big", 2, 4, 0), (S2, "big", 1, 8, 0), (S2, "small", 2, 2, 0), (S2, "small", 1, 4, 0),
                    (S2, "split", 2, 1, 1), (S2, "split", 1, 2, 1), (T2, "only", 2, 2, 0), (T2, "only", 1, 4, 0), (T2, "only", 2, 1, 0),
                    (T2, "only", 1, 2, 0)}
    # a config-2 volume takes the big 3D tile by itself: what only the end-to-end tests run today
    assert lib.dmvs_conv3d_mfma_plan(16, 16, 32, 296, 400, S1, 3) == 2 * 256 + 8 + R.PLAN_V4


def test_what_each_shape_is_there_for():
    G = R.geometry
    # ---- stride 1
    s = R.S1_SHAPES
    for name in ("conv0", "conv2", "conv4", "conv6"):
        g = G(name, "big", *s[0])
        assert (g["tz"], g["ty"]) == (2, 8) and (g["nx"], g["x_last"]) == (2, 4) and (g["ny"], g["y_last"]) == (2, 1) and (g["nz"], g["z_last"]) == (2, 1)
        g = G(name, "small", *s[0])
        assert (g["tz"], g["ty"]) == (2, 2) and (g["ny"], g["y_last"]) == (5, 1) and g["z_last"] == 1 and g["loader"] == "v4" and g["st4"]
        g = G(name, "big", *s[1])
        assert g["flat"] and g["ty"] == 16 and (g["ny"], g["y_last"]) == (2, 1) and g["loader"] == "dword" and not g["st4"]
        assert G(name, "small", *s[1])["y_last"] == 1 and s[1][2] % 4 == 1
        assert s[2][2] % 4 == 2 and G(name, "big", *s[2])["loader"] == "dword" and G(name, "big", *s[2])["z_last"] == 2
        g = G(name, "big", *s[3])
        assert (g["nx"], g["x_last"]) == (3, 4) and (g["nz"], g["z_last"]) == (3, 1) and g["loader"] == "v4"
        assert s[4][2] % 4 == 3 and G(name, "small", *s[4])["nx"] == 3 and G(name, "big", *s[4])["y_last"] == 2
        g = G(name, "small", *s[5])
        assert (g["nx"], g["ny"], g["nz"], g["x_last"], g["y_last"]) == (1, 1, 1, 1, 1) and g["flat"]
    for form, ty in (("big", 16), ("small", 4), ("split", 2)):      # the 2D row: every shape is D flat slices
        for shp in s:
            g = G("conv6_2d", form, *shp)
            assert g["flat"] and g["ty"] == ty and g["nz"] == shp[0]
    assert G("conv6_2d", "small", *s[0])["y_last"] == 1 and G("conv6_2d", "split", *s[0])["y_last"] == 1
    assert (G("conv6", "split", *s[0])["tz"], G("conv6", "split", *s[0])["ty"]) == (2, 1) and G("conv6", "split", *s[1])["ty"] == 2
    # ---- stride 2
    s = R.S2_SHAPES
    assert tuple(R.out_shape("conv1", *t) for t in s) == R.S2_OUT
    assert tuple(R.out_shape("conv5_2d", *t) for t in s) == tuple((t[0],) + o[1:] for t, o in zip(s, R.S2_OUT))
    for name in ("conv1", "conv3", "conv5"):
        g = G(name, "big", *s[0])
        assert (g["tz"], g["ty"]) == (2, 4) and (g["nx"], g["x_last"]) == (2, 4) and (g["ny"], g["y_last"]) == (3, 1) and g["loader"] == "v4"
        assert all(v % 2 == 1 for v in s[1]) and G(name, "big", *s[1])["loader"] == "dword" and not G(name, "big", *s[1])["st4"]
        g = G(name, "big", *s[2])
        assert g["flat"] and g["ty"] == 8 and (g["ny"], g["y_last"]) == (2, 1) and g["x_last"] == 4 and g["loader"] == "v4" and g["st4"]
        g = G(name, "small", *s[2])
        assert g["flat"] and g["ty"] == 4 and (g["ny"], g["y_last"]) == (3, 1)
        g = G(name, "big", *s[3])
        assert g["flat"] and (g["nx"], g["x_last"]) == (3, 1) and g["loader"] == "dword" and s[3][0] == s[2][0] == 2
        g = G(name, "small", *s[4])
        assert not g["flat"] and (g["nz"], g["z_last"]) == (2, 1) and g["st4"]
        assert s[5][0] == 1 and G(name, "big", *s[5])["flat"] and G(name, "small", *s[6])["x_last"] == 2
    assert (G("conv5", "split", *s[0])["tz"], G("conv5", "split", *s[0])["ty"]) == (2, 1) and G("conv5", "split", *s[2])["ty"] == 2
    assert all(G("conv5_2d", f, *t)["flat"] for f in R.forms_of("conv5_2d") for t in s)
    # ---- transposed: tiles on the INPUT grid, one loader (dwords), 8-byte stores (2 W is even)
    s = R.T2_SHAPES
    for name in ("conv9", "conv11"):
        g = G(name, "only", *s[0])
        assert (g["tz"], g["ty"]) == (2, 2) and (g["nx"], g["x_last"]) == (2, 4) and (g["ny"], g["y_last"]) == (3, 1)
        g = G(name, "only", *s[1])
        assert (g["nz"], g["z_last"]) == (2, 1) and g["x_last"] == 1 and g["loader"] == "dword"
        g = G(name, "only", *s[2])
        assert g["flat"] and g["ty"] == 4 and (g["ny"], g["y_last"]) == (3, 1)
        assert G(name, "only", *s[3])["flat"] and s[3][2] % 4 == 2
        g = G(name, "only", *s[4])
        assert (g["nx"], g["x_last"]) == (3, 4) and g["nz"] == 2
        assert G(name, "only", *s[5])["flat"]
    g = G("conv7", "only", *s[0])       # conv7's two-row form: (2,1) and (1,2)
    assert (g["tz"], g["ty"]) == (2, 1) and g["nx"] == 2 and G("conv7", "only", *s[1])["z_last"] == 1
    g = G("conv7", "only", *s[2])
    assert g["flat"] and g["ty"] == 2 and (g["ny"], g["y_last"]) == (5, 1)
    assert all(G("conv7_2d", "only", *t)["flat"] and G("conv7_2d", "only", *t)["ty"] == 2 for t in s)
    assert all(G(n, "only", *t)["loader"] == "dword" for n in ("conv7", "conv9", "conv11", "conv7_2d") for t in s)
    # both input kinds on every table
    for table in (R.S1_SHAPES, R.S2_SHAPES, R.T2_SHAPES):
        assert {R.kind_of(*t) for t in table} == set(R.KINDS)


def test_skipping_condition():
    """The restated condition is true exactly at the marked shapes (and at the transposed rows' single voxel, which has one input
    plane too), false with the knob off, on the dword loader and on the kdepth 1 rows; its live mask is the library's."""
    L, lib = _lib()
    for form in (R.ZFORM_S1, R.ZFORM_S2, R.ZFORM_T2):
        for D in range(1, 7):
            for TZ in (1, 2):
                for oz0 in range(D + 2):
                    assert lib.dmvs_zpad_live_mask(form, D, oz0, TZ) == R.live_mask(form, D, oz0, TZ), (form, D, oz0, TZ)
    assert R.live_mask(R.ZFORM_S2, 2, 0, 1) == 0b110 and R.live_mask(R.ZFORM_S2, 1, 0, 1) == 0b010 and R.live_mask(R.ZFORM_T2, 1, 0, 1) == 0b110
    hit = {(n, s) for n, s in R.cases() if R.skipping(n, *s)}
    want = {(n, s) for n in ("conv1", "conv3", "conv5") for s in R.ZDEAD_SHAPES} | {(n, s) for n in ("conv7", "conv9", "conv11") for s in R.ZSKIP_SHAPES}
    assert hit == want and len(hit) == 3 + 9
    for n, s in R.cases():
        assert not R.skipping(n, *s, knob=0)
    assert not R.skipping("conv1", 2, 18, 72, aligned=False) and not R.skipping("conv1", *R.ZDEAD_TWINS[0]) and R.ZDEAD_TWINS[0][2] % 4 == 2
    assert {(n, s) for n, s in R.zpad_cases() if R.skipping(n, *s)} == want
    assert all(s in R.shapes_of(n) for n, s in R.zpad_cases() + R.single_buf_cases() + list(R.MISALIGNED_CASES) + list(R.EXACT_CASES))
    assert len(R.single_buf_cases()) == 7 * 2
    for n, s in R.MISALIGNED_CASES:
        assert s[2] % 4 == 0 and R.out_shape(n, *s)[2] % 4 == 0


def test_tune_restores(knobs):
    L, lib = _lib()
    for name, bad in (("k3_min_blocks", -1), ("k3_split_blocks", -1), ("k3_single_buf_min_blocks", -1), ("zpad_skip", 2)):
        assert lib.dmvs_tune(name.encode(), bad) == L.EINVAL
    plan = lambda: lib.dmvs_conv3d_mfma_plan(64, 64, 3, 9, 36, R.CONV_S1, 3)  # noqa: E731
    assert plan() == R.expected_plan("conv6", "split", 3, 9, 36)
    knobs(k3_min_blocks=0)
    assert plan() == R.expected_plan("conv6", "big", 3, 9, 36)
    knobs(k3_min_blocks=R.HUGE, k3_split_blocks=0)
    assert plan() == R.expected_plan("conv6", "small", 3, 9, 36)
    knobs(**R.K3_DEFAULTS)
    assert plan() == R.expected_plan("conv6", "split", 3, 9, 36)


# ------------------------------------------------------------------------------------------------ e_ref
def test_e_ref_per_row():
    """Either e_ref is under 4 eps (the floor of 16 eps holds) or the bound is 8 e_ref; printed per row, max and mean."""
    for name in R.ROWS:
        worst = [0.0, 0.0]
        for D, H, W in R.shapes_of(name):
            for with_skip in (False, True):
                f64, e_ref = R.reference(name, D, H, W, with_skip)
                for e in e_ref:
                    assert R.bound_of(e) == (16 * EPS32 if e < 4 * EPS32 else 8 * e)
                assert 0.0 <= e_ref[1] <= e_ref[0] < 64 * EPS32, (name, D, H, W, e_ref)
                worst = [max(worst[0], e_ref[0]), max(worst[1], e_ref[1])]
        print(f"REGCONV e_ref {name}: max {worst[0] / EPS32:.2f} eps  mean {worst[1] / EPS32:.3f} eps")
        assert worst[1] < 4 * EPS32     # the mean bound is the floor on every row


# ------------------------------------------------------------------------------------------------ mutations
LOWEST = {}


@pytest.mark.parametrize("mutation", list(R.MUTATIONS))
def test_mutations_are_caught(mutation):
    low, runs = (float("inf"), None), 0
    for name in R.MUTATIONS[mutation]:
        shapes = R.mutation_shapes(mutation, name)
        assert shapes, (mutation, name)
        for D, H, W in shapes:
            x, w, scale, shift, skip = R.case(name, D, H, W)
            f64, e_ref = R.reference(name, D, H, W, True)
            plain = R.run(name, x, w, scale, shift, True, skip, F32)
            e, b = R.errors(plain, f64), R.bounds(e_ref)
            assert e[0] <= b[0] and e[1] <= b[1], "the unmutated fp32 restatement passes"
            ratio = R.errors(R.run(name, x, w, scale, shift, True, skip, F32, mutation), f64)[0] / R.bound_of(e_ref[0])
            low = min(low, (ratio, f"{name} {D}x{H}x{W}"))
            runs += 1
    LOWEST[mutation] = low
    print(f"REGCONV mutation {mutation}: smallest ratio to the bound {low[0]:.3g} ({low[1]}) over {runs} runs")
    assert runs >= 2 and low[0] >= R.MUTATION_RATIO


def test_mutation_list_covers_the_issue():
    assert len(R.MUTATIONS) == 10 and all(set(v) <= set(R.ROWS) and v for v in R.MUTATIONS.values())
    if len(LOWEST) == len(R.MUTATIONS):
        m = min(LOWEST, key=lambda k: LOWEST[k][0])
        print(f"REGCONV smallest mutation ratio: {LOWEST[m][0]:.3g} ({m}, {LOWEST[m][1]})")


# ------------------------------------------------------------------------------------------------ packing
@pytest.mark.parametrize("name", list(R.ROWS))
def test_pack_mfma_round_trip(name):
    """ops.pack_mfma, then the un-pack restated from dmvs_pack_conv_weights_mfma's three orders, gives the weights back: every
    weight has at least one slot, every slot of a weight holds it, every other slot is zero."""
    from dmvsnet_amd import ops
    cin, cout, mode, kd = R.ROWS[name][:4]
    w = R.make_weight(name, seed=3)
    w = w + torch.sign(w) * 1e-3        # no weight is zero: a packed zero is a pad
    packed = ops.pack_mfma(w, cin, cout, mode, kd).numpy()
    src = np.asarray(R.pack_sources(name))
    assert packed.shape == src.shape
    flat = w.contiguous().view(-1).numpy()
    back = np.full(flat.shape, np.nan, dtype=np.float32)
    back[src[src >= 0]] = packed[src >= 0]
    assert np.array_equal(back, flat)                                   # every weight came back ...
    assert np.array_equal(packed[src >= 0], flat[src[src >= 0]])        # ... from every slot that holds it
    assert (packed[src < 0] == 0).all()
    # packed-K: 27 taps in steps of 2 (conv0) or 4 (conv1) leave one padded tap x Cin channels x 16 rows; conv11: the py = 0 half
    # (8 rows x 4 k lanes) of the 3 (oz, pz) x 3 (ox, px) steps at input offset oy = 1, in each of the 4 chunks
    pads = {"conv0": 1 * 2 * 16, "conv1": 1 * 8 * 16, "conv11": 4 * 9 * 8 * 4}.get(name, 0)
    assert int((src < 0).sum()) == pads, (name, int((src < 0).sum()))


def test_knobs_are_back_at_their_defaults():
    """Last in the file: the library has no getter, so the knobs are set once more; the two that steer the plan are read back."""
    L, lib = _lib()
    for k, v in R.KNOB_DEFAULTS.items():
        assert lib.dmvs_tune(k.encode(), v) == 0
    assert lib.dmvs_conv3d_mfma_plan(64, 64, 3, 9, 36, R.CONV_S1, 3) == R.expected_plan("conv6", "split", 3, 9, 36)
    assert lib.dmvs_conv3d_mfma_plan(16, 16, 32, 296, 400, R.CONV_S1, 3) == 2 * 256 + 8 + R.PLAN_V4
