"""The four Winograd kernels of conv0 / conv2 / conv4 / conv6 on the MI355X -- ``conv0_wino_kernel`` and ``conv_wino_kernel`` at
kdepth 3 (K3w), ``coarse_kernel`` (K3r) and ``zmarch_kernel`` (K3z) -- held to the float64 yardstick of tests/winoconv_ref.py at tile
seams, ragged volumes, on a walk of several tiles per persistent workgroup and under every knob that changes how the work is cut.
tests/test_winoconv_cpu.py asserts what the case tables claim, holds the fp32 emulation to the same bound and shows which mistakes
the criterion catches.

  criterion   e_max and e_mean (distance to float64 over its max-abs), each <= 8 e_ref, 16 * 2^-23 where e_ref < 4 * 2^-23; e_ref
              from fp32 ATen on the CPU; with BatchNorm + ReLU and raw.  The plain bound, no allowance.
  arms        every knob setting of one input is held to float64 by itself (a mistake common to all arms is not hidden) and the arms
              are asserted bit for bit equal: a tile, unit or column accumulates its products in one order whoever computes it.
  guards      the output lies inside a NaN-filled buffer (every element written and finite, the bands on both sides still NaN), the
              input is an aligned view inside a larger NaN-filled buffer (a read outside the tensor is a finding).
  exact       small-integer inputs and weights, and impulses on 27 distinct integer taps: equal to float64 with no tolerance.

Every launch forces its backend through ops.conv3d(..., backend=...).  Every check prints its figures before it asserts (WINOCONV
lines) and the worst ratio per kernel is printed at the end of the module; docs/kernels/K3w_conv_wino.md, K3r_conv_coarse.md and
K3z_conv_zmarch.md keep the measured ones.  No test provokes a fault."""
import functools
import gc

import pytest
import torch

import winoconv_ref as R
from featurenet_ref import q4_halves_to_planar

pytestmark = pytest.mark.gpu

F32, F64 = R.F32, R.F64
GUARD = 64          # NaN floats on either side of a tensor (256 bytes: the tensor stays 16-byte aligned)
WORST = {}          # kernel -> [worst e_max / bound, its case, worst e_mean / bound, its case]
BITS = {}           # what was compared bit for bit -> [pairs equal, pairs]
IDS = lambda v: v if isinstance(v, str) else "x".join(map(str, v))  # noqa: E731
KERNEL = {"wino": "K3w", "coarse": "K3r", "zmarch": "K3z"}


def _tune(**kw):
    from dmvsnet_amd import _lib
    for k, v in kw.items():
        if v is not None:
            _lib.check(_lib.load().dmvs_tune(k.encode(), int(v)), f"dmvs_tune({k})")


@pytest.fixture(autouse=True)
def reset_knobs():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device error is sticky: nothing more is launched on the card from this module
        pytest.exit(f"device error after a test, ending the session: {e}", returncode=3)
    _tune(**R.KNOB_DEFAULTS)
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    for key in sorted(WORST):
        w = WORST[key]
        print(f"WINOCONV worst {key}: e_hip / bound  max {w[0]:.3f} ({w[1]})  mean {w[2]:.3f} ({w[3]})")
    for key in sorted(BITS):
        print(f"WINOCONV same bits {key}: {BITS[key][0]} of {BITS[key][1]} pairs")


def _bits(key, a, b):
    same = torch.equal(a, b)
    n = BITS.setdefault(key, [0, 0])
    n[0] += same
    n[1] += 1
    return same


def compare(tag, key, got, f64, e_ref):
    e, b = R.errors(got, f64), R.bounds(e_ref)
    r = (e[0] / b[0], e[1] / b[1])
    print(f"WINOCONV {key} {tag}: e_hip max {e[0]:.3e} mean {e[1]:.3e}  e_ref max {e_ref[0]:.3e} mean {e_ref[1]:.3e}  "
          f"bound max {b[0]:.3e} mean {b[1]:.3e}  ratio max {r[0]:.3f} mean {r[1]:.3f}")
    w = WORST.setdefault(key, [0.0, "", 0.0, ""])
    for i, v in ((0, r[0]), (2, r[1])):
        if v > w[i]:
            w[i], w[i + 1] = v, tag
    assert got.dtype == F32 and torch.isfinite(got).all(), f"{tag}: non-finite output"
    assert e[0] <= b[0], (key, tag, "max", e[0], e_ref[0])
    assert e[1] <= b[1], (key, tag, "mean", e[1], e_ref[1])


def _guarded(shape, off=0):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD + 8,), float("nan"), device="cuda:0")
    out = buf[GUARD + off:GUARD + off + n].view(shape)
    assert buf.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 4 * off and out.is_contiguous()
    return buf, out, (GUARD + off, GUARD + off + n)


def _check_guarded(tag, buf, out, span):
    torch.cuda.synchronize()
    assert torch.isfinite(out).all(), f"{tag}: output not fully written (or not finite)"
    assert torch.isnan(buf[:span[0]]).all() and torch.isnan(buf[span[1]:]).all(), f"{tag}: wrote outside the output"


def cu(t, off=0):
    """The tensor on the device as a view inside a larger NaN-filled buffer, 16-byte aligned; ``off`` floats past a 16-byte boundary
    otherwise."""
    t = t.to(F32).contiguous()
    _, d, _ = _guarded(tuple(t.shape), off)
    d.copy_(t)
    return d


@functools.lru_cache(maxsize=None)
def _layer(name, bn, exact=None):
    """The layer with every form the library packs for it; ``bn``: folded BatchNorm + ReLU, else raw.  ``exact``: the weights of an
    integer case instead (its shape, and which of the two)."""
    from dmvsnet_amd import ops
    cin, cout, kd, _ = R.ROWS[name]
    if exact is None:
        w, (scale, shift) = R.make_weight(name), (R.make_bn(cout) if bn else (None, None))
    else:
        w, scale, shift = (R.exact_case if exact[0] == "int" else R.impulse_case)(name, *exact[1])[1], None, None
    dev = lambda t: None if t is None else cu(t)  # noqa: E731
    layer = ops.ConvLayer(name, R.CONV_S1, kd, cin, cout, dev(ops.pack_direct(w, False)), dev(ops.pack_mfma(w, cin, cout, R.CONV_S1, kd)),
                          dev(scale), dev(shift), bn, w_wino=dev(ops.pack_wino(w, cin, cout, kd)),
                          w_coarse=dev(ops.pack_coarse(w, cin, cout, kd)), w_zmarch=dev(ops.pack_zmarch(w, cin, cout, kd)))
    assert layer.w_mfma is not None
    for form in R.ROWS[name][3]:
        assert getattr(layer, "w_" + form) is not None, (name, form)
    return layer


def _run(name, form, x, layer, shape, tag, out_off=0, q4=False, skip=None):
    """ops.conv3d on the forced backend into a guarded output; -> a clone of the result (planar)."""
    from dmvsnet_amd import ops
    cout = layer.cout
    oshape = (2, shape[0], cout // 8, shape[1], shape[2], 4) if q4 else (cout,) + tuple(shape)
    buf, out, span = _guarded(oshape, out_off)
    got = ops.conv3d(x, layer, skip=skip, out=out, backend=form, out_q4=q4)
    assert got.data_ptr() == out.data_ptr()
    _check_guarded(tag, buf, out, span)
    return q4_halves_to_planar(out).contiguous() if q4 else out.clone()


def _arms(name, form, shape, arms, key, what, equal=True, in_off=0, out_offs=None):
    """One input, BatchNorm + ReLU and raw, under every knob setting of ``arms`` ({label: knobs}): each arm against float64; the arms
    bit for bit equal to the first one."""
    x = cu(R.case(name, *shape)[0], in_off)
    for bn in (True, False):
        f64, e_ref = R.reference(name, *shape, bn)[:2]
        outs = {}
        for label, knobs in arms.items():
            tag = f"{name} {IDS(shape)} {'bn' if bn else 'raw'} {label}"
            try:
                _tune(**knobs)
                outs[label] = _run(name, form, x, _layer(name, bn), shape, tag, (out_offs or {}).get(label, 0))
            finally:
                _tune(**R.KNOB_DEFAULTS)
            compare(tag, key, outs[label], f64, e_ref)
        first = next(iter(outs))
        for label, o in outs.items():
            if label != first:
                same = _bits(what, o, outs[first])
                assert same or not equal, f"{name} {IDS(shape)} {'bn' if bn else 'raw'}: {label} differs from {first}"


# ------------------------------------------------------------------------------------------------ K3w
@pytest.mark.parametrize("name,shape", R.wino_cases(), ids=IDS)
def test_wino3d(name, shape):
    """Every K3w row at the SMALL shapes, planar; quad-planar at two ragged shapes (conv0 is planar only and must raise)."""
    from dmvsnet_amd import _lib
    _arms(name, "wino", shape, {"default": {}}, "K3w.conv0" if name == "conv0" else "K3w", "-")
    if shape not in R.Q4_SHAPES:
        return
    x = cu(R.case(name, *shape)[0])
    if name == "conv0":
        with pytest.raises(_lib.DmvsError):
            _run(name, "wino", x, _layer(name, True), shape, "conv0 q4", q4=True)
        return
    for bn in (True, False):
        f64, e_ref = R.reference(name, *shape, bn)[:2]
        tag = f"{name} {IDS(shape)} {'bn' if bn else 'raw'} q4"
        got = _run(name, "wino", x, _layer(name, bn), shape, tag, q4=True)
        compare(tag, "K3w.q4", got, f64, e_ref)
        print(f"WINOCONV {tag}: same bits as planar {_bits('K3w planar vs q4', got, _run(name, 'wino', x, _layer(name, bn), shape, tag))}")


@pytest.mark.parametrize("label", list(R.WALK), ids=IDS)
def test_wino3d_walk(label):
    """More tiles than resident workgroups, ragged eighths: the default walk, one tile per workgroup, one and two LDS stages."""
    name, shape, tiles = R.WALK[label]
    from dmvsnet_amd import _lib
    cin, cout, kd = R.ROWS[name][:3]
    assert _lib.load().dmvs_conv3d_wino_plan(cin, cout, *shape, kd) == tiles
    arms = {"default": {}, "persistent0": {"wino_persistent": 0}, "stages1": {"wino_stages": 1}, "stages2": {"wino_stages": 2}}
    _arms(name, "wino", shape, arms, "K3w.conv0.walk" if name == "conv0" else "K3w.walk", "K3w walk arms")


@pytest.mark.parametrize("shape", R.SMALL + (R.WALK["conv0"][1],), ids=IDS)
def test_conv0_grid(shape):
    """conv0 with 8 and with 512 persistent workgroups: at 8 a workgroup walks several tiles already at the small shapes."""
    _arms("conv0", "wino", shape, {"grid8": {"wino_conv0_grid": 8}, "grid512": {"wino_conv0_grid": 512}}, "K3w.conv0.grid", "conv0 grids")


@pytest.mark.parametrize("shape", R.ZPAD_SHAPES, ids=IDS)
def test_wino_zpad(shape):
    """conv2 on K3w with `zpad_skip` off and on, D = 2 .. 5 and the WALK shape where a workgroup changes its ZSKIP case from tile to
    tile: each arm against float64, the arms equal."""
    assert R.wino_zskip("conv2", shape[0]) == (shape[0] <= 4)
    _arms("conv2", "wino", shape, {"zpad0": {"zpad_skip": 0}, "zpad1": {"zpad_skip": 1}}, "K3w.zpad", "K3w zpad arms")


# ------------------------------------------------------------------------------------------------ K3r
@pytest.mark.parametrize("name,shape", R.coarse_cases(), ids=IDS)
def test_coarse(name, shape):
    """Every K3r row at the COARSE shapes: 256 and 32 persistent workgroups, the counted and the conservative stage wait, the skipping
    and the plain step loop."""
    arms = {"grid256": {}, "grid32": {"k3r_grid": 32}, "grid32.wait0": {"k3r_grid": 32, "k3r_counted_wait": 0}}
    if R.ROWS[name][2] == 3:
        arms.update({"grid256.zpad0": {"zpad_skip": 0}, "grid32.zpad0": {"k3r_grid": 32, "zpad_skip": 0}})
    _arms(name, "coarse", shape, arms, "K3r", "K3r arms")


@pytest.mark.parametrize("name,shape", R.alignment_cases(), ids=IDS)
def test_coarse_alignment(name, shape):
    """W % 4 == 0 with the input one float past a 16-byte boundary (V4 false: the dword loader, and no skipping form), then the
    output (st4 false: dword stores), then both: the aligned run's bits, and the float64 bound."""
    for in_off in (0, 1):
        assert R.coarse_v4_st4(shape[2], in_off, 0)[0] == (in_off == 0)
        arms = {f"in+{in_off} out+0": {}, f"in+{in_off} out+1": {}}
        _arms(name, "coarse", shape, arms, "K3r.align", "K3r alignment", in_off=in_off, out_offs={f"in+{in_off} out+1": 1})
    x = R.case(name, *shape)[0]
    for bn in (True, False):
        a = _run(name, "coarse", cu(x), _layer(name, bn), shape, "aligned")
        b = _run(name, "coarse", cu(x, 1), _layer(name, bn), shape, "in+1", out_off=1)
        assert _bits("K3r alignment", a, b), f"{name} {IDS(shape)}: the misaligned run differs from the aligned one"


# ------------------------------------------------------------------------------------------------ K3z
@pytest.mark.parametrize("shape", R.ZMARCH, ids=IDS)
def test_zmarch(shape):
    """K3z under every segment cap and grid of the table: each arm against float64 and equal to the default's bits."""
    arms = {"default": {}}
    arms.update({f"zs{zs}.grid{g}": {"k3z_zs": zs, "k3z_grid": g} for zs in R.ZMARCH_ZS for g in R.ZMARCH_GRIDS if zs or g})
    _arms("conv2", "zmarch", shape, arms, "K3z", "K3z arms")


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("name,form,shape", R.EXACT, ids=IDS)
def test_exact(name, form, shape):
    """Integer inputs and weights, and the impulse input, no BatchNorm, no ReLU: fp32 Winograd is exact on them (the CPU file shows
    it), so the kernel equals float64 with no tolerance."""
    kd = R.ROWS[name][2]
    for kind, (x, w) in (("int", R.exact_case(name, *shape)), ("impulse", R.impulse_case(name, *shape))):
        want = R.conv3d(x, w, 1, kd)
        tag = f"{name} {form} {IDS(shape)} {kind}"
        got = _run(name, form, cu(x), _layer(name, False, (kind, shape)), shape, tag).cpu().double()
        diff = (got - want).abs()
        print(f"WINOCONV exact {tag}: max |diff| {diff.max().item():g} at {diff.argmax().item()} of {tuple(want.shape)}")
        assert torch.equal(got, want), tag


# ------------------------------------------------------------------------------------------------ dispatch
def _skip_reference(name, shape):
    x, w, scale, shift = R.case(name, *shape)
    skip = R.make_input("normal", R.ROWS[name][1], *shape, seed=1)
    f64, _, _ = R.reference(name, *shape, True)
    a32 = R.aten_conv3d(x, w, 1, R.ROWS[name][2], scale, shift, True, skip)
    return skip, f64 + skip.double(), R.errors(a32, f64 + skip.double())


def test_unsupported_is_refused_not_wrong():
    """A forced form outside its cover raises; `auto` on the same call runs another kernel and stays within the float64 bound."""
    from dmvsnet_amd import _lib
    odd, shape = (3, 9, 34), (3, 9, 36)
    lay = _layer("conv2", True)
    # W % 4 != 0
    x = cu(R.case("conv2", *odd)[0])
    for form in ("wino", "zmarch"):
        with pytest.raises(_lib.DmvsError):
            _run("conv2", form, x, lay, odd, f"{form} W % 4")
    f64, e_ref = R.reference("conv2", *odd, True)[:2]
    compare(f"conv2 {IDS(odd)} auto", "auto", _run("conv2", "auto", x, lay, odd, "auto W % 4"), f64, e_ref)
    # a misaligned input view, then a misaligned output
    f64, e_ref = R.reference("conv2", *shape, True)[:2]
    for in_off, out_off in ((1, 0), (0, 1)):
        x = cu(R.case("conv2", *shape)[0], in_off)
        for form in ("wino", "zmarch"):
            with pytest.raises(_lib.DmvsError):
                _run("conv2", form, x, lay, shape, f"{form} in+{in_off} out+{out_off}", out_off)
        compare(f"conv2 {IDS(shape)} auto in+{in_off} out+{out_off}", "auto", _run("conv2", "auto", x, lay, shape, "auto misaligned", out_off), f64, e_ref)
    # a residual
    for name, form in (("conv2", "zmarch"), ("conv4", "coarse"), ("conv6_2d", "coarse")):
        skip, f64, e_ref = _skip_reference(name, shape)
        x, sk = cu(R.case(name, *shape)[0]), cu(skip)
        with pytest.raises(_lib.DmvsError):
            _run(name, form, x, _layer(name, True), shape, f"{form} residual", skip=sk)
        compare(f"{name} {IDS(shape)} auto +skip", "auto", _run(name, "auto", x, _layer(name, True), shape, "auto residual", skip=sk), f64, e_ref)


def test_auto_picks():
    """`auto` is bit for bit the form the dispatch rules name: K3w for conv0 and for conv2 below ZMARCH_MIN_DEPTH, K3z from there up, K3r
    for conv4 / conv6 and their 2D forms at any W; K3w with `use_coarse` off; K3 with `use_wino` off."""
    from dmvsnet_amd import ops
    assert ops.ZMARCH_MIN_DEPTH == R.ZMARCH_MIN_DEPTH == 8
    picks = [("conv0", (3, 9, 68), "wino"), ("conv2", (5, 17, 100), "wino"), ("conv2", (3, 17, 36), "wino"), ("conv2", (9, 10, 68), "zmarch"),
             ("conv2", (8, 8, 8), "zmarch")]
    picks += [(n, s, "coarse") for n in R.COARSE_ROWS for s in ((3, 9, 12), (5, 17, 23))]
    saved = (ops.use_coarse, ops.use_wino, ops.use_zmarch)

    def check(name, shape, form):
        x, lay = cu(R.case(name, *shape)[0]), _layer(name, True)
        a, f = _run(name, "auto", x, lay, shape, f"auto {name}"), _run(name, form, x, lay, shape, f"{form} {name}")
        assert torch.equal(a, f), f"{name} {IDS(shape)}: auto is not {form} (use_coarse {ops.use_coarse}, use_wino {ops.use_wino})"
    try:
        for p in picks:
            check(*p)
        ops.use_coarse = False
        for n in R.COARSE_ROWS:
            check(n, (3, 9, 12), "wino")
            check(n, (5, 17, 23), "mfma")       # W % 4 != 0: K3w's plan declines, K3 runs
        ops.use_coarse, ops.use_wino = True, False
        for n in R.ROWS:
            check(n, (3, 9, 12), "mfma")
        check("conv2", (9, 10, 68), "mfma")
    finally:
        ops.use_coarse, ops.use_wino, ops.use_zmarch = saved


def test_knobs_are_back_at_their_defaults():
    """Last in the file: the library has no getter, so the knobs are set once more; the dispatch switches are read back."""
    from dmvsnet_amd import ops
    _tune(**R.KNOB_DEFAULTS)
    assert ops.use_wino and ops.use_coarse and ops.use_zmarch
