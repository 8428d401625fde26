"""The two regularisation networks on the MI355X as WHOLE networks -- ``CostRegNet.run`` / ``CostRegNet._branch``: the host code that
decides which kernel sees which tensor, on one and on two streams, with the logits and with the fused ``prob`` heads -- held to the
float64 restatement tests/costreg_ref.py.  tests/test_costreg_cpu.py checks that restatement, what the case tables claim and which
mistakes of the chaining code the criterion catches.

  criterion   e_max and e_mean (distance to float64 over its max-abs), each <= 8 e_ref, 16 * 2^-23 where e_ref < 4 * 2^-23; e_ref from
              the fp32 oracle on the CPU (oracle.dmvs_oracle.cost_reg; ``_expectation`` of its logits for the heads), measured in
              this process.  Every other assertion is torch.equal.
  dispatch    a spy around ``_lib.load`` records the C entry, the layer's (Cin, Cout, D, H, W, kdepth) and the return code of every
              launch; the record must equal costreg_ref.expected_launches, ops.launch_log the families of the successful ones.
  settings    costreg_ref.SETTINGS: `auto`, `auto` without K3z / K3r / the whole Winograd family, backend "mfma", backend "direct".

Every check prints its figures before it asserts (COSTREG lines) and the worst ratio per net and setting, with its case, is printed
at the end of the module; docs/kernels/costreg_net.md keeps the measured ones.  No test provokes a fault: the declined head is
answered by the spy without a launch, the poisoned memory is legal uninitialised memory that every kernel overwrites."""
import gc

import pytest
import torch

import costreg_ref as C

pytestmark = pytest.mark.gpu

F32, F64 = C.F32, C.F64
DEV = "cuda:0"
WORST = {}          # key -> [worst e_max / bound, its case, worst e_mean / bound, its case]
SWITCH_DEFAULTS = {"use_wino": True, "use_coarse": True, "use_zmarch": True, "use_prob_fused": True}
LAUNCHES = ("dmvs_conv3d_wino", "dmvs_conv3d_zmarch", "dmvs_conv3d_coarse", "dmvs_conv3d_mfma", "dmvs_conv3d_direct", "dmvs_prob_regress")
ALL = [(r, s) for r in (False, True) for s in C.shapes_of(r)]


def _id(v):
    if isinstance(v, bool):
        return "refine" if v else "full"
    return v if isinstance(v, str) else "x".join(map(str, v))


def _tag(refine, shape, setting=""):
    return f"{_id(refine)} {_id(shape)} {setting}".strip()


@pytest.fixture(autouse=True)
def reset_switches():
    yield
    from dmvsnet_amd import ops
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:      # a device error is sticky: nothing more is launched on the card from this module
        pytest.exit(f"device error after a test, ending the session: {e}", returncode=3)
    for k, v in SWITCH_DEFAULTS.items():
        setattr(ops, k, v)
    ops.launch_log = None
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def report_worst():
    yield
    for key in sorted(WORST):
        w = WORST[key]
        print(f"COSTREG worst {key}: e_hip / bound  max {w[0]:.3f} ({w[1]})  mean {w[2]:.3f} ({w[3]})")


def compare(tag, key, got, f64, e_ref):
    e, b = C.errors(got, f64), C.bounds(e_ref)
    r = (e[0] / b[0], e[1] / b[1])
    print(f"COSTREG {key} {tag}: e_hip max {e[0]:.3e} mean {e[1]:.3e}  e_ref max {e_ref[0]:.3e} mean {e_ref[1]:.3e}  "
          f"bound max {b[0]:.3e} mean {b[1]:.3e}  ratio max {r[0]:.3f} mean {r[1]:.3f}")
    w = WORST.setdefault(key, [0.0, "", 0.0, ""])
    if r[0] > w[0]:
        w[0], w[1] = r[0], tag
    if r[1] > w[2]:
        w[2], w[3] = r[1], tag
    assert got.dtype == F32 and torch.isfinite(got).all(), f"{key} {tag}: non-finite output"
    assert e[0] <= b[0], (key, tag, "max", e[0], e_ref[0])
    assert e[1] <= b[1], (key, tag, "mean", e[1], e_ref[1])


def cu(t):
    t = t.to(DEV, F32).contiguous()
    assert t.data_ptr() % 16 == 0
    return t


class _Spy:
    """The library with the launches of a regularisation net recorded: (entry, (Cin, Cout, D, H, W, kdepth), return code) per call,
    in host order.  ``decline_head`` = n: the n-th dmvs_prob_regress call is answered DMVS_EUNSUPPORTED without launching."""

    def __init__(self, lib, log, decline_head=None):
        self._lib, self._log, self._decline_head, self._heads = lib, log, decline_head, 0

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if name not in LAUNCHES:
            return f

        def call(*args):
            short = name.replace("dmvs_", "")
            if name == "dmvs_prob_regress":       # (x, w, Cin, D, H, W, planes, base, interval, alpha, out, stream)
                dims = (args[2], 2) + tuple(args[3:6]) + (3,)
                self._heads += 1
                if self._heads == self._decline_head:
                    self._log.append((short, tuple(int(d) for d in dims), C.EUNSUPPORTED))
                    return C.EUNSUPPORTED
            elif name in ("dmvs_conv3d_mfma", "dmvs_conv3d_direct"):    # (.., skip, Cin, Cout, D, H, W, mode, kdepth, flags, stream)
                dims = tuple(args[6:11]) + (args[12],)
            else:                                                      # (.., shift, Cin, Cout, D, H, W, kdepth, flags, stream)
                dims = tuple(args[5:11])
            code = f(*args)
            self._log.append((short, tuple(int(d) for d in dims), code))
            return code
        return call


@pytest.fixture(scope="module")
def model():
    from dmvsnet_amd import MVSNet
    net = MVSNet([8], [4], verbose=False)
    net.load_state_dict(C.state_dict())
    net = net.to(DEV)
    net.prepare(torch.device(DEV))
    return net


def _reg(model, refine):
    return (model.cost_regularization_refine if refine else model.cost_regularization)[0]


def _run(reg, sim, setting, side=None, regress=None, decline_head=None):
    """reg.run under the switches of ``setting`` with the spy and the launch log in place -> (result, spy record, launch log)."""
    from dmvsnet_amd import _lib, ops
    real_load, calls = _lib.load, []
    spy = _Spy(real_load(), calls, decline_head)
    ops.launch_log = log = []
    try:
        for k, v in C.switches_of(setting).items():
            setattr(ops, k, v)
        _lib.load = lambda: spy
        out = reg.run(sim, C.backend_of(setting), side, regress)
        torch.cuda.synchronize()
    finally:
        _lib.load = real_load
        for k, v in SWITCH_DEFAULTS.items():
            setattr(ops, k, v)
        ops.launch_log = None
    return out, calls, log


def _regress(refine, shape, affine):
    """The ``regress`` argument of CostRegNet.run on the recipe's planes, as a volume or as ops.AffinePlanes."""
    from dmvsnet_amd import ops
    base, step, vol = C.planes(*shape)
    interval = cu(step)
    planes = ops.AffinePlanes(cu(base), interval, shape[0]) if affine else cu(vol)
    return planes, interval, C.ALPHA[refine]


_LEVEL_OF_LAYER = {"conv2": "c2", "conv4": "c4", "conv7": "y7", "conv9": "y9", "conv11": "y11"}


def _out_of_bound(got, f64, e_ref):
    e, b = C.errors(got, f64), C.bounds(e_ref)
    return None if (e[0] <= b[0] and e[1] <= b[1]) else f"e {e[0]:.3e} / {e[1]:.3e}, bound {b[0]:.3e} / {b[1]:.3e}"


def _locate(reg, refine, shape, setting):
    """Failure path only.  (a) The run again on one stream with every layer's output kept (ops.conv3d wrapped): the first level of
    either branch whose intermediate leaves the bound of ITS e_ref (the fp32 oracle's error at that level).  (b) The product's
    layers run one by one from the yardstick's fp32-rounded intermediates: the first level that leaves its bound there -- `none`
    with a level named under (a) says the kernels are right and the tensor handed to one of them is not."""
    from dmvsnet_amd import ops
    r = C.reference(refine, *shape)
    kept, real = {}, ops.conv3d

    def keeping(x, layer, *a, **kw):
        y = real(x, layer, *a, **kw)
        kept[layer.name.split("@")[0]] = y
        return y
    try:
        ops.conv3d = keeping
        _run(reg, cu(C.sim_volume(refine, *shape)), setting)
    finally:
        ops.conv3d = real
    tag, in_run = reg._packed[0].name.rsplit(".", 1)[0], "none"
    for i, b in enumerate(C.BRANCHES):
        levels = {"conv0": kept[f"{tag}.conv0x2"][8 * i:8 * i + 8]}
        levels.update({v: kept[f"{tag}.{b}.{k}"] for k, v in _LEVEL_OF_LAYER.items()})
        bad = [(k, _out_of_bound(levels[k], r["levels"][f"{b}.{k}"], r["levels_e_ref"][f"{b}.{k}"])) for k in C.LEVEL_KEYS]
        bad = [f"{b}.{k} ({why})" for k, why in bad if why]
        if bad:
            in_run = bad[0]
            break
    return f"in the run: {in_run}; layer by layer from the yardstick: {_locate_layers(reg, refine, shape, setting)}"


def _locate_layers(reg, refine, shape, setting):
    from dmvsnet_amd import ops
    r = C.reference(refine, *shape)
    backend = C.backend_of(setting)
    conv0, small, huge = reg._packed
    ref = lambda k: cu(r["levels"][k])  # noqa: E731
    run = lambda x, layer, **kw: ops.conv3d(x, layer, backend=backend, **kw)  # noqa: E731
    try:
        for k, v in C.switches_of(setting).items():
            setattr(ops, k, v)
        c0 = run(cu(C.sim_volume(refine, *shape)), conv0)
        for i, (b, L) in enumerate(zip(C.BRANCHES, (small, huge))):
            def s1(x, name):
                d1 = L.get(name + "@d1")
                return run(x, d1 if (d1 is not None and x.shape[1] == 1 and backend != "direct") else L[name])
            got = {"conv0": c0[8 * i:8 * i + 8],
                   "c2": s1(run(ref(f"{b}.conv0"), L["conv1"]), "conv2"),
                   "c4": s1(run(ref(f"{b}.c2"), L["conv3"]), "conv4"),
                   "y7": run(s1(run(ref(f"{b}.c4"), L["conv5"]), "conv6"), L["conv7"], skip=ref(f"{b}.c4")),
                   "y9": run(ref(f"{b}.y7"), L["conv9"], skip=ref(f"{b}.c2")),
                   "y11": run(ref(f"{b}.y9"), L["conv11"], skip=ref(f"{b}.conv0"))}
            for k in C.LEVEL_KEYS:
                why = _out_of_bound(got[k], r["levels"][f"{b}.{k}"], r["levels_e_ref"][f"{b}.{k}"])
                if why:
                    return f"{b}.{k} ({why})"
            why = _out_of_bound(ops.conv3d(ref(f"{b}.y11"), L["prob"], backend="direct"), r["f64"][2 * i:2 * i + 2], r["e_ref"])
            if why:
                return f"{b}.prob ({why})"
        torch.cuda.synchronize()
    finally:
        for k, v in SWITCH_DEFAULTS.items():
            setattr(ops, k, v)
    return "none"


# ------------------------------------------------------------------------------------------------ 1. every shape x setting
@pytest.mark.parametrize("refine,shape,setting", C.cases(), ids=_id)
def test_net_against_float64(model, refine, shape, setting):
    """CostRegNet.run in every setting: the four logit channels against ``net_f64``; the launches are the expected entries on the
    expected layers in the expected order."""
    reg, r = _reg(model, refine), C.reference(refine, *shape)
    got, calls, log = _run(reg, cu(C.sim_volume(refine, *shape)), setting)
    assert tuple(got.shape) == (4,) + shape and got.is_contiguous()
    want = C.expected_launches(refine, *shape, setting, False)
    assert calls == want, (_tag(refine, shape, setting), [c for c in zip(calls, want) if c[0] != c[1]][:3], len(calls), len(want))
    assert log == C.families(want)
    try:
        compare(_tag(refine, shape), f"{_id(refine)}.{setting}", got, r["f64"], r["e_ref"])
    except AssertionError as err:
        raise AssertionError(f"{err}; first level out of its bound: {_locate(reg, refine, shape, setting)}") from None


# ------------------------------------------------------------------------------------------------ 2. fused heads
@pytest.mark.parametrize("refine,shape", C.fused_cases(), ids=_id)
def test_fused_heads(model, refine, shape):
    """The `prob` heads regressing their own channels (dmvs_prob_regress), planes as a volume and in affine form, on a side stream:
    against ``heads_f64`` of the yardstick logits, e_ref from the fp32 oracle chain; the two plane forms give the same bits."""
    reg = _reg(model, refine)
    sim, side = cu(C.sim_volume(refine, *shape)), torch.cuda.Stream()
    f64, e_ref = C.heads_reference(refine, *shape)
    want = C.expected_launches(refine, *shape, "auto", True)
    outs = {}
    for form in ("volume", "affine"):
        got, calls, log = _run(reg, sim, "auto", side, _regress(refine, shape, form == "affine"))
        assert tuple(got.shape) == (4,) + shape[1:], (form, got.shape)
        assert calls == want and log == C.families(want), (form, calls)
        compare(f"{_tag(refine, shape)} {form}", f"{_id(refine)}.heads", got, f64, e_ref)
        outs[form] = got
    assert torch.equal(outs["volume"], outs["affine"])


@pytest.mark.parametrize("head", [1, 2])
@pytest.mark.parametrize("refine,shape", C.fused_cases(), ids=_id)
def test_fused_heads_declined(model, refine, shape, head):
    """A head dmvs_prob_regress declines (the spy answers DMVS_EUNSUPPORTED, nothing is launched): the call returns the 4-D logits
    of a second, whole run of the network."""
    reg = _reg(model, refine)
    sim, side = cu(C.sim_volume(refine, *shape)), torch.cuda.Stream()
    plain, _, _ = _run(reg, sim, "auto", side)
    got, calls, log = _run(reg, sim, "auto", side, _regress(refine, shape, True), decline_head=head)
    assert got.dim() == 4 and torch.equal(got, plain)
    first = C.expected_launches(refine, *shape, "auto", True)
    at = 10 * head
    first[at] = first[at][:2] + (C.EUNSUPPORTED,)
    again = C.expected_launches(refine, *shape, "auto", False)
    assert calls == first + again, (head, calls)
    assert log == C.families(first) + C.families(again)


# ------------------------------------------------------------------------------------------------ 3. two streams
@pytest.mark.parametrize("refine,shape", ALL, ids=_id)
def test_two_streams_same_bits(model, refine, shape):
    reg = _reg(model, refine)
    sim, side = cu(C.sim_volume(refine, *shape)), torch.cuda.Stream()
    quiet, qcalls, _ = _run(reg, sim, "auto")
    got, calls, _ = _run(reg, sim, "auto", side)
    assert torch.equal(got, quiet) and calls == qcalls
    if C.fusable(shape[0], shape[2]):
        quiet, qcalls, _ = _run(reg, sim, "auto", None, _regress(refine, shape, True))
        got, calls, _ = _run(reg, sim, "auto", side, _regress(refine, shape, True))
        assert quiet.dim() == 3 and torch.equal(got, quiet) and calls == qcalls


@pytest.mark.parametrize("refine,shape", [(False, (8, 40, 136)), (True, (4, 16, 136))], ids=_id)
def test_two_streams_unsynchronised_producer_and_consumer(model, refine, shape):
    """``sim`` comes out of a chain of device work queued right before ``run`` and is overwritten on the main stream right behind it,
    with no host synchronisation in between -- the order K1 and the next pass's K1 give it in MVSNet._stages.  One run; the bits of
    the quiet run.  The free blocks of both streams' pools are NaN before it (the quiet run would otherwise leave its own, equal
    intermediates where the second run's torch.empty finds them, and a branch that ran ahead of its input would read the right
    values)."""
    reg = _reg(model, refine)
    src, side = cu(C.sim_volume(refine, *shape)), torch.cuda.Stream()
    quiet = reg.run(src, "auto")
    torch.cuda.synchronize()
    big = torch.ones(1 << 26, device=DEV)
    warm = torch.ones(8, device=DEV)          # torch loads a kernel at its first launch: none of that inside the unsynchronised part
    warm.mul_(1.0000001)
    (warm + warm * 0.0).fill_(7.0)
    _poison(refine, shape, side)
    torch.cuda.synchronize()
    for _ in range(8):                      # a few ms of work on the main stream ahead of the producer of `sim`
        big.mul_(1.0000001)
    sim = src + big[:src.numel()].view_as(src) * 0.0
    got = reg.run(sim, "auto", side)
    sim.fill_(7.0)
    torch.cuda.synchronize()
    assert torch.equal(sim, torch.full_like(sim, 7.0))
    assert torch.equal(got, quiet)


# ------------------------------------------------------------------------------------------------ 4. nothing stale is read
def _poison(refine, shape, side):
    """NaN-filled blocks of the sizes of every tensor a run allocates (twice over, plus one block as large as all of them), freed
    into the caching allocator's pools of the current and of the side stream: what torch.empty then hands out is NaN until written.
    -> the fraction of NaN in a fresh torch.empty of the size of conv0x2's output on the current stream."""
    lv = C.levels(refine, *shape)
    vox = [l[0] * l[1] * l[2] for l in lv]
    sizes = [16 * vox[0], 4 * vox[0]] + 2 * [16 * vox[1], 32 * vox[2], 64 * vox[3], 32 * vox[2], 16 * vox[1], 8 * vox[0]]
    sizes = 2 * sizes + [sum(sizes)]
    for st in (None, side):
        ctx = torch.cuda.stream(st) if st is not None else torch.cuda.stream(torch.cuda.current_stream())
        with ctx:
            blocks = [torch.full((n,), float("nan"), device=DEV) for n in sizes]
            del blocks
    probe = torch.empty(sizes[0], device=DEV)
    frac = torch.isnan(probe).float().mean().item()
    del probe
    return frac


@pytest.mark.parametrize("setting", ["auto", "no_wino"])
@pytest.mark.parametrize("refine,shape", ALL, ids=_id)
def test_no_stale_memory_is_read(model, refine, shape, setting):
    """Every intermediate and ``out`` start as NaN: a kernel that leaves part of its output unwritten, or a layer that reads a tensor
    before its producer ran, shows as NaN or as other bits downstream."""
    reg = _reg(model, refine)
    sim, side = cu(C.sim_volume(refine, *shape)), torch.cuda.Stream()
    clean, _, _ = _run(reg, sim, setting, side)
    frac = _poison(refine, shape, side)
    got, _, _ = _run(reg, sim, setting, side)
    print(f"COSTREG poison {_tag(refine, shape, setting)}: NaN fraction of a fresh torch.empty {frac:.2f}")
    assert torch.isfinite(got).all() and torch.equal(got, clean)
    if C.fusable(shape[0], shape[2], setting):
        clean, _, _ = _run(reg, sim, setting, side, _regress(refine, shape, True))
        _poison(refine, shape, side)
        got, _, _ = _run(reg, sim, setting, side, _regress(refine, shape, True))
        assert got.dim() == 3 and torch.isfinite(got).all() and torch.equal(got, clean)


# ------------------------------------------------------------------------------------------------ 5. run to run
@pytest.mark.parametrize("refine,shape,setting", C.cases(), ids=_id)
def test_run_to_run(model, refine, shape, setting):
    reg, sim = _reg(model, refine), cu(C.sim_volume(refine, *shape))
    a, ca, _ = _run(reg, sim, setting)
    b, cb, _ = _run(reg, sim, setting)
    assert torch.equal(a, b) and ca == cb


@pytest.mark.parametrize("refine,shape", ALL, ids=_id)
def test_zmarch_switch_only_matters_from_depth_8(model, refine, shape):
    """Where no level reaches depth 8 `use_zmarch = False` launches the same kernels (the spy record proves it) and gives the same
    bits; where one does, conv2 is the only layer that changes kernel."""
    reg, sim = _reg(model, refine), cu(C.sim_volume(refine, *shape))
    a, ca, _ = _run(reg, sim, "auto")
    b, cb, _ = _run(reg, sim, "no_zmarch")
    deep = C.levels(refine, *shape)[1][0] >= C.ZMARCH_MIN_DEPTH
    assert (ca != cb) == deep
    if not deep:
        assert torch.equal(a, b)
    else:
        assert {e for e, _, _ in ca} - {e for e, _, _ in cb} == {"conv3d_zmarch"}


# ------------------------------------------------------------------------------------------------ 6. packing
@pytest.mark.parametrize("refine", [False, True], ids=_id)
def test_repacking_gives_the_same_bits(model, refine):
    shape = C.shapes_of(refine)[1]
    reg, sim = _reg(model, refine), cu(C.sim_volume(refine, *shape))
    before, _, _ = _run(reg, sim, "auto")
    old = reg._packed
    model._invalidate()
    model.prepare(torch.device(DEV))
    assert reg._packed is not old
    after, _, _ = _run(reg, sim, "auto")
    assert torch.equal(before, after)
    forms = ("w_direct", "w_mfma", "w_wino", "w_coarse", "w_zmarch", "scale", "shift")
    for L0, L1 in zip(old[1:], reg._packed[1:]):
        assert list(L0) == list(L1)
        for name in L0:
            for f in forms:
                a, b = getattr(L0[name], f), getattr(L1[name], f)
                assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), (name, f)
    for L in reg._packed[1:]:
        d1 = sorted(k for k in L if k.endswith("@d1"))
        # pack builds the 2D form of every stride-1 3x3x3 layer K3 has a kdepth-1 row for; the tables' shapes select conv4@d1 in
        # the refine net and conv6@d1 in the full net (costreg_ref.d1_layers), whose conv6 is the only 3D one
        assert d1 == (["conv2@d1", "conv4@d1"] if refine else ["conv2@d1", "conv4@d1", "conv6@d1"])
        used = {n + "@d1" for s in C.shapes_of(refine) for n in C.d1_layers(refine, *s)}
        assert used == ({"conv4@d1"} if refine else {"conv6@d1"}) and used <= set(d1)
        for k in d1:
            assert L[k].kdepth == 1 and L[k].w_mfma is not None and L[k].w_direct is None
