"""K5's synchronised statistics on the MI355X in ONE process and without a process group: the ranks are emulated at the ``ops`` level
(tests/bn_sync_ref.py ``emulate``).  A batch is cut into pieces by whole samples, ``ops.bn_sync_moments`` runs per piece, the moments are
stacked by hand into the gathered buffer, then forward, backward sums and apply run per piece.  The collective adds nothing to the
arithmetic (tests/test_bn_sync_dist_gpu.py asserts that on real process groups).

Yardsticks, none of which is the code under test: the float64 restatement tests/bn_grad_ref.py on the CONCATENATED batch, stock fp32
ATen on the same batch as e_ref, the criterion of tests/test_bn_grad_gpu.py (e_hip <= 8 e_ref per tensor, 16 * 2^-23 where e_ref is
below 4 * 2^-23).  y and g_x of all pieces are measured concatenated, the local g_gamma / g_beta stacked over the ranks, so that every
tensor of every piece is held under the norm its e_ref was measured in (a piece whose outputs are all zero has no norm of its own).
Inputs with a ReLU come from ``first_clean_pieces``: no float64 pre-activation within 1e-5 of the kink (asserted).  A value lies that
close with probability 8e-6, so above RELU_ELEMENTS = 4e5 elements no seed is clean: those cases (V = 5000 at the larger channel
counts) run without the ReLU, as the grid-size cases of tests/test_bn_grad_gpu.py do; the mask is held at every smaller shape.

Every test prints its figures before it asserts (SYNC / OFFSET / EXACT / ORDER lines).  No test provokes a fault."""
import ctypes
import gc

import pytest
import torch

import bn_grad_ref as G
import bn_sync_ref as S

pytestmark = pytest.mark.gpu

# (spatial, pieces): V = 1 and 3 (one lane, 4-byte path), 1024 (exactly one chunk), 1028 and 5000 (several shares, ragged last chunk, a
# share crossing a sample boundary inside a piece of two samples), the 2D and 3D volumes of the bare-operator tests; eight pieces; R = 1
SHAPES = {"v1_n1": ((1, 1, 1), (1, 1)), "v3": ((1, 1, 3), (2, 1)), "chunk": ((1, 4, 256), (1, 2, 1)), "chunk+4": ((1, 4, 257), (2, 1)),
          "v5000": ((1, 8, 625), (1, 2, 1)), "2x5x9": ((2, 5, 9), (1, 2, 1)), "2x5x9_eight": ((2, 5, 9), (1,) * 8),
          "v5000_eight": ((1, 8, 625), (1,) * 8), "one_rank": ((2, 5, 9), (3,))}
RELU_ELEMENTS = 400_000
KEYS = ("y", "g_x", "g_gamma", "g_beta", "mean", "invstd", "running_mean", "running_var")


@pytest.fixture(autouse=True)
def free_gpu_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def running_init(C):
    g = torch.Generator().manual_seed(C)
    return 0.5 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)


def shaped(t, nd):
    """[B,C,D,H,W] -> the 2D modules' [B,C,D*H,W]."""
    return t if nd == 3 else t.reshape(t.shape[:2] + G.spatial_2d(t.shape[2:]))


def run(case, pieces, momentum, running, nd=3, relu=True, **kw):
    from dmvsnet_amd import ops
    xs, gys = (S.split(shaped(case[k], nd).cuda(), pieces) for k in ("x", "gy"))
    return S.emulate(ops, xs, gys, case["gamma"].cuda(), case["beta"].cuda(), momentum, G.BN_EPS, relu, running=running, **kw)


def joined(ranks, f64):
    """Per key (got, float64) under one norm: y / g_x concatenated over the pieces, local sums stacked, per-rank [C] vectors stacked."""
    out = {}
    for k in KEYS:
        join = torch.cat if k in ("y", "g_x") else torch.stack
        out[k] = (join([r[k].cpu() for r in ranks]), join([r[k] for r in f64]))
    return out


def e_refs(case, momentum, running, relu=True):
    e = S.e_ref_of(case, relu)
    rm64, rv64 = G.running_update(running[0], running[1], case["x"], momentum)
    rm32, rv32 = S.running_fp32(case, momentum, running)
    return dict(e, running_mean=G.rel_dist(rm32, rm64), running_var=G.rel_dist(rv32, rv64))


def compare(tag, ranks, case, pieces, momentum, running, relu=True, keys=KEYS):
    f64, ref = S.f64_per_rank(case, pieces, momentum, relu, running=running), e_refs(case, momentum, running, relu)
    rows = []
    for k, (got, want) in joined(ranks, f64).items():
        if k in keys:
            rows.append((k, got, G.rel_dist(got.reshape(want.shape), want), ref[k]))
            print(f"{tag} {k}: e_hip {rows[-1][2]:.3e}  e_ref {ref[k]:.3e}  bound {S.bound_of(ref[k]):.3e}  "
                  f"ratio {rows[-1][2] / S.bound_of(ref[k]):.3f}")
    for k, got, e_hip, e_ref in rows:
        assert got.dtype == torch.float32 and torch.isfinite(got).all(), (tag, k)
        assert e_hip <= S.bound_of(e_ref), (tag, k, e_hip, e_ref)
    return rows


def same_on_all_ranks(ranks):
    return all(torch.equal(r[k], ranks[0][k]) for r in ranks for k in ("mean", "invstd", "running_mean", "running_var"))


# ------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("C", G.CHANNELS)
def test_pieces_against_float64(C, shape):
    from dmvsnet_amd import ops
    spatial, pieces = SHAPES[shape]
    nd = 2 if shape.startswith("2x5x9") and C in (16, 64) else 3   # the 2D layout on half of the channel counts
    V, running = G.volume(spatial), running_init(C)
    relu = sum(pieces) * V * C <= RELU_ELEMENTS
    case, seed = S.first_clean_pieces(C, pieces, spatial) if relu else (S.make_pieces(C, pieces, spatial, 0), 0)
    assert not relu or G.kink_violations(case) == 0
    print(f"SYNC C {C} {shape} {nd}D pieces {pieces} V {V} seed {seed} relu {relu}: S per piece {[ops.bn_plan(C, b, V) for b in pieces]}, "
          f"{'16-byte' if V % 4 == 0 else 'scalar'} path, N {sum(pieces) * V}")
    for momentum in (0.1, 1.0):
        ranks = run(case, pieces, momentum, running, nd, relu)
        assert all(r["N"] == sum(pieces) * V for r in ranks) and same_on_all_ranks(ranks)
        compare(f"SYNC C {C} {shape} momentum {momentum}", ranks, case, pieces, momentum, running, relu,
                keys=KEYS if momentum == 0.1 else ("running_mean", "running_var"))


@pytest.mark.parametrize("C", (8, 64))
def test_offset_pieces(C):
    """Pieces whose means are 1e3, -1e3, 1, -1 and 0 at a standard deviation of 0.1: the pivots of the ranks are six orders of magnitude
    apart, which raw sums around them could not be combined across; moments can."""
    pieces, offsets, spatial = (1, 2, 1, 1, 1), (1e3, -1e3, 1.0, -1.0, 0.0), (1, 4, 257)
    case, seed = S.first_clean_pieces(C, pieces, spatial, offsets, 0.1)
    assert G.kink_violations(case) == 0
    running = running_init(C)
    ranks = run(case, pieces, 0.1, running)
    assert same_on_all_ranks(ranks)
    compare(f"OFFSET C {C} mixed seed {seed}", ranks, case, pieces, 0.1, running)
    # all pieces near 1e3: the variance (1e-2) is eight orders of magnitude below mean^2
    pieces, offsets = (2, 1), (1e3, 1e3)
    case, seed = S.first_clean_pieces(C, pieces, spatial, offsets, 0.1)
    assert G.kink_violations(case) == 0
    ranks = run(case, pieces, 0.1, running)
    compare(f"OFFSET C {C} same seed {seed}", ranks, case, pieces, 0.1, running)


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("pieces", [(1, 1), (1,) * 8])
def test_exact_on_small_integers(pieces):
    """Small-integer inputs, power-of-two counts: every sum of the chain is exact.  Rank r holds r + {-3 .. 3} with its first 256 values
    equal to r, so its pivot is r, every x - p a small integer, f0 and f1 exact in fp32, mean_r and M2_r exact in fp64, and the combine
    exact: mean and invstd are the fp32 roundings of the float64 values (eps taken as the fp32 number the kernel is given), and the
    running buffers at momentum 1 are those of the float64 mean and unbiased variance."""
    C, V, R = 8, 1024, len(pieces)
    g = torch.Generator().manual_seed(R)
    x = torch.randint(-3, 4, (R, C, 1, 4, 256), generator=g).float()
    x.reshape(R, C, V)[:, :, :256] = 0.0
    x += torch.arange(R, dtype=torch.float32).reshape(R, 1, 1, 1, 1)
    case = dict(x=x, gy=torch.ones_like(x), gamma=torch.ones(C), beta=torch.zeros(C))
    ranks = run(case, pieces, 1.0, (torch.zeros(C), torch.ones(C)), relu=False)
    xc = x.double().transpose(0, 1).reshape(C, -1)
    N = xc.shape[1]
    mean = xc.sum(1) / N
    M2 = ((xc - mean[:, None]) ** 2).sum(1)
    eps = torch.tensor(G.BN_EPS, dtype=torch.float32).double()
    invstd = 1.0 / torch.sqrt(M2 / N + eps)
    print(f"EXACT pieces {pieces}: N {N}, mean {mean[:3].tolist()}, var {(M2 / N)[:3].tolist()}")
    for r in ranks:
        for k, want in (("mean", mean), ("invstd", invstd), ("running_mean", mean), ("running_var", M2 / (N - 1))):
            print(f"EXACT {k}: max-abs distance to the fp32 rounding {(r[k].cpu().double() - want.float().double()).abs().max():.3e}")
            assert torch.equal(r[k].cpu(), want.float()), k
    # moments themselves: exact in fp64
    from dmvsnet_amd import ops
    for i, piece in enumerate(S.split(x.cuda(), pieces)):
        assert torch.equal(ops.bn_sync_moments(piece).cpu(), S.moments(piece))


# ------------------------------------------------------------------------------------------------ one rank and eval mode
@pytest.mark.parametrize("C", (8, 16))
@pytest.mark.parametrize("spatial", [(2, 5, 9), (1, 8, 625)])
def test_one_rank_equals_plain_k5(C, spatial):
    """R = 1 through the sync launches against ``ops.bn_relu_forward`` / ``_backward``: torch.equal.  The backward is the same bits by
    construction (same partials, same fold, the one pair added to zero, the same division).  The forward's mean and variance go
    through other fp64 expressions (n mean / n; (f1 - f0^2 / n) / n for f1 / n - (f0 / n)^2) that agree to a few fp64 ulps, which
    moves an fp32 rounding only within 2^-29 of a tie: the inputs here are fixed and none lies there."""
    from dmvsnet_amd import ops
    pieces = (3,)
    case, _ = S.first_clean_pieces(C, pieces, spatial)
    running = running_init(C)
    (r,) = run(case, pieces, 0.1, running)
    x, gy, gamma, beta = (case[k].cuda() for k in ("x", "gy", "gamma", "beta"))
    rm, rv = (t.cuda() for t in running)
    y, mean, invstd = ops.bn_relu_forward(x, gamma, beta, rm, rv, 0.1, G.BN_EPS, True, True)
    gx, gg, gb = ops.bn_relu_backward(x, gy, gamma, beta, mean, invstd, True, True)
    for k, want in (("y", y), ("mean", mean), ("invstd", invstd), ("running_mean", rm), ("running_var", rv), ("g_x", gx), ("g_gamma", gg),
                    ("g_beta", gb)):
        print(f"ONE C {C} {spatial} {k}: equal {torch.equal(r[k], want)}, max-abs distance {(r[k] - want).abs().max().item():.3e}")
    for k, want in (("y", y), ("mean", mean), ("invstd", invstd), ("running_mean", rm), ("running_var", rv), ("g_x", gx), ("g_gamma", gg),
                    ("g_beta", gb)):
        assert torch.equal(r[k], want), k


@pytest.mark.parametrize("nd", (3, 2))
def test_module_without_a_group_and_in_eval_mode_is_the_plain_module(nd):
    """No process group (a group of one) in train mode, and eval mode: the sync module issues no collective and gives bit for bit the
    output, gradients and buffers of ``DiffBatchNormReLU*``."""
    import dmvsnet_amd as da
    from dmvsnet_amd import bn
    C = 16
    case, _ = S.first_clean_pieces(C, (2,), (2, 5, 9))
    x, gy = (shaped(case[k], nd).cuda() for k in ("x", "gy"))
    plain = (da.DiffBatchNormReLU3d if nd == 3 else da.DiffBatchNormReLU2d)(C, momentum=0.3).cuda()
    with torch.no_grad():
        plain.weight.copy_(case["gamma"]), plain.bias.copy_(case["beta"])
    sync = da.convert_sync_batchnorm((da.DiffBatchNormReLU3d if nd == 3 else da.DiffBatchNormReLU2d)(C, momentum=0.3).cuda())
    sync.load_state_dict(plain.state_dict(), strict=True)
    before = dict(bn.sync_launch_counts)
    for mode in ("train", "eval"):
        outs = []
        for m in (plain, sync):
            getattr(m, mode)()
            m.zero_grad()
            xin = x.clone().requires_grad_(True)
            y = m(xin)
            y.backward(gy)
            outs.append(dict(y=y.detach(), g_x=xin.grad, g_gamma=m.weight.grad.clone(), g_beta=m.bias.grad.clone(),
                             **{k: v.clone() for k, v in m.state_dict().items()}))
        for k in outs[0]:
            assert torch.equal(outs[0][k], outs[1][k]), (mode, k)
    assert bn.sync_launch_counts == before and int(sync.num_batches_tracked) == 1


# ------------------------------------------------------------------------------------------------ order, reproducibility, guards
def test_rank_order_and_reproducibility():
    """The gathered rows permuted (both buffers, the same permutation): another order of the fp64 adds, values within the bound; whether
    the bits moved is printed, not asserted.  The same order twice: torch.equal."""
    C, (spatial, pieces) = 16, SHAPES["v5000"]
    case, _ = S.first_clean_pieces(C, pieces, spatial)
    running = running_init(C)
    a, b = run(case, pieces, 0.1, running), run(case, pieces, 0.1, running)
    for ra, rb in zip(a, b):
        for k in KEYS:
            assert torch.equal(ra[k], rb[k]), f"{k} differs between two runs"
    p = run(case, pieces, 0.1, running, order=(2, 0, 1))
    compare("ORDER C 16 v5000 permuted (2, 0, 1)", p, case, pieces, 0.1, running)
    moved = {k: not all(torch.equal(ra[k], rp[k]) for ra, rp in zip(a, p)) for k in KEYS}
    print(f"ORDER bits moved by the permutation: {moved}")


def _band(n, dtype=torch.float32, guard=1024):
    full = torch.full((n + 2 * guard,), float("nan"), dtype=dtype, device="cuda")
    return full, full[guard:guard + n]


def _intact(full, n, guard=1024):
    return bool(torch.isfinite(full[guard:guard + n]).all() and torch.isnan(full[:guard]).all() and torch.isnan(full[guard + n:]).all())


@pytest.mark.parametrize("spatial", [(1, 8, 625), (2, 5, 9)])
def test_guard_bands_and_nan_filled_workspace(spatial):
    """The four entries called on buffers of this test's own: every output NaN-filled inside NaN guard bands, the workspace NaN-filled
    before each launch that uses it, and the gathered buffers followed by NaN rows beyond the R the kernels are told about.  Every
    output is written in full and finite, nothing outside it is touched, and the bits are those of the wrappers' path."""
    from dmvsnet_amd import _lib, ops
    lib, C, pieces = _lib.load(), 16, (2, 1)
    case, _ = S.first_clean_pieces(C, pieces, spatial)
    V, running, R = G.volume(spatial), running_init(C), len(pieces)
    want = run(case, pieces, 0.1, running)
    xs, gys = (S.split(case[k].cuda(), pieces) for k in ("x", "gy"))
    gamma, beta = case["gamma"].cuda(), case["beta"].cuda()
    P, st = ops._ptr, ops._stream()
    ws = torch.empty(lib.dmvs_bn_workspace(C, 2, V), device="cuda")
    g3_full, g3 = _band((R + 2) * C * 3, torch.float64)     # R rows and two NaN rows behind them, inside the bands
    for r, x in enumerate(xs):
        ws.fill_(float("nan"))
        S_r = ops.bn_plan(C, x.shape[0], V)
        assert lib.dmvs_bn_sync_moments(P(x), P(g3[r * C * 3:]), P(ws), x.shape[0], C, V, st) == 0
        assert torch.isfinite(ws[:2 * C * S_r + C]).all() and torch.isnan(ws[2 * C * S_r + C:]).all()
    assert _intact(g3_full, R * C * 3, 1024) and torch.isnan(g3[R * C * 3:]).all()
    sums_full, sums = _band((R + 2) * C * 2, torch.float64)
    outs = []
    for r, (x, gy) in enumerate(zip(xs, gys)):
        n, B = x.numel(), x.shape[0]
        (y_full, y), (m_full, m), (i_full, i) = _band(n), _band(C), _band(C)
        rm, rv = (t.cuda() for t in running)
        N = ctypes.c_long(0)
        code = lib.dmvs_bn_sync_forward(P(x), P(gamma), P(beta), P(rm), P(rv), P(g3), P(y), P(m), P(i), ctypes.byref(N),
                                        B, C, V, R, 0.1, G.BN_EPS, ops.RELU, st)
        assert code == 0 and N.value == sum(pieces) * V
        assert _intact(y_full, n) and _intact(m_full, C) and _intact(i_full, C)
        (gg_full, gg), (gb_full, gb) = _band(C), _band(C)
        ws.fill_(float("nan"))
        assert lib.dmvs_bn_sync_backward_sums(P(x), P(gy), P(gamma), P(beta), P(m), P(i), P(sums[r * C * 2:]), P(gg), P(gb), P(ws), B, C, V,
                                              ops.RELU, st) == 0
        assert _intact(gg_full, C) and _intact(gb_full, C)
        outs.append(dict(y=y, mean=m, invstd=i, running_mean=rm, running_var=rv, g_gamma=gg, g_beta=gb, x=x, gy=gy, N=N.value))
    assert _intact(sums_full, R * C * 2) and torch.isnan(sums[R * C * 2:]).all()
    for r, o in enumerate(outs):
        n = o["x"].numel()
        gx_full, gx = _band(n)
        assert lib.dmvs_bn_sync_backward_apply(P(o["x"]), P(o["gy"]), P(gamma), P(beta), P(o["mean"]), P(o["invstd"]), P(sums), P(gx),
                                               o["x"].shape[0], C, V, R, o["N"], ops.RELU, st) == 0
        assert _intact(gx_full, n)
        o["g_x"] = gx
        for k in KEYS:
            assert torch.equal(o[k].reshape(-1), want[r][k].reshape(-1)), (r, k)
    # the wrappers with NaN rows behind the gathered buffers: the same bits
    padded = run(case, pieces, 0.1, running, pad_rows=2)
    assert all(torch.equal(a[k], b[k]) for a, b in zip(padded, want) for k in KEYS)


def test_bad_gathered_counts_are_refused():
    """A gathered n_r that is no positive integer, or differs between the channels of a rank, and a total below two: DMVS_EINVAL from
    the entry's own look at the buffer, before its launch (y stays NaN)."""
    from dmvsnet_amd import _lib, ops
    C = 8
    x = torch.randn(1, C, 1, 1, 3, device="cuda")
    vec = [torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")]
    good = torch.stack([ops.bn_sync_moments(x), ops.bn_sync_moments(x)])
    ops.bn_sync_forward(x, *vec, good, 0.1, 1e-5, True)
    for r, c, value in ((1, 0, 0.0), (0, 0, -3.0), (1, 0, 2.5), (0, 0, float("nan")), (1, 0, float("inf")), (0, 5, 4.0), (1, 0, 3e9)):
        bad = good.clone()
        bad[r, c, 0] = value
        with pytest.raises(_lib.DmvsError):
            ops.bn_sync_forward(x, *vec, bad, 0.1, 1e-5, True)
    one = torch.randn(1, C, 1, 1, 1, device="cuda")
    with pytest.raises(_lib.DmvsError):   # N = 1
        ops.bn_sync_forward(one, *vec, ops.bn_sync_moments(one)[None], 0.1, 1e-5, True)


def test_need_gx_false_skips_apply_and_collective(monkeypatch):
    """An input that needs no gradient: the sums launch alone (``sync_launch_counts``), weight / bias gradients still the local sums."""
    from dmvsnet_amd import bn, ops
    C = 8
    case, _ = S.first_clean_pieces(C, (2,), (2, 5, 9))
    x, gy, gamma, beta = (case[k].cuda() for k in ("x", "gy", "gamma", "beta"))
    w, b = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    # the Function with a hand-made gather: a world of one through the sync launches (the module would take the plain path)
    import torch.distributed as dist
    monkeypatch.setattr(dist, "all_gather_into_tensor", lambda recv, send, group=None: recv.copy_(send))
    outs = {}
    for need in (True, False):
        before = dict(bn.sync_launch_counts)
        xin = x.clone().requires_grad_(need)
        y = bn._SyncBnReluFn.apply(xin, w, b, torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), 0.1, G.BN_EPS, True, None, 1)
        grads = torch.autograd.grad(y, ([xin] if need else []) + [w, b], gy)
        outs[need] = grads[-2:]
        d = {k: bn.sync_launch_counts[k] - before[k] for k in before}
        print(f"SKIP need_gx {need}: {d}")
        assert d == {"moments": 1, "sums": 1, "apply": int(need), "gather": 1 + int(need)}
    assert torch.equal(outs[True][0], outs[False][0]) and torch.equal(outs[True][1], outs[False][1])
    # and at the wrappers' level: need_gx False is the sums call alone
    ranks = S.emulate(ops, [x], [gy], gamma, beta, 0.1, G.BN_EPS, True, need_gx=False)
    assert ranks[0]["g_x"] is None and torch.equal(ranks[0]["g_gamma"], outs[True][0]) and torch.equal(ranks[0]["g_beta"], outs[True][1])
