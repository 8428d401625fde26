"""Yardstick of the synchronised BatchNorm + ReLU (K5's sync launches): the combine of per-rank moments restated in float64, the raw-sums
combine in fp32 that it replaces (to show what the tables can tell apart), per-rank slices of the float64 restatement of
tests/bn_grad_ref.py on the CONCATENATED batch, the seeded piece generator, and a driver that emulates R ranks in one process through
the four ``ops`` wrappers (it takes ``ops`` as an argument: nothing here imports product code).

A "piece" is what one rank holds: whole samples of the batch.  ``pieces`` = (B_0, .., B_{R-1})."""
import torch

import bn_grad_ref as G

FACTOR = 8.0
EPS32 = 2.0 ** -23


def bound_of(e_ref):
    """The criterion of tests/test_bn_grad_gpu.py: e_hip <= 8 e_ref, and where e_ref < 4 * 2^-23 the bound is 16 * 2^-23."""
    return FACTOR * e_ref if e_ref >= 4 * EPS32 else 16 * EPS32


def split(t, pieces):
    """[sum(pieces), ...] -> the ranks' tensors, by whole samples."""
    assert t.shape[0] == sum(pieces)
    return [p.contiguous() for p in torch.split(t, list(pieces), 0)]


def moments(x, dtype=torch.float64):
    """[C, 3] = (n, mean, M2) per channel of one piece, M2 the sum of squared deviations about the piece's own mean."""
    xc = x.detach().to("cpu", dtype).transpose(0, 1).reshape(x.shape[1], -1)
    n = xc.shape[1]
    mean = xc.sum(1) / n
    return torch.stack((torch.full_like(mean, n), mean, ((xc - mean[:, None]) ** 2).sum(1)), 1)


def combine(gathered):
    """[R, C, 3] moments in rank order -> (N [C], mean [C], biased variance [C], M2 [C]): N = sum n_r, mean = sum n_r mean_r / N,
    M2 = sum (M2_r + n_r (mean_r - mean)^2), var = M2 / N.  In the dtype of ``gathered``, ranks added in the order 0 .. R-1."""
    N, sm = torch.zeros_like(gathered[0, :, 0]), torch.zeros_like(gathered[0, :, 0])
    for r in range(gathered.shape[0]):
        N = N + gathered[r, :, 0]
        sm = sm + gathered[r, :, 0] * gathered[r, :, 1]
    mean = sm / N
    M2 = torch.zeros_like(mean)
    for r in range(gathered.shape[0]):
        d = gathered[r, :, 1] - mean
        M2 = M2 + gathered[r, :, 2] + gathered[r, :, 0] * (d * d)
    return N, mean, M2 / N, M2


def combine_raw_sums_fp32(xs):
    """What must NOT travel: every rank ships (n, sum x, sum x^2) in fp32; var = sum x^2 / N - mean^2.  -> (mean, var) in fp32."""
    n = sum(x.numel() // x.shape[1] for x in xs)
    s1 = sum(x.float().transpose(0, 1).reshape(x.shape[1], -1).sum(1) for x in xs)
    s2 = sum((x.float() ** 2).transpose(0, 1).reshape(x.shape[1], -1).sum(1) for x in xs)
    mean = s1 / n
    return mean, s2 / n - mean * mean


def make_pieces(C, pieces, spatial, seed, offsets=None, std=1.0):
    """The case of ``bn_grad_ref.make_case`` on the concatenated batch (same keys: x, gamma, beta, gy), piece r shifted by offsets[r]
    and scaled by ``std``."""
    B = sum(pieces)
    case = G.make_case(C, B, spatial, seed)
    x = case["x"] * std
    if offsets is not None:
        assert len(offsets) == len(pieces)
        shift = torch.cat([torch.full((b,), float(o)) for b, o in zip(pieces, offsets)])
        x = x + shift.reshape((B,) + (1,) * (x.dim() - 1))
    return dict(case, x=x.contiguous())


def first_clean_pieces(C, pieces, spatial, offsets=None, std=1.0, limit=40):
    """(case, seed) of the first seed whose concatenated case has no pre-activation within KINK_MARGIN of the kink in float64."""
    for seed in range(limit):
        case = make_pieces(C, pieces, spatial, seed, offsets, std)
        if G.kink_violations(case) == 0:
            return case, seed
    raise AssertionError(f"no seed below {limit} without a kink violation for C {C}, pieces {pieces}, {spatial}")


def local_param_grads(case, pieces, relu=True, eps=G.BN_EPS):
    """Per rank (g_gamma, g_beta) in float64: the LOCAL sums of g and g * xhat under the statistics of the concatenated batch."""
    pre, _, mean, invstd = G.forward(case["x"], case["gamma"], case["beta"], relu, eps)
    x, gy = case["x"].double(), case["gy"].double()
    g = torch.where(pre > 0, gy, torch.zeros_like(gy)) if relu else gy
    xhat = (x - G._bc(mean, x)) * G._bc(invstd, x)
    out = []
    for gp, hp in zip(split(g, pieces), split(g * xhat, pieces)):
        out.append((G._per_channel(hp).sum(1), G._per_channel(gp).sum(1)))
    return out


def f64_per_rank(case, pieces, momentum, relu=True, eps=G.BN_EPS, running=None):
    """Everything a rank holds after one step, in float64 on the concatenated batch: per rank a dict y, g_x (the rank's samples),
    g_gamma / g_beta (local sums), mean, invstd, running_mean, running_var (the same for all ranks)."""
    f64 = G.all_f64(case["x"], case["gy"], case["gamma"], case["beta"], relu, eps)
    C = case["x"].shape[1]
    rm0, rv0 = running if running is not None else (torch.zeros(C), torch.ones(C))
    rm, rv = G.running_update(rm0, rv0, case["x"], momentum, eps)
    ys, gxs, loc = split(f64["y"], pieces), split(f64["g_x"], pieces), local_param_grads(case, pieces, relu, eps)
    return [dict(y=ys[r], g_x=gxs[r], g_gamma=loc[r][0], g_beta=loc[r][1], mean=f64["mean"], invstd=f64["invstd"], running_mean=rm,
                 running_var=rv) for r in range(len(pieces))]


def e_ref_of(case, relu=True, eps=G.BN_EPS):
    """e_ref per tensor: stock fp32 ATen on the concatenated batch against float64 on the same.  A rank's g_gamma / g_beta are held to
    the e_ref of the global sums: a local sum is a shorter chain of the same terms, measured over the largest channel as they are."""
    f64 = G.all_f64(case["x"], case["gy"], case["gamma"], case["beta"], relu, eps)
    ref = G.aten_fp32(case["x"], case["gy"], case["gamma"], case["beta"], relu, eps)
    return {k: G.rel_dist(ref[k].reshape(f64[k].shape), f64[k]) for k in f64}


def emulate(ops, xs, gys, gamma, beta, momentum, eps, relu, running=None, need_gx=True, order=None, pad_rows=0):
    """R ranks in one process, through the four wrappers and no process group: moments per piece, the gathered buffer stacked by hand
    (``order``: a permutation of the ranks' rows; ``pad_rows``: that many NaN rows after the R the kernels are told about), forward,
    backward sums and apply per piece.  Device tensors in, per rank a dict of device tensors out (g_x None without ``need_gx``)."""
    R = len(xs)
    C = xs[0].shape[1]
    order = list(range(R)) if order is None else list(order)
    dev = xs[0].device

    def gather(rows):
        buf = torch.stack([rows[r] for r in order] + [torch.full_like(rows[0], float("nan"))] * pad_rows)
        return buf[:R]   # (a view of the first R rows: the NaN rows lie right behind them in memory)

    gathered = gather([ops.bn_sync_moments(x) for x in xs])
    out = []
    for r in range(R):
        rm, rv = (t.to(dev).clone() for t in (running if running is not None else (torch.zeros(C), torch.ones(C))))
        y, mean, invstd, N = ops.bn_sync_forward(xs[r], gamma, beta, rm, rv, gathered, momentum, eps, relu)
        out.append(dict(y=y, mean=mean, invstd=invstd, N=N, running_mean=rm, running_var=rv))
    sums = []
    for r in range(R):
        s, gg, gb = ops.bn_sync_backward_sums(xs[r], gys[r], gamma, beta, out[r]["mean"], out[r]["invstd"], relu)
        sums.append(s)
        out[r].update(g_gamma=gg, g_beta=gb, g_x=None)
    if need_gx:
        gathered2 = gather(sums)
        for r in range(R):
            out[r]["g_x"] = ops.bn_sync_backward_apply(xs[r], gys[r], gamma, beta, out[r]["mean"], out[r]["invstd"], gathered2,
                                                       out[r]["N"], relu)
    return out


def running_fp32(case, momentum, running, eps=G.BN_EPS):
    """The running buffers after one train-mode step of stock fp32 ATen on the concatenated batch (the e_ref of the running buffers)."""
    import torch.nn.functional as F
    rm, rv = running[0].clone().float(), running[1].clone().float()
    F.batch_norm(case["x"].float(), rm, rv, case["gamma"].float(), case["beta"].float(), True, momentum, eps)
    return rm, rv
