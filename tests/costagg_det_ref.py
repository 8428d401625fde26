"""CPU emulation of K1b's deterministic mode (``warp_corr_bwd_src_kernel`` of csrc/warp_corr_bwd.h on the ``FixedSink`` of
csrc/warp_corr_bwd_det.h; the contract in docs/kernels/K1b_warp_corr_backward.md,
"Deterministic mode"): the source-view gradients of tests/warp_corr_grad_ref.py accumulated in FIXED POINT, in torch int64.

  addend    t = w_tap * ((gsim * 2/C) * ref) in fp32, two separately rounded products, from the yardstick's own taps
            (``warp_corr_grad_ref._taps`` on fp32 inputs, with the reference's normalise / un-normalise round trip that the kernel's
            ``ref_order_taps`` makes); a tap outside the image adds nothing
  k         eg = floor(log2(max |gsim|)), er = floor(log2(max |ref|)), E = eg + er + 2 + log2(2 / C), L = ceil(log2(D H W)),
            k = min(62 - L, 50) - E.  A maximum of zero: k = 0 (and every addend is zero).  A maximum that is not finite, or
            E > 127 (an addend may overflow fp32): every element NaN.
  quantum   q = rint(t * 2^k): the product exact in float64, ``torch.round`` = nearest even, then int64
  sum       ``index_add_`` in int64 -- in the order given (``perm``), which must not matter
  result    int64 -> float64 -> * 2^-k -> float32

No product code runs here.  ``MUTATIONS`` are the wrong emulations of the CPU file: ``no_headroom`` drops the addend count from k
(k = 62 - E: neither L nor the cap it feeds), ``truncate`` quantises towards zero."""
import math

import torch

import warp_corr_grad_ref as GR
from warp_corr_grad_ref import F32, F64

I64 = torch.int64
MUTATIONS = ("no_headroom", "truncate")


def floor_log2(x):
    """floor(log2(x)) of a positive finite number (exact: frexp)."""
    assert x > 0 and math.isfinite(x), x
    return math.frexp(x)[1] - 1


def exponent_of(ref, gsim, D, H, W, mutation=None):
    """(k, state) of one sample: state "ok", "zero" (k = 0, the result is all zeros) or "nan" (the result is all NaN)."""
    C = ref.shape[0]
    mg, mr = gsim.abs().max().item(), ref.abs().max().item()
    if not (math.isfinite(mg) and math.isfinite(mr)):   # a NaN maximum included: max() propagates it
        return 0, "nan"
    if mg == 0.0 or mr == 0.0:
        return 0, "zero"
    E = floor_log2(mg) + floor_log2(mr) + 2 + (1 - int(math.log2(C)))
    if E > 127:
        return 0, "nan"
    L = math.ceil(math.log2(D * H * W)) if D * H * W > 1 else 0
    assert 2 ** L >= D * H * W > 2 ** (L - 1) or D * H * W == 1
    return (62 if mutation == "no_headroom" else min(62 - L, 50)) - E, "ok"


def addends(feats, p12, depth, gsim):
    """Per source view (idx [4 N], t [C, 4 N] fp32, inside [4 N]) over the four taps of the N = D H W samples: the fp32 addends the
    kernel forms, the flat element each goes to, and whether the tap is inside the image (outside: t = 0, nothing is added)."""
    feats = [f.detach().to("cpu", F32) for f in feats]
    p12, depth, gsim = (t.detach().to("cpu", F32) for t in (p12, depth, gsim))
    ref = feats[0]
    C, H, W = ref.shape
    D = depth.shape[0]
    inv = torch.tensor(2.0 / C, dtype=F32)
    gw = (gsim.repeat(C // 2, 1, 1, 1) * inv) * ref.view(C, 1, H, W)   # [C,D,H,W]: (g * inv) * ref, one rounding (inv is a power of two)
    out = []
    for v in range(p12.shape[0]):
        idxs, ts, ins = [], [], []
        for raw, inside, idx in GR._taps(p12[v], depth, None, True):
            w = torch.where(inside, raw, torch.zeros((), dtype=F32))
            idxs.append(idx)
            ts.append((w * gw).reshape(C, -1))
            ins.append(inside.reshape(-1))
        out.append((torch.cat(idxs), torch.cat(ts, 1), torch.cat(ins)))
    return out


def quantise(t, k, mutation=None):
    x = t.to(F64) * (2.0 ** k)   # exact: a power of two
    return (torch.trunc(x) if mutation == "truncate" else torch.round(x)).to(I64)


def emulate(feats, p12, depth, gsim, perm_seed=None, mutation=None):
    """[dSrc_v] fp32 [C,H,W] per source view.  ``perm_seed``: add the addends in a random order (None: the taps' own order)."""
    assert mutation is None or mutation in MUTATIONS, mutation
    C, H, W = feats[0].shape
    D = depth.shape[0]
    k, state = exponent_of(feats[0].detach().to("cpu", F32), gsim.detach().to("cpu", F32), D, H, W, mutation)
    nsrc = p12.shape[0]
    if state == "nan":
        return [torch.full((C, H, W), float("nan"), dtype=F32) for _ in range(nsrc)]
    out = []
    for v, (idx, t, _) in enumerate(addends(feats, p12, depth, gsim)):
        q = quantise(t, k, mutation)
        if perm_seed is not None:
            perm = torch.randperm(idx.numel(), generator=torch.Generator().manual_seed(perm_seed + v))
            idx, q = idx[perm], q[:, perm]
        acc = torch.zeros((C, H * W), dtype=I64).index_add_(1, idx, q)
        out.append((acc.to(F64) * (2.0 ** -k)).to(F32).view(C, H, W))
    return out


def sequential_fp32(feats, p12, depth, gsim, perm_seed=None):
    """The same addends summed in fp32 one after the other in the given order (what an atomic path does in SOME order)."""
    C, H, W = feats[0].shape
    out = []
    for v, (idx, t, _) in enumerate(addends(feats, p12, depth, gsim)):
        if perm_seed is not None:
            perm = torch.randperm(idx.numel(), generator=torch.Generator().manual_seed(perm_seed + v))
            idx, t = idx[perm], t[:, perm]
        out.append(torch.zeros((C, H * W), dtype=F32).index_add_(1, idx, t).view(C, H, W))   # CPU index_add_: sequential
    return out


def float64_sums(feats, p12, depth, gsim):
    """Per source view (sum [C,H,W] float64 of the fp32 addends, n [H,W]: the taps inside the image that an element receives)."""
    C, H, W = feats[0].shape
    out = []
    for idx, t, inside in addends(feats, p12, depth, gsim):
        s = torch.zeros((C, H * W), dtype=F64).index_add_(1, idx, t.to(F64))
        n = torch.zeros((H * W,), dtype=F64).index_add_(0, idx, inside.to(F64))
        out.append((s.view(C, H, W), n.view(H, W)))
    return out


def wide_gsim(gsim):
    """``gsim`` with one element of 2^30: the maximum, and with it the grid 2^-k, moves up by about 28 binades, so that ordinary
    addends no longer sit on the grid and the rounding to it shows.  (With i.i.d. normal inputs alone k = 50 - E leaves an fp32 addend
    of 24 significant bits on the grid unless it is below 2^-27 of the bound: nearest-even and truncation then give the same bits.)"""
    g = gsim.clone()
    g[0, 0, 0, 0] = 2.0 ** 30
    return g


def exact_names():
    """The cases on which fp32 forms the tap weights exactly (the CPU file asserts it on every one): CONTENTION and the AFFINE cases
    whose offsets are multiples of 0.5.  There the kernel must equal ``emulate`` bit for bit."""
    cases = GR.all_cases()
    names = [n for n, c in cases.items() if c["table"] == "CONTENTION"]
    names += [GR.affine_name(C, ox, oy) for C in (8, 32) for ox, oy in GR.HALF_OFFSETS]
    assert len(names) == 10 + 16 and all(n in cases for n in names)
    return names
