"""Test infrastructure: yardstick, criterion and case tables of the depth head's FORWARD -- the `prob` convolution (K2,
``conv_cout2_kernel``), its fused form ``dmvs_prob_regress`` and K4 (``depth_regress_kernel``, ``depth_regress_split_kernel``,
``depth_select_kernel``).  No product code here; tests/test_depth_head_cpu.py checks this file against the recorded reference
outputs, the oracle and ATen, asserts the conditions the tables claim and shows which mistakes the criterion catches;
tests/test_depth_head_gpu.py holds the kernels to it.

Restated from the formulas (reference networks/module.py:379,397,454-460, networks/mvsnet.py:15-100), dtype-generic, float64 on the
CPU being the yardstick:

  prob_conv   y[co,v] = sum_{ci,t} w[co,ci,t] x[ci,v+t-1], zero outside the volume: 27 explicit taps, no convolution library.
  head        p = softmax_D(alpha * logits); dsp[c] = sum_d p[c,d] hyp[d]; then ``tail``.
  tail        (lo, hi) = (min, max) of the pair of the row class, the six-stack and its checkerboard window (mode 0) or the
              checkerboard pick (mode 1); conf = 2 (sigmoid(interval / (std_pop(dsp) + 1e-5)) - 0.5).
  affine      plane d = base + d * interval, from the fp32 ``base`` and ``interval`` widened to float64.

Criterion (the project's): e_max = max|a - f64| / max|f64| and e_mean = mean|a - f64| / max|f64|, each e_hip <= 8 e_ref, and
16 * 2^-23 where e_ref < 4 * 2^-23.  e_ref is the distance of the fp32 ORACLE (F.conv3d on the CPU; oracle.dmvs_oracle's
depth_regress_main / _refine) on the same inputs, never of the code under test.

Conditional checks (``sel_cap`` / ``conf_cap``): the kernel's own fp32 ``dsp`` pushed through the float64 ``tail`` is what the
kernel's tail was handed to compute, in exact arithmetic; the caps count the tail's fp32 roundings and do not depend on e_ref."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from head_grad_ref import make_case, select, softmax_expect

F64, F32 = torch.float64, torch.float32
FACTOR = 8.0
EPS32 = 2.0 ** -23
U32 = 2.0 ** -24            # unit roundoff of fp32
CONF_EPS = 1e-5             # mvsnet.py:61,96
MUTATION_RATIO = 20.0       # a mistake counts as caught when it is this many times over bound_of(e_ref)


# ------------------------------------------------------------------------------------------------ criterion
def bound_of(e_ref):
    return FACTOR * e_ref if e_ref >= 4 * EPS32 else 16 * EPS32


def errors(a, f64, keep=None):
    """(e_max, e_mean) of ``a`` against the yardstick, normalised by the yardstick's max-abs; over the elements of the bool mask
    ``keep`` where given.  (0, 0) where both are identically zero."""
    a, f64 = a.detach().to("cpu", F64), f64.detach().to("cpu", F64)
    assert a.shape == f64.shape, (a.shape, f64.shape)
    if keep is not None:
        a, f64 = a[keep], f64[keep]
    diff, scale = (a - f64).abs(), f64.abs().max().item()
    if scale == 0.0:
        return (0.0, 0.0) if diff.max().item() == 0.0 else (float("inf"), float("inf"))
    return diff.max().item() / scale, diff.mean().item() / scale


def bounds(e_ref):
    return bound_of(e_ref[0]), bound_of(e_ref[1])


# ------------------------------------------------------------------------------------------------ restatement
TAPS = [(kz, ky, kx) for kz in range(3) for ky in range(3) for kx in range(3)]
PROB_MUTATIONS = ("seam_tap", "row15_halo", "kz2_last_plane")


def prob_conv(x, w, dtype=F64, mutation=None):
    """x [Cin,D,H,W], w [2,Cin,3,3,3] -> [2,D,H,W].  ``mutation``: a mistake of conv_cout2_kernel, for the CPU file --
    seam_tap: tap (1,1,2) dropped at the columns x in {32 b, 32 b + 1} next to a seam of the 32-wide tiles (both tile grids);
    row15_halo: the last row of a 16-row tile reads, for ky = 2, the tile's upper halo row (16 by - 1) instead of row y + 1;
    kz2_last_plane: depth tap kz = 2 dropped on the last plane of a 4-plane block."""
    x, w = x.to(dtype), w.to(dtype)
    Cin, D, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    zz, yy, xx = torch.arange(D).view(D, 1, 1), torch.arange(H), torch.arange(W).view(1, 1, W)
    out = torch.zeros((w.shape[0], D, H, W), dtype=dtype)
    for kz, ky, kx in TAPS:
        rows = yy + ky     # padded row index of the tap
        if mutation == "row15_halo" and ky == 2:
            rows = torch.where(yy % 16 == 15, 16 * (yy // 16), rows)
        term = torch.einsum("oi,idhw->odhw", w[:, :, kz, ky, kx], xp[:, kz:kz + D][:, :, rows][..., kx:kx + W])
        if mutation == "seam_tap" and (kz, ky, kx) == (1, 1, 2):
            term = term * (xx % 32 > 1).to(dtype)
        if mutation == "kz2_last_plane" and kz == 2:
            term = term * (zz % 4 != 3).to(dtype)
        out = out + term
    return out


def tail(dsp, interval, mode):
    """dsp [4,H,W] -> (sel ([4,H,W] | [H,W]), conf [H,W]): the part behind the four expectations."""
    sel = select(dsp.unsqueeze(0), mode)[0]
    mean = dsp.mean(0)
    std = ((dsp - mean) ** 2).mean(0).sqrt()      # population spread (var(1, unbiased=False))
    return sel, 2 * (torch.sigmoid(interval / (std + CONF_EPS)) - 0.5)


def head(logits, hyp, interval, alpha, mode):
    """logits [4,D,H,W], hyp [D,H,W] -> dict prob [4,D,H,W], dsp [4,H,W], sel, conf, in the inputs' dtype."""
    p, dsp = softmax_expect(logits.unsqueeze(0), hyp.unsqueeze(0), alpha)
    sel, conf = tail(dsp[0], interval, mode)
    return {"prob": p[0], "dsp": dsp[0], "sel": sel, "conf": conf}


def affine_planes(base, interval, D, dtype=F64):
    """[D,H,W].  float64: the yardstick's planes from the fp32 base and interval; float32: the roundings of the kernels and of
    ``AffinePlanes.volume`` (d * interval, then + base)."""
    d = torch.arange(D, dtype=dtype).view(-1, 1, 1)
    return base.to(dtype)[None] + d * interval.to(dtype)


HEAD_MUTATIONS = ("alpha_dropped", "no_normalise", "planes_shifted", "last_block_w1", "q2_plain", "window_parity", "mode1_swap",
                  "unbiased", "no_factor2", "no_eps")


def head_mutated(logits, hyp, interval, alpha, mode, mutation=None):
    """``head`` written out formula by formula with one mistake of K4 built in (None: none; the CPU file holds that to ``head``).

    alpha_dropped   alpha reaches the max search only: exp(l - max(alpha l)).  (The issue's "alpha applied after the
                    max-subtraction", alpha (l - max l), IS alpha l - max(alpha l) for alpha > 0: an identity; this is the nearest
                    mistake that is none.  Visible where alpha != 1.)
    no_normalise    p not divided by the sum
    planes_shifted  the expectation pairs p[d] with plane d + 1 (the last with itself)
    last_block_w1   every lane of the last, ragged 64-pixel block reads pixel W - 1 (the clamp of the dead lanes on the live ones)
    q2_plain        row classes q >= 2 use (lo, hi) instead of (2 lo - hi, 2 hi - lo)
    window_parity   the [0:4] / [2:6] windows of the six-stack swapped
    mode1_swap      mode 1's (1,0) / (1,1) entries swapped
    unbiased        the spread divides by 3
    no_factor2      conf = sigmoid(z) - 0.5
    no_eps          z = interval / std"""
    _, D, H, W = logits.shape
    dt = logits.dtype
    if mutation == "last_block_w1" and W % 64:
        xs = torch.arange(W)
        xs = torch.where(xs >= 64 * (W // 64), W - 1, xs)
        logits, hyp = logits[..., xs], hyp[..., xs]
    z = logits * alpha
    m = z.max(1, keepdim=True)[0]
    e = torch.exp((logits if mutation == "alpha_dropped" else z) - m)
    p = e if mutation == "no_normalise" else e / e.sum(1, keepdim=True)
    planes = hyp[torch.clamp(torch.arange(D) + 1, max=D - 1)] if mutation == "planes_shifted" else hyp
    dsp = (p * planes[None]).sum(1)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    sm, sM = torch.minimum(dsp[0], dsp[1]), torch.maximum(dsp[0], dsp[1])
    hm, hM = torch.minimum(dsp[2], dsp[3]), torch.maximum(dsp[2], dsp[3])
    if mode == 1:
        a, b = (hm, hM) if mutation == "mode1_swap" else (hM, hm)
        sel = torch.where(yy % 2 == 0, torch.where(xx % 2 == 0, sm, sM), torch.where(xx % 2 == 0, a, b))
    else:
        q = yy % 4
        lo, hi = torch.where(q % 2 == 1, hm, sm), torch.where(q % 2 == 1, hM, sM)
        if mutation != "q2_plain":
            lo, hi = torch.where(q >= 2, 2 * lo - hi, lo), torch.where(q >= 2, 2 * hi - lo, hi)
        st = [3 * lo - 2 * hi, 2 * lo - hi, lo, hi, 2 * hi - lo, 3 * hi - 2 * lo]
        upper = ((yy + xx) % 2 == 1) != (mutation == "window_parity")
        sel = torch.stack([torch.where(upper, st[k + 2], st[k]) for k in range(4)])
    mean = (dsp[0] + dsp[1] + dsp[2] + dsp[3]) / 4
    var = sum((dsp[c] - mean) ** 2 for c in range(4)) / (3 if mutation == "unbiased" else 4)
    s = torch.sigmoid(interval / (var.sqrt() + (0.0 if mutation == "no_eps" else CONF_EPS)))
    conf = (1 if mutation == "no_factor2" else 2) * (s - 0.5)
    return {"prob": p.to(dt), "dsp": dsp, "sel": sel, "conf": conf}


# ------------------------------------------------------------------------------------------------ the fp32 oracle (e_ref)
def oracle_head(logits, hyp, interval, alpha, mode):
    """The fp32 oracle on fp32 CPU inputs -> the dict of ``head``.  depth_regress_main has no alpha: it gets alpha * logits, the
    product its own softmax would form (``_expectation`` multiplies first, then softmax)."""
    from oracle import dmvs_oracle as O
    L, hv = logits.unsqueeze(0), hyp.unsqueeze(0)
    if mode == 0:
        o = O.depth_regress_main(L * alpha if alpha != 1.0 else L, hv, interval)
        return {"prob": o["prob_volume"][0], "dsp": o["depth_sub_plus"][0], "sel": o["depth_values_c"][0],
                "conf": o["photometric_confidence"][0]}
    o = O.depth_regress_refine(L, hv, interval, alpha)
    prob = F.softmax(L * alpha if alpha != 1.0 else L, dim=2)[0]     # (refine returns no volume: _expectation's own line)
    return {"prob": prob, "dsp": o["depth_sub_plus_refine"][0], "sel": o["depth"][0], "conf": o["photometric_confidence_refine"][0]}


def oracle_conv(x, w):
    """F.conv3d in fp32 on the CPU: x [Cin,D,H,W], w [2,Cin,3,3,3] -> [2,D,H,W]."""
    return F.conv3d(x.unsqueeze(0), w, padding=1)[0]


# ------------------------------------------------------------------------------------------------ conditional caps
def sel_cap(dsp32, mode0_sel64):
    """Per-element cap on |kernel sel - tail(dsp32)| in mode 0, dsp32 the kernel's own fp32 expectations, counting roundings
    (u = 2^-24; a contraction into an fma only removes some):

      lo, hi are selections: exact.  Row classes q >= 2 form lo' = fl(2 lo - hi), hi' = fl(2 hi - lo) (2 x is exact): one rounding
      each, |d lo'| <= u |lo'|, |d hi'| <= u |hi'|.  A stack entry is fl(fl(a lo') - fl(b hi')) with (a, b) up to (3, 2): the
      inherited errors enter with weights a and b, each product rounds once (<= u a |lo'|, u b |hi'|) and the difference once
      (<= u |entry|).  With |entry| <= a |lo'| + b |hi'| and a + b <= 5:

          |error| <= u (2 a |lo'| + 2 b |hi'| + |entry|) <= 3 u (3 |lo'| + 2 |hi'|) <= 15 u max(|lo'|, |hi'|)

      and max(|lo'|, |hi'|) <= 3 max|dsp| (q >= 2), so 45 u max|dsp| holds for every entry of every row class.  It is a handful
      of fp32 operations on magnitudes up to 5 max|dsp| (15 in the doubled classes), nothing else."""
    return 45 * U32 * dsp32.abs().max().item() * torch.ones_like(mode0_sel64)


CONF_SLOPE = 1.08    # |dconf/dstd| <= 1.08 / interval: conf = tanh(z / 2), z = interval / (std + 1e-5), dz/dstd = -z^2 / interval,
#                      |dconf/dstd| = (z^2 / 2) sech^2(z / 2) / interval, whose maximum over z is 0.88 (at z = 2.4) < 1.08


def conf_cap(dsp32, interval):
    """Per-pixel cap on |kernel conf - tail(dsp32)|, dsp32 the kernel's own fp32 expectations (interval > 0), counting roundings:

      mean    three additions and an exact / 4 on magnitudes <= M = max|dsp|: |dmean| <= (2 + 3 + 4) u M / 4 < 2.5 u M.
      std     the kernel's differences are (e_c - mean') rounded: a common shift dmean turns var into var + dmean^2 exactly, i.e.
              std into sqrt(std^2 + dmean^2); rounding the four differences (<= u |d_c|, |d_c| <= 2 std) moves std by <= 2 u std;
              squares, three additions, the exact / 4 and the square root are relative roundings of var, together < 3 u std.
              |dstd| <= sqrt(std^2 + dmean^2) - std + 5 u std.
      conf    Lipschitz in std with CONF_SLOPE / interval (mean-value theorem, any size of dstd); behind std: the addition of
              1e-5f and the division (z to 3 u relative with the fp32 1e-5; z s (1 - s) <= 0.23), expf to 2 ulp, 1 + e, the division
              (s <= 1) and exact s - 0.5 (Sterbenz) and * 2: < 2 (0.7 + 0.5 + 2) u = 6.4 u, taken as 8 u = 4 * 2^-23.

    A factor 1.5 on the std term covers second-order terms and the 1-ulp latitude of sqrtf / expf on the device."""
    d = dsp32.to(F64)
    M = d.abs().max().item()
    std = ((d - d.mean(0)) ** 2).mean(0).sqrt()
    dmean = 2.5 * U32 * M
    dstd = (std ** 2 + dmean ** 2).sqrt() - std + 5 * U32 * std
    return 1.5 * CONF_SLOPE / float(interval) * dstd + 8 * U32


# ------------------------------------------------------------------------------------------------ case tables
def _rng(seed, tag):
    return np.random.Generator(np.random.PCG64([int(seed), zlib.crc32(tag.encode())]))


# plain `prob`, (Cin, D, H, W, misaligned): W % 4 == 0 takes the V4 form (tiles shifted by one voxel: tile bx owns x in
# 32 bx - 31 .. 32 bx, one extra tile column), every other width -- and a V4 width behind a pointer that is not 16-byte aligned --
# the dword loader.  Tiles are 4 planes x 16 rows x 32 columns.
PROB_SHAPES = (
    (8, 1, 1, 1, False), (8, 1, 1, 4, False), (8, 5, 17, 36, False), (8, 9, 33, 68, False),
    (8, 2, 15, 32, False), (8, 4, 16, 64, False), (8, 1, 33, 32, False), (8, 2, 17, 68, False), (8, 9, 15, 4, False), (8, 2, 1, 64, False),
    (8, 2, 16, 3, False), (8, 4, 15, 31, False), (8, 5, 1, 33, False), (8, 9, 17, 65, False), (8, 4, 33, 1, False), (8, 5, 16, 65, False),
    (2, 5, 17, 36, False), (16, 4, 17, 33, False),
    (8, 5, 17, 36, True),
)
PROB_W_V4, PROB_W_DWORD = (4, 32, 36, 64, 68), (1, 3, 31, 33, 65)
PROB_H, PROB_D = (1, 15, 16, 17, 33), (1, 2, 4, 5, 9)

# dmvs_prob_regress, (D, H, W), Cin 8: each with a hypothesis volume and with AffinePlanes, at alpha 1 and 5
FUSED_SHAPES = ((4, 1, 4), (8, 15, 32), (4, 16, 36), (8, 17, 64), (4, 33, 68), (8, 1, 68), (4, 17, 32), (8, 33, 36), (4, 15, 64),
                (8, 16, 4))
FUSED_D, FUSED_W, FUSED_H = (4, 8), (4, 32, 36, 64, 68), (1, 15, 16, 17, 33)
# (Cin, D, H, W, misaligned) the fused entry declines: D = 5, D = 16, W = 30, odd Cin, misaligned input
FUSED_DECLINED = ((8, 5, 6, 8, False), (8, 16, 6, 8, False), (8, 4, 6, 30, False), (7, 4, 6, 8, False), (8, 4, 6, 8, True))

# K4, (D, H, W).  D picks the instantiation; H = 1, 2, 3 lack row classes on purpose (a kernel must not depend on seeing all four)
K4_FORM = {4: "reg4", 8: "reg8", 32: "split", 64: "split", 1: "generic", 2: "generic", 5: "generic", 16: "generic", 48: "generic"}
K4_SHAPES = (
    (4, 1, 1), (4, 7, 255), (8, 5, 256), (8, 3, 257), (4, 2, 300), (8, 7, 300),
    (32, 1, 1), (32, 7, 63), (64, 5, 64), (64, 3, 65), (32, 2, 130), (64, 7, 130),
    (1, 3, 257), (2, 5, 300), (5, 7, 255), (16, 2, 256), (48, 7, 1),
)
K4_W_THREAD, K4_W_SPLIT, K4_H = (1, 255, 256, 257, 300), (1, 63, 64, 65, 130), (1, 2, 3, 5, 7)
K4_RUNS = ((0, 1.0), (1, 5.0), (0, 5.0), (1, 1.0))     # (mode, alpha): the product's two pairings and the crossed ones
DEPTHS = ("synth", "inverse", "unit", "affine")


def prob_case(Cin, D, H, W, seed=0, gain=1.0):
    """fp32 x [Cin,D,H,W] and a He-sized weight [2,Cin,3,3,3] times ``gain`` (CPU)."""
    g = torch.Generator().manual_seed(104729 * seed + 7919 * Cin + 31 * D + 17 * H + W)
    x = torch.randn((Cin, D, H, W), generator=g)
    w = torch.randn((2, Cin, 3, 3, 3), generator=g) * (gain * (2.0 / (Cin * 27)) ** 0.5)
    return x, w


def planes_of(kind, D, H, W, case, seed):
    """fp32 hypothesis planes [D,H,W] of one DEPTHS set, never smooth across pixels.  synth: make_case's (about 600 mm, 16 mm span,
    per-pixel offset); inverse: uniform in 1/depth from 935 down to 425 mm, as inverse-depth sampling gives, times a per-pixel
    factor within 1 %; unit: 0.5 .. 2, so that a relative error is not hidden behind 600 mm."""
    if kind in ("synth", "affine"):
        return case["hyp"][0]
    g = _rng(seed, f"planes.{kind}.{D}.{H}.{W}")
    jitter = torch.from_numpy(g.random((H, W), dtype=np.float32))
    t = torch.arange(D, dtype=F32).view(-1, 1, 1) / max(D - 1, 1)
    if kind == "inverse":
        return (1.0 / (1.0 / 935.0 + t * (1.0 / 425.0 - 1.0 / 935.0))) * (1.0 + 0.01 * jitter)
    assert kind == "unit"
    return 0.5 + 1.5 * t * (0.9 + 0.1 * jitter)


@functools.lru_cache(maxsize=None)
def k4_case(D, H, W, kind):
    """One K4 case: fp32 CPU logits [4,D,H,W], planes [D,H,W] (affine: ``base`` [H,W] too, planes = the fp32 volume of
    base + d * interval), interval (0-dim fp32).  ``interval``: the step for affine planes (they are made of it); otherwise the
    median over the map of the yardstick's spread at alpha 1, plus 1e-5 -- z = 1 at the median pixel, so that the confidence is
    mid-range on most of the map (asserted in the CPU file, not assumed)."""
    seed = 1000 * D + 10 * H + W
    case = make_case(D, H, W, seed=seed)
    logits = case["logits"][0].contiguous()
    if kind == "affine":
        # z = interval / std is about 1 / (spread of the expected plane INDEX) whatever the step: a bump around a per-pixel plane,
        # common to the four channels as in a trained network's output, keeps that spread near one plane at every D
        d0 = torch.from_numpy(_rng(seed, "affine.peak").random((H, W), dtype=np.float32)) * (D - 1)
        logits = (logits - 0.5 * (torch.arange(D, dtype=F32).view(1, D, 1, 1) - d0) ** 2).contiguous()
        interval = torch.tensor(case["interval"], dtype=F32)
        base = case["hyp"][0, 0].contiguous()
        return {"logits": logits, "base": base, "hyp": affine_planes(base, interval, D, F32), "interval": interval}
    hyp = planes_of(kind, D, H, W, case, seed).to(F32).contiguous()
    _, dsp = softmax_expect(logits.double().unsqueeze(0), hyp.double().unsqueeze(0), 1.0)
    std = ((dsp[0] - dsp[0].mean(0)) ** 2).mean(0).sqrt()
    return {"logits": logits, "base": None, "hyp": hyp, "interval": (std.median() + CONF_EPS).to(F32)}


def yardstick_planes(case):
    D = case["logits"].shape[1]
    return affine_planes(case["base"], case["interval"], D) if case["base"] is not None else case["hyp"].double()


@functools.lru_cache(maxsize=None)
def k4_reference(D, H, W, kind, mode, alpha):
    """(float64 yardstick dict, {name: (e_max, e_mean)} of the fp32 oracle) of one run of a case; computed once, never modified."""
    c = k4_case(D, H, W, kind)
    y = head(c["logits"].double(), yardstick_planes(c), c["interval"].double(), alpha, mode)
    o = oracle_head(c["logits"], c["hyp"], c["interval"], alpha, mode)
    return y, {k: errors(o[k], y[k]) for k in y}


def mid_share(conf64):
    return ((conf64 > 0.05) & (conf64 < 0.95)).double().mean().item()


@functools.lru_cache(maxsize=None)
def fused_case(D, H, W, Cin=8):
    """One fused case: x [Cin,D,H,W], the two branches' weights (gain 3: peaky logits, as make_case's), planes and base / interval
    as ``k4_case`` makes them (kinds synth and affine)."""
    x, w0 = prob_case(Cin, D, H, W, seed=1, gain=3.0)
    _, w1 = prob_case(Cin, D, H, W, seed=2, gain=3.0)
    return {"x": x, "w": (w0, w1), "synth": k4_case(D, H, W, "synth"), "affine": k4_case(D, H, W, "affine")}


@functools.lru_cache(maxsize=None)
def fused_reference(D, H, W, kind, mode, alpha):
    """As k4_reference, with the logits the float64 ``prob_conv`` of the case's input (oracle: F.conv3d in fp32)."""
    c = fused_case(D, H, W)
    k = c[kind]
    L64 = torch.cat([prob_conv(c["x"], w) for w in c["w"]])
    L32 = torch.cat([oracle_conv(c["x"], w) for w in c["w"]])
    y = head(L64, yardstick_planes(k), k["interval"].double(), alpha, mode)
    o = oracle_head(L32, k["hyp"], k["interval"], alpha, mode)
    return y, {n: errors(o[n], y[n]) for n in y}


# impulse response of the plain `prob`: unit impulses whose 3 x 3 x 3 supports are pairwise disjoint over ALL channels, so every
# output voxel is one weight or 0 and fp32 reproduces it exactly
IMPULSE_VOLUME = (9, 33, 68)    # D, H, W
IMPULSE_Z, IMPULSE_Y, IMPULSE_X = (0, 3, 4, 8), (0, 15, 16, 32), (0, 1, 31, 32, 33, 67)


def impulse_sites(Cin=8):
    """[(ci, z, y, x)]: greedily every (z, y, x) of the product of the three lists that keeps a Chebyshev distance >= 3 to the ones
    kept before, walked in an order that spreads them; channels in turn."""
    pts = [(z, y, x) for z in IMPULSE_Z for y in IMPULSE_Y for x in IMPULSE_X]
    order = np.random.Generator(np.random.PCG64(5)).permutation(len(pts))
    kept = []
    for i in order:
        p = pts[i]
        if all(max(abs(a - b) for a, b in zip(p, q)) >= 3 for q in kept):
            kept.append(p)
    return [(k % Cin,) + p for k, p in enumerate(kept)]


def impulse_case(Cin=8):
    D, H, W = IMPULSE_VOLUME
    x = torch.zeros((Cin, D, H, W))
    for ci, z, y, xx in impulse_sites(Cin):
        x[ci, z, y, xx] = 1.0
    _, w = prob_case(Cin, D, H, W, seed=3)
    return x, w


# ------------------------------------------------------------------------------------------------ SPECIAL
def special_one_hot(D, H, W, seed=0):
    """(a) one logit per (pixel, channel) at +80, the rest 0 (alpha 5: 400 before the max-subtraction, finite after it); p is
    one-hot and dsp the chosen plane's depth exactly.  -> (logits [4,D,H,W], hot [4,H,W] int64)."""
    hot = torch.from_numpy(_rng(seed, f"hot.{D}.{H}.{W}").integers(0, D, (4, H, W)))
    return torch.zeros((4, D, H, W)).scatter_(1, hot.unsqueeze(1), 80.0), hot


def special_equal(D, H, W, seed=0):
    """(b) all logits of a pixel equal (one random value per pixel and channel): p = 1 / D."""
    v = torch.from_numpy(_rng(seed, f"equal.{D}.{H}.{W}").standard_normal((4, 1, H, W), dtype=np.float32))
    return v.expand(4, D, H, W).contiguous()


def special_identical(case):
    """(c), (d) four identical channels: the four expectations are the same bits, var == 0."""
    return case["logits"][:1].expand(4, -1, -1, -1).contiguous()


CONF_AT_Z2 = 2 * (1 / (1 + np.exp(-2.0)) - 0.5)   # (c): interval 2e-5, std 0 -> z = 2
