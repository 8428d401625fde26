"""Test infrastructure: a torch restatement of the dual-depth head (K4 / K4b, csrc/depth_regress*.h*) and of the dual-depth loss
(N6 / N6b, csrc/validate.h), forward AND closed-form backward, like costagg_grad_ref.py.  Own code; dtype and device generic: the
tests run it in float64 on the CPU (the yardstick) and, as the "ATen restatement" of the chained-stage test, in fp32 on the GPU
under autograd.

What it restates: ``DepthNet.forward`` / ``.refine`` (networks/mvsnet.py:15-100) with ``depth_regression`` (module.py:454-460),
and ``mvs_loss`` in mode "regression" (loss.py:5-80, 106-159) in the PRODUCT's definition: exact quarter weights at the cell
centres, every 2x2 cell with four valid corners kept, the cell weight equal to the stage weight.

The closed-form backward is written independently of autograd (tests/test_head_grad_cpu.py checks it against
``torch.autograd.gradcheck`` of the forward above).  Gradient edges as in the reference's graph: ``depth_values_c`` is NOT
detached, so the refine pass sends ``sum_c p[c,d] G[c]`` into its hypotheses and from there into the main pass's logits.
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

# Conditions on the golden inputs (asserted by tests/golden/make_golden_head_grad.py, re-asserted by the tests): distances in mm,
# ~16 fp32 ulps of a 600 mm depth, several times the fp32 rounding of a D-term expectation (measured < 2e-4 on the cases).
MARGIN = 1e-3

# name: make_case arguments.  Sizes: odd H and W, H / W not multiples of 4, every row class y % 4 present.
GOLDEN_CASES = {
    "d8_b2_11x9_w05": dict(D=8, B=2, H=11, W=9, weight=0.5, holes=True, seed=511),
    "d8_9x10_w2": dict(D=8, B=1, H=9, W=10, weight=2.0, holes=True, seed=112),
    "d32_7x9_w2": dict(D=32, B=1, H=7, W=9, weight=2.0, holes=True, seed=13),
    "d48_6x9_full": dict(D=48, B=1, H=6, W=9, weight=1.0, holes=False, seed=14),
    "d64_5x6_w05": dict(D=64, B=1, H=5, W=6, weight=0.5, holes=True, seed=15),
}
REFINE_ALPHA = 5.0
# the six stage-passes of config 2 (main D, refine D, h, w)
CONFIG2_STAGES = ((64, 4, 296, 400), (32, 4, 592, 800), (8, 4, 1184, 1600))


# ------------------------------------------------------------------------------------------------ forward
def _yx(H, W, device):
    yy, xx = torch.meshgrid(torch.arange(H, device=device), torch.arange(W, device=device), indexing="ij")
    return yy, xx


def softmax_expect(logits, hyp, alpha):
    """logits [B,4,D,H,W], hyp [B,D,H,W] -> (p [B,4,D,H,W], E [B,4,H,W])."""
    p = torch.softmax(logits * alpha, dim=2)
    return p, (p * hyp.unsqueeze(1)).sum(2)


def select(dsp, mode):
    """dsp [B,4,H,W] -> mode 0: depth_values_c [B,4,H,W] (mvsnet.py:22-56); mode 1: depth [B,H,W] (mvsnet.py:71-91)."""
    H, W = dsp.shape[-2:]
    yy, xx = _yx(H, W, dsp.device)
    sm, sM = torch.minimum(dsp[:, 0], dsp[:, 1]), torch.maximum(dsp[:, 0], dsp[:, 1])
    hm, hM = torch.minimum(dsp[:, 2], dsp[:, 3]), torch.maximum(dsp[:, 2], dsp[:, 3])
    if mode == 1:
        r0, c0 = (yy % 2 == 0), (xx % 2 == 0)
        return torch.where(r0, torch.where(c0, sm, sM), torch.where(c0, hM, hm))
    q = yy % 4
    lo, hi = torch.where(q % 2 == 1, hm, sm), torch.where(q % 2 == 1, hM, sM)
    lo, hi = torch.where(q >= 2, 2 * lo - hi, lo), torch.where(q >= 2, 2 * hi - lo, hi)
    stack = [(3 - t) * lo + (t - 2) * hi for t in range(6)]
    shifted = (yy + xx) % 2 == 1
    return torch.stack([torch.where(shifted, stack[k + 2], stack[k]) for k in range(4)], 1)


def regress_forward(logits, hyp, alpha, mode):
    """-> (depth_sub_plus [B,4,H,W], selection)."""
    _, dsp = softmax_expect(logits, hyp, alpha)
    return dsp, select(dsp, mode)


def sl1(d):
    a = d.abs()
    return torch.where(a < 1, 0.5 * a * a, a - 0.5)


def _centre(a):
    return (((a[:, :-1, :-1] + a[:, :-1, 1:]) + a[:, 1:, :-1]) + a[:, 1:, 1:]) * 0.25


def _valid_cells(mask):
    valid = mask > 0.5
    return valid, valid[:, :-1, :-1] & valid[:, :-1, 1:] & valid[:, 1:, :-1] & valid[:, 1:, 1:]


def loss_set(dsp, gt, mask, weight):
    """What one set of outputs (depth_sub_plus or depth_sub_plus_refine, [B,4,h,w]) adds to the total: 2 (mean_small + mean_huge) +
    var_small + var_huge + the four cell-centre means.  Selection by index: nothing under the mask is touched."""
    valid, cells = _valid_cells(mask)
    B, h, w = gt.shape
    yy, xx = _yx(h, w, gt.device)
    cm = (yy % 2 == xx % 2)[None].expand(B, h, w)
    gbar = _centre(gt)
    total = 0
    for q in range(2):
        d0, d1 = dsp[:, 2 * q], dsp[:, 2 * q + 1]
        total = total + 2 * torch.cat(((sl1(d0 - gt) * weight)[valid], (sl1(d1 - gt) * weight)[valid])).mean()
        a0, a1 = (d0 - gt).abs(), (d1 - gt).abs()
        var_gt = torch.where(a0 < a1, a1, a0)
        total = total + (sl1((d0 - d1).abs() - var_gt) * weight)[valid].mean()
        mn, mx = torch.minimum(d0, d1), torch.maximum(d0, d1)
        for surf in (torch.where(cm, mn, mx), torch.where(~cm, mn, mx)):
            total = total + (sl1(_centre(surf) - gbar) * weight)[cells].mean()
    return total


def head_loss(logits, hyp, rlogits, gt, mask, weight, detach_hypotheses=False):
    """One stage: main pass -> refine pass on depth_values_c -> both loss sets.  -> (loss, outputs dict)."""
    dsp, c = regress_forward(logits, hyp, 1.0, 0)
    dsp_r, depth = regress_forward(rlogits, c.detach() if detach_hypotheses else c, REFINE_ALPHA, 1)
    loss = loss_set(dsp, gt, mask, weight) + loss_set(dsp_r, gt, mask, weight)
    return loss, {"depth_sub_plus": dsp, "depth_values_c": c, "depth_sub_plus_refine": dsp_r, "depth": depth}


# ------------------------------------------------------------------------------------------------ closed-form backward
def fold(route_dsp, g_dsp, g_sel, mode):
    """Upstream gradient G [B,4,H,W] on the four expectations: g_dsp plus what g_sel sends through the checkerboard cases and
    (min, max) of the pair; min / max route to the channel that holds the smaller / larger value of ``route_dsp``."""
    B, _, H, W = route_dsp.shape
    G = torch.zeros_like(route_dsp) if g_dsp is None else g_dsp.clone()
    if g_sel is None:
        return G
    yy, xx = _yx(H, W, route_dsp.device)
    zero = torch.zeros((), dtype=route_dsp.dtype, device=route_dsp.device)
    if mode == 1:
        pair = yy % 2
        is_min = (yy % 2) == (xx % 2)
        glo, ghi = torch.where(is_min, g_sel, zero), torch.where(is_min, zero, g_sel)
    else:
        q = yy % 4
        pair = q % 2
        off = ((yy + xx) % 2) * 2
        glo = sum(g_sel[:, k] * (3 - (k + off)) for k in range(4))
        ghi = sum(g_sel[:, k] * ((k + off) - 2) for k in range(4))
        glo, ghi = torch.where(q >= 2, 2 * glo - ghi, glo), torch.where(q >= 2, 2 * ghi - glo, ghi)
    for p in range(2):
        e0, e1 = route_dsp[:, 2 * p], route_dsp[:, 2 * p + 1]
        here = (pair == p)[None]
        min1, max1 = e1 < e0, e1 > e0
        G[:, 2 * p] += torch.where(here, torch.where(min1, zero, glo) + torch.where(max1, zero, ghi), zero)
        G[:, 2 * p + 1] += torch.where(here, torch.where(min1, glo, zero) + torch.where(max1, ghi, zero), zero)
    return G


def regress_backward(logits, hyp, alpha, mode, g_dsp, g_sel, route_dsp=None, expect=None):
    """-> (g_logits, g_hyp).  ``route_dsp``: the expectations that decide the min / max routing (default: this function's own).
    ``expect``: the expectations E of the factor (hyp - E) (default: this function's own) -- with the forward's fp32
    depth_sub_plus here the result is what the backward kernel is handed to compute, in exact arithmetic."""
    p, E = softmax_expect(logits, hyp, alpha)
    G = fold(E if route_dsp is None else route_dsp, g_dsp, g_sel, mode)
    if expect is not None:
        E = expect
    g_logits = alpha * p * (hyp.unsqueeze(1) - E.unsqueeze(2)) * G.unsqueeze(2)
    return g_logits, (p * G.unsqueeze(2)).sum(1)


def dsl1(u):
    return torch.where(u.abs() < 1, u, torch.sign(u))


def loss_set_backward(dsp, gt, mask, weight, g_total=1.0):
    """d loss_set / d dsp as a gather: own terms plus a quarter of each of the up to four cells a pixel is a corner of."""
    valid, cells = _valid_cells(mask)
    n, nc = int(valid.sum()), int(cells.sum())
    out = torch.zeros_like(dsp)
    if n == 0:
        return out
    B, h, w = gt.shape
    yy, xx = _yx(h, w, gt.device)
    cm = (yy % 2 == xx % 2)[None].expand(B, h, w)
    gbar = _centre(gt)
    zero = torch.zeros((), dtype=dsp.dtype, device=dsp.device)
    k = g_total * weight / n
    for q in range(2):
        d0, d1 = dsp[:, 2 * q], dsp[:, 2 * q + 1]
        o0, o1 = k * dsl1(d0 - gt), k * dsl1(d1 - gt)          # 2 * mean over 2n
        a0, a1 = (d0 - gt).abs(), (d1 - gt).abs()
        far1 = a0 < a1
        du = k * dsl1((d0 - d1).abs() - torch.where(far1, a1, a0))
        sd = torch.sign(d0 - d1)
        o0 = o0 + du * (sd - torch.where(far1, zero, torch.sign(d0 - gt)))
        o1 = o1 + du * (-sd - torch.where(far1, torch.sign(d1 - gt), zero))
        if nc > 0:
            mn, mx = torch.minimum(d0, d1), torch.maximum(d0, d1)
            D = []
            for surf in (torch.where(cm, mn, mx), torch.where(~cm, mn, mx)):
                dc = torch.where(cells, dsl1(_centre(surf) - gbar), zero) * (g_total * weight * 0.25 / nc)
                full = torch.zeros_like(d0)
                full[:, :-1, :-1] += dc
                full[:, :-1, 1:] += dc
                full[:, 1:, :-1] += dc
                full[:, 1:, 1:] += dc
                D.append(full)
            gmin, gmax = torch.where(cm, D[0], D[1]), torch.where(cm, D[1], D[0])
            # the channel the forward's min / max returned: channel 0 only where strictly smaller / larger, so an exact tie
            # (it happens: two fp32 expectations of one pixel in ~1e5) sends both quarters to channel 1, as csrc/validate.h does
            min0, max0 = d0 < d1, d0 > d1
            o0 = o0 + torch.where(min0, gmin, zero) + torch.where(max0, gmax, zero)
            o1 = o1 + torch.where(min0, zero, gmin) + torch.where(max0, zero, gmax)
        out[:, 2 * q] = torch.where(valid, o0, zero)
        out[:, 2 * q + 1] = torch.where(valid, o1, zero)
    return out


def chain_f64(case, edge=True):
    """The whole stage in float64 with the closed-form backward.  -> dict: loss, the four outputs, g_logits, g_rlogits, g_c (the
    refine pass's gradient on depth_values_c), g_dsp, g_dsp_refine.  ``edge`` False: the hypotheses edge is dropped."""
    L, hyp, Lr, gt, mask = (case[k].double() for k in ("logits", "hyp", "rlogits", "gt", "mask"))
    w = float(case["weight"])
    with torch.no_grad():
        loss, out = head_loss(L, hyp, Lr, gt, mask, w)
        g_dsp = loss_set_backward(out["depth_sub_plus"], gt, mask, w)
        g_dsp_r = loss_set_backward(out["depth_sub_plus_refine"], gt, mask, w)
        g_Lr, g_c = regress_backward(Lr, out["depth_values_c"], REFINE_ALPHA, 1, g_dsp_r, None)
        g_L, _ = regress_backward(L, hyp, 1.0, 0, g_dsp, g_c if edge else None)
    return dict(out, loss=loss, g_logits=g_L, g_rlogits=g_Lr, g_c=g_c, g_dsp=g_dsp, g_dsp_refine=g_dsp_r)


# ------------------------------------------------------------------------------------------------ conditions
def reference_cells(valid):
    """(all-valid cells, cells the reference's ``grid_sample(mask) >= 1`` keeps) for valid [B,h,w] bool: the grid of
    Monte_Carlo_sampling_loss in mode "center" (loss.py:111-130), restated."""
    B, h, w = valid.shape
    y, x = torch.meshgrid([torch.arange(0, h - 1, dtype=torch.float32), torch.arange(0, w - 1, dtype=torch.float32)], indexing="ij")
    y, x = y.unsqueeze(0) + 0.5, x.unsqueeze(0) + 0.5
    grid = torch.stack(((x / ((w - 1) / 2) - 1).repeat(B, 1, 1), (y / ((h - 1) / 2) - 1).repeat(B, 1, 1)), dim=3)
    m = F.grid_sample(valid.float().unsqueeze(1), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    return int(_valid_cells(valid.float())[1].sum()), int((m >= 1.0).sum())


def condition_violations(case, margin=MARGIN):
    """List of violated conditions (empty: the case is admissible).  (a) the two depths of each pair differ by more than the margin,
    in both passes, at every pixel; (b) at valid pixels no |est - gt| and no ||a - b| - var_gt| lies within the margin of 1 or of
    0, and the two |. - gt| of a pair do not tie; (c) the reference's cell mask drops no all-valid cell."""
    out = chain_f64(case)
    gt, valid = case["gt"].double(), case["mask"] > 0.5
    bad = []
    for name in ("depth_sub_plus", "depth_sub_plus_refine"):
        dsp = out[name]
        for q in range(2):
            d0, d1 = dsp[:, 2 * q], dsp[:, 2 * q + 1]
            if not ((d0 - d1).abs() > margin).all():
                bad.append(f"(a) {name} pair {q}: min gap {(d0 - d1).abs().min().item():.2e}")
            a0, a1 = (d0 - gt).abs()[valid], (d1 - gt).abs()[valid]
            u = ((d0 - d1).abs()[valid] - torch.maximum(a0, a1)).abs()
            for what, v in (("|est-gt|", torch.cat((a0, a1))), ("||a-b|-var_gt|", u)):
                gap = min(v.min().item(), (v - 1).abs().min().item()) if v.numel() else 1.0
                if not gap > margin:
                    bad.append(f"(b) {name} pair {q} {what}: {gap:.2e} from 0 / the knee")
            if a0.numel() and not ((a0 - a1).abs() > margin).all():
                bad.append(f"(b) {name} pair {q}: |.-gt| tie {(a0 - a1).abs().min().item():.2e}")
    cells, kept = reference_cells(valid)
    if cells != kept or cells == 0:
        bad.append(f"(c) all-valid cells {cells}, the reference keeps {kept}")
    return bad


# ------------------------------------------------------------------------------------------------ seeded inputs
def _rng(seed, tag):
    return np.random.Generator(np.random.PCG64([int(seed), zlib.crc32(tag.encode())]))


def make_case(D, H, W, B=1, weight=1.0, holes=True, seed=0, refine_D=4):
    """synth-style inputs of one stage (PCG64 streams, plain fp32 NumPy arithmetic): a smooth ground-truth surface around 600 mm,
    hypothesis planes spanning ~16 mm around it with a per-pixel offset, peaky logits (expectations spread over the span: both
    branches of the smooth-L1 carry weight), a mask with holes and values 0, 0.5, 0.75, 1.  torch CPU fp32 tensors."""
    g = _rng(seed, f"head.{D}.{H}.{W}.{B}")
    yy = np.arange(H, dtype=np.float32)[None, :, None]
    xx = np.arange(W, dtype=np.float32)[None, None, :]
    ph = g.random((B, 1, 1), dtype=np.float32)
    gt = (np.float32(600.0) + np.float32(40.0) * np.sin(np.float32(0.37) * yy + ph) + np.float32(30.0) * np.cos(np.float32(0.23) * xx - ph)
          + np.float32(0.5) * g.standard_normal((B, H, W), dtype=np.float32)).astype(np.float32)
    off = (np.float32(8.0) * (g.random((B, H, W), dtype=np.float32) - np.float32(0.5))).astype(np.float32)
    step = np.float32(16.0 / max(D - 1, 1))
    d = np.arange(D, dtype=np.float32)[None, :, None, None] - np.float32((D - 1) / 2)
    hyp = (gt[:, None] + off[:, None] + d * step).astype(np.float32)
    logits = (np.float32(3.0) * g.standard_normal((B, 4, D, H, W), dtype=np.float32)).astype(np.float32)
    rlogits = g.standard_normal((B, 4, refine_D, H, W), dtype=np.float32)
    if holes:
        r = g.random((B, H, W), dtype=np.float32)
        mask = np.where(r < 0.08, 0.0, np.where(r < 0.14, 0.5, np.where(r < 0.25, 0.75, 1.0))).astype(np.float32)
    else:
        mask = np.ones((B, H, W), dtype=np.float32)
    t = torch.from_numpy
    return {"logits": t(logits), "hyp": t(hyp), "rlogits": t(rlogits), "gt": t(gt), "mask": t(mask), "weight": float(weight),
            "interval": float(step)}


def golden_case(g, name):
    """A case dict from the arrays of tests/golden/op_head_grad.npz."""
    case = {k: torch.from_numpy(g[f"{name}.{k}"]) for k in ("logits", "hyp", "rlogits", "gt", "mask")}
    case["weight"], case["interval"] = float(g[f"{name}.weight"]), float(g[f"{name}.interval"])
    return case


def rel_dist(a, b64):
    """max-abs distance of ``a`` to the float64 tensor ``b64``, normalised by b64's max-abs."""
    b64 = b64.detach().double().cpu()
    return (a.detach().double().cpu() - b64).abs().max().item() / b64.abs().max().item()
