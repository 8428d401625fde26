"""Yardstick of K1's forward (``warp_corr_q4_kernel`` / ``warp_corr_kernel`` of csrc/warp_corr.hip): a restatement of the fused warp +
two-group correlation + view sum in PIXEL coordinates, parametrised by ``dtype`` -- float64 is the yardstick, the same text in float32
on stock ATen (CPU) gives the e_ref of the project's criterion -- the criterion itself, the q4 kernel's window rule restated on the
host, and the fixed case tables of tests/test_warp_corr_{cpu,gpu}.py.  No product code runs here, no ``grid_sample`` and no
normalise / un-normalise round trip, so the restatement is defined on one-row and one-column maps.

  p = rot (x, y, 1) d + trans;  z == 0 -> z + 1e-5;  ix = px / pz, iy = py / pz;  x0 = floor(ix), tx = ix - x0 (same in y);
  four taps (x0 | x0 + 1, y0 | y0 + 1) with weights (1 - tx | tx) (1 - ty | ty), a tap outside the image counts zero on its own;
  sim[g, d] = sum over views of the mean over k of ref[2k + g] * warped[2k + g].

Layouts: features V x [C,H,W]; p12 [V-1,12] (rot 9 + trans 3, the kernel's own input); depth [D,H,W]; result [2,D,H,W].

Criterion (``errors`` / ``bounds``): e_max = max|a - f64| / max|f64| and e_mean = mean|a - f64| / max|f64|, each under the project's
rule e_hip <= 8 e_ref, 16 * 2^-23 where e_ref < 4 * 2^-23 (``hypotheses_ref.bound_of``).  Where the yardstick is identically zero
the output has to be zero bit for bit.  The generic kernel, which keeps the reference's normalise / un-normalise round trip, gets
``op_order_allowance`` added to its MAX bound on the WINDOWS table alone (where e_ref sits on the criterion's floor and that round
trip shows): the displacement those roundings can cause, times the yardstick's slope.  Its mean bound, and its max bound on every
other table, are the plain ones."""
import math
import zlib

import numpy as np
import torch

import costagg_grad_ref as G
from hypotheses_ref import bound_of   # noqa: F401  (the criterion; re-exported for the two test files)
from dmvsnet_amd import synth

F64, F32, F16 = torch.float64, torch.float32, torch.float16
TW, TH = 32, 8                      # the q4 kernel's tile
BOX_EPS = 1.0 / 64.0                # its slack on the corner bounds
WINQ = {1: 2552, 2: 3408, 3: 5112, 4: 10232}   # window capacity in 16-byte quads per window selector (q4_winq of 4 / 3 / 2 / 1 per CU)
MUTATIONS = ("shift_1_256", "align_corners_false", "border_clamp", "groups_swapped", "last_view_dropped", "next_plane", "divisor_c",
             "window_from_dmax")


# ------------------------------------------------------------------------------------------------ the restatement
def coordinates(p12_v, depth):
    """Source-pixel coordinates (ix, iy) [D,H,W] of one view in ``depth``'s dtype."""
    dt = depth.dtype
    _, H, W = depth.shape
    P = p12_v.to(dt)
    x, y = torch.arange(W, dtype=dt).view(1, 1, W), torch.arange(H, dtype=dt).view(1, H, 1)
    rx, ry, rz = (P[3 * r] * x + P[3 * r + 1] * y + P[3 * r + 2] for r in range(3))
    px, py, pz = rx * depth + P[9], ry * depth + P[10], rz * depth + P[11]
    pz = torch.where(pz == 0, pz + 1e-5, pz)
    return px / pz, py / pz


def tile_window_from_dmax(p12_v, depth):
    """The mutation ``window_from_dmax``: per 32 x 8 tile the window the q4 kernel would stage if its corner bound took the tile's
    LARGEST hypothesis only -> inclusive (x0, x1, y0, y1) per pixel, each [1,H,W]."""
    dt = depth.dtype
    _, H, W = depth.shape
    out = [torch.empty((1, H, W), dtype=dt) for _ in range(4)]
    for ty in range(0, H, TH):
        for tx in range(0, W, TW):
            ys, xs = slice(ty, min(ty + TH, H)), slice(tx, min(tx + TW, W))
            dmax = depth[:, ys, xs].max()
            cx, cy = torch.tensor([float(xs.start), float(xs.stop - 1)], dtype=dt), torch.tensor([float(ys.start), float(ys.stop - 1)], dtype=dt)
            P = p12_v.to(dt)
            pts = [(P[0] * a + P[1] * b + P[2], P[3] * a + P[4] * b + P[5], P[6] * a + P[7] * b + P[8]) for a in cx for b in cy]
            ix = torch.stack([(r[0] * dmax + P[9]) / (r[2] * dmax + P[11]) for r in pts]).clamp(-1, W)
            iy = torch.stack([(r[1] * dmax + P[10]) / (r[2] * dmax + P[11]) for r in pts]).clamp(-1, H)
            box = (torch.floor(ix.min() - BOX_EPS), torch.floor(ix.max() + BOX_EPS) + 1,
                   torch.floor(iy.min() - BOX_EPS), torch.floor(iy.max() + BOX_EPS) + 1)
            for o, b in zip(out, box):
                o[:, ys, xs] = b
    return out


def warp_corr_ref(feats, p12, depth, dtype=F64, mutation=None):
    """feats: V tensors [C,H,W]; p12 [V-1,12]; depth [D,H,W] -> [2,D,H,W] in ``dtype``.  ``mutation``: one of MUTATIONS (the CPU
    file's sensitivity test), None for the operation itself."""
    assert mutation is None or mutation in MUTATIONS, mutation
    feats = [f.detach().to("cpu", dtype) for f in feats]
    p12, depth = p12.detach().to("cpu", dtype), depth.detach().to("cpu", dtype)
    ref = feats[0]
    C, H, W = ref.shape
    D = depth.shape[0]
    assert p12.shape == (len(feats) - 1, 12) and depth.shape == (D, H, W)
    if mutation == "next_plane":
        depth = depth[[min(d + 1, D - 1) for d in range(D)]]
    total = torch.zeros((2, D, H, W), dtype=dtype)
    nsrc = len(feats) - 1 - (1 if mutation == "last_view_dropped" else 0)
    for v in range(nsrc):
        ix, iy = coordinates(p12[v], depth)
        if mutation == "shift_1_256":
            ix, iy = ix + 1.0 / 256, iy + 1.0 / 256
        if mutation == "align_corners_false":   # ((g + 1) * n - 1) / 2 for g = i / ((n - 1) / 2) - 1
            ix, iy = ix * W / (W - 1) - 0.5, iy * H / (H - 1) - 0.5
        x0, y0 = torch.floor(ix), torch.floor(iy)
        tx, ty = ix - x0, iy - y0
        win = tile_window_from_dmax(p12[v], depth) if mutation == "window_from_dmax" else None
        src = feats[v + 1].reshape(C, H * W)
        warped = torch.zeros((C, D, H, W), dtype=dtype)
        for dy, wy in ((0, 1 - ty), (1, ty)):
            for dx, wx in ((0, 1 - tx), (1, tx)):
                xi, yi = x0 + dx, y0 + dy
                inside = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)   # false for a NaN coordinate
                if win is not None:
                    inside = inside & (xi >= win[0]) & (xi <= win[1]) & (yi >= win[2]) & (yi <= win[3])
                if mutation == "border_clamp":
                    inside = torch.isfinite(xi) & torch.isfinite(yi)
                w = torch.where(inside, wx * wy, torch.zeros((), dtype=dtype))
                idx = (torch.nan_to_num(yi).clamp(0, H - 1) * W + torch.nan_to_num(xi).clamp(0, W - 1)).long()
                warped = warped + w * src[:, idx.reshape(-1)].view(C, D, H, W)
        prod = warped.view(C // 2, 2, D, H, W) * ref.view(C // 2, 2, 1, H, W)
        total = total + (prod.sum(0) / C if mutation == "divisor_c" else prod.mean(0))
    return total.flip(0) if mutation == "groups_swapped" else total


# ------------------------------------------------------------------------------------------------ the criterion
def errors(a, f64):
    """(e_max, e_mean) of ``a`` against the yardstick, in float64; (0, 0) where both are identically zero, inf where only the
    yardstick is."""
    a, f64 = a.detach().to("cpu", F64), f64.detach().to("cpu", F64)
    assert a.shape == f64.shape, (a.shape, f64.shape)
    scale = f64.abs().max().item()
    diff = (a - f64).abs()
    if scale == 0.0:
        z = 0.0 if diff.max().item() == 0.0 else math.inf
        return z, z
    return diff.max().item() / scale, diff.mean().item() / scale


def bounds(e_ref, allowance=0.0):
    """(bound on e_max, bound on e_mean) from the fp32 restatement's (e_max, e_mean); ``allowance`` (see the function of that name)
    goes to the max bound only."""
    return bound_of(e_ref[0]) + allowance, bound_of(e_ref[1])


def op_order_allowance(feats, p12, depth):
    """What the REFERENCE'S OP ORDER may add to (e_max, e_mean): the generic kernel (like homo_warping + grid_sample) does not sample
    at ix = px / pz but normalises and un-normalises it first.  With u = 2^-24 and hw = (W - 1) / 2, each step rounds once:

        q = fl(ix / hw)  |dq| <= u |q|      g = fl(q - 1)  |dg| <= u |g|      s = fl(g + 1)  |ds| <= u |s|      s / 2 is exact
        ix' = fl((s / 2) (W - 1))           |d| <= u |ix'|

    so |ix' - ix| <= hw (u |q| + u |q - 1| + u |q|) + u |ix| = u (3 |ix| + |ix - hw|) =: dx (at most 3.5 u (W - 1) inside the image),
    and the same in y.  The sample is a continuous, piecewise bilinear function of (ix, iy) (zero padding included), so it moves by at
    most dx Gx + dy Gy, where Gx is the largest |d sim / d ix| over the cells the box [ix +- dx] x [iy +- dy] touches: inside a cell
    d sim / d ix = (1 - ty) A(y0) + ty A(y0 + 1) with A(r) = <ref, src[r, x0 + 1] - src[r, x0]> per group, hence |.| <= max |A(r)| over
    the rows touched.  Summed over the views, in float64 from the yardstick's own numbers (terms of order dx^2 ~ 1e-10 are dropped).
    -> the max over the elements, relative to max|f64|; 0 on a map where the yardstick is zero.  Nothing here comes from a kernel's
    output.  Where it is used: ``allowance``."""
    u = 2.0 ** -24
    feats = [f.detach().to("cpu", F64) for f in feats]
    p12, depth = p12.detach().to("cpu", F64), depth.detach().to("cpu", F64)
    ref = feats[0]
    C, H, W = ref.shape
    D = depth.shape[0]
    refg = ref.view(C // 2, 2, 1, H, W)

    def corr(src, xi, yi):   # <ref, src[yi, xi]> per group with zero padding -> [2,D,H,W]
        inside = (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)
        idx = (yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)).long().reshape(-1)
        tap = src[:, idx].view(C // 2, 2, D, H, W)
        return (tap * refg).mean(0) * inside

    total = torch.zeros((2, D, H, W), dtype=F64)
    for v in range(p12.shape[0]):
        ix, iy = coordinates(p12[v], depth)
        ix, iy = torch.nan_to_num(ix).clamp(-3, W + 2), torch.nan_to_num(iy).clamp(-3, H + 2)   # beyond: every tap in reach is padding
        dx, dy = u * (3 * ix.abs() + (ix - (W - 1) / 2).abs()), u * (3 * iy.abs() + (iy - (H - 1) / 2).abs())
        src = feats[v + 1].reshape(C, H * W)
        xs = sorted_pair(torch.floor(ix - dx), torch.floor(ix + dx))
        ys = sorted_pair(torch.floor(iy - dy), torch.floor(iy + dy))
        gx = torch.zeros((2, D, H, W), dtype=F64)
        gy = torch.zeros((2, D, H, W), dtype=F64)
        for x0 in xs:
            for y0 in ys:
                t = [[corr(src, x0 + a, y0 + b) for a in (0, 1)] for b in (0, 1)]   # t[row][col]
                gx = torch.maximum(gx, torch.maximum((t[0][1] - t[0][0]).abs(), (t[1][1] - t[1][0]).abs()))
                gy = torch.maximum(gy, torch.maximum((t[1][0] - t[0][0]).abs(), (t[1][1] - t[0][1]).abs()))
        total = total + dx * gx + dy * gy
    scale = warp_corr_ref(feats, p12, depth, F64).abs().max().item()
    return 0.0 if scale == 0.0 else total.max().item() / scale


def sorted_pair(lo, hi):
    """(lo, hi), or (lo,) where the two are the same everywhere."""
    return (lo,) if torch.equal(lo, hi) else (lo, hi)


# ------------------------------------------------------------------------------------------------ the q4 window rule on the host
def q4_tile_windows(sx, ox, sy, oy, H, W):
    """[(tile x, tile y, pieces)]: the window (16-byte pieces per quad plane) the q4 kernel stages for every 32 x 8 tile under the
    projection ix = sx * x + ox, iy = sy * y + oy (depth-independent): the corner bound of warp_corr.hip restated on the host."""
    out = []
    f = np.float32
    for ty in range(0, H, TH):
        for tx in range(0, W, TW):
            xs = [f(sx) * f(x) + f(ox) for x in (tx, min(tx + TW - 1, W - 1))]
            ys = [f(sy) * f(y) + f(oy) for y in (ty, min(ty + TH - 1, H - 1))]
            cx = np.clip(xs, -1.0, W)
            cy = np.clip(ys, -1.0, H)
            x0, x1 = max(int(np.floor(cx.min() - BOX_EPS)), -1), min(int(np.floor(cx.max() + BOX_EPS)) + 1, W + 1)
            y0, y1 = max(int(np.floor(cy.min() - BOX_EPS)), -1), min(int(np.floor(cy.max() + BOX_EPS)) + 1, H + 1)
            out.append((tx, ty, (x1 - x0 + 1) * (y1 - y0 + 1)))
    return out


def _q4_window_pieces(sx, ox, sy, oy, H, W):
    """The set of window sizes of ``q4_tile_windows``."""
    return {n for _, _, n in q4_tile_windows(sx, ox, sy, oy, H, W)}


def q4_modes_of(C):
    """The slab modes a channel count has: 0 .. log2(C / 4)."""
    return tuple(range({8: 2, 16: 3, 32: 4}[C]))


def q4_mode(npix, C, winq):
    """Slab mode 0 .. 3 the fp32 q4 kernel picks for a window of ``npix`` pieces, or "global" (the exact global-tap path): mode m
    stages 2^m slabs of NQ >> m quad planes at a plane pitch of (WINQ / (NQ >> m)) & ~3 pieces, the first mode whose pitch holds the
    window wins, the last one has a single plane per slab (pitch WINQ); beyond WINQ nothing fits."""
    nq = C // 4
    if npix > winq:
        return "global"
    last = q4_modes_of(C)[-1]
    for m in range(last):
        if npix <= (winq // (nq >> m)) & ~3:
            return m
    return last


# ------------------------------------------------------------------------------------------------ inputs
def seed_of(name):
    return zlib.crc32(name.encode())


def features(name, V, C, H, W):
    """V x [C,H,W] fp32, i.i.d. standard normal (never smoothed: a wrong tap weight must show).  Draws below 2^-13 in magnitude are
    drawn again, so that no value becomes an fp16 subnormal when an fp16 case rounds it (how v_dot2_f32_f16 treats subnormals is
    not what these tests are about); that is 1e-4 of the draws."""
    g = torch.Generator().manual_seed(seed_of(name))
    x = torch.randn((V, C, H, W), generator=g, dtype=F32)
    while True:
        small = x.abs() < 2.0 ** -13
        if not small.any():
            return list(x)
        x[small] = torch.randn((int(small.sum()),), generator=g, dtype=F32)


def as_fp16(feats):
    """The fp16 twin's inputs: the values rounded to fp16 (cast back up for the yardstick and e_ref)."""
    return [f.to(F16) for f in feats]


def synth_depth(name, D, H, W, sigma=5.0):
    """500 + (240 / D) d + N(0, sigma), as costagg_grad_ref.make_case."""
    g = torch.Generator().manual_seed(seed_of(name) ^ 0x5EED)
    return 500.0 + (240.0 / D) * torch.arange(D, dtype=F32).view(D, 1, 1) + sigma * torch.randn((D, H, W), generator=g, dtype=F32)


def p12_of_cams(cams, dtype=F64):
    """cams [V,2,4,4] -> [V-1,12]: rot 9 + trans 3 of (K E)_src @ inverse((K E)_ref), composed in float64."""
    cams = cams.to(F64)

    def compose(pair):
        P = pair[0].clone()
        P[:3, :4] = pair[1, :3, :3] @ pair[0, :3, :4]
        return P
    inv = torch.inverse(compose(cams[0]))
    rows = []
    for v in range(1, cams.shape[0]):
        P = compose(cams[v]) @ inv
        rows.append(torch.cat((P[:3, :3].reshape(-1), P[:3, 3])))
    return torch.stack(rows).to(dtype)


def affine_p12(sx, ox, sy, oy):
    """Depth-independent projection ix = sx x + ox, iy = sy y + oy."""
    return torch.tensor([[sx, 0, ox, 0, sy, oy, 0, 0, 1, 0, 0, 0]], dtype=F32)


def _case(table, name, C, feats, depth, cams=None, p12=None, nonzero_e_ref=True):
    """One case: ``cams`` [V,2,4,4] (the GPU file derives p12 with ops.relative_proj, the CPU file in float64) or a literal ``p12``."""
    return dict(table=table, name=name, C=C, feats=feats, depth=depth, cams=cams, p12=p12, nonzero_e_ref=nonzero_e_ref)


def _synth_case(table, name, C, V, D, H, W, cams=None):
    cams = synth.synth_cameras(4 * H, 4 * W, V)["stage1"][0] if cams is None else cams
    return _case(table, name, C, features(name, V, C, H, W), synth_depth(name, D, H, W), cams=cams)


# ------------------------------------------------------------------------------------------------ the case tables
# (C, V, D, H, W): below one tile; exactly one tile; ragged by one in both directions; C = 32 below a tile; three tiles in x and y;
# two tiles, D = DC; DC = 8 with one plane in the last chunk; DC = 4 with one plane in the last chunk; C = 32 over four chunks; D = 48
SHAPES = ((8, 2, 1, 2, 2), (8, 3, 2, 8, 32), (16, 3, 3, 9, 33), (32, 2, 4, 7, 31), (8, 3, 5, 17, 70), (8, 3, 8, 8, 64), (8, 3, 9, 10, 40),
          (16, 3, 5, 12, 36), (32, 3, 13, 9, 65), (16, 2, 48, 16, 40))
# (C, nsrc) at (H, W) = (16, 64), D = 4: 7 is where C = 8 switches to 80 KB windows, 8 / 9 the corner-table boundary, 16 the maximum
VIEWS = ((8, 1), (8, 6), (8, 7), (8, 8), (8, 9), (8, 16), (32, 8), (32, 9), (32, 16))
EDGE_SHAPES = ((8, 3, 3, 1, 1), (16, 3, 2, 1, 65), (8, 3, 4, 33, 1))   # one pixel, one row, one column
AFFINE_OFFSETS = ((0, 0), (-0.5, 0.5), (-1, -1), (-1.5, 0), (0.5, -0.5), (33, 0), (0, 9), (1e9, -1e9), (0.25, 8.75))
AFFINE_SHAPE = (3, 9, 33)   # (D, H, W)
# (sx, ox, sy, oy, H, W): tile (0, 0) of each map owns a window of the size its comment names; test_warp_corr_cpu.py asserts which
# slab mode that is per (C, window selector).  The thresholds between modes are 316 / 636 / 1276 / 2552 pieces at selector 1,
# 424 / 852 / 1704 / 3408 at 2, 636 / 1276 / 2556 / 5112 at 3 and 1276 / 2556 / 5116 / 10232 at 4.
WINDOWS = (
    (1.0, 0.25, 0.5, 0.25, 9, 36),      # 33 x 5 = 165 pieces
    (1.5, 0.25, 0.75, 0.25, 12, 52),    # 336
    (1.5, 0.25, 1.25, 0.25, 14, 52),    # 528
    (2.0, 0.25, 1.5, 0.25, 16, 68),     # 768
    (2.0, 0.25, 2.0, 0.25, 20, 68),     # 1024
    (2.75, 0.25, 2.0, 0.25, 20, 92),    # 1392
    (2.75, 0.25, 3.0, 0.25, 26, 92),    # 2001
    (3.5, 0.25, 3.5, 0.25, 30, 116),    # 2860
    (3.5, 0.25, 4.5, 0.25, 40, 128),    # 3630
    (4.25, 0.25, 5.5, 0.25, 44, 140),   # 5360
    (4.75, 0.25, 8.5, 0.25, 72, 160),   # 9089
)
WINDOWS_D = 2
SCATTER_SHAPE = (8, 32, 128)   # (D, H, W): 4 x 4 tiles
SCATTER_V = 3
SPECIAL_SHAPE = (3, 12, 40)    # (D, H, W) of the two literal projections: tiles 0 (holds x = 0) and 1 (does not)


def shapes_cases():
    return {f"shape-c{C}-v{V}-d{D}-{H}x{W}": _synth_case("SHAPES", f"shape-c{C}-v{V}-d{D}-{H}x{W}", C, V, D, H, W)
            for C, V, D, H, W in SHAPES}


def views_cases():
    return {f"views-c{C}-n{n}": _synth_case("VIEWS", f"views-c{C}-n{n}", C, n + 1, 4, 16, 64) for C, n in VIEWS}


def edge_cases():
    return {f"edge-c{C}-v{V}-d{D}-{H}x{W}": _synth_case("EDGE_SHAPES", f"edge-c{C}-v{V}-d{D}-{H}x{W}", C, V, D, H, W)
            for C, V, D, H, W in EDGE_SHAPES}


def affine_cases():
    """Unit scale, the offsets of AFFINE_OFFSETS, hypotheses 256 / 512 / 1024 drawn per pixel and plane: x + ox is exact in fp32 (or
    beyond 2^24, far outside the image, where its rounding does not matter) and multiplying and dividing by a power of two is exact,
    so kernel, fp32 restatement and yardstick sample the very same positions -- integers, half pixels, exactly -1 / W / H."""
    D, H, W = AFFINE_SHAPE
    out = {}
    for C in (8, 32):
        for ox, oy in AFFINE_OFFSETS:
            name = f"affine-c{C}-{ox:g}_{oy:g}"
            g = torch.Generator().manual_seed(seed_of(name) ^ 0x5EED)
            depth = 2.0 ** (8 + torch.randint(0, 3, (D, H, W), generator=g)).to(F32)
            out[name] = _case("AFFINE", name, C, features(name, 2, C, H, W), depth, p12=affine_p12(1.0, ox, 1.0, oy), nonzero_e_ref=False)
    return out


def windows_cases():
    out = {}
    for k, (sx, ox, sy, oy, H, W) in enumerate(WINDOWS):
        for C in (8, 16, 32):
            name = f"window{k}-c{C}-{H}x{W}"
            depth = (500.0 + 10.0 * torch.arange(WINDOWS_D, dtype=F32)).view(-1, 1, 1).expand(WINDOWS_D, H, W).contiguous()
            out[name] = _case("WINDOWS", name, C, features(name, 2, C, H, W), depth, p12=affine_p12(sx, ox, sy, oy))
            out[name]["geometry"] = (sx, ox, sy, oy, H, W)
    return out


def outlier_position(k):
    """(plane, row, column) inside tile k = 0 .. 15 of the hypothesis outlier: the tile's first pixel, its last pixel, then a walk
    over all 8 rows (every wave of the workgroup owns two of them) and over the planes, in columns within 5 of the tile's left or
    right edge (a nearer hypothesis moves the sample by ~10 px along the baseline: from the middle of a tile it would land among
    the other samples)."""
    if k == 0:
        return 0, 0, 0
    if k == 1:
        return 1, TH - 1, TW - 1
    return k % 8, k % TH, (k % 5 if k % 2 == 0 else TW - 1 - k % 5)


def scatter_cameras():
    """Three of five synth cameras with the MIDDLE one as the reference: the two source views sit on opposite sides of it, so a
    nearer hypothesis moves the sample left in one view and right in the other (baseline 60 either way)."""
    H, W = SCATTER_SHAPE[1:]
    return synth.synth_cameras(4 * H, 4 * W, 5)["stage1"][0][[2, 0, 4]].clone()


def scatter_cases():
    """``outlier``: every hypothesis 740 +- 2 but one of 500 per tile (outlier_position); ``checker``: the refine passes'
    checkerboard of two interleaved depth levels, 450 / 850 (+ 3 d +- 2)."""
    D, H, W = SCATTER_SHAPE
    cams = scatter_cameras()
    out = {}
    for C in (8, 16):
        name = f"scatter-outlier-c{C}"
        g = torch.Generator().manual_seed(seed_of(name) ^ 0x5EED)
        depth = 738.0 + 4.0 * torch.rand((D, H, W), generator=g, dtype=F32)
        for k in range((H // TH) * (W // TW)):
            d, r, c = outlier_position(k)
            depth[d, (k // (W // TW)) * TH + r, (k % (W // TW)) * TW + c] = 500.0
        out[name] = _case("SCATTER", name, C, features(name, SCATTER_V, C, H, W), depth, cams=cams)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    for C, Dc in ((8, 8), (16, 8), (32, 4)):
        name = f"scatter-checker-c{C}"
        g = torch.Generator().manual_seed(seed_of(name) ^ 0x5EED)
        level = torch.where((xx + yy) % 2 == 0, 450.0, 850.0).to(F32)
        depth = level[None] + 3.0 * torch.arange(Dc, dtype=F32).view(Dc, 1, 1) - 2.0 + 4.0 * torch.rand((Dc, H, W), generator=g, dtype=F32)
        out[name] = _case("SCATTER", name, C, features(name, SCATTER_V, C, H, W), depth, cams=cams)
    return out


def special_cases():
    """zero-denominator: pz = x d is exactly 0 on the pixel column x = 0 in every precision (the + 1e-5 patch applies in kernel, fp32
    and float64 alike; the tiles holding x = 0 take the q4 kernel's global-tap path).  behind: pz = -d everywhere, ix = -x, iy = -y
    (global-tap path; only taps of row / column 0 are inside the image).  behind-mirrored: the same denominator with ix = W - 1 - x,
    iy = H - 1 - y, every sample inside.  turned: costagg_grad_ref.turned_cameras, a source camera INSIDE the sampled volume -- the
    denominator changes sign inside tiles."""
    D, H, W = SPECIAL_SHAPE
    out = {}
    lit = {"zero-denominator": [1, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0], "behind": [1, 0, 0, 0, 1, 0, 0, 0, -1, 0, 0, 0],
           "behind-mirrored": [1, 0, -(W - 1), 0, 1, -(H - 1), 0, 0, -1, 0, 0, 0]}
    for key, row in lit.items():
        for C in (8, 32):
            name = f"special-{key}-c{C}"
            out[name] = _case("SPECIAL", name, C, features(name, 2, C, H, W), synth_depth(name, D, H, W),
                              p12=torch.tensor([row], dtype=F32), nonzero_e_ref=False)
    C, V, D, H, W = 8, 4, 8, 12, 40
    out["special-turned"] = _synth_case("SPECIAL", "special-turned", C, V, D, H, W, cams=G.turned_cameras(H, W, V)[0])
    return out


def reference(case, p12):
    """(float64 yardstick, (e_max, e_mean) of the fp32 restatement) of a case under the fp32 ``p12`` handed to the kernel.  An fp16
    case passes its rounded features in ``case["feats"]``; both runs see them cast up."""
    feats = [f.float() for f in case["feats"]]
    f64 = warp_corr_ref(feats, p12, case["depth"], F64)
    return f64, errors(warp_corr_ref(feats, p12, case["depth"], F32), f64)


def allowance(case, p12):
    """What an implementation with the reference's op order (the generic kernel; the fp32 oracle) may add to its MAX bound:
    ``op_order_allowance`` on the WINDOWS table, nothing anywhere else.  WINDOWS is where the plain rule cannot hold for that op order:
    its projections sx x + ox are nearly exact in fp32, so e_ref sits below the criterion's floor (asserted in the CPU file, with the
    oracle's excess over the plain bound) while the round trip's displacement grows with W.  The mean bound is never widened."""
    return op_order_allowance([f.float() for f in case["feats"]], p12, case["depth"]) if case["table"] == "WINDOWS" else 0.0


def all_cases():
    out = {}
    for table in (shapes_cases, views_cases, edge_cases, affine_cases, windows_cases, scatter_cases, special_cases):
        out.update(table())
    return out


def outside_share(p12, depth):
    """Share of the (view, plane, pixel) samples with at least one bilinear tap outside the image (float64 coordinates)."""
    _, H, W = depth.shape
    out = n = 0
    for v in range(p12.shape[0]):
        ix, iy = coordinates(p12[v].to(F64), depth.to(F64))
        x0, y0 = torch.floor(ix), torch.floor(iy)
        inside = (x0 >= 0) & (x0 + 1 <= W - 1) & (y0 >= 0) & (y0 + 1 <= H - 1)
        out += (~inside).sum().item()
        n += inside.numel()
    return out / n
