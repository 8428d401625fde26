"""Test infrastructure: criterion, restated launch geometry, fp32 emulation and case tables of the four Winograd F(2x2, 3x3) kernels
that run conv0 / conv2 / conv4 / conv6 of the regularisation nets -- ``conv0_wino_kernel`` and ``conv_wino_kernel`` at kdepth 3 (K3w,
csrc/conv3d_wino.hip), ``coarse_kernel`` (K3r, csrc/conv3d_coarse.hip) and ``zmarch_kernel`` (K3z, csrc/conv3d_zmarch.hip).  No
product code here; tests/test_winoconv_cpu.py asserts what the tables claim from the geometry restated below, holds the emulation to
the criterion and shows which mistakes it catches; tests/test_winoconv_gpu.py holds the kernels to it.

Yardstick: regconv_ref.conv3d in float64 (stride 1; the plain convolution is not restated again), e_ref from fp32 ATen on the CPU
(regconv_ref.aten_conv3d), never from a HIP kernel.  Criterion (featurenet_ref's bound_of / errors): e_max = max|a - f64| / max|f64|
and e_mean = mean|a - f64| / max|f64|, each e_hip <= 8 e_ref, and 16 * 2^-23 where e_ref < 4 * 2^-23 -- the plain bound with no
allowance: ``wino_emulate`` in fp32, with its products accumulated in the most pessimistic order any of the four kernels could have,
stays inside it on every input the GPU file uses (the CPU file asserts that).

Geometry, restated from the sources:
  K3w   a workgroup owns TZ planes x TY rows x 32 columns (kWCfgs); tile list x, z, y for kdepth 3 and x, y, z otherwise; XCD b % 8
        walks the (b % 8)-th contiguous eighth of the list in steps of grid / 8 (XcdTileWalk); grid = min(xcd_grid(tiles), resident),
        resident = 256 * clamp(160 KB / LDS bytes, 1, 2) (launch_wino), `wino_conv0_grid` for conv0.  conv2 on D <= 4 takes the
        ZSKIP instantiation, whose chunk body is compiled once per tile case zc = (oz0 == 0) | (min(D - oz0, TZ + 1) - 1) << 1.
  K3r   a unit is an 8 x 8 group of outputs of one plane (x fastest, then z, then y); workgroup b: XCD b % 8, cout group
        (b / 8) % ncg, slot b / 8 / ncg of nslots = grid / 8 / ncg; it takes the units slot, slot + nslots, ... of its XCD's eighth.
        V4 (16-byte loader) and st4 (16-byte stores) are independent: W % 4 == 0 and the base of the input / output aligned.  The
        step loop is compiled once per dead-tap set (none, tap 0, tap 2, both) for kdepth 3, V4, D <= 4.
  K3z   a column is an 8 x 8 group x all D planes (x fastest, then y); XCD b % 8 owns an eighth of the column list, its nslots =
        grid / 8 workgroups take whole columns round-robin and split the planes of the last partial round into equal contiguous
        ranges; a range walks z segments (a range end or `k3z_zs` cuts one), a segment of n planes runs n + 2 stages with the tap
        masks 1, 2, 4 (n = 1) or 1, 3, 7 x (n - 2), 6, 4."""
import functools

import torch

from featurenet_ref import MUTATION_RATIO, bound_of, bounds, errors  # noqa: F401  (the criterion; re-exported)
from regconv_ref import (F32, F64, KINDS, ZFORM_S1, ZPAD_MAX_DEPTH, _bn_relu_skip, _gen, aten_conv3d, conv3d,  # noqa: F401
                         kind_of, live_mask, make_bn, make_input)

CONV_S1 = 0                                           # include/dmvs.h
LDS_BYTES = 160 * 1024
# name -> (cin, cout, kdepth, forms)
ROWS = {
    "conv0": (2, 16, 3, ("wino",)), "conv2": (16, 16, 3, ("wino", "zmarch")), "conv4": (32, 32, 3, ("wino", "coarse")),
    "conv6": (64, 64, 3, ("wino", "coarse")), "conv4_2d": (32, 32, 1, ("coarse",)), "conv6_2d": (64, 64, 1, ("wino", "coarse")),
}
WINO_ROWS = tuple(n for n, r in ROWS.items() if "wino" in r[3])
COARSE_ROWS = tuple(n for n, r in ROWS.items() if "coarse" in r[3])
KNOB_DEFAULTS = {"wino_stages": 0, "wino_persistent": 1, "wino_conv0_grid": 512, "k3r_grid": 256, "k3r_counted_wait": 1, "k3z_grid": 0,
                 "k3z_zs": 0, "zpad_skip": 1}
ZMARCH_MIN_DEPTH = 8                                  # dmvsnet_amd/ops.py


# ------------------------------------------------------------------------------------------------ K3w geometry
# the row of kWCfgs that serves (name, D): (KD, MB, MBW, TZ, TRW, GPC); conv2 on a depth-1 volume has a flat row of its own
_WCFG = {"conv2_flat": (3, 1, 1, 1, 2, 1), "conv2": (3, 1, 1, 2, 1, 1), "conv4": (3, 2, 2, 1, 1, 1), "conv6": (3, 4, 2, 1, 1, 1),
         "conv6_2d": (1, 4, 2, 1, 1, 1)}


def wino_cfg(name, D):
    return _WCFG["conv2_flat" if name == "conv2" and D == 1 else name]


def wino_geom(name, D):
    """WinoGeom of the row: TZ, TY and the LDS bytes of ONE stage; conv0_wino_kernel: 2 planes x 8 rows, the filters and both tile
    stages in one allocation (launch_conv0_wino)."""
    if name == "conv0":
        ps0 = 4 * 10 * 40
        ps = ps0 + (32 - ps0 % 64 + 64) % 64
        return dict(TZ=2, TY=8, lds=(2 * 4 * 256 + 2 * ((2 * ps + 63) & ~63)) * 4, ci_ch=2)
    KD, MB, MBW, TZ, TRW, GPC = wino_cfg(name, D)
    ntr = 4 // (MB // MBW)
    TY = 2 * ntr * TRW
    iz, iy = (TZ + 2 if KD == 3 else TZ), TY + 2
    ps0 = iz * iy * 40
    ps = ps0 + (32 - ps0 % 64 + 64) % 64
    tile_f = (4 * GPC * ps + 63) & ~63
    return dict(TZ=TZ, TY=TY, lds=(tile_f + KD * GPC * MB * 16 * 64) * 4, ci_ch=4 * GPC)


def wino_counts(name, D, H, W):
    g = wino_geom(name, D)
    return -(-W // 32), -(-H // g["TY"]), -(-D // g["TZ"])


def wino_tiles(name, D, H, W):
    nx, ny, nz = wino_counts(name, D, H, W)
    return nx * ny * nz


def wino_resident(name, D, stages=0):
    """launch_wino: every row of ROWS prefers one LDS stage; `wino_stages` 2 takes two wherever they fit."""
    lds1 = wino_geom(name, D)["lds"]
    single = stages != 2 or 2 * lds1 > LDS_BYTES
    lds = lds1 if single else 2 * lds1
    return 256 * max(1, min(2, LDS_BYTES // lds)), (1 if single else 2)


def wino_grid(name, D, H, W, stages=0, persistent=1, conv0_grid=512):
    n = wino_tiles(name, D, H, W)
    full = 8 * (-(-n // 8))
    if not persistent:
        return full
    return min(full, conv0_grid if name == "conv0" else wino_resident(name, D, stages)[0])


def wino_tile_of(name, D, H, W, tid):
    """(ox0, oy0, oz0) of position ``tid`` of the tile list."""
    g = wino_geom(name, D)
    nx, ny, nz = wino_counts(name, D, H, W)
    bx, r = tid % nx, tid // nx
    if ROWS[name][2] == 3:
        bz, by = r % nz, r // nz
    else:
        by, bz = r % ny, r // ny
    return bx * 32, by * g["TY"], bz * g["TZ"]


def xcd_walk(ntiles, grid, b):
    """XcdTileWalk: the list positions workgroup ``b`` of ``grid`` visits, in order."""
    per = (ntiles + 7) >> 3
    out, vb = [], b
    while (vb >> 3) < per and (vb & 7) * per + (vb >> 3) < ntiles:
        out.append((vb & 7) * per + (vb >> 3))
        vb += grid
    return out


def wino_zskip(name, D, knob=1):
    """launch_wino: `if constexpr (KD == 3 && TZ == 2 && !ZSKIP) if (zpad_skip_wanted(a.D))` -- conv2's general row only."""
    return name == "conv2" and D != 1 and bool(knob) and D <= ZPAD_MAX_DEPTH


def wino_zcase(D, oz0, TZ=2):
    return int(oz0 == 0) | (min(D - oz0, TZ + 1) - 1) << 1


def wino_zcase_live(zc, TZ=2):
    """wino_zcase_live: the live (output plane, depth tap) pairs of a tile case, from zpad_live_mask on a stand-in volume."""
    return live_mask(ZFORM_S1, (zc >> 1) + 1, 0, TZ) if zc & 1 else live_mask(ZFORM_S1, TZ + (zc >> 1) + 1, TZ, TZ)


# ------------------------------------------------------------------------------------------------ K3r geometry
_RCFG = {"conv4": 2, "conv6": 1, "conv4_2d": 2, "conv6_2d": 2}      # kRCfgs: 16-channel output blocks per workgroup (NCB)


def coarse_ncg(name):
    return ROWS[name][1] // (16 * _RCFG[name])


def coarse_units(name, D, H, W, grid=256):
    """{(xcd, cout group, slot): [(ox0, oy0, oz), ...]} of every workgroup of the launch, in the order it walks them."""
    ngx, ngy, ncg = -(-W // 8), -(-H // 8), coarse_ncg(name)
    ngroups = ngx * ngy * D
    per, nslots = (ngroups + 7) >> 3, grid // 8 // ncg
    out = {}
    for b in range(grid):
        xcd, q = b & 7, b >> 3
        cg, slot = q % ncg, q // ncg
        mine = min(per, ngroups - xcd * per)
        units = []
        for g in range(xcd * per + slot, xcd * per + max(mine, 0), nslots):
            gx, r = g % ngx, g // ngx
            units.append((8 * gx, 8 * (r // D), r % D))
        out[xcd, cg, slot] = units
    return out


def coarse_v4_st4(W, in_off=0, out_off=0):
    """dmvs_conv3d_coarse: the 16-byte loader and the 16-byte stores, each from W % 4 and ITS tensor's base."""
    return W % 4 == 0 and in_off % 4 == 0, W % 4 == 0 and out_off % 4 == 0


def coarse_dead(name, D, oz):
    """The dead-tap set of a unit: bit 0 = depth tap 0, bit 1 = depth tap 2 meets only zero padding."""
    if ROWS[name][2] != 3:
        return 0
    dead = ~live_mask(ZFORM_S1, D, oz, 1)
    return (dead & 1) | ((dead >> 1) & 2)


def coarse_skipping(name, D, W, in_off=0, knob=1):
    """launch_coarse: `if constexpr (KD == 3 && V4) if (zpad_skip_wanted(a.D))`."""
    return ROWS[name][2] == 3 and coarse_v4_st4(W, in_off)[0] and bool(knob) and D <= ZPAD_MAX_DEPTH


# ------------------------------------------------------------------------------------------------ K3z geometry
def zmarch_resident():
    plane = 20 * 10
    ps = plane + (32 - plane % 64 + 64) % 64
    ni = (16 * ps // 4 + 63) // 64
    lds = (2 * ni * 256 + (4 * ((ni + 3) // 4) - ni) * 256 + 2 * 4 * 4 * 64 * 2) * 4
    return 256 * min(2, LDS_BYTES // lds)


def zmarch_grid(D, H, W, grid=0):
    ncols = -(-W // 8) * -(-H // 8)
    return min(grid or zmarch_resident(), 8 * (-(-ncols * D // 8)))


def zmarch_plan(D, H, W, grid=0, zs=0):
    """{workgroup: [(ox0, oy0, z0, planes), ...]}: the z segments of every workgroup of the launch in order; an empty list is a
    workgroup that exits at once (no column in its XCD's eighth, or an empty share of the tail round)."""
    ngx, ngy = -(-W // 8), -(-H // 8)
    ncols, per = ngx * ngy, (ngx * ngy + 7) >> 3
    g, cap = zmarch_grid(D, H, W, grid), (zs or D)
    nslots, out = g >> 3, {}
    for b in range(g):
        xcd, slot = b & 7, b >> 3
        mine = min(per, ncols - xcd * per)
        out[b] = segs = []
        if mine <= 0:
            continue
        rounds = mine // nslots
        tail_c, tail_planes = rounds * nslots, (mine - rounds * nslots) * D
        tp0, tp1 = tail_planes * slot // nslots, tail_planes * (slot + 1) // nslots
        vfull = rounds * D
        p1, p = vfull + tp1 - tp0, 0
        while p < p1:
            if p < vfull:
                z0, c = p % D, (p // D) * nslots + slot
                lim = D - z0
            else:
                q = tp0 + p - vfull
                z0, c = q % D, tail_c + q // D
                lim = min(D - z0, p1 - p)
            col = xcd * per + c
            n = min(lim, cap)
            segs.append((8 * (col % ngx), 8 * (col // ngx), z0, n))
            p += n
    return out


def zmarch_masks(n):
    """The tap masks (bit kz) of the n + 2 stages of a segment of n planes."""
    return [1, 2, 4] if n == 1 else [1, 3] + [7] * (n - 2) + [6, 4]


# ------------------------------------------------------------------------------------------------ F(2x2, 3x3) in fp32
def _bt4(d0, d1, d2, d3):
    return d0 - d2, d1 + d2, d2 - d1, d1 - d3


def wino_emulate(name, x, w, scale=None, shift=None, relu=False, dtype=F32, mutation=None, param=None):
    """The row as Winograd F(2x2, 3x3) per plane, direct over the depth taps: filters U = G g G^T in float64, rounded once; patches
    V = B^T d B, the products accumulated per transform position as ONE serial chain over (4-channel group, depth tap, channel) --
    no kernel adds more terms one after another --, outputs A^T M A, then scale / shift / ReLU: everything behind the filter
    transform in ``dtype``.  x [Cin,D,H,W] (kdepth 1: D independent slices), w [Cout,Cin,kd,3,3].  ``mutation`` (``param``): one
    mistake of a kernel --
    pairs_skipped       the (output plane, depth tap) pairs of ``param`` left out: a live mask that is off by one plane, K3z's segment
                        seam (tap 0 of the first plane of a segment), conv0's tap 2
    halo_col_zero       the halo column ox0 - 1 read as zero at every x seam of ``param`` columns
    halo_row_zero       the halo row oy0 - 1 read as zero at every y seam of ``param`` rows
    at_sign             the last sign of A^T's second row along y: m1 - m2 + m3"""
    cin, cout, kd = ROWS[name][:3]
    C, D, H, W = x.shape
    assert C == cin and tuple(w.shape) == (cout, cin, kd, 3, 3), (name, x.shape, w.shape)
    He, We, pz = H + H % 2, W + W % 2, kd // 2
    xp = torch.zeros((C, D + 2 * pz, He + 2, We + 2), dtype=dtype)
    xp[:, pz:pz + D, 1:1 + H, 1:1 + W] = x.to(dtype)
    G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=F64)
    U = torch.einsum("ai,ockij,bj->abock", G, w.to(F64), G).to(dtype).reshape(16, cout, cin, kd)
    d = [[xp[:, :, i:i + He - 1:2, j:j + We - 1:2] for j in range(4)] for i in range(4)]     # d[i][j]: [C, D + 2 pz, Ty, Tx]
    ty, tx = torch.arange(He // 2).view(-1, 1), torch.arange(We // 2)
    if mutation == "halo_col_zero":
        keep = ((2 * tx) % param != 0) | (tx == 0)
        d = [[d[i][j] * keep.to(dtype) if j == 0 else d[i][j] for j in range(4)] for i in range(4)]
    if mutation == "halo_row_zero":
        keep = ((2 * ty) % param != 0) | (ty == 0)
        d = [[d[i][j] * keep.to(dtype) if i == 0 else d[i][j] for j in range(4)] for i in range(4)]
    cols = [_bt4(d[0][j], d[1][j], d[2][j], d[3][j]) for j in range(4)]              # cols[j][a]
    V = torch.stack([v for a in range(4) for v in _bt4(cols[0][a], cols[1][a], cols[2][a], cols[3][a])])   # [16, C, D + 2 pz, Ty, Tx]
    skipped = set(param) if mutation == "pairs_skipped" else ()
    M = torch.zeros((16, cout, D) + tuple(V.shape[3:]), dtype=dtype)
    for g0 in range(0, cin, 4):
        for kz in range(kd):
            for c in range(g0, min(g0 + 4, cin)):
                term = U[:, :, c, kz].view(16, cout, 1, 1, 1) * V[:, c, kz:kz + D].unsqueeze(1)
                for oz in [p[0] for p in skipped if p[1] == kz and 0 <= p[0] < D]:
                    term[:, :, oz] = 0
                M = M + term
    M = M.view(4, 4, *M.shape[1:])
    r1 = M[1] - M[2] + M[3] if mutation == "at_sign" else M[1] - M[2] - M[3]
    rows = (M[0] + M[1] + M[2], r1)                       # A^T M: rows[r][b]
    out = torch.zeros((cout, D, He, We), dtype=dtype)
    for r in range(2):
        out[:, :, r::2, 0::2] = rows[r][0] + rows[r][1] + rows[r][2]
        out[:, :, r::2, 1::2] = rows[r][1] - rows[r][2] - rows[r][3]
    return _bn_relu_skip(out[:, :, :H, :W], scale, shift, relu, None, dtype)


def mutate(name, mutation, param, x, w, scale, shift, relu, dtype=F32):
    """One mistake of a kernel on the emulation or on the fp32 restatement --
    pairs_skipped, halo_col_zero, halo_row_zero, at_sign     on ``wino_emulate`` (see there)
    plane_d_taken       the last plane of an odd depth is the partial z tile's SECOND plane: what plane D of a volume one (zero) plane
                        deeper would hold
    half_left_out       K3r's channel half h = 1 -- the second half of every stage of ``param`` input channels -- never summed
    chunk_next_tile     the last chunk of ``param[0]`` input channels taken from the next tile of the walk, ``param[1]`` columns on
    bn_next_block       scale / shift of the neighbouring 16-channel block
    halves_swapped      conv0's two branches (output channels 0-7 and 8-15) change places"""
    kd = ROWS[name][2]
    run = lambda xx, sc=scale, sh=shift: conv3d(xx, w, 1, kd, sc, sh, relu, None, dtype)  # noqa: E731
    if mutation in ("pairs_skipped", "halo_col_zero", "halo_row_zero", "at_sign"):
        return wino_emulate(name, x, w, scale, shift, relu, dtype, mutation, param)
    if mutation == "plane_d_taken":
        out = run(x)
        out[:, -1] = run(torch.cat((x, torch.zeros_like(x[:, :1])), 1))[:, -1]
        return out
    if mutation == "half_left_out":
        x = x.clone()
        for s in range(0, x.shape[0], param):
            x[s + param // 2:s + param] = 0
        return run(x)
    if mutation == "chunk_next_tile":
        n, step = param
        x = x.clone()
        moved = torch.zeros_like(x[-n:])
        moved[..., :-step] = x[-n:, ..., step:]
        x[-n:] = moved
        return run(x)
    if mutation == "bn_next_block":
        idx = (torch.arange(scale.numel()) + 16) % scale.numel()
        return run(x, None if scale is None else scale[idx], None if shift is None else shift[idx])
    if mutation == "halves_swapped":
        out = run(x)
        return torch.cat((out[8:], out[:8]))
    raise KeyError(mutation)


# ------------------------------------------------------------------------------------------------ case tables
# (D, H, W); on the kdepth 1 rows D counts independent slices
SMALL = ((1, 1, 4), (2, 5, 36), (3, 9, 68), (4, 10, 64), (5, 17, 100))
Q4_SHAPES = ((2, 5, 36), (3, 9, 68))
# more tiles than `resident`, the count no multiple of 8, the last tile partial in x and y: label -> (row, shape, tiles)
WALK = {
    "conv2.skip": ("conv2", (4, 290, 196), 518), "conv2.plain": ("conv2", (5, 194, 196), 525), "conv2.flat": ("conv2", (1, 1170, 196), 518),
    "conv4": ("conv4", (3, 194, 196), 525), "conv6": ("conv6", (3, 98, 196), 525), "conv6_2d": ("conv6_2d", (3, 98, 196), 525),
    "conv0": ("conv0", (5, 194, 196), 525),
}
# The last two are not in the issue's table, which names two classes its seven shapes do not reach: the plain kernel on the 16-byte
# loader at D = 5 ((5,17,23) has W % 4 == 3) and the dead-tap set "both", which needs D = 1 on the 16-byte loader ((1,1,1) has W = 1)
COARSE = ((1, 1, 1), (2, 5, 7), (3, 9, 12), (4, 10, 68), (5, 17, 23), (8, 8, 8), (3, 17, 44), (5, 17, 20), (1, 3, 4))
COARSE_GRIDS = (256, 32)
ALIGNMENT_SHAPES = ((4, 10, 68), (3, 9, 12))
ZMARCH = ((1, 1, 4), (1, 9, 8), (2, 9, 12), (3, 17, 36), (9, 10, 68), (17, 10, 12))
ZMARCH_ZS = (0, 1, 2, 3, 5)
ZMARCH_GRIDS = (0, 8, 16, 64)
ZPAD_SHAPES = ((2, 5, 36), (3, 9, 68), (4, 10, 64), (5, 17, 100), (4, 290, 196))      # conv2 on K3w, `zpad_skip` 0 and 1


def wino_cases():
    return [(n, s) for n in WINO_ROWS for s in SMALL]


def q4_cases():
    return [(n, s) for n in ("conv2", "conv4", "conv6", "conv6_2d") for s in Q4_SHAPES]


def coarse_cases():
    return [(n, s) for n in COARSE_ROWS for s in COARSE]


def alignment_cases():
    return [(n, s) for n in COARSE_ROWS for s in ALIGNMENT_SHAPES]


def gpu_cases():
    """Every (row, shape) whose input a GPU test reads."""
    seen = wino_cases() + [v[:2] for v in WALK.values()] + coarse_cases() + [("conv2", s) for s in ZMARCH] + [("conv2", s) for s in ZPAD_SHAPES]
    return list(dict.fromkeys(seen))


# (row, form, shape): integer inputs and weights, the result equal to float64 with no tolerance; one WALK shape per kernel
EXACT = (("conv0", "wino", (5, 17, 100)), ("conv0", "wino", (5, 194, 196)), ("conv2", "wino", (3, 9, 68)), ("conv2", "wino", (1, 1, 4)),
         ("conv2", "wino", (5, 194, 196)), ("conv2", "zmarch", (9, 10, 68)), ("conv2", "zmarch", (3, 17, 36)), ("conv4", "wino", (3, 9, 68)),
         ("conv4", "coarse", (3, 17, 44)), ("conv6", "wino", (4, 10, 64)), ("conv6", "coarse", (5, 17, 23)), ("conv6", "coarse", (3, 98, 196)),
         ("conv4_2d", "coarse", (2, 5, 7)), ("conv6_2d", "wino", (2, 5, 36)), ("conv6_2d", "coarse", (4, 10, 68)))

_K3W3D, _TZ2 = ("conv2", "conv4", "conv6"), ("conv0", "conv2")
# mistake -> [(row, table shapes that claim to expose it, param)]
MUTATIONS = {
    # the live mask off by one plane: tap 0 dead on plane 1 as well, tap 2 on plane D - 2
    "live_mask_off_by_one": [(n, tuple(s for s in SMALL + COARSE if s[0] >= 2), "live") for n in ("conv2", "conv4", "conv6")],
    "plane_d_taken": [(n, tuple(s for s in SMALL if s[0] % 2 == 1 and s[0] > 1), None) for n in _TZ2],
    "segment_seam": [("conv2", tuple(s for s in ZMARCH if s[0] >= 3), "seam")],
    "half_left_out": [(n, COARSE, 16 if ROWS[n][2] == 3 else 32) for n in COARSE_ROWS],
    "chunk_next_tile": [(n, tuple(s for s in SMALL if s[2] > 32), (4, 32)) for n in _K3W3D + ("conv6_2d",)]
    + [(n, tuple(s for s in COARSE if s[2] > 8), (16 if ROWS[n][2] == 3 else 32, 8)) for n in COARSE_ROWS],
    "halo_col_zero": [(n, tuple(s for s in SMALL if s[2] > 32), 32) for n in WINO_ROWS]
    + [(n, tuple(s for s in COARSE if s[2] > 8), 8) for n in COARSE_ROWS] + [("conv2", tuple(s for s in ZMARCH if s[2] > 8), 8)],
    "halo_row_zero": [(n, tuple(s for s in SMALL if s[1] > 8), "ty") for n in WINO_ROWS]
    + [(n, tuple(s for s in COARSE if s[1] > 8), 8) for n in COARSE_ROWS] + [("conv2", tuple(s for s in ZMARCH if s[1] > 8), 8)],
    "bn_next_block": [(n, COARSE, None) for n in COARSE_ROWS] + [(n, SMALL, None) for n in ("conv4", "conv6", "conv6_2d")],
    "halves_swapped": [("conv0", SMALL, None)],
    "conv0_tap2_dropped": [("conv0", tuple(s for s in SMALL if s[0] >= 2), "tap2")],
    "at_sign": [(n, tuple(s for s in (SMALL if "wino" in ROWS[n][3] else COARSE) if s[1] >= 2), None) for n in ROWS],
}
_EMULATED = {"live_mask_off_by_one": "pairs_skipped", "segment_seam": "pairs_skipped", "conv0_tap2_dropped": "pairs_skipped"}


def mutation_args(mutation, name, shape, param):
    """(name of the mistake for ``mutate``, its param) at one shape."""
    D = shape[0]
    if param == "live":
        return "pairs_skipped", ((1, 0), (D - 2, 2))
    if param == "seam":       # `k3z_zs` = 2: every segment but a column's first starts at an even plane z0 >= 2
        return "pairs_skipped", tuple((z, 0) for z in range(2, D, 2))
    if param == "tap2":
        return "pairs_skipped", tuple((z, 2) for z in range(D))
    if param == "ty":
        return mutation, wino_geom(name, D)["TY"]
    return _EMULATED.get(mutation, mutation), param


# ------------------------------------------------------------------------------------------------ inputs and references
def make_weight(name, seed=0):
    """He-scaled [Cout,Cin,kd,3,3]."""
    cin, cout, kd = ROWS[name][:3]
    return torch.randn((cout, cin, kd, 3, 3), generator=_gen(21, seed, cin, cout, kd)) * (1.0 / (cin * 9 * kd) ** 0.5)


@functools.lru_cache(maxsize=None)
def case(name, D, H, W):
    """(x, w, scale, shift): the input kind by the shape; a folded BatchNorm."""
    cin, cout = ROWS[name][:2]
    scale, shift = make_bn(cout)
    return make_input(kind_of(D, H, W), cin, D, H, W), make_weight(name), scale, shift


@functools.lru_cache(maxsize=None)
def reference(name, D, H, W, bn):
    """(float64 yardstick, (e_max, e_mean) of fp32 ATen) with BatchNorm + ReLU (``bn``) or raw; the convolution itself is computed
    once per case and never modified."""
    x, w, scale, shift = case(name, D, H, W)
    kd = ROWS[name][2]
    if not bn:
        f64, raw32 = conv3d(x, w, 1, kd), aten_conv3d(x, w, 1, kd)
        return f64, errors(raw32, f64), raw32
    raw64, _, raw32 = reference(name, D, H, W, False)
    f64 = _bn_relu_skip(raw64, scale, shift, True, None, F64)
    return f64, errors(_bn_relu_skip(raw32, scale, shift, True, None, F32), f64), None


@functools.lru_cache(maxsize=None)
def exact_case(name, D, H, W):
    """x in -3 .. 3, w in -2 .. 2: G g G^T is a multiple of 1/4 and every sum an integer multiple of 1/4 far below 2^24, so fp32
    Winograd in any order gives the float64 result exactly."""
    cin, cout, kd = ROWS[name][:3]
    g = _gen(22, cin, cout, kd, D, H, W)
    return torch.randint(-3, 4, (cin, D, H, W), generator=g).float(), torch.randint(-2, 3, (cout, cin, kd, 3, 3), generator=g).float()


def impulse_positions(name, D, H, W):
    """Voxels of the impulse input: both corners, the interior, and the first voxel behind an x / y seam of every tile size in use
    (8 and 32 columns; 4, 8 and 16 rows)."""
    zm = D // 2
    pos = {(0, 0, 0), (D - 1, H - 1, W - 1), (zm, min(3, H - 1), min(5, W - 1))}
    pos |= {(zm, min(y, H - 1), min(x, W - 1)) for y in (4, 8, 16) for x in (8, 32)}
    return sorted(pos)


@functools.lru_cache(maxsize=None)
def impulse_case(name, D, H, W):
    """An impulse per position of ``impulse_positions`` in every input channel (1 + ci % 3) and 27 (9) distinct integer taps per
    channel pair: the output around an impulse spells the filter out, so a tap that goes to the wrong voxel shows exactly."""
    cin, cout, kd = ROWS[name][:3]
    x = torch.zeros((cin, D, H, W))
    for z, y, xx in impulse_positions(name, D, H, W):
        x[:, z, y, xx] = 1.0 + torch.arange(cin) % 3
    taps = torch.arange(1, 9 * kd + 1, dtype=F32).view(1, 1, kd, 3, 3)
    pair = ((torch.arange(cout).view(-1, 1) * 7 + torch.arange(cin) * 3) % 5).float().view(cout, cin, 1, 1, 1)
    return x, taps + 27 * pair
