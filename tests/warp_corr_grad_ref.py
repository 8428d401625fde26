"""Yardstick of K1b, the backward of the fused warp + correlation (``warp_corr_bwd_ref_kernel`` / ``warp_corr_bwd_src_kernel`` of
csrc/warp_corr_bwd.h): the gradients of L = <gsim, sim> with respect to the feature maps, in closed form over the PIXEL-coordinate
text of tests/warp_corr_ref.py (``coordinates``, the four taps, a tap outside the image counts zero on its own), parametrised by
``dtype`` -- float64 is the yardstick, the same text in float32 on stock ATen (CPU, sequential ``index_add_``) gives e_ref.

  dRef[c, y, x]        = (2 / C) sum_v sum_d gsim[c & 1, d, y, x] * warped_v[c, d, y, x]            (a gather)
  dSrc_v[c, tap]      += w_tap * (2 / C) * gsim[c & 1, d, y, x] * ref[c, y, x]   for the 4 taps of every sample (a scatter)

No product code runs here, no autograd and no ``grid_sample``; tests/test_warp_corr_grad_cpu.py ties the text to float64 autograd
through ``costagg_grad_ref.cost_agg_f64`` and to the reference's recorded gradients.

Cases: the seven tables of ``warp_corr_ref.all_cases()`` plus CONTENTION (below), each with an upstream gradient ``gsim_of(name)``
(i.i.d. normal fp32, seeded by the case's name).

Criterion, per gradient tensor (dRef and every dSrc_v on its own): ``warp_corr_ref.errors`` / ``bounds`` -- e_max and e_mean
relative to the tensor's max-abs, each <= 8 e_ref, 16 * 2^-23 where e_ref < 4 * 2^-23; a tensor whose yardstick is identically zero
has to be zero bit for bit.  ``bounds_of`` says which of the two bounds a table asserts:

  SHAPES, VIEWS, AFFINE, SCATTER, SPECIAL   plain max and mean bound.
  WINDOWS      the MEAN bound only (with finiteness and the guards).  K1b samples with ``ref_order_taps``, the reference's op order:
               it normalises the coordinate to [-1, 1] and un-normalises it again, four extra fp32 roundings that move a sample by
               up to 3.5 * 2^-24 * (W - 1) px, while the projections of this table (sx x + ox) are so simple that e_ref sits below
               the criterion's floor.  The fp32 restatement with that round trip added (``ref_order=True``), on the CPU: worst
               e / bound over SHAPES, VIEWS, AFFINE, SCATTER, SPECIAL and CONTENTION 0.41 (max) and 0.26 (mean); on WINDOWS the
               plain max bound is exceeded on 29 of 33 cases, by up to 4.8 x, while the mean stays at <= 0.023 of its bound
               (test_warp_corr_grad_cpu.py asserts both halves).  The forward's generic kernel behaves the same way for the same
               reason (``warp_corr_ref.op_order_allowance``).  This is the only exclusion.
  EDGE_SHAPES  the expectation is NOT this restatement: with (n - 1) / 2 = 0 the reference's normalised coordinate is NaN or
               infinite, every tap is outside and every gradient exactly zero.  ``costagg_grad_ref.grads_f64`` says so for every
               source gradient; its dRef is NaN (stock ATen's CPU grid_sample forms NaN * 0 in its forward), where zero padding
               gives 0: see test_warp_corr_grad_cpu.py::test_one_row_and_one_column_maps_have_zero_gradients.
  CONTENTION   many-to-one projections on AFFINE_SHAPE (up to all 891 samples of a view add into ONE element per channel), exact
               coordinates, so e_ref sits near the floor while the atomics may arrive in any order.  Mean bound plain; max bound
               max(plain, A) with A = ``summation_allowance``: per gradient element (n - 1) * 2^-24 * sum |t_i| over its n addends,
               the standard bound of a sum of n fp32 numbers taken in ANY order, relative to the tensor's max-abs.  Computed in
               float64 from the yardstick's own addends, nothing in it comes from a kernel's output.  About 1e-3 at 891 addends;
               one lost addend is about 3e-2.

MUTATIONS are the wrong backward kernels of the CPU file's sensitivity test."""
import functools

import torch

import warp_corr_ref as R
from warp_corr_ref import F32, F64, errors, bounds   # noqa: F401  (the criterion; re-exported for the two test files)

U32 = 2.0 ** -24
MUTATIONS = ("w01_w10_swapped", "border_clamp", "x1in_wm1", "groups_swapped", "divisor_c", "chunk_tail_dropped",
             "last_view_dropped_dref", "dsrc_view_shifted", "align_corners_false")
DCH = 8                            # planes per chunk of the scatter kernel
PLAIN_TABLES = ("SHAPES", "VIEWS", "AFFINE", "SCATTER", "SPECIAL")
TABLES = PLAIN_TABLES + ("WINDOWS", "CONTENTION", "EDGE_SHAPES")
# (sx, ox, sy, oy) on AFFINE_SHAPE: every sample on one pixel; on the centre of four; on the last pixel (x1 = W, y1 = H: two zero-weight
# taps outside); two samples per axis on a half-pixel lattice; four per column on a quarter-pixel lattice
CONTENTION = ((0, 16, 0, 4), (0, 16.5, 0, 3.25), (0, 32, 0, 8), (0.5, 0, 0.5, 0), (0.25, 4, 1, 0))
# AFFINE offsets that are multiples of 0.5 (weights 0, 1/4, 1/2, 1: a one-hot dSrc is exact) / integers (one tap of weight 1: a one-hot
# dRef is exact); test_warp_corr_grad_cpu.py asserts both, test_warp_corr_grad_gpu.py probes them
HALF_OFFSETS = ((0, 0), (-0.5, 0.5), (-1, -1), (-1.5, 0), (0.5, -0.5), (33, 0), (0, 9), (1e9, -1e9))
INT_OFFSETS = ((0, 0), (-1, -1), (33, 0), (0, 9), (1e9, -1e9))
SEAM_SHAPE = (2, 9, 65)            # (D, H, W): x = 63 | 64 is the seam of the backward's 64 x 4 tile, y = 3 | 4 and 8 its rows
SEAM_NAME = "probe-seam-c16-1_1"


# ------------------------------------------------------------------------------------------------ the restatement
def _taps(p12_v, depth, mutation, ref_order):
    """The four taps of every sample of one view, in ATen's order (nw, ne, sw, se): [(raw weight, inside, flat index)], each
    [D,H,W] but the index ([D*H*W], clamped into the image for addressing)."""
    dt = depth.dtype
    _, H, W = depth.shape
    ix, iy = R.coordinates(p12_v, depth)
    if ref_order:   # the reference's normalise / un-normalise round trip (what ref_order_taps does), one rounding per step
        ix = ((ix / ((W - 1) / 2) - 1.0) + 1.0) / 2.0 * (W - 1)
        iy = ((iy / ((H - 1) / 2) - 1.0) + 1.0) / 2.0 * (H - 1)
    if mutation == "align_corners_false":
        ix, iy = ix * W / (W - 1) - 0.5, iy * H / (H - 1) - 0.5
    x0, y0 = torch.floor(ix), torch.floor(iy)
    tx, ty = ix - x0, iy - y0
    out = []
    for dy, wy in ((0, 1 - ty), (1, ty)):
        for dx, wx in ((0, 1 - tx), (1, tx)):
            xi, yi = x0 + dx, y0 + dy
            xmax = W if (mutation == "x1in_wm1" and dx == 1) else W - 1
            inside = (xi >= 0) & (xi <= xmax) & (yi >= 0) & (yi <= H - 1)   # false for a NaN coordinate
            if mutation == "border_clamp":
                inside = torch.isfinite(xi) & torch.isfinite(yi)
            idx = (torch.nan_to_num(yi).clamp(0, H - 1) * W + torch.nan_to_num(xi).clamp(0, W - 1)).long().reshape(-1)
            out.append((torch.nan_to_num(wx * wy).to(dt), inside, idx))
    return out


def grads_ref(feats, p12, depth, gsim, dtype=F64, mutation=None, ref_order=False):
    """feats: V tensors [C,H,W]; p12 [V-1,12]; depth [D,H,W]; gsim [2,D,H,W] -> [dL/dfeat_v] (V tensors [C,H,W] in ``dtype``) for
    L = <gsim, sim>.  ``mutation``: one of MUTATIONS, None for the operation itself.  ``ref_order``: with the reference's normalise /
    un-normalise round trip on the coordinates (the op-order check of the CPU file; never part of a yardstick)."""
    assert mutation is None or mutation in MUTATIONS, mutation
    feats = [f.detach().to("cpu", dtype) for f in feats]
    p12, depth, gsim = (t.detach().to("cpu", dtype) for t in (p12, depth, gsim))
    ref = feats[0]
    C, H, W = ref.shape
    D = depth.shape[0]
    nsrc = len(feats) - 1
    assert p12.shape == (nsrc, 12) and depth.shape == (D, H, W) and gsim.shape == (2, D, H, W)
    zero = torch.zeros((), dtype=dtype)
    inv = (1.0 if mutation == "divisor_c" else 2.0) / C
    gc = (gsim.flip(0) if mutation == "groups_swapped" else gsim).repeat(C // 2, 1, 1, 1) * inv   # [C,D,H,W]: channel c takes group c & 1
    gw = gc * ref.view(C, 1, H, W)                                                                # dL/dwarped
    dk = D - 1 if (mutation == "chunk_tail_dropped" and D % DCH) else D
    gref = torch.zeros((C, H, W), dtype=dtype)
    gsrc = []
    for v in range(nsrc):
        taps = _taps(p12[v], depth, mutation, ref_order)
        src = feats[v + 1].reshape(C, H * W)
        if not (mutation == "last_view_dropped_dref" and v == nsrc - 1):
            warped = torch.zeros((C, D, H, W), dtype=dtype)
            for raw, inside, idx in taps:
                warped = warped + torch.where(inside, raw, zero) * src[:, idx].view(C, D, H, W)
            gref = gref + (gc * warped).sum(1)
        raws = [t[0] for t in taps]
        if mutation == "w01_w10_swapped":
            raws[1], raws[2] = raws[2], raws[1]
        g = torch.zeros((C, H * W), dtype=dtype)
        for (_, inside, idx), raw in zip(taps, raws):
            val = torch.where(inside, raw, zero) * gw
            g.index_add_(1, idx.view(D, H * W)[:dk].reshape(-1), val[:, :dk].reshape(C, -1))
        gsrc.append(g.view(C, H, W))
    if mutation == "dsrc_view_shifted":
        gsrc = gsrc[1:] + gsrc[:1]
    return [gref] + gsrc


def summation_allowance(feats, p12, depth, gsim):
    """Per gradient tensor (A, slope), both relative to the tensor's max-abs (0 where that is zero), in float64 from the yardstick's
    own addends t_i = w_tap * (2 / C) * gsim * ref (dSrc) and (2 / C) * gsim * w_tap * src_tap (dRef):
      A      max over the elements of (n - 1) * 2^-24 * sum |t_i|, n = the element's addends with a non-zero weight: what summing n
             fp32 numbers in any order may differ from the exact sum by (to first order; Higham, Accuracy and Stability, 4.2);
      slope  max over the elements of sum |t_i / w_tap|: what an element moves by per unit of weight error (the CPU file's bound on
             the distance between two float64 statements)."""
    feats = [f.detach().to("cpu", F64) for f in feats]
    p12, depth, gsim = (t.detach().to("cpu", F64) for t in (p12, depth, gsim))
    ref = feats[0]
    C, H, W = ref.shape
    D = depth.shape[0]
    gc = (gsim.repeat(C // 2, 1, 1, 1) * (2.0 / C)).abs()
    gw = gc * ref.abs().view(C, 1, H, W)
    grads = grads_ref(feats, p12, depth, gsim, F64)
    s_ref, u_ref, n_ref = torch.zeros((C, H, W), dtype=F64), torch.zeros((C, H, W), dtype=F64), torch.zeros((H, W), dtype=F64)
    out = []
    for v in range(p12.shape[0]):
        src = feats[v + 1].reshape(C, H * W).abs()
        s, u, n = torch.zeros((C, H * W), dtype=F64), torch.zeros((C, H * W), dtype=F64), torch.zeros((H * W,), dtype=F64)
        for raw, inside, idx in _taps(p12[v], depth, None, False):
            w = torch.where(inside, raw, torch.zeros((), dtype=F64))
            s.index_add_(1, idx, (w * gw).reshape(C, -1))
            u.index_add_(1, idx, (inside * gw).reshape(C, -1))
            n.index_add_(0, idx, (w != 0).to(F64).reshape(-1))
            tap = src[:, idx].view(C, D, H, W)
            s_ref += (gc * w * tap).sum(1)
            u_ref += (gc * inside * tap).sum(1)
            n_ref += (w != 0).to(F64).sum(0)
        out.append(((n - 1).clamp(min=0) * U32 * s, u))
    out.insert(0, ((n_ref - 1).clamp(min=0) * U32 * s_ref, u_ref))
    res = []
    for (a, u), g in zip(out, grads):
        scale = g.abs().max().item()
        res.append((0.0, 0.0) if scale == 0.0 else (a.max().item() / scale, u.max().item() / scale))
    return res


# ------------------------------------------------------------------------------------------------ cases
def gsim_of(name, D, H, W):
    """The upstream gradient of a case: [2,D,H,W] fp32, i.i.d. standard normal, seeded by the name."""
    g = torch.Generator().manual_seed(R.seed_of(name) ^ 0x651D)
    return torch.randn((2, D, H, W), generator=g, dtype=F32)


def _literal_case(table, name, C, shape, p12):
    """The AFFINE recipe (``warp_corr_ref.affine_cases``): hypotheses 256 / 512 / 1024 drawn per pixel and plane."""
    D, H, W = shape
    g = torch.Generator().manual_seed(R.seed_of(name) ^ 0x5EED)
    depth = 2.0 ** (8 + torch.randint(0, 3, (D, H, W), generator=g)).to(F32)
    return R._case(table, name, C, R.features(name, 2, C, H, W), depth, p12=p12, nonzero_e_ref=False)


def contention_cases():
    out = {}
    for C in (8, 32):
        for sx, ox, sy, oy in CONTENTION:
            name = f"contention-c{C}-{sx:g}_{ox:g}_{sy:g}_{oy:g}"
            out[name] = _literal_case("CONTENTION", name, C, R.AFFINE_SHAPE, R.affine_p12(sx, ox, sy, oy))
    return out


def seam_case():
    """The one-hot probes' extra case: ix = x + 1, iy = y + 1 on a map with an x tile seam (W = 65)."""
    return _literal_case("PROBE", SEAM_NAME, 16, SEAM_SHAPE, R.affine_p12(1, 1, 1, 1))


@functools.lru_cache(maxsize=None)
def all_cases():
    """name -> case (``warp_corr_ref._case`` plus ``gsim``): the forward's tables and CONTENTION.  Shared and never modified."""
    out = dict(R.all_cases())
    out.update(contention_cases())
    for name, c in out.items():
        c["gsim"] = gsim_of(name, *c["depth"].shape)
    return out


def affine_name(C, ox, oy):
    return f"affine-c{C}-{ox:g}_{oy:g}"


def reference(case, p12):
    """([float64 gradients], [(e_max, e_mean) of the fp32 restatement per tensor]) under the fp32 ``p12`` handed to the kernel."""
    g64 = grads_ref(case["feats"], p12, case["depth"], case["gsim"], F64)
    g32 = grads_ref(case["feats"], p12, case["depth"], case["gsim"], F32)
    return g64, [errors(a, b) for a, b in zip(g32, g64)]


def allowances(case, p12):
    """Per tensor what goes into the max bound beside the plain one: ``summation_allowance`` on CONTENTION, 0 anywhere else."""
    if case["table"] != "CONTENTION":
        return [0.0] * len(case["feats"])
    return [a for a, _ in summation_allowance(case["feats"], p12, case["depth"], case["gsim"])]


def bounds_of(table, e_ref, allowance=0.0):
    """(bound on e_max or None where the table does not assert it, bound on e_mean) of one gradient tensor."""
    assert table in TABLES and table != "EDGE_SHAPES", table
    b = bounds(e_ref)
    if table == "WINDOWS":
        return None, b[1]
    return (max(b[0], allowance) if table == "CONTENTION" else b[0]), b[1]


def one_hot(D, H, W, g, d, y, x):
    out = torch.zeros((2, D, H, W), dtype=F32)
    out[g, d, y, x] = 1.0
    return out


def probe_voxels(D, H, W):
    """(d, y, x) of the one-hot probes on a map: the four corners, a pixel of each edge, an interior pixel, a pixel of the last
    (partial, H = 9) tile row; on a map wider than the backward's 64-column tile also both sides of the x seam in the rows either side
    of the y seam and in the last row."""
    vox = [(0, 0, 0), (D - 1, 0, W - 1), (1 % D, H - 1, 0), (0, H - 1, W - 1), (0, 0, W // 2), (D - 1, H - 1, W // 2 - 3), (1 % D, H // 2, 0),
           (0, H // 2 - 1, W - 1), (D - 1, H // 2, W // 2), (0, H - 1, 7)]
    if W > 64:
        vox += [(d % D, y, x) for d, (y, x) in enumerate((y, x) for y in (3, 4, 8) for x in (63, 64))]
    return vox


def probe_cases():
    """(name, case, dSrc exact, dRef exact) of the one-hot probes."""
    out = []
    for C in (8, 32):
        for ox, oy in HALF_OFFSETS:
            name = affine_name(C, ox, oy)
            out.append((name, all_cases()[name], True, (ox, oy) in INT_OFFSETS))
    out.append((SEAM_NAME, seam_case(), True, True))
    return out
