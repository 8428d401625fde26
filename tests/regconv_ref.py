"""Test infrastructure: yardstick, criterion and case tables of K3's regularisation convs -- the thirteen (Cin, Cout, mode, kdepth)
rows of ``kCfgs`` (csrc/conv3d_mfma.hip) that CostRegNet and the refine net run: conv1 / conv3 / conv5 (stride 2), conv7 / conv9 /
conv11 (transposed), the K3 fall-backs of conv0 / conv2 / conv4 / conv6 (stride 1) and the three 2D (kdepth 1) refine rows.  No
product code here; tests/test_regconv_cpu.py checks this file against ATen in float64, asserts what the tables claim and shows which
mistakes the criterion catches; tests/test_regconv_gpu.py holds the kernels to it.

Restated from the formulas, dtype-generic, float64 on the CPU being the yardstick, tap by tap as shifted-slice sums (padded copy,
strided slices, einsum; no convolution library), x [Cin,D,H,W]:

  conv3d    y[co,oz,oy,ox] = sum_{ci,kz,ky,kx} w[co,ci,kz,ky,kx] x[ci, s oz + kz - kd // 2, s oy + ky - 1, s ox + kx - 1], zero outside;
            padding (kd // 2, 1, 1); stride 2: Do = (D + 1) // 2 (kd 3) or D (kd 1: D counts independent slices), Ho = (H + 1) // 2,
            Wo = (W + 1) // 2.
  deconv3d  the transposed form as a SCATTER: input (z, y, x) through tap (kz, ky, kx) adds w[ci,co,kz,ky,kx] x[ci,z,y,x] to output
            (2 z + kz - 1, 2 y + ky - 1, 2 x + kx - 1); the output is exactly (2 D, 2 H, 2 W) (output_padding 1), (D, 2 H, 2 W) for kd 1.
  both      then y * scale + shift, then the ReLU, then + skip: the residual goes in BEHIND the ReLU (tests/test_gpu_parity.py::_conv_ref
            and the kernels' epilogues).

Criterion (the project's, featurenet_ref's bound_of / errors): e_max = max|a - f64| / max|f64| and e_mean = mean|a - f64| / max|f64|,
each e_hip <= 8 e_ref, and 16 * 2^-23 where e_ref < 4 * 2^-23.  e_ref is the distance of the same operation in fp32 on stock ATen on
the CPU (``aten_*`` below), never of a HIP kernel."""
import functools

import torch
import torch.nn.functional as F

from featurenet_ref import HUGE, MUTATION_RATIO, bound_of, bounds, errors  # noqa: F401  (the criterion; re-exported)

F64, F32 = torch.float64, torch.float32
CONV_S1, CONV_S2, DECONV_S2 = 0, 1, 2               # include/dmvs.h
PLAN_MBS, PLAN_V4 = 1 << 17, 1 << 16                # dmvs_conv3d_mfma_plan: M-block split, W % 4 == 0 (conv rows only)
ZFORM_S1, ZFORM_S2, ZFORM_T2 = 0, 1, 2              # csrc/common.h
ZPAD_MAX_DEPTH = 4                                  # csrc/common.h kZpadMaxDepth


def _bn_relu_skip(out, scale, shift, relu, skip, dtype, before_relu=False):
    if scale is not None:
        out = out * scale.to(dtype).view(-1, 1, 1, 1) + shift.to(dtype).view(-1, 1, 1, 1)
    if before_relu and skip is not None:
        out, skip = out + skip.to(dtype), None
    if relu:
        out = torch.relu(out)
    return out if skip is None else out + skip.to(dtype)


# ------------------------------------------------------------------------------------------------ restatement
def conv3d(x, w, stride, kd, scale=None, shift=None, relu=False, skip=None, dtype=F64, mutation=None, param=None):
    """x [Cin,D,H,W], w [Cout,Cin,kd,3,3] -> [Cout,Do,Ho,Wo].  ``mutation`` (with ``param``): one mistake of a kernel, for the CPU file --
    do_floor          stride 2, kd 3: Do = D // 2, the last plane of an odd depth never written (left zero)
    s2_origin_late    stride 2: the tap origin one voxel late along every strided axis
    mblock_swap       channels co and co + 32 swapped (the two M blocks of a Cout = 64 row)
    skip_before_relu  the residual added in front of the ReLU
    kz0_dropped       depth tap 0 left out (live wherever an output plane oz >= 1 exists: D >= 3 at stride 2)
    chunk_left_out    the last chunk of ``param`` input channels never accumulated"""
    x, w = x.to(dtype), w.to(dtype)
    Cin, D, H, W = x.shape
    Cout = w.shape[0]
    assert tuple(w.shape) == (Cout, Cin, kd, 3, 3) and kd in (1, 3) and stride in (1, 2), (x.shape, w.shape, kd, stride)
    if mutation == "chunk_left_out":
        x = x.clone()
        x[Cin - param:] = 0
    pz, sz = kd // 2, (stride if kd == 3 else 1)
    Do, Ho, Wo = (D + sz - 1) // sz, (H + stride - 1) // stride, (W + stride - 1) // stride
    xp = torch.zeros((Cin, D + 2 * pz + 2, H + 4, W + 4), dtype=dtype)       # (two spare voxels per axis for s2_origin_late)
    xp[:, pz:pz + D, 1:1 + H, 1:1 + W] = x
    late = int(mutation == "s2_origin_late" and stride == 2)
    lz = late if kd == 3 else 0
    out = torch.zeros((Cout, Do, Ho, Wo), dtype=dtype)
    for kz in range(kd):
        if mutation == "kz0_dropped" and kd == 3 and kz == 0:
            continue
        for ky in range(3):
            for kx in range(3):
                sl = xp[:, kz + lz:kz + lz + sz * (Do - 1) + 1:sz, ky + late:ky + late + stride * (Ho - 1) + 1:stride,
                        kx + late:kx + late + stride * (Wo - 1) + 1:stride]
                out = out + torch.einsum("oc,cdhw->odhw", w[:, :, kz, ky, kx], sl)
    if mutation == "do_floor" and stride == 2 and kd == 3:
        out[:, D // 2:] = 0
    if mutation == "mblock_swap" and Cout == 64:
        out = torch.cat((out[32:], out[:32]))
    return _bn_relu_skip(out, scale, shift, relu, skip, dtype, mutation == "skip_before_relu")


def deconv3d(x, w, kd, scale=None, shift=None, relu=False, skip=None, dtype=F64, mutation=None, param=None):
    """x [Cin,D,H,W], w [Cin,Cout,kd,3,3] -> [Cout, 2 D | D, 2 H, 2 W], as a scatter.  ``mutation``: one mistake of a kernel --
    outpad_edge       the last output plane / row / column (2 n - 1: the one output_padding 1 adds) without its contribution.  It has
                      one only: tap 2 of the last input voxel in this scatter statement, tap 0 of the flipped kernel of the gather form
    tap_of_swapped    the parity -> tap map swapped along every strided axis: taps 0 and 2 change places (csrc tap_of)
    pym_parity_swapped  output rows 2 y and 2 y + 1 of the convolution swapped (the two halves of conv11's y-parity-merged rows)
    plane_wrap        the (input plane D - 1, tap 0) pair of the gather form -- input plane D, padding -- read as plane 0: output plane
                      2 D - 1 also gets what plane 0 sends through tap 0 (to plane -1, dropped)
    skip_before_relu, chunk_left_out  as in ``conv3d``"""
    x, w = x.to(dtype), w.to(dtype)
    Cin, D, H, W = x.shape
    Cout = w.shape[1]
    assert tuple(w.shape) == (Cin, Cout, kd, 3, 3) and kd in (1, 3), (x.shape, w.shape, kd)
    if mutation == "chunk_left_out":
        x = x.clone()
        x[Cin - param:] = 0
    if mutation == "tap_of_swapped":
        w = w.flip(3, 4) if kd == 1 else w.flip(2, 3, 4)
    Do = 2 * D if kd == 3 else D
    pz = 1 if kd == 3 else 0
    frame = torch.zeros((Cout, Do + 2 * pz, 2 * H + 2, 2 * W + 2), dtype=dtype)     # index o + 1 holds output voxel o
    for kz in range(kd):
        zs = slice(kz, kz + 2 * D, 2) if kd == 3 else slice(None)
        for ky in range(3):
            for kx in range(3):
                frame[:, zs, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += torch.einsum("co,cdhw->odhw", w[:, :, kz, ky, kx], x)
    out = frame[:, pz:pz + Do, 1:1 + 2 * H, 1:1 + 2 * W].clone()
    if mutation == "plane_wrap" and kd == 3:
        out[:, Do - 1] += frame[:, 0, 1:1 + 2 * H, 1:1 + 2 * W]
    if mutation == "outpad_edge":
        if kd == 3:
            out[:, -1] = 0
        out[:, :, -1] = 0
        out[..., -1] = 0
    if mutation == "pym_parity_swapped":
        out = out[:, :, torch.arange(2 * H) ^ 1]
    return _bn_relu_skip(out, scale, shift, relu, skip, dtype, mutation == "skip_before_relu")


# ------------------------------------------------------------------------------------------------ fp32 ATen (e_ref)
def aten_conv3d(x, w, stride, kd, scale=None, shift=None, relu=False, skip=None, dtype=F32):
    """F.conv3d with the arguments of tests/test_gpu_parity.py::_conv_ref."""
    y = F.conv3d(x.to(dtype)[None], w.to(dtype), None, (stride if kd == 3 else 1, stride, stride), (kd // 2, 1, 1))[0]
    return _bn_relu_skip(y, scale, shift, relu, skip, dtype)


def aten_deconv3d(x, w, kd, scale=None, shift=None, relu=False, skip=None, dtype=F32):
    if kd == 3:
        y = F.conv_transpose3d(x.to(dtype)[None], w.to(dtype), None, 2, 1, 1)[0]
    else:
        y = F.conv_transpose3d(x.to(dtype)[None], w.to(dtype), None, (1, 2, 2), (0, 1, 1), (0, 1, 1))[0]
    return _bn_relu_skip(y, scale, shift, relu, skip, dtype)


# ------------------------------------------------------------------------------------------------ rows
# name -> (cin, cout, mode, kd, M, MB, ci_ch, pym, nmb): the row of kCfgs; nmb = 2: conv7's two-row form (NMB of launch_deconv)
ROWS = {
    "conv0": (2, 16, CONV_S1, 3, 16, 1, 2, 0, 1), "conv1": (8, 16, CONV_S2, 3, 16, 1, 1, 0, 1),
    "conv2": (16, 16, CONV_S1, 3, 16, 1, 4, 0, 1), "conv3": (16, 32, CONV_S2, 3, 32, 1, 2, 0, 1),
    "conv4": (32, 32, CONV_S1, 3, 32, 1, 2, 0, 1), "conv5": (32, 64, CONV_S2, 3, 32, 2, 2, 0, 1),
    "conv6": (64, 64, CONV_S1, 3, 32, 2, 4, 0, 1), "conv7": (64, 32, DECONV_S2, 3, 16, 2, 8, 0, 2),
    "conv9": (32, 16, DECONV_S2, 3, 16, 1, 4, 0, 1), "conv11": (16, 8, DECONV_S2, 3, 16, 1, 4, 1, 1),
    "conv5_2d": (32, 64, CONV_S2, 1, 32, 2, 2, 0, 1), "conv6_2d": (64, 64, CONV_S1, 1, 32, 2, 4, 0, 1),
    "conv7_2d": (64, 32, DECONV_S2, 1, 16, 2, 8, 0, 2),
}
MODE_TAG = {CONV_S1: "DMVS_CONV_S1", CONV_S2: "DMVS_CONV_S2", DECONV_S2: "DMVS_DECONV_S2"}
# tile form -> (k3_min_blocks, k3_split_blocks); None = the library default.  `only`: launch_deconv reads neither knob
K3_KNOBS = {"big": (0, None), "small": (HUGE, 0), "split": (None, None), "only": (None, None)}
K3_DEFAULTS = {"k3_min_blocks": 768, "k3_split_blocks": 1024}
KNOB_DEFAULTS = {**K3_DEFAULTS, "k3_single_buf_min_blocks": 0, "zpad_skip": 1, "k3_deconv_prefetch": 1}

# (D, H, W) of the INPUT; on kd = 1 rows D counts slices
S1_SHAPES = ((3, 9, 36), (1, 17, 33), (2, 5, 30), (5, 3, 68), (4, 10, 67), (1, 1, 1))
S2_SHAPES = ((4, 18, 72), (3, 17, 67), (2, 18, 72), (2, 10, 130), (5, 6, 8), (1, 5, 8), (1, 2, 3))
S2_OUT = ((2, 9, 36), (2, 9, 34), (1, 9, 36), (1, 5, 65), (3, 3, 4), (1, 3, 4), (1, 1, 2))      # of the kd = 3 rows
T2_SHAPES = ((2, 5, 36), (3, 3, 33), (1, 9, 20), (1, 6, 30), (4, 2, 68), (1, 1, 1))
# the shapes at which a skipping instantiation runs (kd = 3 rows, knob on, aligned input), and their plain twins.  (1,1,1) is not marked
# in the issue's table; it has one input plane like (1,9,20) and takes ZSKIP too
ZDEAD_SHAPES, ZDEAD_TWINS = ((2, 18, 72),), ((2, 10, 130), (1, 5, 8))
ZSKIP_SHAPES, ZSKIP_TWINS = ((1, 9, 20), (1, 6, 30), (1, 1, 1)), ((2, 5, 36),)


def mode_of(name):
    return ROWS[name][2]


def stride_of(name):
    return 2 if mode_of(name) == CONV_S2 else 1


def shapes_of(name):
    return {CONV_S1: S1_SHAPES, CONV_S2: S2_SHAPES, DECONV_S2: T2_SHAPES}[mode_of(name)]


def forms_of(name):
    """The tile forms of a row: big and plain small; the M-block split (what the default knobs pick at every size of the tables) on
    the MB = 2 conv rows; the transposed rows have one form."""
    if mode_of(name) == DECONV_S2:
        return ("only",)
    return ("big", "small", "split") if ROWS[name][5] == 2 else ("big", "small")


def out_shape(name, D, H, W):
    _, _, mode, kd = ROWS[name][:4]
    if mode == CONV_S1:
        return D, H, W
    if mode == CONV_S2:
        return ((D + 1) // 2 if kd == 3 else D), (H + 1) // 2, (W + 1) // 2
    return (2 * D if kd == 3 else D), 2 * H, 2 * W


def tile_of(name, form, D, H, W):
    """(TZ, TY, split) restated from conv_tile_choice / launch_deconv for the knobs of K3_KNOBS[form]: tiles of TZ x TY x 32 voxels of
    the OUTPUT grid, of the INPUT grid on the transposed rows.  (Every size of the tables stays under 768 big and 1024 small tiles.)"""
    _, _, mode, kd, _, MB, _, _, nmb = ROWS[name]
    if mode == DECONV_S2:
        flat = kd == 1 or D == 1
        return ((1, 2, 0) if flat else (2, 1, 0)) if nmb == 2 else ((1, 4, 0) if flat else (2, 2, 0))
    Do = out_shape(name, D, H, W)[0]
    flat, s1 = kd == 1 or Do == 1, mode == CONV_S1
    if form == "big":
        return (1, 16 if s1 else 8, 0) if flat else (2, 8 if s1 else 4, 0)
    if form == "split":
        assert MB == 2
        return (1, 2, 1) if flat else (2, 1, 1)
    return (1, 4, 0) if flat else (2, 2, 0)


def expected_plan(name, form, D, H, W):
    """dmvs_conv3d_mfma_plan: TZ * 256 + TY, bit 17 for the split form, bit 16 for W % 4 == 0 -- on the conv rows; the transposed
    rows have ONE tile loader (dwords) and the library reports the tile alone."""
    tz, ty, split = tile_of(name, form, D, H, W)
    if mode_of(name) == DECONV_S2:
        return tz * 256 + ty
    return tz * 256 + ty + (PLAN_MBS if split else 0) + (PLAN_V4 if W % 4 == 0 else 0)


def geometry(name, form, D, H, W):
    """The tile grid of a launch: counts (nx, ny, nz), the extent of the LAST tile along each axis (x_last of 32, y_last of TY, z_last
    of TZ), the loader and whether the epilogue may store 16 bytes."""
    tz, ty, split = tile_of(name, form, D, H, W)
    tr = mode_of(name) == DECONV_S2
    gd, gh, gw = (D, H, W) if tr else out_shape(name, D, H, W)
    last = lambda n, t: n - (-(-n // t) - 1) * t  # noqa: E731
    return dict(tz=tz, ty=ty, split=split, flat=tz == 1, nx=-(-gw // 32), ny=-(-gh // ty), nz=-(-gd // tz),
                x_last=last(gw, 32), y_last=last(gh, ty), z_last=last(gd, tz),
                loader="dword" if tr or W % 4 else "v4", st4=(not tr) and out_shape(name, D, H, W)[2] % 4 == 0)


def live_mask(form, D, oz0, TZ):
    """zpad_live_mask as tests/test_zpad_host.py states it: each form on an indicator volume (1 inside, 0 in the padding) through its
    textbook definition; bit 3 p + kz is set when plane oz0 + p of the tile picks up a 1 through depth tap kz."""
    inside = lambda z: 0 <= z < D  # noqa: E731
    mask = 0
    for p in range(TZ):
        z = oz0 + p
        if form in (ZFORM_S1, ZFORM_S2):
            s = 1 if form == ZFORM_S1 else 2
            if z >= (D + 2 - 3) // s + 1:
                continue
            for kz in range(3):
                mask |= int(inside(s * z - 1 + kz)) << (3 * p + kz)
        else:       # scatter: input plane j reaches output plane 2 j - 1 + kz; base plane z owns outputs 2 z (tap 1), 2 z + 1 (taps 2, 0)
            if z >= D:
                continue
            for kz in range(3):
                o = 2 * z + (0 if kz == 1 else 1)
                mask |= int((o + 1 - kz) % 2 == 0 and inside((o + 1 - kz) // 2)) << (3 * p + kz)
    return mask


def skipping(name, D, H, W, knob=1, aligned=True):
    """Whether the launch takes a zero-padding-skipping instantiation (launch_conv_tile_v: ZDEAD = 1; launch_deconv_tile: ZSKIP):
    knob on and D <= 4, then -- stride 2: a flat tile (Do == 1), 16-byte loads, and tap 0 the ONLY dead depth tap (D == 2);
    transposed: one input plane, whose tap 0 reads the padding plane D."""
    _, _, mode, kd = ROWS[name][:4]
    if not knob or D > ZPAD_MAX_DEPTH or kd != 3 or mode == CONV_S1:
        return False
    if mode == CONV_S2:
        return out_shape(name, D, H, W)[0] == 1 and W % 4 == 0 and aligned and (~live_mask(ZFORM_S2, D, 0, 1) & 7) == 1
    return D == 1 and not (live_mask(ZFORM_T2, D, 0, 1) & 1)


def cases():
    """[(row, (D, H, W))]: one GPU test each; the forms and residual variants of a row run on one input."""
    return [(name, s) for name in ROWS for s in shapes_of(name)]


def single_buf_cases():
    """The 3D conv rows (launch_conv_tile_v's KD == 3: the only ones `k3_single_buf_min_blocks` reaches) at their first two shapes."""
    return [(name, s) for name in ROWS if ROWS[name][3] == 3 and mode_of(name) != DECONV_S2 for s in shapes_of(name)[:2]]


def zpad_cases():
    out = [(n, s) for n in ("conv1", "conv3", "conv5") for s in ZDEAD_SHAPES + ZDEAD_TWINS]
    return out + [(n, s) for n in ("conv7", "conv9", "conv11") for s in ZSKIP_SHAPES + ZSKIP_TWINS]


MISALIGNED_CASES = (("conv2", (3, 9, 36)), ("conv1", (4, 18, 72)))
EXACT_CASES = (("conv2", (3, 9, 36)), ("conv2", (1, 17, 33)), ("conv1", (4, 18, 72)), ("conv1", (3, 17, 67)), ("conv11", (2, 5, 36)),
               ("conv11", (3, 3, 33)), ("conv11", (1, 9, 20)))

# mistake -> the rows it applies to
_CONV = tuple(n for n in ROWS if mode_of(n) != DECONV_S2)
_T2 = tuple(n for n in ROWS if mode_of(n) == DECONV_S2)
MUTATIONS = {
    "do_floor": ("conv1", "conv3", "conv5"), "s2_origin_late": tuple(n for n in ROWS if mode_of(n) == CONV_S2),
    "outpad_edge": _T2, "tap_of_swapped": _T2, "pym_parity_swapped": ("conv11",),
    "mblock_swap": tuple(n for n in _CONV if ROWS[n][1] == 64), "skip_before_relu": tuple(ROWS),
    "kz0_dropped": ("conv1", "conv3", "conv5"), "plane_wrap": ("conv7", "conv9", "conv11"), "chunk_left_out": tuple(ROWS),
}


def mutation_shapes(mutation, name):
    """The shapes of the row's table at which the mistake changes anything."""
    s = shapes_of(name)
    if mutation == "do_floor":
        return tuple(t for t in s if t[0] % 2 == 1 and t[0] > 1)     # (D = 1: D // 2 planes is no plane at all)
    if mutation == "kz0_dropped":
        return tuple(t for t in s if t[0] >= 3)
    if mutation in ("pym_parity_swapped", "mblock_swap", "s2_origin_late", "outpad_edge", "tap_of_swapped", "plane_wrap"):
        return tuple(t for t in s if t[1] * t[2] >= 64)
    return s


# ------------------------------------------------------------------------------------------------ inputs
KINDS = ("normal", "relu")


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def kind_of(*shape):
    """The input kind of a case: alternating over the tables, fixed by the shape."""
    return KINDS[sum(shape) % 2]


def make_input(kind, C, D, H, W, seed=0):
    """fp32 [C,D,H,W]: seeded normal, or the post-ReLU-like |N(0,1)| + 1 (what every layer but the first reads in the networks)."""
    x = torch.randn((C, D, H, W), generator=_gen(11, seed, C, D, H, W))
    return x if kind == "normal" else x.abs() + 1.0


def make_weight(name, seed=0):
    """He-scaled, [Cout,Cin,kd,3,3], [Cin,Cout,kd,3,3] on a transposed row."""
    cin, cout, mode, kd = ROWS[name][:4]
    a, b = (cin, cout) if mode == DECONV_S2 else (cout, cin)
    return torch.randn((a, b, kd, 3, 3), generator=_gen(12, seed, cin, cout, mode, kd)) * (1.0 / (cin * 9 * kd) ** 0.5)


def make_bn(cout, seed=0):
    """Folded BatchNorm as tests/test_gpu_parity.py::_layer draws it: scale in 0.5 .. 1.5, shift 0.2 N(0,1)."""
    g = _gen(13, seed, cout)
    return 0.5 + torch.rand(cout, generator=g), 0.2 * torch.randn(cout, generator=g)


def run(name, x, w, scale, shift, relu, skip=None, dtype=F64, mutation=None, aten=False):
    """The row's operation on the restatement (or its ATen twin)."""
    _, _, mode, kd, _, _, ci_ch = ROWS[name][:7]
    if mode == DECONV_S2:
        if aten:
            return aten_deconv3d(x, w, kd, scale, shift, relu, skip, dtype)
        return deconv3d(x, w, kd, scale, shift, relu, skip, dtype, mutation, ci_ch)
    if aten:
        return aten_conv3d(x, w, stride_of(name), kd, scale, shift, relu, skip, dtype)
    return conv3d(x, w, stride_of(name), kd, scale, shift, relu, skip, dtype, mutation, ci_ch)


@functools.lru_cache(maxsize=None)
def case(name, D, H, W):
    """(x, w, scale, shift, skip): the input kind by the shape; folded BN + ReLU; a normal residual of the output's shape."""
    cin, cout = ROWS[name][:2]
    scale, shift = make_bn(cout)
    return make_input(kind_of(D, H, W), cin, D, H, W), make_weight(name), scale, shift, make_input("normal", cout, *out_shape(name, D, H, W), seed=1)


@functools.lru_cache(maxsize=None)
def reference(name, D, H, W, with_skip):
    """(float64 yardstick, (e_max, e_mean) of fp32 ATen); computed once, never modified."""
    x, w, scale, shift, skip = case(name, D, H, W)
    if with_skip:      # the residual goes in behind everything else: exact in float64 up to its own rounding
        f64 = reference(name, D, H, W, False)[0] + skip.double()
    else:
        f64 = run(name, x, w, scale, shift, True)
    return f64, errors(run(name, x, w, scale, shift, True, skip if with_skip else None, F32, aten=True), f64)


@functools.lru_cache(maxsize=None)
def exact_case(name, D, H, W):
    """Small integers: x in -3 .. 3, w in -2 .. 2, no BN, no ReLU, an integer residual: every partial sum is an integer below 2^24
    (64 x 27 x 6 at most), so fp32 in any order gives the float64 result exactly."""
    cin, cout, mode, kd = ROWS[name][:4]
    g = _gen(14, cin, cout, D, H, W)
    a, b = (cin, cout) if mode == DECONV_S2 else (cout, cin)
    x = torch.randint(-3, 4, (cin, D, H, W), generator=g).float()
    w = torch.randint(-2, 3, (a, b, kd, 3, 3), generator=g).float()
    skip = torch.randint(-9, 10, (cout, *out_shape(name, D, H, W)), generator=g).float()
    return x, w, skip


# ------------------------------------------------------------------------------------------------ packing orders
def pack_sources(name):
    """dmvs_pack_conv_weights_mfma restated: for every packed float the flat index of its source in the PyTorch weight, -1 for a
    packed zero.  Three orders: packed-K (ci_ch < KK: several taps share a k-step), plain, transposed (with the y-parity merge of
    ``pym``: row r of the fragment is channel r % 8 of y parity r // 8)."""
    cin, cout, mode, kd, M, MB, ci_ch, pym, _ = ROWS[name]
    KK, NT = (2 if M == 32 else 4), 9 * kd
    GPC = ci_ch // KK
    tap_of = lambda p, o: 1 if p == 0 else (2 if o == 0 else 0)  # noqa: E731
    src = []
    for ci0 in range(0, cin, ci_ch):
        if mode != DECONV_S2 and ci_ch < KK:
            tpg = KK // ci_ch
            for st in range(-(-NT // tpg)):
                for mb in range(MB):
                    for lane in range(64):
                        co, k = mb * M + lane % M, lane // M
                        ci, t = ci0 + k % ci_ch, st * tpg + k // ci_ch
                        src.append((co * cin + ci) * NT + t if co < cout and t < NT else -1)
        elif mode != DECONV_S2:
            for t in range(NT):
                for g in range(GPC):
                    for mb in range(MB):
                        for lane in range(64):
                            co, ci = mb * M + lane % M, ci0 + g * KK + lane // M
                            src.append((co * cin + ci) * NT + t if co < cout else -1)
        else:
            npz = 2 if kd == 3 else 1
            for oz in range(npz):
                for oy in range(2):
                    for ox in range(2):
                        for g in range(GPC):
                            for pz in range(oz, npz):
                                for py in range(1 if pym else oy, 2):
                                    for px in range(ox, 2):
                                        for mb in range(MB):
                                            kz = tap_of(pz, oz) if kd == 3 else 0
                                            for lane in range(64):
                                                row = lane % M
                                                co, ci = (row % 8 if pym else mb * M + row), ci0 + g * KK + lane // M
                                                pyl = row // 8 if pym else py
                                                t = (kz * 3 + tap_of(pyl, oy)) * 3 + tap_of(px, ox)
                                                src.append((ci * cout + co) * NT + t if co < cout and pyl >= oy else -1)
    return src
