"""Test infrastructure: yardstick, criterion and case tables of the FeatureNet kernels -- K3s (``conv2d_c8_kernel``) and the fused
``conv0_fused_kernel``, K3 in its 2D modes (stride-1 3x3 with kdepth 1, CONV2D_K5S2, CONV2D_K1; the SKIP_UP2 / OUT_Q4 / IN_VIEWS
epilogues and loaders), K3w's three 2D rows and ``fpn_wino_kernel``.  No product code here; tests/test_featurenet_cpu.py checks this
file against ATen, the oracle and the recorded reference outputs, asserts what the tables claim and shows which mistakes the criterion
catches; tests/test_featurenet_gpu.py holds the kernels to it.

Restated from the formulas (reference networks/module.py:274-340), dtype-generic, float64 on the CPU being the yardstick, tap by tap
as shifted-slice sums over a [C,V,H,W] stack (the V views are independent images):

  conv      y[co,v,oy,ox] = sum_{ci,ky,kx} w[co,ci,ky,kx] x[ci,v,s oy + ky - k//2, s ox + kx - k//2], zero outside the image;
            k = 3 / 5 / 1, Ho = (H + 1) // 2 for s = 2; then y * scale + shift and the ReLU.
  up2_add   y[.., i, j] + skip[.., i // 2, j // 2]  (nearest upsample by index).
  fpn_head  conv3x3(b_lat + w_lat . lat + up2(td)): FeatureNet's level-3 merge (module.py:333-336).
  fpn       the whole FeatureNet from a state_dict: three levels, both channel halves of each.
  q4        [C,V,H,W] <-> [2,V,C/8,H,W,4]: two quad-planar halves per view (the DMVS_OUT_Q4 epilogue), channel
            half * C/2 + 4 cq + r at [half, v, cq, y, x, r].

Criterion (the project's, hypotheses_ref.bound_of with warp_corr_ref's errors / bounds): e_max = max|a - f64| / max|f64| and
e_mean = mean|a - f64| / max|f64|, each e_hip <= 8 e_ref, and 16 * 2^-23 where e_ref < 4 * 2^-23.  e_ref is the distance of the same
operation in fp32 on stock ATen on the CPU (``aten_*`` below; oracle.dmvs_oracle.feature_net for the whole net), never of a HIP
kernel.  The Winograd forms get the same, plain bound: ``wino_conv`` below is F(2x2, 3x3) in fp32 with the kernels' transforms, and
the CPU file holds it to the plain criterion on the WINO_2D and FPN inputs."""
import functools

import torch
import torch.nn.functional as F

from hypotheses_ref import bound_of  # noqa: F401  (the criterion's bound; re-exported)
from warp_corr_ref import bounds, errors  # noqa: F401

F64, F32 = torch.float64, torch.float32
BN_EPS = 1e-5
MUTATION_RATIO = 20.0       # a mistake counts as caught when it is this many times over bound_of(e_ref)
CONV_S1, CONV2D_K5S2, CONV2D_K1 = 0, 3, 4           # include/dmvs.h
PLAN_MBS, PLAN_V4 = 1 << 17, 1 << 16                # dmvs_conv3d_mfma_plan: M-block split, 16-byte tile loader (W % 4 == 0)
HUGE = 1 << 30


# ------------------------------------------------------------------------------------------------ restatement
def conv(x, w, stride=1, scale=None, shift=None, relu=False, dtype=F64, mutation=None, param=None):
    """x [C,V,H,W], w [Co,C,k,k] -> [Co,V,Ho,Wo].  ``mutation`` (with ``param``): one mistake of a kernel, for the CPU file --
    strip_edge      the kx = 0 tap (the left neighbour lane's partial sum) dropped at the first stored pixel of every strip but the
                    first: x = param * s (param 62: K3s, 60: the fused kernel)
    halo_row_zero   the row above a row block (y0 - 1) read as zero: the ky = 0 tap dropped at y = param * b
    view_bleed      row H of view v reads row 0 of view v + 1 (what lies behind it in a [C][V][H][W] stack) instead of zero
    in_views_ch4    a 3-channel image stack read as 4 channels: the fourth is channel 0 of the next view, weighted like channel 2
    k5s2_ho_floor   stride 2 with Ho = H // 2, Wo = W // 2: the last row / column of an odd size never written (left zero)
    k5s2_origin     stride 2: the tap origin one pixel late along an axis of odd size
    bn_shift_after_relu   channel 1's shift added behind the ReLU"""
    x, w = x.to(dtype), w.to(dtype)
    if mutation == "in_views_ch4" and x.shape[0] == 3:
        nxt = torch.zeros_like(x[:1])
        nxt[:, :-1] = x[:1, 1:]
        x, w = torch.cat((x, nxt)), torch.cat((w, w[:, 2:3]), 1)
    C, V, H, W = x.shape
    Co, Ci, k, k2 = w.shape
    assert Ci == C and k == k2 and k in (1, 3, 5) and stride in (1, 2), (x.shape, w.shape, stride)
    p = k // 2
    Ho, Wo = ((H + 1) // 2, (W + 1) // 2) if stride == 2 else (H, W)
    xp = torch.zeros((C, V, H + 2 * p + 2, W + 2 * p + 2), dtype=dtype)     # (two spare rows / columns for k5s2_origin)
    xp[:, :, p:p + H, p:p + W] = x
    if mutation == "view_bleed" and p:
        xp[:, :-1, p + H, p:p + W] = x[:, 1:, 0]
    late = mutation == "k5s2_origin" and stride == 2
    oy, ox = int(late and H % 2 == 1), int(late and W % 2 == 1)
    yy, xx = torch.arange(Ho).view(Ho, 1), torch.arange(Wo)
    out = torch.zeros((Co, V, Ho, Wo), dtype=dtype)
    for ky in range(k):
        for kx in range(k):
            sl = xp[:, :, ky + oy:ky + oy + stride * (Ho - 1) + 1:stride, kx + ox:kx + ox + stride * (Wo - 1) + 1:stride]
            term = torch.einsum("oc,cvhw->ovhw", w[:, :, ky, kx], sl)
            if mutation == "strip_edge" and k == 3 and kx == 0:
                term = term * (xx % param != 0).to(dtype)
            if mutation == "halo_row_zero" and k == 3 and ky == 0:
                term = term * (yy % param != 0).to(dtype)
            out = out + term
    if mutation == "k5s2_ho_floor" and stride == 2:
        out[:, :, H // 2:] = 0
        out[..., W // 2:] = 0
    if scale is not None:
        out = out * scale.to(dtype).view(-1, 1, 1, 1)
    if mutation == "bn_shift_after_relu" and shift is not None and relu:
        sh = shift.to(dtype).clone()
        late_sh = torch.zeros_like(sh)
        late_sh[1], sh[1] = sh[1], 0.0
        return torch.relu(out + sh.view(-1, 1, 1, 1)) + late_sh.view(-1, 1, 1, 1)
    if shift is not None:
        out = out + shift.to(dtype).view(-1, 1, 1, 1)
    return torch.relu(out) if relu else out


def up2_add(y, skip, mutation=None):
    """y [C,V,H,W] + skip [C,V,H/2,W/2] at (i // 2, j // 2).  ``mutation`` up2_round: at ((i + 1) // 2, (j + 1) // 2), clamped."""
    H, W = y.shape[-2:]
    assert tuple(skip.shape[-2:]) == (H // 2, W // 2) and H % 2 == 0 and W % 2 == 0, (y.shape, skip.shape)
    iy, ix = torch.arange(H) // 2, torch.arange(W) // 2
    if mutation == "up2_round":
        iy, ix = ((torch.arange(H) + 1) // 2).clamp(max=H // 2 - 1), ((torch.arange(W) + 1) // 2).clamp(max=W // 2 - 1)
    return y + skip.to(y.dtype)[:, :, iy][..., ix]


def fused_conv0(x, l0, l1, dtype=F64, mutation=None, param=None):
    """conv0.1(conv0.0(x)), x [3,V,H,W], each layer (w, scale, shift) with ReLU.  ``mutation``: mid_unmasked_rows / _cols -- the
    intermediate one row (column) outside the image is conv0.0 EVALUATED there (relu(shift + the taps that still reach the image))
    instead of conv0.1's zero padding; every other name goes to conv0.1 (``conv``)."""
    if mutation in ("mid_unmasked_rows", "mid_unmasked_cols"):
        rows = mutation == "mid_unmasked_rows"
        C, V, H, W = x.shape
        xe = torch.zeros((C, V, H + 2 * rows, W + 2 * (not rows)), dtype=x.dtype)
        xe[:, :, rows:rows + H, (not rows):(not rows) + W] = x
        out = conv(conv(xe, l0[0], 1, l0[1], l0[2], True, dtype), l1[0], 1, l1[1], l1[2], True, dtype)
        return out[:, :, 1:-1] if rows else out[..., 1:-1]
    mid = conv(x, l0[0], 1, l0[1], l0[2], True, dtype)
    return conv(mid, l1[0], 1, l1[1], l1[2], True, dtype, mutation, param)


def fpn_head(lat, td, w_lat, b_lat, w3, dtype=F64, mutation=None):
    """lat [8,V,H,W], td [32,V,H/2,W/2], w_lat [32,8], b_lat [32], w3 [16,32,3,3] -> [16,V,H,W].  ``mutation``: bias_dropped;
    bias_leak (the lateral bias also on the ring that is out3's zero padding: a ones plane that is non-zero outside the image);
    up2_round."""
    intra = conv(lat, w_lat.view(*w_lat.shape[:2], 1, 1), 1, None, None if mutation == "bias_dropped" else b_lat, False, dtype)
    intra = up2_add(intra, td.to(dtype), mutation)
    if mutation == "bias_leak":
        C, V, H, W = intra.shape
        ring = b_lat.to(dtype).view(-1, 1, 1, 1).expand(C, V, H + 2, W + 2).clone()
        ring[:, :, 1:-1, 1:-1] = intra
        return conv(ring, w3, dtype=dtype)[:, :, 1:-1, 1:-1]
    return conv(intra, w3, dtype=dtype)


def planar_to_q4(p):
    """[C,V,H,W] -> [2,V,C/8,H,W,4]."""
    C, V, H, W = p.shape
    return p.view(2, C // 8, 4, V, H, W).permute(0, 3, 1, 4, 5, 2).contiguous()


def q4_halves_to_planar(o, mutation=None):
    """[2,V,Cq,H,W,4] (the DMVS_OUT_Q4 epilogue: two quad-planar halves per view) -> [2 * Cq * 4,V,H,W].  ``mutation``:
    q4_halves_swapped; q4_perm (channel 4 k + r read at 4 k + (r + 1) % 4)."""
    if mutation == "q4_halves_swapped":
        o = o.flip(0)
    if mutation == "q4_perm":
        o = o[..., [1, 2, 3, 0]]
    halves = [h.permute(1, 4, 0, 2, 3).reshape(-1, h.shape[0], h.shape[2], h.shape[3]) for h in o]
    return torch.cat(halves, 0)


FEATURE_CBR = (("conv0.0", 1), ("conv0.1", 1), ("conv1.0", 2), ("conv1.1", 1), ("conv1.2", 1), ("conv2.0", 2), ("conv2.1", 1),
               ("conv2.2", 1))


def folded(sd, name, dtype=F64, p="feature"):
    """(w, scale, shift) of a conv + eval-mode BatchNorm of the state_dict, folded in ``dtype``."""
    g = lambda k: sd[f"{p}.{name}.bn.{k}"].to(dtype)  # noqa: E731
    scale = g("weight") / torch.sqrt(g("running_var") + BN_EPS)
    return sd[f"{p}.{name}.conv.weight"], scale, g("bias") - g("running_mean") * scale


def fpn(sd, imgs, dtype=F64, mutation=None, p="feature"):
    """The whole FeatureNet (module.py:274-340): imgs [V,3,H,W] -> [o1 [64,V,H/4,W/4], o2 [32,V,H/2,W/2], o3 [16,V,H,W]], the first
    half of each level's channels being stageK, the second stageK_c.  ``mutation`` goes to the level-3 merge."""
    x = imgs.permute(1, 0, 2, 3).to(dtype)
    c = {}
    for name, stride in FEATURE_CBR:
        w, scale, shift = folded(sd, name, dtype, p)
        x = conv(x, w, stride, scale, shift, True, dtype)
        c[name] = x
    c0, c1, c2 = c["conv0.1"], c["conv1.2"], c["conv2.2"]
    o1 = conv(c2, sd[f"{p}.out1.weight"], dtype=dtype)
    intra = up2_add(conv(c1, sd[f"{p}.inner1.weight"], shift=sd[f"{p}.inner1.bias"], dtype=dtype), c2)
    o2 = conv(intra, sd[f"{p}.out2.weight"], dtype=dtype)
    w_lat = sd[f"{p}.inner2.weight"]
    o3 = fpn_head(c0, intra, w_lat.reshape(w_lat.shape[0], -1), sd[f"{p}.inner2.bias"], sd[f"{p}.out3.weight"], dtype, mutation)
    return [o1, o2, o3]


def oracle_fpn(sd, imgs):
    """The fp32 oracle (ATen on the CPU) in ``fpn``'s output form."""
    from oracle import dmvs_oracle as O
    o = O.feature_net(sd, imgs)
    return [torch.cat((o[f"stage{k}"], o[f"stage{k}_c"]), 1).permute(1, 0, 2, 3).contiguous() for k in (1, 2, 3)]


# ------------------------------------------------------------------------------------------------ fp32 ATen (e_ref)
def aten_conv(x, w, stride=1, scale=None, shift=None, relu=False, dtype=F32):
    y = F.conv2d(x.to(dtype).permute(1, 0, 2, 3), w.to(dtype), None, stride, w.shape[-1] // 2)
    if scale is not None:
        y = y * scale.to(dtype).view(1, -1, 1, 1)
    if shift is not None:
        y = y + shift.to(dtype).view(1, -1, 1, 1)
    return (torch.relu(y) if relu else y).permute(1, 0, 2, 3).contiguous()


def aten_up2_add(y, skip):
    up = F.interpolate(skip.permute(1, 0, 2, 3), scale_factor=2, mode="nearest").permute(1, 0, 2, 3)
    return y + up.to(y.dtype)


def aten_fused_conv0(x, l0, l1, dtype=F32):
    return aten_conv(aten_conv(x, l0[0], 1, l0[1], l0[2], True, dtype), l1[0], 1, l1[1], l1[2], True, dtype)


def aten_fpn_head(lat, td, w_lat, b_lat, w3, dtype=F32):
    intra = aten_up2_add(aten_conv(lat, w_lat.view(*w_lat.shape[:2], 1, 1), shift=b_lat, dtype=dtype), td.to(dtype))
    return aten_conv(intra, w3, dtype=dtype)


# ------------------------------------------------------------------------------------------------ F(2x2, 3x3) in fp32
def _bt4(d0, d1, d2, d3):
    return d0 - d2, d1 + d2, d2 - d1, d1 - d3


def wino_conv(x, w, dtype=F32):
    """Stride-1 3x3 conv as Winograd F(2x2, 3x3) the way K3w forms it: filters U = G g G^T in float64 on the host, rounded once;
    patches V = B^T d B, products accumulated over the channels per transform position, outputs A^T M A -- everything behind the
    filter transform in ``dtype``.  x [C,V,H,W], w [Co,C,3,3] -> [Co,V,H,W]."""
    C, V, H, W = x.shape
    He, We = H + H % 2, W + W % 2
    xp = torch.zeros((C, V, He + 2, We + 2), dtype=dtype)
    xp[:, :, 1:1 + H, 1:1 + W] = x.to(dtype)
    G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=F64)
    U = torch.einsum("ai,ocij,bj->ocab", G, w.to(F64), G).to(dtype)
    d = [[xp[:, :, i:i + He - 1:2, j:j + We - 1:2] for j in range(4)] for i in range(4)]
    cols = [_bt4(d[0][j], d[1][j], d[2][j], d[3][j]) for j in range(4)]          # cols[j][a]
    Vt = [_bt4(cols[0][a], cols[1][a], cols[2][a], cols[3][a]) for a in range(4)]   # Vt[a][b]
    M = [[torch.einsum("oc,cvhw->ovhw", U[:, :, a, b], Vt[a][b]) for b in range(4)] for a in range(4)]
    rows = [[M[0][b] + M[1][b] + M[2][b], M[1][b] - M[2][b] - M[3][b]] for b in range(4)]   # rows[b][r]
    out = torch.zeros((w.shape[0], V, He, We), dtype=dtype)
    for r in range(2):
        out[:, :, r::2, 0::2] = rows[0][r] + rows[1][r] + rows[2][r]
        out[:, :, r::2, 1::2] = rows[1][r] - rows[2][r] - rows[3][r]
    return out[:, :, :H, :W]


def wino_fpn_head(lat, td, w_lat, b_lat, w3, dtype=F32):
    """fpn_wino_kernel's form: ONE Winograd convolution over the 8 lateral channels and a constant-one plane, with the composite
    filters w3 o w_lat and w3 . b_lat (folded in float64 on the host), and the 32 upsampled top-down channels with w3."""
    comp = torch.einsum("oikl,ic->ockl", w3.to(F64), torch.cat((w_lat.to(F64), b_lat.to(F64).view(-1, 1)), 1))
    iy, ix = torch.arange(lat.shape[-2]) // 2, torch.arange(lat.shape[-1]) // 2
    x = torch.cat((lat, torch.ones_like(lat[:1]), td[:, :, iy][..., ix]))
    return wino_conv(x, torch.cat((comp, w3.to(F64)), 1), dtype)


# ------------------------------------------------------------------------------------------------ inputs
KINDS = ("normal", "relu")


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def make_input(kind, C, V, H, W, seed=0):
    """fp32 [C,V,H,W]: seeded normal, or the post-ReLU-like |N(0,1)| + 1."""
    x = torch.randn((C, V, H, W), generator=_gen(1, seed, C, V, H, W))
    return x if kind == "normal" else x.abs() + 1.0


def make_weight(cout, cin, k, seed=0):
    return torch.randn((cout, cin, k, k), generator=_gen(2, seed, cout, cin, k)) * (1.0 / (cin * k * k) ** 0.5)


def make_bn(cout, seed=0):
    """Folded BatchNorm as tests/test_gpu_parity.py::_layer draws it: scale in 0.5 .. 1.5, shift 0.2 N(0,1)."""
    g = _gen(3, seed, cout)
    return 0.5 + torch.rand(cout, generator=g), 0.2 * torch.randn(cout, generator=g)


def kind_of(*shape):
    """The input kind of a case: alternating over the tables, fixed by the shape."""
    return KINDS[sum(shape) % 2]


# ------------------------------------------------------------------------------------------------ case tables
# K3s.  c8_rows values; R = the value rounded up to a multiple of 4, 0 = the launcher's own choice, which is 8 at these sizes
C8_ROWS = (0, 4, 12, 20, 32)
STRIP, STRIPF, C8_NS = 62, 60, 4        # csrc/conv2d_c8.hip
# (V, H, W).  The issue's eight shapes and (1,22,3): with them alone no H is two rows into a last block (see c8_seam_classes)
C8_SHAPES = ((1, 1, 1), (1, 3, 2), (2, 5, 61), (1, 9, 62), (2, 13, 63), (3, 21, 124), (1, 23, 125), (2, 33, 187), (1, 22, 3))
FUSED_W = (1, 2, 59, 60, 61, 62, 119, 120, 121, 181)
C8_SEAM_CLASSES = ("H<R", "H=R+1", "H=2R+9", "last+1", "last+2")


def c8_rows_of(value, V, H, W, strip=STRIP):
    """R of csrc/conv2d_c8.hip::c8_rows for dmvs_tune("c8_rows") = value (restated: the library exports no plan for K3s)."""
    nstrips = -(-W // strip)
    if value > 0:
        return -(-value // C8_NS) * C8_NS
    slots, sv, R = 256 * 4 * 2, nstrips * V, 32
    for k in range(1, 17):
        n = k * slots // sv
        if n < 1:
            continue
        r = -(-H // n)
        if r <= 24:
            R = max(r, 8)
            break
    return -(-R // C8_NS) * C8_NS


def c8_seam_classes(R, H):
    out = set()
    if H < R:
        out.add("H<R")
    if H == R + 1:
        out.add("H=R+1")
    if H == 2 * R + 9:
        out.add("H=2R+9")
    if H > R and H % R == 1:
        out.add("last+1")
    if H > R and H % R == 2:
        out.add("last+2")
    return out


def fused_vh():
    """(V, H) of the fused kernel's cases: those of C8_SHAPES, one per H; each runs at every width of FUSED_W."""
    seen = {}
    for V, H, _ in C8_SHAPES:
        seen.setdefault(H, V)
    return tuple((V, H) for H, V in seen.items())


# K3 2D.  One entry per FeatureNet row of kCfgs (csrc/conv3d_mfma.hip:830-840): name -> (cin, cout, mode, k, MB)
K3_ROWS = {
    "conv0.0": (4, 8, CONV_S1, 3, 1), "conv0.1": (8, 8, CONV_S1, 3, 1), "conv1.0": (8, 16, CONV2D_K5S2, 5, 1),
    "conv1.x": (16, 16, CONV_S1, 3, 1), "conv2.0": (16, 32, CONV2D_K5S2, 5, 1), "conv2.x": (32, 32, CONV_S1, 3, 1),
    "out3": (32, 16, CONV_S1, 3, 1), "out1": (32, 64, CONV2D_K1, 1, 2), "inner1": (16, 32, CONV2D_K1, 1, 1),
    "inner2": (8, 32, CONV2D_K1, 1, 1),
}
# tile form -> (k3_min_blocks, k3_split_blocks); None = the library default (768 / 1024)
K3_KNOBS = {"big": (0, None), "small": (HUGE, 0), "default": (None, None)}
K3_DEFAULTS = {"k3_min_blocks": 768, "k3_split_blocks": 1024}
K3_S1_SHAPES = ((2, 17, 36), (1, 15, 33), (2, 33, 30), (3, 4, 68), (1, 1, 1))
K3_K5S2_SHAPES = ((2, 18, 70), (1, 17, 67), (2, 33, 130), (1, 5, 8), (1, 2, 3))
K3_K5S2_OUT = ((9, 35), (9, 34), (17, 65), (3, 4), (1, 2))
K3_SKIP_SHAPES = ((2, 18, 36), (1, 34, 68), (3, 4, 72))


def k3_forms(name):
    """The tile forms of a row: big and plain small; `default` as well where it is a third one (out1, the only MB = 2 row)."""
    return ("big", "small", "default") if K3_ROWS[name][4] == 2 else ("big", "small")


def k3_expected_plan(name, form):
    """(TZ, TY, split bit) under K3_KNOBS[form] at every shape of the tables (they all stay under 768 big-tile workgroups)."""
    stride = 2 if K3_ROWS[name][2] == CONV2D_K5S2 else 1
    if form == "big":
        return (1, 16 if stride == 1 else 8, 0)
    if form == "default" and K3_ROWS[name][4] == 2:
        return (1, 2, 1)
    return (1, 4, 0)


def k3_shapes(name):
    return K3_K5S2_SHAPES if K3_ROWS[name][2] == CONV2D_K5S2 else K3_S1_SHAPES


def k3_2d_cases():
    """[(row, (V, H, W))] of K3_2D; the forms (k3_forms) and epilogues (planar; OUT_Q4 where cout % 8 == 0; IN_VIEWS on conv0.0) of
    a row run on one input."""
    return [(name, s) for name in K3_ROWS for s in k3_shapes(name)]


def k3_skip_cases():
    return [(name, s) for name in ("out1", "inner1", "inner2") for s in K3_SKIP_SHAPES]


# K3w 2D.  The kdepth = 1 rows of kWCfgs (csrc/conv3d_wino.hip): name -> (cin, cout, rows of a workgroup's tile)
WINO_ROWS = {"conv1.x": (16, 16, 16), "conv2.x": (32, 32, 8), "out3": (32, 16, 16)}
WINO_BN = {"conv1.x": True, "conv2.x": True, "out3": False}      # folded BN + ReLU as FeatureNet's layers of that shape carry them
WINO_SHAPES = ((1, 1, 4), (2, 17, 36), (3, 9, 100), (1, 31, 68))
# tile rows -> the shapes whose plan exceeds the persistent grid: the issue's (8 x 7 x 11 = 616 tiles, a multiple of 8) and one of
# 7 x 7 x 11 = 539 tiles, where the XCDs' eighths are not all full (539 % 8 = 3)
WINO_MULTI = {16: ((11, 98, 228), (11, 98, 196)), 8: ((11, 50, 228), (11, 50, 196))}
# launch_wino: `const unsigned resident = 256u * (unsigned)std::max<size_t>(1, std::min<size_t>(2, (160 * 1024) / lds));` and
# `grid = std::min(xcd_grid(a.nx * a.ny * a.nz), g_wino_persistent ? resident : 0xffffffffu)`: at most 2 x 256 workgroups
WINO_RESIDENT = 512


def wino_cases():
    return [(name, s) for name, (_, _, ty) in WINO_ROWS.items() for s in WINO_SHAPES + WINO_MULTI[ty]]


def wino_tiles(name, V, H, W):
    ty = WINO_ROWS[name][2]
    return -(-W // 32) * -(-H // ty) * V


# fpn_wino_kernel: tiles of 16 rows x 32 columns, grid min(xcd_grid(tiles), 256)
FPN_SHAPES = ((1, 2, 8), (2, 18, 40), (1, 34, 72), (3, 30, 104), (9, 82, 168))
FPN_DECLINED = ((1, 9, 16), (1, 8, 36), (2, 17, 44))     # H odd, W % 8 == 4, both
FPN_GRID = 256


def fpn_tiles(V, H, W):
    return -(-W // 32) * -(-H // 16) * V


# whole net, (V, H, W) with H % 4 == W % 4 == 0
NET_SHAPES = ((2, 36, 72), (1, 20, 44), (3, 64, 136))


def net_level3_fused(H, W):
    """dmvs_conv3d_wino_fpn2 takes the level-3 merge: `if ((H & 1) || (W & 7)) return DMVS_EUNSUPPORTED`."""
    return H % 2 == 0 and W % 8 == 0


# mistake -> the table that must catch it
MUTATIONS = {
    "strip_edge": "C8", "halo_row_zero": "C8", "view_bleed": "C8", "bn_shift_after_relu": "C8",
    "strip_edge_fused": "FUSED", "halo_row_zero_fused": "FUSED", "mid_unmasked_rows": "FUSED", "mid_unmasked_cols": "FUSED",
    "in_views_ch4": "K3_2D", "k5s2_ho_floor": "K3_2D", "k5s2_origin": "K3_2D", "q4_halves_swapped": "K3_2D", "q4_perm": "K3_2D",
    "up2_round": "K3_SKIP",
    "bias_leak": "FPN", "bias_dropped": "FPN", "up2_round_fpn": "FPN",
}


# ------------------------------------------------------------------------------------------------ cases and references
@functools.lru_cache(maxsize=None)
def conv_case(cin, cout, k, V, H, W, bn=True, seed=0):
    """(x [cin,V,H,W], w, scale, shift): the input kind by the shape; folded BN + ReLU where ``bn``."""
    x = make_input(kind_of(V, H, W), cin, V, H, W, seed)
    scale, shift = make_bn(cout, seed) if bn else (None, None)
    return x, make_weight(cout, cin, k, seed), scale, shift


@functools.lru_cache(maxsize=None)
def conv_reference(cin, cout, k, stride, V, H, W, bn=True, seed=0):
    """(float64 yardstick, (e_max, e_mean) of fp32 ATen) of a conv case; computed once, never modified."""
    x, w, scale, shift = conv_case(cin, cout, k, V, H, W, bn, seed)
    f64 = conv(x, w, stride, scale, shift, bn)
    return f64, errors(aten_conv(x, w, stride, scale, shift, bn), f64)


@functools.lru_cache(maxsize=None)
def fused_case(V, H, W):
    """(x [3,V,H,W], l0, l1): the image stack (channel-major) and the two layers (w, scale, shift)."""
    x = make_input(kind_of(V, H, W), 3, V, H, W, seed=5)
    return x, (make_weight(8, 3, 3, 5),) + make_bn(8, 5), (make_weight(8, 8, 3, 6),) + make_bn(8, 6)


@functools.lru_cache(maxsize=None)
def fused_reference(V, H, W):
    x, l0, l1 = fused_case(V, H, W)
    f64 = fused_conv0(x, l0, l1)
    return f64, errors(aten_fused_conv0(x, l0, l1), f64)


@functools.lru_cache(maxsize=None)
def skip_case(cin, cout, V, H, W):
    """A CONV2D_K1 case with bias (scale 1, as FeatureNet packs inner1 / inner2) and a half-resolution residual."""
    x = make_input(kind_of(V, H, W), cin, V, H, W, seed=7)
    return x, make_weight(cout, cin, 1, 7), torch.ones(cout), make_bn(cout, 7)[1], make_input("normal", cout, V, H // 2, W // 2, seed=8)


@functools.lru_cache(maxsize=None)
def skip_reference(cin, cout, V, H, W):
    x, w, scale, shift, sk = skip_case(cin, cout, V, H, W)
    f64 = up2_add(conv(x, w, 1, scale, shift), sk)
    return f64, errors(aten_up2_add(aten_conv(x, w, 1, scale, shift), sk), f64)


@functools.lru_cache(maxsize=None)
def fpn_case(V, H, W):
    """(lat [8,V,H,W], td [32,V,H/2,W/2], w_lat [32,8], b_lat [32], w3 [16,32,3,3]); lat and td post-ReLU-like or normal by shape."""
    kind = kind_of(V, H, W)
    return (make_input(kind, 8, V, H, W, seed=9), make_input(kind, 32, V, H // 2, W // 2, seed=10),
            make_weight(32, 8, 1, 9).view(32, 8), make_bn(32, 9)[1], make_weight(16, 32, 3, 9))


@functools.lru_cache(maxsize=None)
def fpn_reference(V, H, W):
    c = fpn_case(V, H, W)
    f64 = fpn_head(*c)
    return f64, errors(aten_fpn_head(*c), f64)


FEATURE_SHAPES = {"conv0.0": (8, 3, 3), "conv0.1": (8, 8, 3), "conv1.0": (16, 8, 5), "conv1.1": (16, 16, 3), "conv1.2": (16, 16, 3),
                  "conv2.0": (32, 16, 5), "conv2.1": (32, 32, 3), "conv2.2": (32, 32, 3)}
FEATURE_PLAIN = {"out1": (64, 32, 1, False), "inner1": (32, 16, 1, True), "inner2": (32, 8, 1, True), "out2": (32, 32, 3, False),
                 "out3": (16, 32, 3, False)}


@functools.lru_cache(maxsize=None)
def net_state_dict(seed=0, p="feature"):
    """A FeatureNet state_dict (the reference's keys) that keeps activations of order one through the eleven layers: conv weights
    N(0, 2 / fan_in), BN weight 0.5 .. 1.5, bias and running_mean 0.1 N, running_var 0.5 .. 1.5, lateral biases 0.1 N."""
    sd = {}
    for name, (co, ci, k) in FEATURE_SHAPES.items():
        g = _gen(4, seed, co, ci, k, len(sd))
        sd[f"{p}.{name}.conv.weight"] = torch.randn((co, ci, k, k), generator=g) * (2.0 / (ci * k * k)) ** 0.5
        sd[f"{p}.{name}.bn.weight"] = 0.5 + torch.rand(co, generator=g)
        sd[f"{p}.{name}.bn.bias"] = 0.1 * torch.randn(co, generator=g)
        sd[f"{p}.{name}.bn.running_mean"] = 0.1 * torch.randn(co, generator=g)
        sd[f"{p}.{name}.bn.running_var"] = 0.5 + torch.rand(co, generator=g)
        sd[f"{p}.{name}.bn.num_batches_tracked"] = torch.zeros((), dtype=torch.int64)
    for name, (co, ci, k, bias) in FEATURE_PLAIN.items():
        g = _gen(5, seed, co, ci, k, len(sd))
        sd[f"{p}.{name}.weight"] = torch.randn((co, ci, k, k), generator=g) * (1.0 / (ci * k * k)) ** 0.5
        if bias:
            sd[f"{p}.{name}.bias"] = 0.1 * torch.randn(co, generator=g)
    return sd


@functools.lru_cache(maxsize=None)
def net_images(V, H, W):
    return torch.rand((V, 3, H, W), generator=_gen(6, V, H, W))


def halves(t):
    """The stageK / stageK_c channel halves of a level."""
    return t[:t.shape[0] // 2], t[t.shape[0] // 2:]


@functools.lru_cache(maxsize=None)
def net_reference(V, H, W):
    """([three float64 levels], [per level: ((e_max, e_mean) of the fp32 oracle on stageK, the same on stageK_c)])."""
    sd, imgs = net_state_dict(), net_images(V, H, W)
    f64 = fpn(sd, imgs)
    return f64, [tuple(errors(a, b) for a, b in zip(halves(o), halves(y))) for o, y in zip(oracle_fpn(sd, imgs), f64)]
