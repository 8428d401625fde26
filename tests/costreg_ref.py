"""Test infrastructure: yardstick, criterion, launch table and case tables of the two regularisation networks as WHOLE networks --
``CostRegNet.run`` / ``CostRegNet._branch`` (dmvsnet_amd/mvsnet.py), the host code that chains K3w / K3z / K3r / K3 / K2 and the fused
``prob`` head into the two U-Nets of a pass.  No product code here; tests/test_costreg_cpu.py checks this file against the oracle in
float64, asserts what the tables claim and shows which mistakes the criterion catches; tests/test_costreg_gpu.py holds the networks
to it.

Restated from the formulas (reference networks/module.py:342-436), independently of the product and of the oracle:

  net_f64     eval-mode CostRegNet / CostRegNet_refine in float64: the convolutions of tests/regconv_ref.py (padded copy, strided
              slices, einsum; the transposed ones as a scatter), BatchNorm written out from the running statistics in float64
              (never folded in fp32), the ReLU in FRONT of the skip addition, the refine net's conv5 / conv6 / conv7 as 2D layers on
              the single plane, the branches concatenated small, huge.
  heads_f64   the softmax expectation over D of each of the four channels in float64: what ops.prob_regress writes.

Criterion (the project's, featurenet_ref.errors / bounds): e_max = max|a - f64| / max|f64| and e_mean = mean|a - f64| / max|f64|,
each e_hip <= 8 e_ref, and 16 * 2^-23 where e_ref < 4 * 2^-23.  e_ref is the distance of the fp32 oracle (oracle.dmvs_oracle.cost_reg,
stock ATen on the CPU; ``_expectation`` of its logits for the heads), never of a HIP kernel.

``expected_launches`` restates which C entry every layer of a run goes to from the rules of dmvsnet_amd/ops.py (_FORMS, conv3d) and
the entries' argument checks (csrc/conv3d_wino.hip, conv3d_zmarch.hip, conv3d_coarse.hip) -- by reading them, not by calling them."""
import functools

import torch

from featurenet_ref import MUTATION_RATIO, bound_of, bounds, errors  # noqa: F401  (the criterion; re-exported)
from regconv_ref import conv3d, deconv3d

F64, F32 = torch.float64, torch.float32
BN_EPS = 1e-5
EUNSUPPORTED = -2                                     # include/dmvs.h
ZMARCH_MIN_DEPTH = 8                                  # dmvsnet_amd/ops.py
PROB_FUSED_DEPTHS = (4, 8)                            # dmvsnet_amd/ops.py
BRANCHES = ("small", "huge")
# the tensors of a branch a failing network test is located by: conv0's half, the two skips, the three up-path sums
LEVEL_KEYS = ("conv0", "c2", "c4", "y7", "y9", "y11")
PREFIX = {False: "cost_regularization.0", True: "cost_regularization_refine.0"}
ALPHA = {False: 1.0, True: 5.0}                       # DepthNet.forward / DepthNet.refine (mvsnet.py:19-20,68-69)


# ------------------------------------------------------------------------------------------------ restatement
def _bn(sd, p, y, dtype):
    """Eval-mode BatchNorm from the running statistics, in ``dtype``: (y - mean) / sqrt(var + eps) * weight + bias."""
    g = lambda k: sd[f"{p}.bn.{k}"].to(dtype).view(-1, 1, 1, 1)  # noqa: E731
    return (y - g("running_mean")) / torch.sqrt(g("running_var") + BN_EPS) * g("weight") + g("bias")


def _w5(w):
    """A 2D weight [a,b,3,3] as the kdepth-1 form [a,b,1,3,3] of regconv_ref."""
    return w.unsqueeze(2) if w.dim() == 4 else w


def _cbr(sd, p, x, stride, dtype):
    w = _w5(sd[p + ".conv.weight"])
    return torch.relu(_bn(sd, p, conv3d(x, w, stride, w.shape[2], dtype=dtype), dtype))


def _dbr(sd, p, x, skip, dtype, before_relu=False):
    """Transposed conv + BN + ReLU, then + skip (module.py:394-396: ``conv4 + self.conv7(x)``)."""
    w = _w5(sd[p + ".conv.weight"])
    y = _bn(sd, p, deconv3d(x, w, w.shape[2], dtype=dtype), dtype)
    if skip is None:
        return torch.relu(y)
    skip = skip.to(dtype)
    return torch.relu(y + skip) if before_relu else torch.relu(y) + skip


def _stride1_on_plane(sd, p, x, dtype, mutation):
    """A stride-1 3x3x3 layer on a level that may be one plane deep.  The product then runs the middle 3x3 slice as a 2D layer
    (``@d1``); ``mutation`` d1_slice0 builds that layer from depth slice 0."""
    w = sd[p + ".conv.weight"]
    if mutation == "d1_slice0" and w.dim() == 5 and x.shape[1] == 1:
        return torch.relu(_bn(sd, p, conv3d(x, w[:, :, 0:1], 1, 1, dtype=dtype), dtype))
    return _cbr(sd, p, x, 1, dtype)


def _bottleneck_wrong_tap(sd, p, x, stride, dtype):
    """A 2D layer of the refine bottleneck run as 3D with zero planes around the single plane and its filter at depth tap 0: the
    tap meets the padding plane only."""
    w = sd[p + ".conv.weight"]
    w3 = torch.zeros((w.shape[0], w.shape[1], 3, 3, 3), dtype=w.dtype)
    w3[:, :, 0] = w
    return torch.relu(_bn(sd, p, conv3d(x, w3, stride, 3, dtype=dtype), dtype))


def net_f64(sd, prefix, x, refine, keys=None, dtype=F64, mutation=None):
    """x [2,D,H,W] -> logits [4,D,H,W] (cat(small, huge)); with ``keys`` (an iterable of "<branch>.<LEVEL_KEYS name>", or True for all)
    also a dict of those intermediates.  ``mutation``: one mistake of the host code that chains the layers, for the CPU file --
    small_reads_huge_c2   the small branch's up-path adds the huge branch's c2
    conv0_halves_swapped  each branch runs on the other's half of the fused conv0
    d1_slice0             the 2D form of a stride-1 layer on a one-plane level built from depth slice 0 instead of 1
    skip_before_relu      the three skips added in front of the ReLU
    skip_dropped          conv9's skip left out
    refine_bottleneck_3d  the refine net's conv5 / conv6 run as 3D on a zero-padded plane with the filter at depth tap 0"""
    x = x.to(dtype)
    assert x.dim() == 4 and x.shape[0] == 2, x.shape
    t = {}
    for b in BRANCHES:
        t[f"{b}.conv0"] = _cbr(sd, f"{prefix}.cosR_{b}.conv0", x, 1, dtype)
    if mutation == "conv0_halves_swapped":
        t["small.conv0"], t["huge.conv0"] = t["huge.conv0"], t["small.conv0"]
    for b in BRANCHES:
        p = f"{prefix}.cosR_{b}"
        t[f"{b}.c2"] = _stride1_on_plane(sd, p + ".conv2", _cbr(sd, p + ".conv1", t[f"{b}.conv0"], 2, dtype), dtype, mutation)
        t[f"{b}.c4"] = _stride1_on_plane(sd, p + ".conv4", _cbr(sd, p + ".conv3", t[f"{b}.c2"], 2, dtype), dtype, mutation)
    before = mutation == "skip_before_relu"
    out = []
    for b in BRANCHES:
        p = f"{prefix}.cosR_{b}"
        c4 = t[f"{b}.c4"]
        if refine:
            assert c4.shape[1] == 1 and sd[p + ".conv5.conv.weight"].dim() == 4, "the refine bottleneck is 2D on a single plane"
        if refine and mutation == "refine_bottleneck_3d":
            y = _bottleneck_wrong_tap(sd, p + ".conv6", _bottleneck_wrong_tap(sd, p + ".conv5", c4, 2, dtype), 1, dtype)
        else:
            y = _stride1_on_plane(sd, p + ".conv6", _cbr(sd, p + ".conv5", c4, 2, dtype), dtype, mutation)
        c2 = t["huge.c2"] if (mutation == "small_reads_huge_c2" and b == "small") else t[f"{b}.c2"]
        t[f"{b}.y7"] = _dbr(sd, p + ".conv7", y, c4, dtype, before)
        t[f"{b}.y9"] = _dbr(sd, p + ".conv9", t[f"{b}.y7"], None if mutation == "skip_dropped" else c2, dtype, before)
        t[f"{b}.y11"] = _dbr(sd, p + ".conv11", t[f"{b}.y9"], t[f"{b}.conv0"], dtype, before)
        out.append(conv3d(t[f"{b}.y11"], sd[p + ".prob.weight"], 1, 3, dtype=dtype))
    logits = torch.cat(out, 0)
    if keys is None:
        return logits
    return logits, (dict(t) if keys is True else {k: t[k] for k in keys})


def heads_f64(logits, planes, alpha):
    """logits [4,D,H,W], ``planes`` a [D,H,W] volume or (base [H,W], interval): plane d = base + d * interval -> [4,H,W], the softmax
    expectation over D of every channel, in float64."""
    z = logits.to(F64) * float(alpha)
    D = z.shape[1]
    if isinstance(planes, (tuple, list)):
        base, interval = planes
        step = interval.to(F64).reshape(()) if torch.is_tensor(interval) else torch.tensor(float(interval), dtype=F64)
        planes = base.to(F64)[None] + torch.arange(D, dtype=F64).view(-1, 1, 1) * step
    planes = planes.to(F64)
    assert tuple(planes.shape) == tuple(z.shape[1:]), (planes.shape, z.shape)
    e = torch.exp(z - z.max(1, keepdim=True)[0])
    return (e * planes[None]).sum(1) / e.sum(1)


# ------------------------------------------------------------------------------------------------ fp32 oracle (e_ref)
def oracle_net(sd, prefix, x, refine, keys=False):
    """oracle.dmvs_oracle.cost_reg on the CPU, in the dtype of ``sd`` / ``x``: logits [4,D,H,W]; with ``keys`` also the branch
    intermediates, formed with the oracle's own layer functions in the order of its cost_reg_branch / _refine."""
    from oracle import dmvs_oracle as O
    xb = x[None]
    logits = O.cost_reg(sd, prefix, xb, refine)[0]
    if not keys:
        return logits
    t = {}
    for b in BRANCHES:
        p = f"{prefix}.cosR_{b}"
        c0 = O._cbr3(sd, p + ".conv0", xb, 1)
        c2 = O._cbr3(sd, p + ".conv2", O._cbr3(sd, p + ".conv1", c0, 2), 1)
        c4 = O._cbr3(sd, p + ".conv4", O._cbr3(sd, p + ".conv3", c2, 2), 1)
        if refine:
            c4s = c4.squeeze(2)
            y7 = (c4s + O._dbr2(sd, p + ".conv7", O._cbr2(sd, p + ".conv6", O._cbr2(sd, p + ".conv5", c4s, 2, 1), 1, 1))).unsqueeze(2)
        else:
            y7 = c4 + O._dbr3(sd, p + ".conv7", O._cbr3(sd, p + ".conv6", O._cbr3(sd, p + ".conv5", c4, 2), 1))
        y9 = c2 + O._dbr3(sd, p + ".conv9", y7)
        y11 = c0 + O._dbr3(sd, p + ".conv11", y9)
        for k, v in zip(LEVEL_KEYS, (c0, c2, c4, y7, y9, y11)):
            t[f"{b}.{k}"] = v[0]
    return logits, t


def oracle_heads(logits32, planes32, alpha):
    """oracle._expectation on fp32 logits [4,D,H,W] and an fp32 plane volume -> [4,H,W]."""
    from oracle import dmvs_oracle as O
    return O._expectation(logits32[None], planes32[None], float(alpha))[1][0]


# ------------------------------------------------------------------------------------------------ recipe
SEED = 0
DEPTH_MIN = 425.0
# The DTU planes 425 + 2.65 d, the interval rounded to a multiple of 2^-10 (2.650390625): d * interval and 425 + d * interval are
# then exact in fp32 for every d < 8, however the sum is formed (fused or not) -- the affine form and the materialised volume are the
# same planes to the bit, in fp32 and in float64.
INTERVAL = round(2.5 * 1.06 * 1024) / 1024


def _gen(*key):
    s = 0
    for k in key:
        s = (s * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


@functools.lru_cache(maxsize=None)
def state_dict(seed=SEED):
    """synth.synth_state_dict on an MVSNet([8], [4]) template: the reference's keys, the project's non-degenerate recipe."""
    from dmvsnet_amd import MVSNet, synth
    return synth.synth_state_dict(MVSNet([8], [4], verbose=False).state_dict(), seed)


@functools.lru_cache(maxsize=None)
def sim_volume(refine, D, H, W):
    """fp32 [2,D,H,W], similarity-like: uniform in [-0.5, 1.5] (a group-wise correlation of unit-scale features)."""
    return torch.rand((2, D, H, W), generator=_gen(31, int(refine), D, H, W)) * 2.0 - 0.5


def planes(D, H, W):
    """(base [H,W], interval 0-dim, volume [D,H,W]) in fp32; the volume as ops.AffinePlanes.volume forms it (d * step, then + base)."""
    base = torch.full((H, W), DEPTH_MIN, dtype=F32)
    step = torch.tensor(INTERVAL, dtype=F32)
    return base, step, base[None] + torch.arange(D, dtype=F32).view(-1, 1, 1) * step


@functools.lru_cache(maxsize=None)
def reference(refine, D, H, W):
    """dict: f64 (logits), levels (float64 intermediates), e_ref, levels_e_ref (per intermediate), oracle32 (the fp32 oracle's
    logits); computed once, never modified."""
    sd, x = state_dict(), sim_volume(refine, D, H, W)
    f64, levels = net_f64(sd, PREFIX[refine], x, refine, keys=True)
    o32, olev = oracle_net(sd, PREFIX[refine], x, refine, keys=True)
    return dict(f64=f64, levels=levels, e_ref=errors(o32, f64), oracle32=o32,
                levels_e_ref={k: errors(olev[k], levels[k]) for k in levels})


@functools.lru_cache(maxsize=None)
def heads_reference(refine, D, H, W):
    """(float64 heads [4,H,W] of the yardstick logits, (e_max, e_mean) of the fp32 oracle chain)."""
    r = reference(refine, D, H, W)
    _, _, vol = planes(D, H, W)
    f64 = heads_f64(r["f64"], vol, ALPHA[refine])
    return f64, errors(oracle_heads(r["oracle32"], vol, ALPHA[refine]), f64)


# ------------------------------------------------------------------------------------------------ case tables
# (D, H, W), all multiples of 8, with the claim each shape is there for (tests/test_costreg_cpu.py asserts every one)
FULL_SHAPES = (
    (8, 8, 8),        # the smallest legal volume: one tile column and row per level, conv6 on a single voxel through @d1, head fusable
    (8, 24, 40),      # W/4 = 10, W/8 = 5: K3r's unaligned loader and store; odd extents at the bottom; head fusable
    (16, 16, 48),     # conv2 on depth 8: `auto` takes K3z; conv6 on 2 planes (dead depth taps); head not fusable
    (32, 8, 72),      # conv2 on depth 16; H/8 = 1, W/8 = 9
    (8, 40, 136),     # several tiles per row at full resolution, ragged against 32 / 64 / 128; W/2 = 68, W/4 = 34, W/8 = 17
)
REFINE_SHAPES = (
    (4, 8, 8),        # the smallest
    (4, 24, 40),      # W % 4 != 0 at the two lowest levels (10, 5), odd extents at the lowest (3 x 5)
    (4, 16, 136),     # several tiles, ragged
    (4, 40, 72),      # W/8 = 9; more rows than a row tile
)
SETTINGS = ("auto", "no_zmarch", "no_coarse", "no_wino", "mfma", "direct")
DIRECT_SHAPES = 2     # backend="direct" runs on the two smallest volumes of each table only


def shapes_of(refine):
    return REFINE_SHAPES if refine else FULL_SHAPES


def backend_of(setting):
    return setting if setting in ("mfma", "direct") else "auto"


def switches_of(setting):
    """The ops module switches of a setting (every other one at its default)."""
    return {"use_zmarch": setting != "no_zmarch", "use_coarse": setting != "no_coarse", "use_wino": setting != "no_wino"}


def cases():
    """[(refine, (D, H, W), setting)] of the GPU file."""
    out = []
    for refine in (False, True):
        for i, s in enumerate(shapes_of(refine)):
            out += [(refine, s, st) for st in SETTINGS if st != "direct" or i < DIRECT_SHAPES]
    return out


def fusable(D, W, setting="auto"):
    """ops.prob_fusable with the default switches."""
    return backend_of(setting) in ("auto", "mfma") and D in PROB_FUSED_DEPTHS and W % 4 == 0


def fused_cases():
    return [(refine, s) for refine in (False, True) for s in shapes_of(refine) if fusable(s[0], s[2])]


def levels(refine, D, H, W):
    """The four levels (D, H, W) of a branch: the volume, behind conv1, conv3, conv5.  A stride-2 3D layer halves every axis
    ((n + 1) // 2); the refine net's conv5 is 2D and keeps its single plane."""
    h = lambda n: (n + 1) // 2  # noqa: E731
    l1 = (h(D), h(H), h(W))
    l2 = tuple(h(n) for n in l1)
    l3 = (l2[0] if refine else h(l2[0]), h(l2[1]), h(l2[2]))
    return (D, H, W), l1, l2, l3


def d1_layers(refine, D, H, W):
    """The stride-1 3D layers that run through their ``@d1`` 2D form: those on a level one plane deep (the refine net's conv6 is a
    2D layer already)."""
    lv = levels(refine, D, H, W)
    names = [n for n, l in (("conv2", 1), ("conv4", 2)) if lv[l][0] == 1]
    return names + (["conv6"] if not refine and lv[3][0] == 1 else [])


def _stride1(name, cin, cout, lv, kd, setting, aligned):
    """The launches of one stride-1 3x3 layer, the declined ones first (ops.conv3d walking _FORMS in order)."""
    dims = (cin, cout) + tuple(lv) + (kd,)
    if setting in ("mfma", "direct"):
        return [(f"conv3d_{setting}", dims, 0)]
    sw = switches_of(setting)
    out, v4 = [], lv[2] % 4 == 0 and aligned
    if name == "conv2" and kd == 3 and sw["use_zmarch"] and sw["use_wino"] and lv[0] >= ZMARCH_MIN_DEPTH:
        if v4:
            return [("conv3d_zmarch", dims, 0)]
        out.append(("conv3d_zmarch", dims, EUNSUPPORTED))     # the entry checks W % 4 and the alignment itself
    if name in ("conv4", "conv6") and sw["use_coarse"] and sw["use_wino"]:
        return out + [("conv3d_coarse", dims, 0)]              # K3r has a dword loader and store: it declines neither
    if sw["use_wino"] and lv[2] % 4 == 0:                      # (`auto` asks dmvs_conv3d_wino_plan first: negative for W % 4 != 0)
        if aligned:
            return out + [("conv3d_wino", dims, 0)]
        out.append(("conv3d_wino", dims, EUNSUPPORTED))
    return out + [("conv3d_mfma", dims, 0)]


def expected_launches(refine, D, H, W, setting, fused, aligned=True):
    """[(C entry without its dmvs_ prefix, (Cin, Cout, D, H, W, kdepth) of the layer as the entry gets them, return code)] of every
    launch of CostRegNet.run, in host order: conv0x2, the small branch, the huge branch; per branch conv1 .. conv7, conv9, conv11,
    prob.  ``fused``: the heads go to dmvs_prob_regress.  ``aligned``: every tensor 16-byte aligned (what torch's allocator gives)."""
    lv = levels(refine, D, H, W)
    d1 = d1_layers(refine, D, H, W) if setting != "direct" else []
    k3 = "conv3d_direct" if setting == "direct" else "conv3d_mfma"
    kb = 1 if refine else 3                                     # the bottleneck layers conv5 / conv6 / conv7
    s1 = lambda n, ci, co, l, kd: _stride1(n, ci, co, lv[l], kd, setting, aligned)  # noqa: E731
    kd_of = lambda n, kd=3: 1 if n in d1 else kd  # noqa: E731
    branch = [(k3, (8, 16) + lv[0] + (3,), 0)] + s1("conv2", 16, 16, 1, kd_of("conv2"))
    branch += [(k3, (16, 32) + lv[1] + (3,), 0)] + s1("conv4", 32, 32, 2, kd_of("conv4"))
    branch += [(k3, (32, 64) + lv[2] + (kb,), 0)] + s1("conv6", 64, 64, 3, kd_of("conv6", kb))
    branch += [(k3, (64, 32) + lv[3] + (kb,), 0), (k3, (32, 16) + lv[2] + (3,), 0), (k3, (16, 8) + lv[1] + (3,), 0)]
    branch += [("prob_regress" if fused else "conv3d_direct", (8, 2) + lv[0] + (3,), 0)]
    return s1("conv0", 2, 16, 0, 3) + branch + branch


def families(launches):
    """ops.launch_log of the successful launches: K2 logs conv3d_direct, the heads prob_head, everything else conv3d_mfma."""
    fam = lambda e, dims: "prob_head" if dims[1] == 2 else ("conv3d_direct" if e == "conv3d_direct" else "conv3d_mfma")  # noqa: E731
    return [fam(e, dims) for e, dims, code in launches if code == 0]


# ------------------------------------------------------------------------------------------------ mutations
MUTATIONS = ("small_reads_huge_c2", "conv0_halves_swapped", "d1_slice0", "skip_before_relu", "skip_dropped", "refine_bottleneck_3d")


def mutation_cases(mutation):
    """[(refine, shape)] at which the mistake changes anything."""
    both = [(r, s) for r in (False, True) for s in shapes_of(r)]
    if mutation == "d1_slice0":
        return [(r, s) for r, s in both if d1_layers(r, *s)]
    if mutation == "refine_bottleneck_3d":
        return [(r, s) for r, s in both if r]
    return both
