"""Test infrastructure: yardstick, criterion and case tables of the fusion filter N4 (``dmvsnet_amd/csrc/fusion.hip``:
``geo_pair``, both ``geo_consistency_kernel``s, both ``fuse_view_kernel``s, ``fuse_scan_kernel``, ``fuse_emit_kernel``).  No
product code here: tests/test_fusion_ref_cpu.py pins this file against the oracle run in float64 and the recorded reference
outputs and asserts what the tables claim; tests/test_fusion_ref_gpu.py holds the kernels to it.

Restated in NumPy float64 from the reference's statement of the operation (filter/pcd.py:151-344, filter/dypcd_tanks.py:164-304),
the chain UNFOLDED as the reference writes it:

  pair        back-project with inv(K_ref); E_src . inv(E_ref); K_src; divide; a four-tap bilinear gather at the PIXEL coordinate
              (a tap outside the image contributes zero, the weights multiply the taps: a NaN tap under a zero weight is NaN);
              inv(K_src); E_ref . inv(E_src); K_ref; z += 1e-5 where z == 0; divide; dist, rel.  The static filter patches a zero
              reference depth to 1e-4, the ladder does not.  -> rz, dist, rel per pixel.
  pair_P      the same statement on a literal P[33] (A1, b1, A2, t2, K_ref as the kernels take them).
  view        votes, the nine level counts, the depth sum in source order, the photo / geo / final masks, the averaged depth,
              the world points of the final pixels in row-major order.
  geometry    256 pixels per workgroup over the row-major index, 64-lane waves, per-workgroup counts and their exclusive scan;
              the per-pair kernel: 256 columns per workgroup, one row per ``blockIdx.y``.

Criterion on values (the project's): e_max = max|a - f64| / max|f64| and e_mean likewise, each e_hip <= 8 e_ref, 16 * 2^-23
where e_ref < 4 * 2^-23; e_ref is the distance of the fp32 ORACLE (oracle/fusion_oracle.py on the CPU), never of code under test.

Criterion on verdicts: per case band_dist = 8 max|dist_oracle32 - dist64|, band_rel likewise (the maximum over the pixels within
twice the filter's widest gate: ``bands``); a pixel is decided true at gate
(td, tr) when dist64 < td - band_dist and rel64 < tr - band_rel, decided false when either is beyond the gate by the band or
not finite; every decided pixel must carry exactly that verdict.  The undecided share is capped (a condition on the inputs)."""
import numpy as np

F64 = np.float64
FACTOR = 8.0
EPS32 = 2.0 ** -23
WG = 256                 # pixels per workgroup of the fused pass / columns per workgroup of the per-pair kernels
WAVE = 64
N_LEVELS = 9             # gates i = 2..10
LEVELS = tuple(range(2, 11))
Z_PATCH = 1e-5           # pcd.py:194
D_PATCH = 1e-4           # pcd.py:219
STATIC_CAP = 0.01        # undecided share per case, static gate
LADDER_CAP = 0.08        # per case and ladder gate
STATIC_GATE = (1.0, 0.01)
LADDER_BASES = (0.25, 1.0 / 1300)
MAX_PIXELS = 131369      # 343 x 383, the largest input of the tables


# ------------------------------------------------------------------------------------------------ criterion
def bound_of(e_ref):
    return FACTOR * e_ref if e_ref >= 4 * EPS32 else 16 * EPS32


def errors(a, f64, keep=None):
    """(e_max, e_mean) of ``a`` against the yardstick over the elements of ``keep``, normalised by the yardstick's max-abs there."""
    a, f64 = np.asarray(a, F64), np.asarray(f64, F64)
    assert a.shape == f64.shape, (a.shape, f64.shape)
    if keep is not None:
        a, f64 = a[keep], f64[keep]
    if not a.size:
        return 0.0, 0.0
    diff, scale = np.abs(a - f64), np.abs(f64).max()
    if scale == 0.0:
        return (0.0, 0.0) if diff.max() == 0.0 else (float("inf"), float("inf"))
    return float(diff.max() / scale), float(diff.mean() / scale)


def bounds(e_ref):
    return bound_of(e_ref[0]), bound_of(e_ref[1])


# ------------------------------------------------------------------------------------------------ the 1-ulp rule
def _ulps(a, b):
    """Per-element distance in fp32 ulps (a, b: float32 arrays of one shape)."""
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def _check_xyz(a, b):
    """[N,3] fp32 point sets in the same order: every coordinate within 1 ulp, or -- where the fp64 sum cancels to
    (almost) zero and its sign or exponent depends on the reduction order (torch.mm in ViewFilter.finish vs the emit
    kernel's fma chain) -- within fp64 rounding of the point's scale.  -> number of differing values."""
    a, b = np.asarray(a, np.float32).reshape(-1, 3), np.asarray(b, np.float32).reshape(-1, 3)
    assert a.shape == b.shape
    if not a.size:
        return 0
    scale = np.maximum(np.abs(a).max(1, keepdims=True), 1.0).astype(np.float64)
    ok = (_ulps(a, b) <= 1) | (np.abs(a.astype(np.float64) - b) <= 1e-12 * scale)
    assert ok.all(), (int((~ok).sum()), a[~ok.any(1)][:3], b[~ok.any(1)][:3])
    return int((a.view(np.int32) != b.view(np.int32)).sum())


# ------------------------------------------------------------------------------------------------ restatement: one pair
def _grid(H, W):
    y, x = np.meshgrid(np.arange(H, dtype=F64), np.arange(W, dtype=F64), indexing="ij")
    return x, y


def taps(xs, ys, H, W):
    """The four taps of the bilinear sample at pixel coordinate (xs, ys): [(yi, xi, weight, inside)] with float indices."""
    with np.errstate(invalid="ignore"):
        x0, y0 = np.floor(xs), np.floor(ys)
        tx, ty = xs - x0, ys - y0
        out = []
        for dy, wy in ((0.0, 1.0 - ty), (1.0, ty)):
            for dx, wx in ((0.0, 1.0 - tx), (1.0, tx)):
                xi, yi = x0 + dx, y0 + dy
                out.append((yi, xi, wx * wy, (xi >= 0) & (xi <= W - 1) & (yi >= 0) & (yi <= H - 1)))
    return out


def bilinear_zero(src, xs, ys):
    """Explicit four-tap gather; a tap outside contributes zero; weight * tap, so 0 * NaN = NaN as grid_sample has it."""
    H, W = src.shape
    out = np.zeros(xs.shape, F64)
    with np.errstate(invalid="ignore"):
        for yi, xi, w, inside in taps(xs, ys, H, W):
            yc, xc = np.where(inside, yi, 0.0).astype(np.int64), np.where(inside, xi, 0.0).astype(np.int64)
            out = out + np.where(inside, w * src[yc, xc], 0.0)
    return out


def _gates(rx, ry, rz, Kr, d, ladder):
    H, W = d.shape
    x, y = _grid(H, W)
    with np.errstate(all="ignore"):
        kx = Kr[0, 0] * rx + Kr[0, 1] * ry + Kr[0, 2] * rz
        ky = Kr[1, 0] * rx + Kr[1, 1] * ry + Kr[1, 2] * rz
        kz = Kr[2, 0] * rx + Kr[2, 1] * ry + Kr[2, 2] * rz
        kz = np.where(kz == 0, kz + Z_PATCH, kz)
        xr, yr = kx / kz, ky / kz
        dist = np.sqrt((xr - x) ** 2 + (yr - y) ** 2)
        dref = d if ladder else np.where(d == 0, D_PATCH, d)
        rel = np.abs(rz - dref) / dref
    return rz, dist, rel


def pair(d_ref, K_ref, E_ref, d_src, K_src, E_src, ladder=False):
    """One (reference, source) pair from the cameras -> (rz, dist, rel) float64 [H,W]."""
    d, s = np.asarray(d_ref, np.float32).astype(F64), np.asarray(d_src, np.float32).astype(F64)
    Kr, Er, Ks, Es = (np.asarray(m, np.float32).astype(F64) for m in (K_ref, E_ref, K_src, E_src))
    H, W = d.shape
    x, y = _grid(H, W)
    with np.errstate(all="ignore"):
        Kri, Ksi = np.linalg.inv(Kr), np.linalg.inv(Ks)
        fwd, back = Es @ np.linalg.inv(Er), Er @ np.linalg.inv(Es)
        pix = np.stack((x, y, np.ones_like(x))).reshape(3, -1)
        cam = Kri @ (pix * d.reshape(-1))
        cam_src = fwd[:3, :3] @ cam + fwd[:3, 3:4]
        h = Ks @ cam_src
        xs, ys = (h[0] / h[2]).reshape(H, W), (h[1] / h[2]).reshape(H, W)
        sd = bilinear_zero(s, xs, ys)
        lift = Ksi @ (np.stack((xs, ys, np.ones_like(xs))).reshape(3, -1) * sd.reshape(-1))
        rep = back[:3, :3] @ lift + back[:3, 3:4]
    rx, ry, rz = (rep[i].reshape(H, W) for i in range(3))
    return _gates(rx, ry, rz, Kr, d, ladder)


def split_P(P):
    P = np.asarray(P, np.float32).astype(F64).reshape(33)
    return P[0:9].reshape(3, 3), P[9:12], P[12:21].reshape(3, 3), P[21:24], P[24:33].reshape(3, 3)


def make_P(A1=None, b1=(0, 0, 0), A2=None, t2=(0, 0, 0), K_ref=None):
    eye = np.eye(3)
    return np.concatenate([np.asarray(eye if A1 is None else A1, F64).ravel(), np.asarray(b1, F64),
                           np.asarray(eye if A2 is None else A2, F64).ravel(), np.asarray(t2, F64),
                           np.asarray(eye if K_ref is None else K_ref, F64).ravel()]).astype(np.float32)


def project_P(d_ref, P):
    """(xs, ys) float64 of every reference pixel under a literal P."""
    d = np.asarray(d_ref, np.float32).astype(F64)
    A1, b1 = split_P(P)[:2]
    x, y = _grid(*d.shape)
    with np.errstate(all="ignore"):
        h = [(A1[i, 0] * x + A1[i, 1] * y + A1[i, 2]) * d + b1[i] for i in range(3)]
        return h[0] / h[2], h[1] / h[2]


def pair_P(d_ref, d_src, P, ladder=False):
    """The same statement with A1, b1, A2, t2, K_ref given (fp32 P widened) -> (rz, dist, rel)."""
    d, s = np.asarray(d_ref, np.float32).astype(F64), np.asarray(d_src, np.float32).astype(F64)
    _, _, A2, t2, Kr = split_P(P)
    xs, ys = project_P(d_ref, P)
    with np.errstate(all="ignore"):
        sd = bilinear_zero(s, xs, ys)
        r = [(A2[i, 0] * xs + A2[i, 1] * ys + A2[i, 2]) * sd + t2[i] for i in range(3)]
    return _gates(r[0], r[1], r[2], Kr, d, ladder)


def verdict(dist, rel, td, tr):
    """Strict gates; NaN and inf compare false."""
    with np.errstate(invalid="ignore"):
        return (dist < td) & (rel < tr)


def gate_list(ladder, dist, rel, fp32_args=True):
    """[(td, tr)] of the filter: the single gate, or the nine of the ladder.  The kernels take the gate (the bases) as fp32
    arguments (``fp32_args``); the reference compares with Python floats."""
    c = (lambda v: float(np.float32(v))) if fp32_args else float
    if not ladder:
        return [(c(dist), c(rel))]
    return [(i * c(dist), i * c(rel)) for i in LEVELS]


# ------------------------------------------------------------------------------------------------ restatement: one view
def geo_static(votes, thres_view):
    return votes >= thres_view


def geo_dynamic(votes, levels, nsrc):
    geo = votes >= nsrc + 1                      # never true (dypcd_tanks.py:233), restated as the reference has it
    for i in range(2, min(nsrc, 10) + 1):
        geo = geo | (levels[i - 2] >= i)
    return geo


def emit_points(final, avg64, Kinv, Einv):
    """World points of the final pixels in row-major order, float64 [N,3]."""
    ys, xs = np.nonzero(final)
    d = np.asarray(avg64, F64)[final]
    cam = np.asarray(Kinv, F64) @ (np.stack((xs.astype(F64), ys.astype(F64), np.ones(len(d)))) * d)
    return (np.asarray(Einv, F64) @ np.vstack((cam, np.ones(len(d)))))[:3].T


def view(d_ref, cam_ref, confs321, thresholds123, src_depths, src_cams=None, thres_view=2, dynamic=False, dist=None, rel=None,
         P=None, fp32_args=True):
    """Everything ViewFilter.finish / fuse_view state for one reference view, in float64.  ``confs321`` = (conf3, conf2, conf1),
    ``thresholds123`` = (t1, t2, t3); sources by cameras (unfolded chain) or by literal ``P`` [nsrc,33]."""
    if dist is None:
        dist, rel = LADDER_BASES if dynamic else STATIC_GATE
    gates = gate_list(dynamic, dist, rel, fp32_args)
    d = np.asarray(d_ref, np.float32).astype(F64)
    nsrc = len(src_depths)
    out = {"rz": [], "dist": [], "rel": [], "ok": []}
    votes, levels, dsum = np.zeros(d.shape, np.int64), np.zeros((N_LEVELS,) + d.shape, np.int64), np.zeros(d.shape, F64)
    for s in range(nsrc):
        if P is None:
            rz, di, re = pair(d_ref, cam_ref[0], cam_ref[1], src_depths[s], src_cams[s][0], src_cams[s][1], dynamic)
        else:
            rz, di, re = pair_P(d_ref, src_depths[s], P[s], dynamic)
        ok = verdict(di, re, *gates[-1])
        if dynamic:
            for k, (td, tr) in enumerate(gates):
                levels[k] += verdict(di, re, td, tr)
        votes += ok
        dsum = dsum + np.where(ok, rz, 0.0)
        for k, v in zip(("rz", "dist", "rel", "ok"), (rz, di, re, ok)):
            out[k].append(v)
    c3, c2, c1 = confs321
    t1, t2, t3 = (float(np.float32(t)) if fp32_args else float(t) for t in thresholds123)
    photo = (np.asarray(c3) > t3) & (np.asarray(c2) > t2) & (np.asarray(c1) > t1)
    geo = geo_dynamic(votes, levels, nsrc) if dynamic else geo_static(votes, thres_view)
    d_base = d if dynamic else np.where(d == 0, D_PATCH, d)
    avg = (dsum + d_base) / (votes + 1)
    final = photo & geo
    out.update(votes=votes, levels=levels, depth_sum=dsum, photo=photo, geo=geo, final=final, depth_avg=avg, gates=gates)
    if cam_ref is not None:
        K, E = (np.asarray(m, np.float32).astype(F64) for m in cam_ref)
        out["xyz"] = emit_points(final, avg, np.linalg.inv(K), np.linalg.inv(E))
    return out


# ------------------------------------------------------------------------------------------------ launch geometry
def workgroups(H, W):
    return (H * W + WG - 1) // WG


def ragged_lanes(H, W):
    """Lanes of the last workgroup of the fused pass that own no pixel."""
    return workgroups(H, W) * WG - H * W


def wg_counts(final):
    f = np.asarray(final).reshape(-1) != 0
    n = workgroups(1, f.size)
    return np.pad(f, (0, n * WG - f.size)).reshape(n, WG).sum(1).astype(np.int32)


def wave_counts(final):
    f = np.asarray(final).reshape(-1) != 0
    n = workgroups(1, f.size)
    return np.pad(f, (0, n * WG - f.size)).reshape(n, WG // WAVE, WAVE).sum(2).astype(np.int32)


def scan_offsets(counts):
    """Exclusive scan with the total appended: offsets[b] = sum counts[0..b), offsets[n] = total."""
    return np.concatenate(([0], np.cumsum(np.asarray(counts, np.int64)))).astype(np.int32)


def scan_passes(nblk):
    """Turns of fuse_scan_kernel's loop; every turn after the first adds a carry."""
    return (nblk + WG - 1) // WG


def pair_grid(H, W):
    """(blockIdx.x count, blockIdx.y count, idle lanes of the last column block) of the per-pair kernels."""
    nx = (W + WG - 1) // WG
    return nx, H, nx * WG - W


# ------------------------------------------------------------------------------------------------ fp32 emulation of geo_pair
def emul_pair32(d_ref, d_src, P, ladder=False):
    """geo_pair in the kernel's own operation order: NumPy float32, one rounding per operation, no contraction.  CPU-only, to
    size the criterion and to prove the exact cases; never a yardstick on the GPU.  -> (rz, dist, rel, sd) float32."""
    f = np.float32
    d, s, P = np.asarray(d_ref, f), np.asarray(d_src, f), np.asarray(P, f).reshape(33)
    H, W = d.shape
    fy, fx = np.meshgrid(np.arange(H, dtype=f), np.arange(W, dtype=f), indexing="ij")
    with np.errstate(all="ignore"):
        hx = (P[0] * fx + P[1] * fy + P[2]) * d + P[9]
        hy = (P[3] * fx + P[4] * fy + P[5]) * d + P[10]
        hz = (P[6] * fx + P[7] * fy + P[8]) * d + P[11]
        xs, ys = hx / hz, hy / hz
        wm1, hm1 = f(W - 1), f(H - 1)
        x0f, y0f = np.floor(xs), np.floor(ys)
        tx, ty = xs - x0f, ys - y0f
        x0in, x1in = (x0f >= 0) & (x0f <= wm1), (x0f >= -1) & (x0f <= wm1 - f(1))
        y0in, y1in = (y0f >= 0) & (y0f <= hm1), (y0f >= -1) & (y0f <= hm1 - f(1))

        def clampi(v, hi):           # (int)fminf(fmaxf(v, 0), hi): fmaxf drops a NaN operand
            return np.fmin(np.fmax(v, f(0)), hi).astype(np.int64)

        x0, x1, y0, y1 = clampi(x0f, wm1), clampi(x0f + f(1), wm1), clampi(y0f, hm1), clampi(y0f + f(1), hm1)
        one, zero = f(1), f(0)
        sd = (np.where(x0in & y0in, (one - tx) * (one - ty) * s[y0, x0], zero) + np.where(x1in & y0in, tx * (one - ty) * s[y0, x1], zero)
              + np.where(x0in & y1in, (one - tx) * ty * s[y1, x0], zero) + np.where(x1in & y1in, tx * ty * s[y1, x1], zero))
        rx = (P[12] * xs + P[13] * ys + P[14]) * sd + P[21]
        ry = (P[15] * xs + P[16] * ys + P[17]) * sd + P[22]
        rz = (P[18] * xs + P[19] * ys + P[20]) * sd + P[23]
        kx = P[24] * rx + P[25] * ry + P[26] * rz
        ky = P[27] * rx + P[28] * ry + P[29] * rz
        kz = P[30] * rx + P[31] * ry + P[32] * rz
        kz = np.where(kz == 0, kz + f(0.00001), kz)
        xr, yr = kx / kz, ky / kz
        dist = np.sqrt((xr - fx) * (xr - fx) + (yr - fy) * (yr - fy))
        dref = d if ladder else np.where(d == 0, f(1e-4), d)
        rel = np.abs(rz - dref) / dref
    assert all(a.dtype == f for a in (rz, dist, rel, sd))
    return rz, dist, rel, sd


def emul_verdict32(dist, rel, td, tr, level=None):
    """The kernel's comparison: fp32 thresholds, (float)i * base for ladder level i."""
    f = np.float32
    td, tr = (f(td), f(tr)) if level is None else (f(level) * f(td), f(level) * f(tr))
    with np.errstate(invalid="ignore"):
        return (dist < td) & (rel < tr)


# ------------------------------------------------------------------------------------------------ the fp32 oracle, per pair
def oracle_pair(d_ref, cam_ref, d_src, cam_src, ladder=False, double=False):
    """oracle/fusion_oracle.py's reprojection on the CPU and the distances formed from it as its checks form them
    -> (rz, dist, rel) as float64 arrays holding the oracle's values (fp32, or float64 when ``double``).
    The reference normalises the sample coordinate by (H - 1) / 2 and (W - 1) / 2 and has no result for a map of one row or
    one column; there the oracle runs on the maps with one row / column of zeros appended -- a zero tap weighs what a tap
    outside the image weighs -- and the appended pixels are dropped."""
    import torch
    from oracle import fusion_oracle as FO
    H, W = d_ref.shape
    pad = ((0, int(H == 1)), (0, int(W == 1)))
    dt = torch.float64 if double else torch.float32
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dt)   # noqa: E731
    dr, ds = T(np.pad(np.asarray(d_ref, np.float32), pad)), T(np.pad(np.asarray(d_src, np.float32), pad))
    cams = (T(cam_ref[0]), T(cam_ref[1]), ds, T(cam_src[0]), T(cam_src[1]))
    if not ladder:
        _, _, dist, rel = FO.check_geometric_consistency(dr, *cams)
        rz = FO.reproject_with_depth(dr, *cams)[0]
    else:
        y_ref, x_ref = torch.meshgrid(torch.arange(0, dr.shape[0]), torch.arange(0, dr.shape[1]), indexing="ij")
        rz, xr, yr = FO.reproject_with_depth(dr, *cams)
        dist = torch.sqrt((xr - x_ref) ** 2 + (yr - y_ref) ** 2)
        rel = (rz - dr).abs() / dr          # dypcd_tanks.py:176: the raw depth, no patch
    return tuple(t.double().numpy()[:H, :W] for t in (rz, dist, rel))


def oracle_view_avg(d_ref, cam_ref, src_depths, src_cams, dynamic, dist=None, rel=None):
    """The averaged depth as filter_depth forms it from the fp32 oracle's pairs (pcd.py:283-299, dypcd_tanks.py:236-248): fp32
    sum of the accepted reprojections in source order plus the (patched) reference depth, over votes + 1 in float64.
    -> (avg float64 [H,W], votes)."""
    if dist is None:
        dist, rel = LADDER_BASES if dynamic else STATIC_GATE
    td, tr = gate_list(dynamic, dist, rel)[-1]
    d = np.asarray(d_ref, np.float32)
    votes, dsum = np.zeros(d.shape, np.int64), np.zeros(d.shape, np.float32)
    for s, c in zip(src_depths, src_cams):
        rz, di, re = oracle_pair(d_ref, cam_ref, s, c, dynamic)
        ok = verdict(di, re, td, tr)
        votes += ok
        dsum = dsum + np.where(ok, rz, 0.0).astype(np.float32)
    d_base = d if dynamic else np.where(d == 0, np.float32(D_PATCH), d)
    return (dsum + d_base).astype(F64) / (votes + 1), votes


def bands(o32, f64, gates):
    """(band_dist, band_rel) = 8 max |oracle32 - f64| over the pixels where both are finite and that lie within twice the
    filter's widest gate in float64 (the neighbourhood in which a rounding error can change a verdict; a hole pixel whose
    distance is thousands of pixels has an fp32 error of whole pixels and is decided false by any band)."""
    td, tr = gates[-1]
    with np.errstate(invalid="ignore"):
        near = (f64[1] < 2 * td) & (f64[2] < 2 * tr)
    out = []
    for a, b in ((o32[1], f64[1]), (o32[2], f64[2])):
        fin = np.isfinite(a) & np.isfinite(b) & near
        out.append(FACTOR * float(np.abs(a[fin] - b[fin]).max()) if fin.any() else 0.0)
    return tuple(out)


def decided(dist64, rel64, td, tr, band):
    """(decided true, decided false) at gate (td, tr)."""
    bd, br = band
    with np.errstate(invalid="ignore"):
        yes = (dist64 < td - bd) & (rel64 < tr - br)
        no = (dist64 > td + bd) | (rel64 > tr + br) | ~np.isfinite(dist64) | ~np.isfinite(rel64)
    return yes, no


def undecided_share(dist64, rel64, td, tr, band):
    yes, no = decided(dist64, rel64, td, tr, band)
    return float((~(yes | no)).mean())


# ------------------------------------------------------------------------------------------------ case tables
# SCENES: synth_fusion_scene(H, W, V, seed); reference view 0 against sources 1..V-1.  (H, W, V, seed, class)
SCENES = (
    (37, 53, 4, 1, "ragged against 256"),
    (3, 257, 4, 1, "per-pair blockIdx.x = 1 with one lane in use"),
    (2, 513, 4, 1, "per-pair blockIdx.x = 2 with one lane in use"),
    (1, 300, 4, 1, "one row"),
    (300, 1, 4, 1, "one column: W - 1 = 0, every x1 tap outside"),
    (96, 128, 5, 0, "the golden scene"),
)
SCENE_CONF = (0.1, 0.2, 0.3)


def scene(H, W, V, seed):
    from dmvsnet_amd import synth
    cams, depths, confs, imgs = synth.synth_fusion_scene(H, W, V, seed=seed)
    cam = lambda v: (cams[v, 1, :3, :3].copy(), cams[v, 0].copy())   # noqa: E731
    return depths, confs, cam


# EXACT: A1 = A2 = K_ref = I, t2 = 0, b1 = (sx d, sy d, 0); reference depth the power of two d, source depth d (1 + 2^-k).
EXACT_HW = (6, 9)
EXACT_D = 4.0


def exact_case(sx, sy, k=8, H=EXACT_HW[0], W=EXACT_HW[1], d=EXACT_D):
    d_ref = np.full((H, W), d, np.float32)
    d_src = np.full((H, W), d * (1.0 + 2.0 ** -k), np.float32)
    return d_ref, d_src, make_P(b1=(sx * d, sy * d, 0.0))


# (name, sx, sy, L, R, T, B): where the shift puts xs / ys of the first and last column / row, and the columns (rows) that
# have a tap left of (right of, above, below) the image; negative indices count from the last column / row
EXACT_SHIFTS = (
    ("xs=-1", -1.0, 0.0, (0,), (), (), (-1,)),
    ("xs=-0.5|W-1.5", -0.5, 0.0, (0,), (), (), (-1,)),
    ("xs=0|W-1", 0.0, 0.0, (), (-1,), (), (-1,)),                 # x1 = W, y1 = H under weight zero
    ("xs=W-0.5", 0.5, 0.0, (), (-1,), (), (-1,)),
    ("xs=W", 1.0, 0.0, (), (-2, -1), (), (-1,)),
    ("ys=-1", 0.0, -1.0, (), (-1,), (0,), ()),
    ("ys=-0.5|H-1.5", 0.0, -0.5, (), (-1,), (0,), ()),
    ("ys=H-0.5", 0.0, 0.5, (), (-1,), (), (-1,)),
    ("ys=H", 0.0, 1.0, (), (-1,), (), (-2, -1)),
    ("corners-", -0.375, -0.5, (0,), (), (0,), ()),
    ("corners+", 0.375, 0.5, (), (-1,), (), (-1,)),
    ("corners-+", -0.375, 0.5, (0,), (), (), (-1,)),
    ("corners+-", 0.375, -0.5, (), (-1,), (0,), ()),
    ("3-4-5", 0.75, 1.0, (), (-1,), (), (-2, -1)),
    ("all-outside", 16.0, 0.0, (), tuple(range(-EXACT_HW[1], 0)), (), (-1,)),      # sd = 0, kz == 0: the 1e-5 patch
)


def tap_sides(xs, ys, H, W):
    """Columns with a tap left / right of the image, rows with a tap above / below it, from the restated taps."""
    L = R = T = B = False
    for yi, xi, _, _ in taps(xs, ys, H, W):
        L, R, T, B = L | (xi < 0), R | (xi > W - 1), T | (yi < 0), B | (yi > H - 1)
    cols = lambda m: tuple(np.nonzero(m.any(0))[0].tolist())   # noqa: E731
    rows = lambda m: tuple(np.nonzero(m.any(1))[0].tolist())   # noqa: E731
    return cols(L), cols(R), rows(T), rows(B)


def _step(v, up):
    return float(np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf)))


# strict gates: (name, sx, sy, k, td, tr, verdict); dist = hypot(sx, sy), rel = 2^-k
EXACT_GATES = (
    ("dist on the gate", 0.5, 0.0, 8, 0.5, 1.0, False),
    ("dist one step under the gate", 0.5, 0.0, 8, _step(0.5, True), 1.0, True),
    ("dist one step over the gate", 0.5, 0.0, 8, _step(0.5, False), 1.0, False),
    ("dist 3-4-5 on the gate", 0.75, 1.0, 8, 1.25, 1.0, False),
    ("dist 3-4-5 under the gate", 0.75, 1.0, 8, _step(1.25, True), 1.0, True),
    ("rel on the gate", 0.0, 0.0, 8, 1.0, 2.0 ** -8, False),
    ("rel one step under the gate", 0.0, 0.0, 8, 1.0, _step(2.0 ** -8, True), True),
    ("rel one step over the gate", 0.0, 0.0, 8, 1.0, _step(2.0 ** -8, False), False),
)
# ladder with bases 1/4 and 2^-10: (name, sx, k, levels i that pass)
EXACT_LADDER_BASES = (0.25, 2.0 ** -10)
EXACT_LADDER = (
    ("shift 0.5", 0.5, 12, tuple(range(3, 11))),
    ("rel 2^-8", 0.0, 8, tuple(range(5, 11))),
    ("shift 0.75 and rel 2^-8", 0.75, 8, tuple(range(5, 11))),
    ("shift 2.5", 2.5, 12, ()),
    ("nothing in the way", 0.0, 12, tuple(range(2, 11))),
)


def interior(H, W, sx, sy):
    """Pixels all of whose four taps lie inside the image under the shift (where the exact scaffold samples c itself)."""
    x, y = _grid(H, W)
    xs, ys = x + sx, y + sy
    return (np.floor(xs) >= 0) & (np.floor(xs) + 1 <= W - 1) & (np.floor(ys) >= 0) & (np.floor(ys) + 1 <= H - 1)


# HOSTILE: values put into the exact scaffold (name, where, value)
HOSTILE_VALUES = (("nan", np.nan), ("inf", np.inf), ("neg", -4.0), ("zero", 0.0))

# EMIT: (H, W) and the patterns of final pixels
EMIT_SIZES = ((1, 1), (1, 63), (1, 64), (1, 65), (1, 255), (1, 256), (1, 257), (257, 256), (342, 384), (343, 383))
EMIT_PATTERNS = ("none", "all", "last", "wave_edges", "one_full_wg", "half")
WAVE_EDGE_LANES = (63, 64, 127, 128, 191, 192, 255)


def emit_pattern(name, H, W):
    n = H * W
    f = np.zeros(n, bool)
    if name == "all":
        f[:] = True
    elif name == "last":
        f[-1] = True
    elif name == "wave_edges":
        lane = np.arange(n) % WG
        f = np.isin(lane, WAVE_EDGE_LANES)
    elif name == "one_full_wg":
        b = workgroups(H, W) // 2
        f[b * WG:(b + 1) * WG] = True
    elif name == "half":
        f = np.random.default_rng(n).random(n) < 0.5
    else:
        assert name == "none"
    return f.reshape(H, W)


def emit_depths(H, W):
    """Averaged depths for the hand-made masks: dyadic, different at every pixel of a workgroup."""
    p = np.arange(H * W, dtype=F64)
    return (512.0 + (p % 1021) * 0.125).reshape(H, W)


EMIT_K = np.array([[64.0, 0, 30.5], [0, 64.0, 20.25], [0, 0, 1]], np.float32)
EMIT_E = np.array([[0.8, -0.6, 0, 12.5], [0.6, 0.8, 0, -7.25], [0, 0, 1, 100.0], [0, 0, 0, 1]], np.float32)

# SOURCES: (dynamic, nsrc)
SOURCES = ((True, 1), (True, 2), (True, 9), (True, 10), (False, 1), (False, 2), (False, 16))
SOURCES_HW = (37, 53)
