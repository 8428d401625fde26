"""Yardstick of the hypothesis-plane kernels (N2: ``hyp_first_kernel`` / ``hyp_next_kernel`` of csrc/layout.hip): a restatement of the
plane formulas, written from the kernels' comments and the oracle's docstrings, parametrised by ``dtype`` -- float64 is the yardstick,
the same text in float32 on stock ATen (CPU) gives the e_ref of the project's criterion -- plus the fixed case tables of the tests.
No product code here, and no ``F.interpolate``: the x2 resize is written out tap by tap.

  first stage   itv = (dmax - dmin) / (D - 1); plane d = dmin + d * itv, minus itv where row % 2 == col % 2, else plus itv.
                Inverse sampling: 1 / linspace(1 / lo, 1 / hi, D) for the shifted ends (dmin -/+ itv, dmax -/+ itv); the interval is
                recomputed from the shifted ends before each variant and the last one is returned.
  later stages  pix = ratio * ((dv[-1] - dv[0]) / n); the coarse pixel (r, c) spans last - (D + 2) / 2 * pix .. last + (D - 2) / 2 * pix
                where r % 2 == c % 2 and last - (D - 2) / 2 * pix .. last + (D + 2) / 2 * pix elsewhere, sampled linearly or in inverse
                depth; interval D * pix / (D - 1); then the x2 bilinear resize with half-pixel centres (source coordinate
                (dst + .5) / 2 - .5 clamped at 0, far tap clamped at the last row / column).  ``up == 1``: no resize.
  affine form   base = plane 0 of the linear form; volume = base + d * interval.

Layouts: depth values [n] or [1,n]; last [h,w]; planes [D,H,W]; intervals 0-dim."""
import torch

EPS32 = 2.0 ** -23
FACTOR = 8.0


def bound_of(e_ref):
    """The project's criterion: e_hip <= 8 e_ref, and 16 * 2^-23 where e_ref < 4 * 2^-23."""
    return FACTOR * e_ref if e_ref >= 4 * EPS32 else 16 * EPS32


def rel_dist(a, b):
    """max|a - b| / max|b| in float64."""
    a, b = a.detach().to("cpu", torch.float64), b.detach().to("cpu", torch.float64)
    return ((a - b).abs().max() / b.abs().max()).item()


def finite_part(a, f64):
    """(a, f64) restricted to the elements where the float64 yardstick is finite, and whether ``a`` is non-finite exactly where the
    yardstick is (one first-stage case has an end of its inverse-depth range at exactly 0: see ``first_cases``)."""
    a, f64 = a.detach().to("cpu", torch.float64), f64.detach().to("cpu", torch.float64)
    ok = torch.isfinite(f64)
    return a[ok], f64[ok], bool(torch.equal(torch.isfinite(a), ok))


def _t(x, dtype):
    return x.detach().to("cpu", dtype)


def parity(h, w):
    """True where row % 2 == col % 2."""
    return (torch.arange(h).view(h, 1) % 2) == (torch.arange(w).view(1, w) % 2)


def linspace(a, b, n, mid=None):
    """torch.linspace(a, b, n) written out: step = (b - a) / (n - 1); element i counts from ``a`` below the split n // 2 and back from
    ``b`` from there on.  ``mid`` moves the split (the mutation test; the two branches are the same number in exact arithmetic)."""
    i = torch.arange(n, dtype=a.dtype)
    step = (b - a) / (n - 1)
    return torch.where(i < (n // 2 if mid is None else mid), a + step * i, b - step * (n - 1 - i))


# ------------------------------------------------------------------------------------------------ first stage
def first(dv, D, H, W, inverse, dtype=torch.float64, mid=None):
    """-> (planes [D,H,W], interval)."""
    dv = _t(dv, dtype).reshape(-1)
    dmin, dmax = dv[0], dv[-1]
    itv = (dmax - dmin) / (D - 1)
    same = parity(H, W)
    if not inverse:
        plane = (dmin + torch.arange(D, dtype=dtype) * itv).view(D, 1, 1)
        return torch.where(same, plane - itv, plane + itv), itv
    lo, hi = dmin - itv, dmax - itv
    itv = (hi - lo) / (D - 1)
    vn = 1 / linspace(1 / lo, 1 / hi, D, mid)
    lo, hi = dmin + itv, dmax + itv
    itv = (hi - lo) / (D - 1)
    vp = 1 / linspace(1 / lo, 1 / hi, D, mid)
    return torch.where(same, vn.view(D, 1, 1), vp.view(D, 1, 1)), itv


# ------------------------------------------------------------------------------------------------ later stages
def pix_interval(dv, ratio, dtype=torch.float64, n=None):
    """ratio * depth_interval; depth_interval divides the range by n, the NUMBER of depth values (not n - 1)."""
    dv = _t(dv, dtype).reshape(-1)
    return ratio * ((dv[-1] - dv[0]) / (dv.numel() if n is None else n))


def spans(last, pix, D, inverse):
    """The two per-pixel sample sets [D,h,w] around ``last``: (r % 2 == c % 2 variant, the other one)."""
    ar = torch.arange(D, dtype=last.dtype).view(D, 1, 1)

    def span(below, above):
        lo, hi = last - below / 2 * pix, last + above / 2 * pix
        if not inverse:
            return lo + ar * ((hi - lo) / (D - 1))
        ilo, ihi = 1 / lo, 1 / hi
        return 1 / (ilo + ar * ((ihi - ilo) / (D - 1)))

    return span(D + 2, D - 2), span(D - 2, D + 2)


def coarse(last, pix, D, inverse):
    """-> (planes [D,h,w] at last's resolution, interval)."""
    vn, vp = spans(last, pix, D, inverse)
    return torch.where(parity(*last.shape), vn, vp), (D * pix) / (D - 1)


def half_pixel_taps(n_out, n_in, dtype):
    """(near index, far index, far weight) per output row / column of the x2 resize with half-pixel centres."""
    s = ((torch.arange(n_out, dtype=dtype) + 0.5) * 0.5 - 0.5).clamp(min=0)
    i0 = s.floor().long()
    return i0, (i0 + 1).clamp(max=n_in - 1), s - i0.to(dtype)


def upsample2(vol, taps=half_pixel_taps):
    """[D,h,w] -> [D,2h,2w], bilinear."""
    _, h, w = vol.shape
    y0, y1, ly = taps(2 * h, h, vol.dtype)
    x0, x1, lx = taps(2 * w, w, vol.dtype)
    hy, ly, hx, lx = (1 - ly).view(1, -1, 1), ly.view(1, -1, 1), (1 - lx).view(1, 1, -1), lx.view(1, 1, -1)
    r0, r1 = vol[:, y0], vol[:, y1]
    return hy * (hx * r0[:, :, x0] + lx * r0[:, :, x1]) + ly * (hx * r1[:, :, x0] + lx * r1[:, :, x1])


def later(last, dv, ratio, D, inverse, up=2, dtype=torch.float64):
    """-> (planes [D,up*h,up*w], interval)."""
    assert up in (1, 2)
    vol, itv = coarse(_t(last, dtype), pix_interval(dv, ratio, dtype), D, inverse)
    return (upsample2(vol) if up == 2 else vol), itv


def affine_volume(base, itv, D):
    """base [H,W] + d * interval -> [D,H,W]."""
    return base[None] + torch.arange(D, dtype=base.dtype).view(D, 1, 1) * itv


# ------------------------------------------------------------------------------------------------ the case tables
def depth_values(name):
    """fp32 [n].  synth192: 425 + 2.65 i (425 .. 931.15); synth2: its two ends (n = 2: depth_interval divides by n, so the later
    stages see another pix, the first stage the same planes); small48: 2.0 .. 10.0 in 48 steps."""
    if name == "small48":
        return torch.linspace(2.0, 10.0, 48, dtype=torch.float64).float()
    full = 425.0 + torch.arange(192, dtype=torch.float32) * 2.65
    return full if name == "synth192" else full[[0, -1]].clone()


FIRST_SHAPES = ((2, 1, 1), (5, 3, 257), (8, 6, 8), (48, 2, 300), (64, 5, 33))   # (D, H, W)
FIRST_DEPTHS = ("synth192", "synth2", "small48")
# (h, w, D, ratio): one pixel; one row, W = 260 (two blocks of 256 in x); odd sizes, W = 258; W = 256, exactly one block; odd sizes,
# W = 130; D = 64 on a tiny map; one column with a non-integer ratio; odd D; ratio 1
LATER_SHAPES = ((1, 1, 2, 1.0), (1, 130, 8, 2.0), (3, 129, 8, 2.0), (5, 128, 32, 3.0), (7, 65, 48, 4.0), (2, 3, 64, 4.0),
                (9, 1, 4, 1.5), (4, 6, 5, 2.0), (6, 8, 16, 1.0))
SAME_SHAPES = ((1, 1), (3, 257), (5, 256), (2, 255))   # up == 1: (h, w)
SAME_DEPTHS = (5, 8, 24)
# lower end and smallest width of ``last`` per depth range; the width grows to 20 plane spacings (pix) where that is more
LAST_RANGE = {"synth192": (560.0, 160.0), "small48": (8.0, 2.0)}
MIN_SPACINGS = 20.0


def first_cases():
    """name -> dict(D, H, W, dv).  In 5-3x257-small48 the shifted lower end dmin - itv = 2 - 8 / 4 is exactly 0 in every precision:
    1 / lo is infinite and the r % 2 == c % 2 half of the inverse planes is NaN in the kernel, the reference and here alike.  The case
    stays (its linear forms and the other half are ordinary); comparisons go through ``finite_part``."""
    return {f"{D}-{H}x{W}-{dn}": dict(D=D, H=H, W=W, dv=depth_values(dn)) for D, H, W in FIRST_SHAPES for dn in FIRST_DEPTHS}


def make_last(h, w, dv, ratio, lo, width, seed):
    """i.i.d. uniform per pixel (never smooth: a wrong tap weight must show) over max(width, 20 pix), fp32."""
    pix = pix_interval(dv, ratio).item()
    g = torch.Generator().manual_seed(seed)
    return (lo + max(width, MIN_SPACINGS * pix) * torch.rand((h, w), generator=g, dtype=torch.float64)).float()


def later_cases():
    """name -> dict(h, w, D, ratio, up, dv, last): up == 2 on both depth ranges (the small one for D <= 16 only: beyond that the
    sample span reaches the pole of 1 / lo), then up == 1."""
    out = {}
    for k, (h, w, D, ratio) in enumerate(LATER_SHAPES):
        for dn in ("synth192", "small48") if D <= 16 else ("synth192",):
            dv = depth_values(dn)
            out[f"up2-{h}x{w}-D{D}-r{ratio:g}-{dn}"] = dict(h=h, w=w, D=D, ratio=ratio, up=2, dv=dv,
                                                           last=make_last(h, w, dv, ratio, *LAST_RANGE[dn], 100 + k))
    dv = depth_values("synth192")
    for k, (h, w) in enumerate(SAME_SHAPES):
        for D in SAME_DEPTHS:
            out[f"up1-{h}x{w}-D{D}"] = dict(h=h, w=w, D=D, ratio=1.0, up=1, dv=dv,
                                            last=make_last(h, w, dv, 1.0, *LAST_RANGE["synth192"], 200 + 10 * k + D))
    return out
