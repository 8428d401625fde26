"""What the K1b GPU test files share (test_warp_corr_grad_gpu.py: the default mode, test_costagg_det_gpu.py: the deterministic one):
the case tables with their cached float64 references, guarded buffers, one guarded ``launch`` for both modes, and the comparison
under a table's bounds with the worst ratios it has seen.  A plain module: no tests, no fixtures, no pytest settings."""
import functools

import torch

import warp_corr_grad_ref as GR

F32 = torch.float32
GUARD = 1024
SENTINEL = 12345.0
CASES = GR.all_cases()
BY_TABLE = {t: [n for n, c in CASES.items() if c["table"] == t] for t in GR.TABLES}
PROBES = {name: (case, src_exact, ref_exact) for name, case, src_exact, ref_exact in GR.probe_cases()}
WORST = {}   # (route, table) -> [worst e_max / bound, worst e_mean / bound]


def print_worst(*routes):
    """The WORST lines of the given routes (each test file prints its own at the end of its module)."""
    for (route, table), (rmax, rmean) in sorted(WORST.items()):
        if route in routes:
            note = "  (max not asserted: plain bound)" if table == "WINDOWS" else ""
            print(f"K1B WORST {route} {table}: e_hip / bound max {rmax:.3f} mean {rmean:.3f}{note}")


# ------------------------------------------------------------------------------------------------ shared, computed once
def case_of(name):
    return PROBES[name][0] if name in PROBES else CASES[name]


@functools.lru_cache(maxsize=None)
def p12_of(name):
    """The fp32 p12 both sides get (CPU tensor)."""
    from dmvsnet_amd import ops
    c = case_of(name)
    return c["p12"].clone() if c["p12"] is not None else ops.relative_proj(c["cams"].cuda().contiguous()).cpu()


@functools.lru_cache(maxsize=None)
def ref_of(name):
    """([float64 gradients], [(e_max, e_mean) of the fp32 restatement], [max-bound allowance]) per tensor.  Never modified."""
    return GR.reference(CASES[name], p12_of(name)) + (GR.allowances(CASES[name], p12_of(name)),)


@functools.lru_cache(maxsize=None)
def dev_feats(name):
    from dmvsnet_amd import ops
    return [ops.hwc_to_q4(f.permute(1, 2, 0).contiguous().cuda()) for f in case_of(name)["feats"]]


def guarded(C, H, W, fill):
    """A [C,H,W] view filled with ``fill`` in the middle of a larger buffer of SENTINEL."""
    n = C * H * W
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    out = buf[GUARD:GUARD + n].view(C, H, W)
    out.fill_(fill)
    return buf, out


def guards_intact(buf):
    want = torch.full((GUARD,), SENTINEL, device="cuda").view(torch.int32)
    return torch.equal(buf[:GUARD].view(torch.int32), want) and torch.equal(buf[-GUARD:].view(torch.int32), want)


def launch(name, gsim=None, feats=None, want_ref=True, want=None, mode="atomic", variant=0, workspace=None, expect="finite"):
    """One guarded launch of a case -> (gref or None, [gsrc_v or None]).  ``want``: the source views asked for (None: all).  gref
    starts as NaN.  ``mode`` "atomic": ``ops.warp_corr_backward`` adds into gsrc, which start as zeros and are all finite afterwards, a
    view not asked for still all zero.  "det": ``ops.warp_corr_backward_det`` (``variant``, ``workspace``) writes gsrc, which start as
    NaN; afterwards every wanted one is what ``expect`` says ("finite", so: written, or "nan"), a view not asked for still all NaN."""
    from dmvsnet_amd import ops
    assert mode in ("atomic", "det") and expect in ("finite", "nan")
    det = mode == "det"
    c = case_of(name)
    C, (D, H, W) = c["C"], c["depth"].shape
    feats = dev_feats(name) if feats is None else feats
    nsrc = len(feats) - 1
    want = set(range(nsrc)) if want is None else set(want)
    gsim = c["gsim"] if gsim is None else gsim
    rbuf, gref = guarded(C, H, W, float("nan"))
    sbufs = [guarded(C, H, W, float("nan") if det else 0.0) for _ in range(nsrc)]
    args = (feats[0], feats[1:], p12_of(name).cuda(), c["depth"].cuda(), gsim.cuda(), gref if want_ref else None,
            [g if v in want else None for v, (_, g) in enumerate(sbufs)])
    if det:
        ops.warp_corr_backward_det(*args, workspace=workspace, variant=variant)
    else:
        ops.warp_corr_backward(*args)
    torch.cuda.synchronize()
    assert guards_intact(rbuf), f"{name}: wrote outside gref"
    if not want_ref:
        assert torch.isnan(gref).all(), f"{name}: gref touched though not asked for"
    elif not det:
        assert torch.isfinite(gref).all(), f"{name}: gref elements not written (or not finite)"
    for v, (buf, g) in enumerate(sbufs):
        assert guards_intact(buf), f"{name}: wrote outside gsrc[{v}]"
        if v not in want:
            assert torch.isnan(g).all() if det else not g.any(), f"{name}: gsrc[{v}] touched though not asked for"
        elif expect == "finite":
            assert torch.isfinite(g).all(), f"{name}: gsrc[{v}] has elements that were not written (or are not finite)"
        else:
            assert torch.isnan(g).all(), f"{name}: gsrc[{v}] is not all NaN"
    return (gref if want_ref else None), [g if v in want else None for v, (_, g) in enumerate(sbufs)]


def compare(tag, table, got, f64, e_ref, allowance=0.0, route="direct"):
    """One gradient tensor under its table's bounds; prints before it asserts."""
    e = GR.errors(got, f64)
    plain = GR.bounds(e_ref)
    bmax, bmean = GR.bounds_of(table, e_ref, allowance)
    shown = plain[0] if bmax is None else bmax
    print(f"K1B {tag}: e_hip max {e[0]:.3e} mean {e[1]:.3e}  e_ref max {e_ref[0]:.3e} mean {e_ref[1]:.3e}  allowance {allowance:.3e}  "
          f"ratio max {e[0] / shown:.3f}{' (not asserted)' if bmax is None else ''} mean {e[1] / bmean:.3f}")
    assert got.dtype == F32 and tuple(got.shape) == tuple(f64.shape), tag
    assert torch.isfinite(got).all(), tag
    if f64.abs().max().item() == 0.0:
        assert torch.equal(got.cpu(), torch.zeros(got.shape)), f"{tag}: the yardstick is identically zero"
        return
    w = WORST.setdefault((route, table), [0.0, 0.0])
    w[0], w[1] = max(w[0], e[0] / shown), max(w[1], e[1] / bmean)
    if bmax is not None:
        assert e[0] <= bmax, (tag, "max", e[0], e_ref[0], allowance)
    assert e[1] <= bmean, (tag, "mean", e[1], e_ref[1])


def compare_all(name, grads, route="direct", only=None):
    """grads[0] = dRef, grads[1 + v] = dSrc_v (None: not asked for) against the case's yardstick."""
    g64, e_ref, allow = ref_of(name)
    assert len(grads) == len(g64)
    for k, g in enumerate(grads):
        if g is not None and (only is None or k in only):
            compare(f"{name} {route} {'dRef' if k == 0 else f'dSrc{k - 1}'}", CASES[name]["table"], g, g64[k], e_ref[k], allow[k], route)
