"""GPU (-m gpu): the fusion filter N4 held to the float64 restatement of tests/fusion_ref.py -- ``geo_pair`` through both
``geo_consistency_kernel``s and both ``fuse_view_kernel``s, ``fuse_scan_kernel``, ``fuse_emit_kernel``.

Yardsticks, none of them code under test: the float64 restatement, the fp32 oracle on the CPU (oracle/fusion_oracle.py), and
exact expectations where the inputs make every value representable.  The C entries are called through ``_lib.load()`` with
pointers into larger buffers: every output (and every input map) sits between guard bands that must come back bit for bit.

  SCENES      values e_hip <= 8 e_ref on max and mean (``OPEN``: gates at +inf; ``PAIR``: pixels both sides accept), verdicts of
              every decided pixel (``VERDICT``), per pair and through the fused pass with its scan and emission
  EXACT       tap boundaries, corners, the kz == 0 patch, strict gates, ladder levels, geo forms, zero depths, dyadic points
  HOSTILE     NaN, inf, negative, zero; a NaN neighbour under a zero weight; hz == 0, hz < 0, xs = 1e30
  ACCUMULATE  += on pre-filled sums, NULL outputs, two runs
  SOURCES     1..16 sources, stage and scalar confidences, reversed order, against the restatement
  EMIT        counts, offsets, order and points at every workgroup / wave seam and with one and two scan carries

Every test prints its figures before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import fusion_ref as R
from dmvsnet_amd import _lib
from dmvsnet_amd.fusion import fold_projection

pytestmark = pytest.mark.gpu

PAD = 67                       # guard elements on either side: leaves every pointer aligned to its element only
INF = float("inf")
_FILL = {torch.float32: (np.int32, 0x7fc0a5a5), torch.float64: (np.int64, 0x7ff8a5a5a5a5a5a5), torch.int32: (np.int32, 0x7fc0a5a5),
         torch.uint8: (np.uint8, 0xa5)}
_NP = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32, torch.uint8: np.uint8}


class Guard:
    """A device array inside a larger buffer filled with a NaN pattern (floats) / 0x7fc0a5a5 / 0xa5."""

    def __init__(self, shape, dtype, init=None):
        self.shape, self.dtype = tuple(int(v) for v in np.atleast_1d(shape)), dtype
        self.n = int(np.prod(self.shape))
        bits, fill = _FILL[dtype]
        host = np.full(self.n + 2 * PAD, fill, bits)
        if init is not None:
            host[PAD:PAD + self.n] = np.ascontiguousarray(np.broadcast_to(init, self.shape), _NP[dtype]).reshape(-1).view(bits)
        self.before = host.copy()
        self.buf = torch.from_numpy(host).cuda()
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + PAD * self.buf.element_size())

    def raw(self):
        """Interior as stored (bit patterns), after asserting that the bands are untouched."""
        host = self.buf.cpu().numpy()
        assert host[:PAD].tobytes() == self.before[:PAD].tobytes(), "leading guard band written"
        assert host[PAD + self.n:].tobytes() == self.before[PAD + self.n:].tobytes(), "trailing guard band written"
        return host[PAD:PAD + self.n]

    def get(self):
        return self.raw().view(_NP[self.dtype]).reshape(self.shape).copy()

    def untouched(self):
        """bool per element: still the fill pattern."""
        return (self.raw() == _FILL[self.dtype][1]).reshape(self.shape)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


f32, f64, i32, u8 = torch.float32, torch.float64, torch.int32, torch.uint8
PAIR_OUTS = ("mask", "rep", "votes", "dsum", "lv")


def run_pair(d_ref, d_src, P, td, tr, ladder, outs=PAIR_OUTS, init=None):
    """One launch of dmvs_geo_consistency(_ladder); ``outs``: the outputs that are not NULL; ``init``: start values of the
    accumulators (zero otherwise).  -> dict of host arrays."""
    H, W = d_ref.shape
    init = init or {}
    g = {"ref": Guard((H, W), f32, d_ref), "src": Guard((H, W), f32, d_src), "P": Guard((33,), f32, P)}
    spec = {"mask": ((H, W), u8, None), "rep": ((H, W), f32, None), "votes": ((H, W), i32, init.get("votes", 0)),
            "dsum": ((H, W), f32, init.get("dsum", 0.0)), "lv": ((R.N_LEVELS, H, W), i32, init.get("lv", 0))}
    for k in outs:
        if k != "lv" or ladder:
            g[k] = Guard(*spec[k])
    p = lambda k: g[k].ptr if k in g else None   # noqa: E731
    lib = _lib.load()
    if ladder:
        code = lib.dmvs_geo_consistency_ladder(g["ref"].ptr, g["src"].ptr, g["P"].ptr, H, W, float(td), float(tr), p("lv"), p("mask"),
                                               p("rep"), p("votes"), p("dsum"), _stream())
    else:
        code = lib.dmvs_geo_consistency(g["ref"].ptr, g["src"].ptr, g["P"].ptr, H, W, float(td), float(tr), p("mask"), p("rep"),
                                        p("votes"), p("dsum"), _stream())
    _lib.check(code, "dmvs_geo_consistency")
    torch.cuda.synchronize()
    out = {k: v.get() for k, v in g.items()}
    for k in ("ref", "src", "P"):      # inputs are read only
        assert g[k].raw().tobytes() == g[k].before[PAD:PAD + g[k].n].tobytes(), k
    return out


def run_view(d_ref, c3, c2, c1, srcs, P, th, dynamic, thres_view, td, tr):
    """dmvs_fuse_view -> dict of host arrays plus the guards (for run_emit)."""
    H, W = d_ref.shape
    nsrc, nblk = len(srcs), R.workgroups(H, W)
    lib = _lib.load()
    assert int(lib.dmvs_fuse_workgroups(H, W)) == nblk
    gin = [Guard((H, W), f32, a) for a in (d_ref, c3, c2, c1)] + [Guard((H, W), f32, s) for s in srcs]
    g = {"masks": Guard((3, H, W), u8), "avg": Guard((H, W), f32), "avg64": Guard((H, W), f64), "counts": Guard((nblk,), i32)}
    ptrs = (ctypes.c_void_p * nsrc)(*[x.ptr.value for x in gin[4:]])
    Ph = np.ascontiguousarray(np.asarray(P, np.float32).reshape(nsrc, 33))
    t1, t2, t3 = (float(v) for v in th)
    code = lib.dmvs_fuse_view(gin[0].ptr, gin[1].ptr, gin[2].ptr, gin[3].ptr, H, W, nsrc, ptrs, Ph.ctypes.data_as(ctypes.c_void_p),
                              t1, t2, t3, int(dynamic), int(thres_view), float(td), float(tr), g["masks"].ptr, g["avg"].ptr,
                              g["avg64"].ptr, g["counts"].ptr, _stream())
    _lib.check(code, "dmvs_fuse_view")
    torch.cuda.synchronize()
    out = {k: v.get() for k, v in g.items()}
    out["avg64_untouched"] = g["avg64"].untouched()
    for x in gin:
        assert x.raw().tobytes() == x.before[PAD:PAD + x.n].tobytes()
    return out


def run_emit(masks, avg64, counts, Kinv, Einv):
    """dmvs_fuse_emit on host arrays -> offsets, xyz, and which rows of xyz are untouched."""
    _, H, W = masks.shape
    nblk = R.workgroups(H, W)
    g = {"masks": Guard((3, H, W), u8, masks), "avg64": Guard((H, W), f64, avg64), "counts": Guard((nblk,), i32, counts),
         "offsets": Guard((nblk + 1,), i32), "xyz": Guard((H * W, 3), f32)}
    kinv, einv = np.ascontiguousarray(Kinv, np.float64), np.ascontiguousarray(Einv, np.float64)
    code = _lib.load().dmvs_fuse_emit(g["masks"].ptr, g["avg64"].ptr, g["counts"].ptr, H, W, kinv.ctypes.data_as(ctypes.c_void_p),
                                      einv.ctypes.data_as(ctypes.c_void_p), g["offsets"].ptr, g["xyz"].ptr, _stream())
    _lib.check(code, "dmvs_fuse_emit")
    torch.cuda.synchronize()
    for k in ("masks", "avg64", "counts"):
        assert g[k].raw().tobytes() == g[k].before[PAD:PAD + g[k].n].tobytes(), k
    return g["offsets"].get(), g["xyz"].get(), g["xyz"].untouched().all(1)


def _fmt(v):
    return "/".join(f"{x:.3g}" for x in v)


def _hold(tag, what, e_hip, e_ref):
    b = R.bounds(e_ref)
    print(f"{tag} {what}: e_hip {_fmt(e_hip)} e_ref {_fmt(e_ref)} bound {_fmt(b)} e_hip/bound {_fmt((e_hip[0] / b[0], e_hip[1] / b[1]))}")
    return e_hip[0] <= b[0] and e_hip[1] <= b[1]


def _check_emit(masks, avg64, counts, Kinv, Einv, tag):
    """Scan + emission against the restated geometry and the float64 points."""
    final = masks[2] != 0
    assert np.array_equal(counts, R.wg_counts(final)), tag
    offsets, xyz, untouched = run_emit(masks, avg64, counts, Kinv, Einv)
    n = int(final.sum())
    want = R.emit_points(final, avg64, Kinv, Einv)
    print(f"EMIT {tag}: workgroups {len(counts)} scan turns {R.scan_passes(len(counts))} count {n}")
    assert np.array_equal(offsets, R.scan_offsets(counts)), tag
    assert int(offsets[-1]) == n
    assert untouched[n:].all() and not untouched[:n].any(), tag
    nd = R._check_xyz(xyz[:n], want.astype(np.float32))     # row-major order: a permuted row is far more than 1 ulp off
    return n, nd


# ------------------------------------------------------------------------------------------------ SCENES
_SCENE_CACHE = {}


def _scene_ref(idx, ladder):
    """Restatement, fp32 oracle, bands and folded P of every pair of a SCENES row (computed once, never changed)."""
    key = (idx, ladder)
    if key not in _SCENE_CACHE:
        H, W, V, seed, _ = R.SCENES[idx]
        depths, confs, cam = R.scene(H, W, V, seed)
        gates = R.gate_list(ladder, *(R.LADDER_BASES if ladder else R.STATIC_GATE))
        pairs = []
        for v in range(1, V):
            f = R.pair(depths[0], *cam(0), depths[v], *cam(v), ladder)
            o = R.oracle_pair(depths[0], cam(0), depths[v], cam(v), ladder)
            pairs.append({"f64": f, "o32": o, "band": R.bands(o, f, gates), "P": fold_projection(*cam(0), *cam(v))})
        _SCENE_CACHE[key] = (depths, confs, cam, gates, pairs)
    return _SCENE_CACHE[key]


def _verdicts(tag, f, band, gates, planes, cap):
    """Every decided pixel of every gate carries the restated verdict; the undecided share is within the cap."""
    worst, wrong = 0.0, 0
    for (td, tr), got in zip(gates, planes):
        yes, no = R.decided(f[1], f[2], td, tr, band)
        worst = max(worst, float((~(yes | no)).mean()))
        wrong += int((got[yes] != 1).sum() + (got[no] != 0).sum())
    print(f"VERDICT {tag}: band_dist {band[0]:.3g} band_rel {band[1]:.3g} undecided {worst:.4f} cap {cap} wrong {wrong}")
    assert worst <= cap, tag
    assert wrong == 0, tag


@pytest.mark.parametrize("ladder", [False, True], ids=["static", "ladder"])
@pytest.mark.parametrize("idx", range(len(R.SCENES)), ids=[f"{s[0]}x{s[1]}" for s in R.SCENES])
def test_scene_pairs(idx, ladder):
    depths, _, _, gates, pairs = _scene_ref(idx, ladder)
    H, W = depths[0].shape
    base = R.LADDER_BASES if ladder else R.STATIC_GATE
    fails = []
    for v, pr in enumerate(pairs, 1):
        f, o = pr["f64"], pr["o32"]
        tag = f"{H}x{W} {'ladder' if ladder else 'static'} src {v}"
        # gates open: the mask is true wherever distance and relative difference are finite, depth_reproj is rz there
        op = run_pair(depths[0], depths[v], pr["P"], INF, INF, ladder)
        fin = np.isfinite(f[1]) & np.isfinite(f[2])
        assert np.array_equal(op["mask"] != 0, fin), (tag, int(((op["mask"] != 0) != fin).sum()))
        assert set(np.unique(op["mask"]).tolist()) <= {0, 1}
        fin_o = fin & np.isfinite(o[1]) & np.isfinite(o[2])
        if not _hold("OPEN", tag, R.errors(op["rep"], f[0], fin_o), R.errors(o[0], f[0], fin_o)):
            fails.append(("open", tag))
        assert (op["rep"][~fin] == 0).all()
        # the real gates
        out = run_pair(depths[0], depths[v], pr["P"], base[0], base[1], ladder)
        m = out["mask"] != 0
        planes = list(out["lv"]) if ladder else [out["mask"]]
        _verdicts(tag, f, pr["band"], gates, planes, R.LADDER_CAP if ladder else R.STATIC_CAP)
        assert np.array_equal(out["votes"], out["mask"].astype(np.int32)) and set(np.unique(out["mask"]).tolist()) <= {0, 1}
        if ladder:
            assert np.array_equal(out["lv"][8], out["votes"]) and set(np.unique(out["lv"]).tolist()) <= {0, 1}
        assert (out["rep"][~m] == 0).all() and out["dsum"].tobytes() == out["rep"].tobytes()
        both = m & R.verdict(o[1], o[2], *gates[-1])
        if not _hold("PAIR", tag + f" accepted {int(both.sum())}", R.errors(out["rep"], f[0], both), R.errors(o[0], f[0], both)):
            fails.append(("pair", tag))
    assert not fails, fails


def _check_fused(tag, d_ref, cam_ref, c321, th, srcs, src_cams, thres_view, dynamic):
    """The fused pass + scan + emission against the restatement: masks by the verdict rule, depth_avg by e_hip <= 8 e_ref over
    the pixels whose sources are all decided, counts / offsets / order / points by the restated geometry."""
    H, W = d_ref.shape
    base = R.LADDER_BASES if dynamic else R.STATIC_GATE
    want = R.view(d_ref, cam_ref, c321, th, srcs, src_cams, thres_view, dynamic)
    P = np.stack([fold_projection(*cam_ref, *c) for c in src_cams])
    out = run_view(d_ref, c321[0], c321[1], c321[2], srcs, P, th, dynamic, thres_view, *base)
    masks = out["masks"]
    assert set(np.unique(masks).tolist()) <= {0, 255}
    keep, worst = np.ones((H, W), bool), 0.0
    for s in range(len(srcs)):
        f = (want["rz"][s], want["dist"][s], want["rel"][s])
        band = R.bands(R.oracle_pair(d_ref, cam_ref, srcs[s], src_cams[s], dynamic), f, want["gates"])
        for td, tr in want["gates"]:
            yes, no = R.decided(f[1], f[2], td, tr, band)
            keep &= yes | no
            worst = max(worst, float((~(yes | no)).mean()))
    cap = R.LADDER_CAP if dynamic else R.STATIC_CAP
    wrong = [int(((masks[k] != 0) != want[n])[keep if k else np.ones_like(keep)].sum()) for k, n in enumerate(("photo", "geo", "final"))]
    print(f"VERDICT {tag}: sources {len(srcs)} all-decided {keep.mean():.4f} worst undecided per gate {worst:.4f} cap {cap} "
          f"wrong photo/geo/final {wrong} final {int((masks[2] != 0).sum())}")
    assert worst <= cap, tag
    assert wrong == [0, 0, 0], tag
    o_avg, o_votes = R.oracle_view_avg(d_ref, cam_ref, srcs, src_cams, dynamic)
    assert np.array_equal(o_votes[keep], want["votes"][keep])          # the yardstick flips no decided pixel
    ok = _hold("PAIR", tag + " depth_avg", R.errors(out["avg"], want["depth_avg"], keep), R.errors(o_avg, want["depth_avg"], keep))
    final = masks[2] != 0
    assert np.array_equal(out["avg64_untouched"], ~final), tag         # written at final pixels only
    assert np.array_equal(out["avg64"][final].astype(np.float32), out["avg"][final])
    K, E = (np.asarray(m, np.float32) for m in cam_ref)
    n, _ = _check_emit(masks, out["avg64"], out["counts"], np.linalg.inv(K).astype(np.float64), np.linalg.inv(E).astype(np.float64), tag)
    assert ok, tag
    return n, out


@pytest.mark.parametrize("dynamic", [False, True], ids=["static", "dynamic"])
@pytest.mark.parametrize("idx", range(len(R.SCENES)), ids=[f"{s[0]}x{s[1]}" for s in R.SCENES])
def test_scene_fused(idx, dynamic):
    depths, confs, cam, _, _ = _scene_ref(idx, dynamic)
    V = len(depths)
    c321 = (confs[0][2], confs[0][1], confs[0][0])
    _check_fused(f"{depths[0].shape[0]}x{depths[0].shape[1]} {'dynamic' if dynamic else 'static'}", depths[0], cam(0), c321,
                 R.SCENE_CONF, depths[1:], [cam(v) for v in range(1, V)], 2, dynamic)


# ------------------------------------------------------------------------------------------------ EXACT
def _exact_pair(tag, d_ref, d_src, P, td, tr, ladder):
    """One launch whose every output must equal the restatement's exactly.  -> (outputs, restatement)."""
    f = R.pair_P(d_ref, d_src, P, ladder)
    gates = R.gate_list(ladder, td, tr)
    out = run_pair(d_ref, d_src, P, td, tr, ladder)
    ok = R.verdict(f[1], f[2], *gates[-1])
    rep = np.where(ok, f[0], 0.0).astype(np.float32)
    same = [np.array_equal(out["mask"], ok.astype(np.uint8)), out["rep"].tobytes() == rep.tobytes(),
            np.array_equal(out["votes"], ok.astype(np.int32)), out["dsum"].tobytes() == rep.tobytes()]
    if ladder:
        lv = np.stack([R.verdict(f[1], f[2], a, b) for a, b in gates]).astype(np.int32)
        same.append(np.array_equal(out["lv"], lv))
    print(f"EXACT {tag} {'ladder' if ladder else 'static'} gate {td:.9g}/{tr:.9g}: accepted {int(ok.sum())} of {ok.size} "
          f"mask/rep/votes/dsum{'/levels' if ladder else ''} equal {same}")
    assert all(same), tag
    return out, f


@pytest.mark.parametrize("ladder", [False, True], ids=["static", "ladder"])
@pytest.mark.parametrize("row", R.EXACT_SHIFTS, ids=[r[0] for r in R.EXACT_SHIFTS])
def test_exact_taps(row, ladder):
    """Projections exactly on the tap boundaries: gates open (every pixel's rz is output, the all-outside row reaches the
    kz == 0 patch: without it the distance is NaN and the mask false) and a gate that the fully sampled pixels pass."""
    name, sx, sy = row[:3]
    d_ref, d_src, P = R.exact_case(sx, sy, 8)
    out, f = _exact_pair(name + " open", d_ref, d_src, P, INF, INF, ladder)
    assert (out["mask"] == 1).all()
    inner = R.interior(*R.EXACT_HW, sx, sy)
    assert (out["rep"][inner] == d_src[0, 0]).all()
    if name == "all-outside":
        assert not inner.any() and (out["rep"] == 0).all()
    # rel = 2^-8 where all four taps are inside; a partial sample is far off
    td, tr = (4.0, 2.0 ** -6) if not ladder else (0.4, 2.0 ** -6 / 10)
    out, _ = _exact_pair(name + " gated", d_ref, d_src, P, td, tr, ladder)
    assert np.array_equal(out["mask"] != 0, inner | (f[2] < 2.0 ** -6))
    assert inner.sum() >= (0 if name == "all-outside" else 8)


@pytest.mark.parametrize("row", R.EXACT_GATES, ids=[r[0] for r in R.EXACT_GATES])
def test_exact_gates(row):
    name, sx, sy, k, td, tr, verdict = row
    d_ref, d_src, P = R.exact_case(sx, sy, k)
    out, f = _exact_pair(name, d_ref, d_src, P, td, tr, False)
    inner = R.interior(*R.EXACT_HW, sx, sy)
    assert inner.sum() >= 8 and (out["mask"][inner] == int(verdict)).all()
    assert (f[1][inner] == np.hypot(sx, sy)).all() and (f[2][inner] == 2.0 ** -k).all()


@pytest.mark.parametrize("row", R.EXACT_LADDER, ids=[r[0] for r in R.EXACT_LADDER])
def test_exact_ladder_levels(row):
    name, sx, k, levels = row
    d_ref, d_src, P = R.exact_case(sx, 0.0, k)
    out, _ = _exact_pair(name, d_ref, d_src, P, *R.EXACT_LADDER_BASES, True)
    inner = R.interior(*R.EXACT_HW, sx, 0.0)
    assert inner.sum() >= 8
    for i in R.LEVELS:
        assert (out["lv"][i - 2][inner] == int(i in levels)).all(), (name, i)


def _exact_view(tag, d_ref, conf, srcs, P, dynamic, thres_view, td, tr, cam=None, exact_avg=True):
    want = R.view(d_ref, cam, (conf, conf, conf), (0.5, 0.5, 0.5), srcs, None, thres_view, dynamic, td, tr, P=P)
    out = run_view(d_ref, conf, conf, conf, srcs, P, (0.5, 0.5, 0.5), dynamic, thres_view, td, tr)
    same = [np.array_equal(out["masks"][k], np.where(want[n], 255, 0)) for k, n in enumerate(("photo", "geo", "final"))]
    final = want["final"]
    if exact_avg:
        same.append(out["avg"].tobytes() == want["depth_avg"].astype(np.float32).tobytes())
        same.append(np.array_equal(out["avg64"][final], want["depth_avg"][final]))
    same.append(np.array_equal(out["avg64_untouched"], ~final))
    same.append(np.array_equal(out["counts"], R.wg_counts(final)))
    print(f"EXACT {tag}: geo {int(want['geo'].sum())} final {int(final.sum())} of {final.size} photo/geo/final/[avg/avg64/]written/counts equal {same}")
    assert all(same), tag
    return out, want


def _conf(H, W):
    c = np.full((H, W), 0.75, np.float32)
    c[:, 0] = 0.25              # photo mask false in the first column; 0.5 itself fails the strict comparison
    c[0, 1] = 0.5
    return c


@pytest.mark.parametrize("shift,geo", [(0.5, True), (0.75, False)])
def test_exact_fused_dynamic_level(shift, geo):
    """Three sources at dist = shift under bases 1/4, 2^-10: level[1] counts gate i = 3 (dist < 0.75); 3 >= 3 holds at 0.5."""
    H, W = R.EXACT_HW
    cases = [R.exact_case(s * shift, 0.0, 12) for s in (1, -1, 1)]
    d_ref, P = cases[0][0], np.stack([c[2] for c in cases])
    out, want = _exact_view(f"dynamic shift {shift}", d_ref, _conf(H, W), [c[1] for c in cases], P, True, 2, *R.EXACT_LADDER_BASES)
    inner = R.interior(H, W, shift, 0.0) & R.interior(H, W, -shift, 0.0)
    assert inner.sum() >= 8 and ((out["masks"][1][inner] != 0) == geo).all()
    assert (want["levels"][1][inner] == (3 if geo else 0)).all() and (want["levels"][0][inner] == 0).all()


@pytest.mark.parametrize("nsrc", [1, 3])
def test_exact_fused_static_thres_view(nsrc):
    H, W = R.EXACT_HW
    cases = [R.exact_case(0.25 * s, 0.0, 8) for s in range(nsrc)]
    d_ref, P = cases[0][0], np.stack([c[2] for c in cases])
    inner = R.interior(H, W, 0.25 * (nsrc - 1), 0.0)
    for tv, geo in ((1, True), (nsrc, True), (nsrc + 1, False)):
        out, _ = _exact_view(f"static nsrc {nsrc} thres_view {tv}", d_ref, _conf(H, W), [c[1] for c in cases], P, False, tv, 1.0, 0.01)
        assert inner.sum() >= 8 and ((out["masks"][1][inner] != 0) == geo).all()


def test_exact_zero_reference_depth():
    """d = 0 with b1 = (2, 1, 1): every pixel projects to (2, 1) and samples c = fp32(1e-4).  The static filter patches the
    depth to 1e-4 (rel = 0, accepted within dist 1.5 of (2, 1)); the ladder divides by zero: all nine gates false."""
    H, W = R.EXACT_HW
    c = np.float32(1e-4)
    d_ref, d_src, P = np.zeros((H, W), np.float32), np.full((H, W), c, np.float32), R.make_P(b1=(2.0, 1.0, 1.0))
    x, y = R._grid(H, W)
    near = np.hypot(x - 2, y - 1) < 1.5
    out, _ = _exact_pair("zero depth", d_ref, d_src, P, 1.5, 0.01, False)
    assert np.array_equal(out["mask"] != 0, near) and near.sum() == 9 and (out["rep"][near] == c).all()
    out, _ = _exact_pair("zero depth", d_ref, d_src, P, 0.75, 0.005, True)            # last gate 7.5 px, 0.05
    assert not out["lv"].any() and not out["mask"].any()
    # averaged depth: (sum + d_base) / (votes + 1) with d_base = fp32(1e-4) under the static filter, 0 under the ladder
    conf = _conf(H, W)
    # (2 c + fp32(1e-4)) rounds once in fp32, the quotient once more, and fp32(1e-4) is 3e-9 off 1e-4: 4 * 2^-24 holds all three
    out, want = _exact_view("zero depth static", d_ref, conf, [d_src, d_src], np.stack([P, P]), False, 2, 1.5, 0.01, exact_avg=False)
    assert (out["avg"][~near] == c).all() and ((out["masks"][1] != 0) == near).all()
    assert (np.abs(out["avg"].astype(np.float64) - want["depth_avg"]) <= 4 * 2.0 ** -24 * want["depth_avg"]).all()
    out, _ = _exact_view("zero depth dynamic", d_ref, conf, [d_src, d_src], np.stack([P, P]), True, 2, 0.75, 0.005)
    assert (out["avg"] == 0).all() and not out["masks"][1].any()


def test_exact_average_and_points():
    """Dyadic depths, cameras and inverses: the averaged depth and the world points have no rounding at all."""
    H, W = R.EXACT_HW
    cases = [R.exact_case(0.0, 0.0, k) for k in (8, 9, 10)]
    d_ref, P = cases[0][0], np.stack([c[2] for c in cases])
    K = np.array([[4.0, 0, 2.0], [0, 8.0, 1.0], [0, 0, 1.0]], np.float32)
    E = np.array([[0, -1.0, 0, 16.0], [1.0, 0, 0, -8.0], [0, 0, 1.0, 0.5], [0, 0, 0, 1.0]], np.float32)
    out, want = _exact_view("dyadic points", d_ref, _conf(H, W), [c[1] for c in cases], P, False, 3, 1.0, 0.01, cam=(K, E))
    avg = (4.0 * 3 + 4.0 * (2.0 ** -8 + 2.0 ** -9 + 2.0 ** -10) + 4.0) / 4
    assert (out["avg"][:-1, :-1] == np.float32(avg)).all()
    Kinv, Einv = np.linalg.inv(K.astype(np.float64)), np.linalg.inv(E.astype(np.float64))
    offsets, xyz, untouched = run_emit(out["masks"], out["avg64"], out["counts"], Kinv, Einv)
    n = int(want["final"].sum())
    pts = R.emit_points(want["final"], want["depth_avg"], Kinv, Einv)
    assert n > 20 and int(offsets[-1]) == n and untouched[n:].all()
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
    assert xyz[:n].tobytes() == pts.astype(np.float32).tobytes() and xyz[:n].tobytes() == want["xyz"].astype(np.float32).tobytes()


# ------------------------------------------------------------------------------------------------ HOSTILE
def _hostile_maps(which, value, sx, sy):
    d_ref, d_src, P = R.exact_case(sx, sy, 8)
    m = d_ref if which == "ref" else d_src
    m[2, 3] = m[0, 0] = m[-1, -1] = m[3, 0] = value
    return d_ref, d_src, P


@pytest.mark.parametrize("ladder", [False, True], ids=["static", "ladder"])
@pytest.mark.parametrize("shift", [(0.0, 0.0), (0.375, 0.5), (-0.5, 0.0)], ids=["zero-weights", "inside", "half"])
@pytest.mark.parametrize("which", ["ref", "src"])
@pytest.mark.parametrize("name,value", R.HOSTILE_VALUES, ids=[v[0] for v in R.HOSTILE_VALUES])
def test_hostile_values(name, value, which, shift, ladder):
    """NaN, inf, negative and zero depths in either map; at shift (0, 0) the neighbours of a NaN source pixel sample it under
    a zero weight and are NaN too, as grid_sample has it.  Verdicts and values as the restatement's under IEEE rules."""
    d_ref, d_src, P = _hostile_maps(which, value, *shift)
    for td, tr in ((INF, INF), (4.0, 2.0 ** -6)):
        if ladder:
            td, tr = td / 10, tr / 10
        out, f = _exact_pair(f"{name} in {which} shift {shift}", d_ref, d_src, P, td, tr, ladder)
    if name == "nan" and which == "src" and shift == (0.0, 0.0):
        assert np.isnan(f[0][2, 2]) and np.isnan(f[0][1, 3]) and np.isnan(f[0][1, 2]) and not np.isnan(f[0][2, 4])
        assert out["mask"][2, 2] == 0 and out["mask"][2, 4] == 1
    if name == "neg" and which == "ref":
        assert f[2][2, 3] < 0                        # a negative reference depth passes the rel gate: the reference's behaviour


HOSTILE_P = (
    ("hz == 0, hx == hy == 0", dict(A1=np.zeros((3, 3)))),
    ("hz < 0", dict(b1=(0.0, 0.0, -2 * R.EXACT_D))),
    ("hz < 0 shifted", dict(b1=(-4 * R.EXACT_D, -2 * R.EXACT_D, -2 * R.EXACT_D))),
    ("xs = 1e30", dict(b1=(1e30 * R.EXACT_D, 0.0, 0.0))),
    ("ys = -1e30", dict(b1=(0.0, -1e30 * R.EXACT_D, 0.0))),
)


@pytest.mark.parametrize("ladder", [False, True], ids=["static", "ladder"])
@pytest.mark.parametrize("name,kw", HOSTILE_P, ids=[p[0] for p in HOSTILE_P])
def test_hostile_projection(name, kw, ladder):
    d_ref, d_src, _ = R.exact_case(0.0, 0.0, 8)
    P = R.make_P(**kw)
    xs, _ = R.project_P(d_ref, P)
    if name.startswith("hz == 0"):
        assert np.isnan(xs).all()
    for td, tr in ((INF, INF), (40.0, 2.0 ** -6)):
        if ladder:
            td, tr = td / 10, tr / 10
        out, f = _exact_pair(name, d_ref, d_src, P, td, tr, ladder)
    if name == "hz < 0 shifted":
        assert out["mask"].any()                     # behind the camera and accepted: nothing in the reference objects


# ------------------------------------------------------------------------------------------------ ACCUMULATE
@pytest.mark.parametrize("ladder", [False, True], ids=["static", "ladder"])
def test_accumulate_and_null_outputs(ladder):
    depths, _, _, _, pairs = _scene_ref(0, ladder)
    H, W = depths[0].shape
    base = R.LADDER_BASES if ladder else R.STATIC_GATE
    args = (depths[0], depths[1], pairs[0]["P"], base[0], base[1], ladder)
    fresh = run_pair(*args)
    again = run_pair(*args)
    outs = [k for k in PAIR_OUTS if k != "lv" or ladder]
    assert all(fresh[k].tobytes() == again[k].tobytes() for k in outs)
    rng = np.random.default_rng(7)
    init = {"votes": rng.integers(-5, 1000, (H, W)).astype(np.int32), "dsum": (rng.random((H, W)) * 3000).astype(np.float32),
            "lv": rng.integers(0, 50, (R.N_LEVELS, H, W)).astype(np.int32)}
    acc = run_pair(*args, init=init)
    same = {"votes": np.array_equal(acc["votes"], init["votes"] + fresh["votes"]),
            "dsum": acc["dsum"].tobytes() == (init["dsum"] + fresh["rep"]).tobytes(),
            "mask": acc["mask"].tobytes() == fresh["mask"].tobytes(), "rep": acc["rep"].tobytes() == fresh["rep"].tobytes()}
    if ladder:
        same["lv"] = np.array_equal(acc["lv"], init["lv"] + fresh["lv"])
    print(f"EXACT accumulate {'ladder' if ladder else 'static'}: accepted {int(fresh['mask'].sum())} equal {same}")
    assert all(same.values()), same
    for drop in outs:
        part = run_pair(*args, outs=[k for k in outs if k != drop])
        assert drop not in part and all(part[k].tobytes() == fresh[k].tobytes() for k in outs if k != drop), drop


@pytest.mark.parametrize("dynamic", [False, True], ids=["static", "dynamic"])
def test_fused_two_runs_bit_equal(dynamic):
    depths, confs, cam, _, pairs = _scene_ref(0, dynamic)
    base = R.LADDER_BASES if dynamic else R.STATIC_GATE
    P = np.stack([p["P"] for p in pairs])
    a, b = (run_view(depths[0], confs[0][2], confs[0][1], confs[0][0], depths[1:], P, R.SCENE_CONF, dynamic, 2, *base) for _ in range(2))
    assert all(a[k].tobytes() == b[k].tobytes() for k in ("masks", "avg", "avg64", "counts"))


# ------------------------------------------------------------------------------------------------ SOURCES
@pytest.mark.parametrize("dynamic,nsrc", R.SOURCES, ids=[f"{'dynamic' if d else 'static'}-{n}" for d, n in R.SOURCES])
def test_sources(dynamic, nsrc):
    H, W = R.SOURCES_HW
    depths, confs, cam = R.scene(H, W, nsrc + 1, nsrc)
    depths[0][0, :] = 0.0                          # zero reference depths in the first row
    tv = min(2, nsrc)
    tag = f"{'dynamic' if dynamic else 'static'} nsrc {nsrc}"
    srcs = list(range(1, nsrc + 1))
    stage = (confs[0][2], confs[0][1], confs[0][0])
    n1, _ = _check_fused(tag + " stage conf", depths[0], cam(0), stage, (0.1, 0.2, 0.3), [depths[s] for s in srcs], [cam(s) for s in srcs],
                         tv, dynamic)
    n2, _ = _check_fused(tag + " scalar conf", depths[0], cam(0), (stage[0],) * 3, (0.4,) * 3, [depths[s] for s in srcs],
                         [cam(s) for s in srcs], tv, dynamic)
    rev = srcs[::-1]
    n3, _ = _check_fused(tag + " reversed", depths[0], cam(0), stage, (0.1, 0.2, 0.3), [depths[s] for s in rev], [cam(s) for s in rev],
                         tv, dynamic)
    assert (n1 + n2 + n3 > 0) == (not dynamic or nsrc > 1)     # one source: the dynamic gates start at two views


# ------------------------------------------------------------------------------------------------ EMIT
@pytest.mark.parametrize("H,W", R.EMIT_SIZES, ids=[f"{h}x{w}" for h, w in R.EMIT_SIZES])
def test_emit_on_hand_made_masks(H, W):
    """dmvs_fuse_emit alone: counts from the restated geometry, depth_avg64 NaN at every pixel that is not final."""
    Kinv, Einv = np.linalg.inv(R.EMIT_K.astype(np.float64)), np.linalg.inv(R.EMIT_E.astype(np.float64))
    rng = np.random.default_rng(H * W)
    for name in R.EMIT_PATTERNS:
        final = R.emit_pattern(name, H, W)
        masks = np.stack((rng.integers(0, 2, (H, W)) * 255, rng.integers(0, 2, (H, W)) * 255, np.where(final, 255, 0))).astype(np.uint8)
        avg64 = np.where(final, R.emit_depths(H, W), np.nan)
        n, nd = _check_emit(masks, avg64, R.wg_counts(final), Kinv, Einv, f"{H}x{W} {name}")
        assert n == int(final.sum())
        if name == "all":
            assert n == H * W
