"""CPU: the boundary of K1b's pre-summed scatter -- the two C entries are declared and exported under the unchanged ABI version, the
capacity entry answers, the Python wrapper and the C entry refuse what they cannot launch before any device is touched, the keyword
reaches ``cost_agg`` / ``DiffCostAgg`` / ``DiffMVSNet``, and the box restatement the GPU file counts workgroups with
(tests/costagg_presum_ref.py) says what it should on the two capacity cases and on a seam case."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import costagg_presum_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dmvs_warp_corr_backward_presum_cap", "dmvs_warp_corr_backward_presum")


def test_entries_are_declared_and_exported_under_abi_140():
    from dmvsnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "dmvs.h")).read()
    declared = set(re.findall(r"\b(dmvs_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define DMVS_VERSION 140\b", header)
    assert lib.dmvs_version() == _lib.ABI_VERSION == 140
    assert len(_lib.SIGNATURES["dmvs_warp_corr_backward_presum"][1]) == 18
    # the existing entries keep their declarations
    assert len(_lib.SIGNATURES["dmvs_warp_corr_backward"][1]) == 13 and len(_lib.SIGNATURES["dmvs_warp_corr_backward_det"][1]) == 16


@pytest.mark.parametrize("C", (8, 16, 32))
def test_capacity_is_positive_and_smaller_with_variant_bit_1(C):
    from dmvsnet_amd import _lib, ops
    for det in (False, True):
        full, rev = ops.warp_corr_backward_presum_cap(C, det), ops.warp_corr_backward_presum_cap(C, det, 1)
        small, small_rev = ops.warp_corr_backward_presum_cap(C, det, 2), ops.warp_corr_backward_presum_cap(C, det, 3)
        assert full == rev > small == small_rev > 0 and small <= 256
        # two workgroups of 8 window channels in a CU's 160 KB of LDS
        assert 2 * full * 8 * (8 if det else 4) <= 160 * 1024
    assert ops.warp_corr_backward_presum_cap(C, True) <= ops.warp_corr_backward_presum_cap(C, False)
    lib = _lib.load()
    for bad in ((12, 0, 0), (C, 0, 4), (C, 1, -1)):
        assert lib.dmvs_warp_corr_backward_presum_cap(*bad) == 0, bad


def _args(C=8, D=3, H=9, W=33, nsrc=2):
    q4 = lambda: torch.zeros((C // 4, H, W, 4))   # noqa: E731
    return dict(ref_q4=q4(), src_q4=[q4() for _ in range(nsrc)], proj12=torch.zeros((nsrc, 12)), depth_dhw=torch.ones((D, H, W)),
                gsim=torch.zeros((2, D, H, W)), gref=torch.zeros((C, H, W)), gsrc=[torch.zeros((C, H, W)) for _ in range(nsrc)])


def test_wrapper_extends_the_deterministic_one():
    from dmvsnet_amd import ops
    a = list(inspect.signature(ops.warp_corr_backward).parameters)
    b = inspect.signature(ops.warp_corr_backward_presum).parameters
    assert list(b)[:len(a)] == a and list(b)[len(a):] == ["deterministic", "workspace", "variant", "path_counts"]
    assert b["deterministic"].default is False and b["workspace"].default is None and b["variant"].default == 0
    assert b["path_counts"].default is None


def refused(match, **kw):
    from dmvsnet_amd import ops
    from dmvsnet_amd._lib import DmvsError
    with pytest.raises(DmvsError, match=match):
        ops.warp_corr_backward_presum(**kw)


def test_wrapper_refuses_without_a_device():
    for det in (False, True):
        refused("HIP device", **_args(), deterministic=det)
        refused(r"warp_corr_backward_presum: variant", **_args(), deterministic=det, variant=4)
        refused(r"warp_corr_backward_presum: variant", **_args(), deterministic=det, variant=-1)
        refused(r"warp_corr_backward_presum: path_counts", **_args(), deterministic=det, path_counts=torch.zeros(3))
        refused(r"warp_corr_backward_presum: path_counts", **_args(), deterministic=det, path_counts=torch.zeros(2, dtype=torch.int32))
        a = _args()
        a["gsim"] = torch.zeros((2, 4, 9, 33))
        refused(r"\bwarp_corr_backward_presum: ", **a, deterministic=det)
    need = 8 * 2 * 8 * 9 * 33
    refused(r"warp_corr_backward_presum: a workspace of", **_args(), deterministic=True,
            workspace=torch.zeros((need // 8 - 1,), dtype=torch.int64))
    # the atomic mode ignores the workspace: the next refusal is the device's
    refused("HIP device", **_args(), deterministic=False, workspace=torch.zeros((1,), dtype=torch.int64))


def test_c_entry_refuses_what_the_existing_entries_refuse_before_any_launch():
    """The raw entry on host dummies: every case returns before a HIP call, and nothing is dereferenced before it."""
    from dmvsnet_amd import _lib
    lib = _lib.load()
    dummy = (ctypes.c_float * 16)()
    p = ctypes.cast(dummy, ctypes.c_void_p)
    views = lambda *ps: (ctypes.c_void_p * len(ps))(*ps)   # noqa: E731

    def call(det, ref=p, src=None, nsrc=2, gsrc=None, C=8, D=3, H=9, W=33, ws=None, ws_bytes=0, variant=0):
        src = views(*[p] * min(max(nsrc, 1), 17)) if src is None else src
        return lib.dmvs_warp_corr_backward_presum(ref, src, nsrc, p, p, p, p, gsrc, C, D, H, W, det, ws, ws_bytes, variant, None, None)

    table = [(dict(ref=None), _lib.EINVAL), (dict(nsrc=0), _lib.EINVAL), (dict(nsrc=17), _lib.EINVAL), (dict(D=0), _lib.EINVAL),
             (dict(H=0), _lib.EINVAL), (dict(W=0), _lib.EINVAL), (dict(C=12), _lib.EUNSUPPORTED),
             (dict(C=32, H=4096, W=4096), _lib.EUNSUPPORTED), (dict(src=views(p, None)), _lib.EINVAL), (dict(variant=4), _lib.EINVAL),
             (dict(variant=-1), _lib.EINVAL)]
    for kw, code in table:
        assert call(0, **kw) == call(1, **kw) == code, kw
    need = lib.dmvs_warp_corr_backward_det_workspace(8, 9, 33, 1)
    odd = ctypes.c_void_p((p.value & ~7) + 4)
    for ws, ws_bytes in ((None, need), (odd, need), (ctypes.c_void_p(p.value & ~7), need - 1)):
        for variant in range(4):
            assert call(1, gsrc=views(p, None), ws=ws, ws_bytes=ws_bytes, variant=variant) == _lib.EINVAL, (ws, ws_bytes)


def test_the_keyword_reaches_cost_agg_the_module_and_the_model():
    import dmvsnet_amd
    from dmvsnet_amd import costagg, train
    assert inspect.signature(costagg.cost_agg).parameters["presum"].default is False
    assert inspect.signature(costagg.DiffCostAgg.__init__).parameters["presum"].default is False
    assert inspect.signature(train.DiffMVSNet.__init__).parameters["presum"].default is False
    assert list(inspect.signature(costagg.cost_agg).parameters)[:4] == ["features", "proj_matrices", "depth_values", "deterministic"]
    assert set(costagg.presum_launch_counts) == set(costagg.launch_counts) == {"bwd_ref", "bwd_src_views"}
    assert costagg.presum_launch_counts is not costagg.launch_counts and costagg.presum_launch_counts is not costagg.det_launch_counts
    assert not hasattr(dmvsnet_amd, "presum_launch_counts") and not hasattr(dmvsnet_amd, "warp_corr_backward_presum")
    m = costagg.DiffCostAgg("variance", 8, deterministic=True, presum=True)
    assert m.presum is True and m.deterministic is True
    assert costagg.DiffCostAgg("variance", 8).presum is False
    net = train.DiffMVSNet([8, 8, 8], [4, 2, 1], presum=True)
    assert net.cost_aggregation.presum is True and net.cost_aggregation.deterministic is None
    assert train.DiffMVSNet([8, 8, 8], [4, 2, 1]).cost_aggregation.presum is False
    with pytest.raises(dmvsnet_amd._lib.DmvsError, match="HIP kernels only"):   # presum changes no refusal of cost_agg
        costagg.cost_agg([torch.zeros((1, 8, 4, 4))] * 2, torch.zeros((1, 2, 2, 4, 4)), torch.ones((1, 2, 4, 4)), presum=True)


# ------------------------------------------------------------------------------------------------ the box restatement
def test_capacity_cases_sit_on_both_sides_of_the_test_capacity():
    from dmvsnet_amd import ops
    cap = ops.warp_corr_backward_presum_cap(8, False, 2)
    assert cap == ops.warp_corr_backward_presum_cap(8, True, 2) == 256
    at, over = PR.capacity_cases(cap)
    for case, want, path in ((at, cap, 0), (over, cap + 1, 1)):
        D, H, W = case["depth"].shape
        assert (D, H) == PR.CAP_SHAPE_DH and W == cap + 1 and ((W - 1) // 2) & ((W - 1) // 2 - 1) == 0   # (W - 1) / 2 a power of two
        for dch in (8, 4):
            bx = PR.boxes(case["p12"][0], case["depth"], dch)
            assert len(bx) == ((W + 63) // 64) * 2
            for (tx, ty, c), box in bx.items():
                if tx == 0:   # one row (the last), every column of the map but the first / every column
                    assert box == (1 - path, W - 1, H - 1, H - 1) and PR.texels(box) == want and PR.path_of(box, cap) == path
                else:
                    assert box is None and PR.path_of(box, cap) == 2
        tiles = (W + 63) // 64
        for variant in (2, 3):
            counts = PR.predict(case["p12"], case["depth"], 8, cap, variant)
            assert counts == ([2, 0, 2 * (tiles - 1)] if path == 0 else [0, 2, 2 * (tiles - 1)])
        # at the full capacity both are windowed
        assert PR.predict(case["p12"], case["depth"], 8, ops.warp_corr_backward_presum_cap(8, True, 0), 0)[:2] == [2, 0]


def test_boxes_of_a_seam_case():
    """Offset (-0.5, 0.5): x0 = x - 1, x1 = x, y0 = y, y1 = y + 1, no sample on an integer.  Runs no product code: it holds the test
    helper the GPU file counts workgroups with to boxes worked out by hand, and passes with or without the feature."""
    case = PR.seam_cases()[PR.seam_name(32, -0.5, 0.5)]
    D, H, W = case["depth"].shape
    assert (D, H, W) == PR.SEAM_SHAPE == (9, 9, 130)
    bx = PR.boxes(case["p12"][0], case["depth"], 8)
    assert len(bx) == 3 * 3 * 2
    cols = {0: (0, 63), 1: (63, 127), 2: (127, 129)}   # x = 0 loses its left tap; neighbouring tiles share a column
    rows = {0: (0, 4), 1: (4, 8), 2: (8, 8)}           # neighbouring tile rows share a row; y = 8 loses its lower taps
    for (tx, ty, c), box in bx.items():
        assert box == cols[tx] + rows[ty], (tx, ty, c)
    assert PR.texels(bx[(0, 0, 0)]) == 320 and PR.texels(bx[(1, 1, 1)]) == 325 and PR.texels(bx[(2, 2, 0)]) == 3
    # C = 32: four quad groups.  Full capacity: every workgroup windowed; test capacity: the full tiles of the full tile rows fall back
    assert PR.predict(case["p12"], case["depth"], 32, 960) == [4 * 18, 0, 0]
    assert PR.predict(case["p12"], case["depth"], 32, 256) == [4 * 10, 4 * 8, 0]
    assert PR.predict(case["p12"], case["depth"], 32, 256, variant=1) == [4 * 15, 4 * 12, 0]   # chunks of 4: 4 + 4 + 1 planes
    # a view that is not asked for launches nothing
    assert PR.predict(case["p12"], case["depth"], 32, 256, views=()) == [0, 0, 0]


def test_the_op_order_restatement_itself_exceeds_the_plain_max_bound_on_seams():
    """Runs no product code (it passes with or without the feature).  What licenses the WINDOWS rule for SEAMS in the GPU file: (W - 1) / 2 = 64.5 is no power of two, so the reference's normalise /
    un-normalise round trip (``ref_order_taps``) moves a sample by ulps while e_ref sits at the criterion's floor.  The fp32 restatement
    WITH the round trip -- no kernel runs here -- exceeds the plain max bound on every case (1.27 - 2.11 x on dRef) and keeps the mean
    below 0.05 of its bound; without the round trip it is e_ref itself."""
    import warp_corr_grad_ref as GR
    for name, c in PR.seam_cases().items():
        g64, e_ref = GR.reference(c, c["p12"])
        gro = GR.grads_ref(c["feats"], c["p12"], c["depth"], c["gsim"], GR.F32, ref_order=True)
        ratios = []
        for k in range(2):
            e, b = GR.errors(gro[k], g64[k]), GR.bounds(e_ref[k])
            ratios.append((e[0] / b[0], e[1] / b[1]))
        print(f"PRESUM {name}: op-order restatement / plain bound (max, mean) dRef {ratios[0]}, dSrc {ratios[1]}")
        assert max(r[0] for r in ratios) > 1.0, name
        if name.endswith("-0_0"):   # where the GPU file keeps the plain max bound: dSrc of the identity cases
            assert ratios[1][0] < 1.0, name
        assert all(r[1] < 0.05 for r in ratios), name
