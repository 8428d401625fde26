"""CPU: the boundary of K1b's deterministic mode -- the two C entries are declared and exported under the unchanged ABI version, the
workspace size is the int64 sums and nothing else, both Python wrappers (one validation body) refuse what they cannot launch with a
``DmvsError`` that names the public function, and both C entries (one entry body) answer the same code for the same bad argument list
(no GPU is touched: every refusal happens before a launch)."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dmvs_warp_corr_backward_det_workspace", "dmvs_warp_corr_backward_det")


def test_entries_are_declared_and_exported_under_abi_140():
    from dmvsnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "dmvs.h")).read()
    declared = set(re.findall(r"\b(dmvs_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define DMVS_VERSION 140\b", header)
    assert lib.dmvs_version() == _lib.ABI_VERSION == 140
    # the existing entry keeps its declaration
    assert "dmvs_warp_corr_backward" in declared and len(_lib.SIGNATURES["dmvs_warp_corr_backward"][1]) == 13
    assert len(_lib.SIGNATURES["dmvs_warp_corr_backward_det"][1]) == 16


@pytest.mark.parametrize("C", (8, 16, 32))
def test_workspace_is_the_int64_sums(C):
    from dmvsnet_amd import _lib, ops
    lib = _lib.load()
    for H, W, nact in ((1, 1, 1), (9, 33, 1), (9, 65, 3), (128, 160, 16), (512, 640, 4), (7, 31, 0)):
        assert lib.dmvs_warp_corr_backward_det_workspace(C, H, W, nact) == 8 * nact * C * H * W
        assert ops.warp_corr_backward_det_workspace(C, H, W, nact) == 8 * nact * C * H * W
    for bad in ((12, 9, 33, 1), (C, 0, 33, 1), (C, 9, 0, 1), (C, 9, 33, -1), (C, 9, 33, 17)):
        assert lib.dmvs_warp_corr_backward_det_workspace(*bad) == 0, bad


def _args(C=8, D=3, H=9, W=33, nsrc=2):
    q4 = lambda: torch.zeros((C // 4, H, W, 4))   # noqa: E731
    return dict(ref_q4=q4(), src_q4=[q4() for _ in range(nsrc)], proj12=torch.zeros((nsrc, 12)), depth_dhw=torch.ones((D, H, W)),
                gsim=torch.zeros((2, D, H, W)), gref=torch.zeros((C, H, W)), gsrc=[torch.zeros((C, H, W)) for _ in range(nsrc)])


def test_wrapper_mirrors_the_atomic_one():
    from dmvsnet_amd import ops
    a = list(inspect.signature(ops.warp_corr_backward).parameters)
    b = inspect.signature(ops.warp_corr_backward_det).parameters
    assert list(b)[:len(a)] == a and list(b)[len(a):] == ["workspace", "variant"]
    assert b["variant"].default == 0 and b["workspace"].default is None


WRAPPERS = ("warp_corr_backward", "warp_corr_backward_det")   # one validation body: both refuse the same, each under its own name


def refused(what, args, match=None):
    from dmvsnet_amd import ops
    from dmvsnet_amd._lib import DmvsError
    with pytest.raises(DmvsError, match=match or rf"\b{what}: "):
        getattr(ops, what)(**args)


def test_wrapper_refuses_cpu_tensors():
    for what in WRAPPERS:
        refused(what, _args(), match="HIP device")


@pytest.mark.parametrize("field,shape", [("gsim", (2, 4, 9, 33)), ("gsim", (1, 3, 9, 33)), ("proj12", (3, 12)), ("proj12", (2, 9)),
                                         ("depth_dhw", (1, 3, 9, 33)), ("gref", (4, 9, 33)), ("ref_q4", (9, 33, 8)),
                                         ("ref_q4", (2, 9, 32, 4))])
def test_wrapper_refuses_wrong_shapes(field, shape):
    for what in WRAPPERS:
        a = _args()
        a[field] = torch.zeros(shape)
        refused(what, a)


def test_wrapper_refuses_wrong_lists_and_workspaces():
    for what in WRAPPERS:
        a = _args()
        a["gsrc"] = a["gsrc"][:1]
        refused(what, a)
        a = _args()
        a["gsrc"][1] = torch.zeros((8, 9, 32))
        refused(what, a)
        a = _args()
        a["src_q4"][0] = torch.zeros((2, 9, 34, 4))
        refused(what, a)


def test_both_c_entries_refuse_the_same_before_any_launch():
    """The raw entries on host dummies: every case below returns before a HIP call, and nothing is dereferenced before it."""
    import ctypes
    from dmvsnet_amd import _lib
    lib = _lib.load()
    dummy = (ctypes.c_float * 16)()
    p = ctypes.cast(dummy, ctypes.c_void_p)
    views = lambda *ps: (ctypes.c_void_p * len(ps))(*ps)   # noqa: E731

    def call(det, ref=p, src=None, nsrc=2, gsrc=None, C=8, D=3, H=9, W=33, ws=None, ws_bytes=0, variant=0):
        src = views(*[p] * min(max(nsrc, 1), 17)) if src is None else src
        head = (ref, src, nsrc, p, p, p, p, gsrc, C, D, H, W)
        if det:
            return lib.dmvs_warp_corr_backward_det(*head, ws, ws_bytes, variant, None)
        return lib.dmvs_warp_corr_backward(*head, None)

    table = [(dict(ref=None), _lib.EINVAL), (dict(nsrc=0), _lib.EINVAL), (dict(nsrc=17), _lib.EINVAL), (dict(D=0), _lib.EINVAL),
             (dict(H=0), _lib.EINVAL), (dict(W=0), _lib.EINVAL), (dict(C=12), _lib.EUNSUPPORTED),
             (dict(C=32, H=4096, W=4096), _lib.EUNSUPPORTED), (dict(src=views(p, None)), _lib.EINVAL)]
    for kw, code in table:
        assert call(False, **kw) == call(True, **kw) == code, kw
    assert call(True, variant=2) == _lib.EINVAL
    # a wanted view: the deterministic entry needs an 8-byte aligned workspace that is large enough
    need = lib.dmvs_warp_corr_backward_det_workspace(8, 9, 33, 1)
    odd = ctypes.c_void_p((p.value & ~7) + 4)
    for ws, ws_bytes in ((None, need), (odd, need), (ctypes.c_void_p(p.value & ~7), need - 1)):
        assert call(True, gsrc=views(p, None), ws=ws, ws_bytes=ws_bytes) == _lib.EINVAL, (ws, ws_bytes)


def test_cost_agg_takes_the_keyword_and_exports_nothing_new():
    import dmvsnet_amd
    from dmvsnet_amd import costagg
    assert inspect.signature(costagg.cost_agg).parameters["deterministic"].default is None
    assert inspect.signature(costagg.DiffCostAgg.__init__).parameters["deterministic"].default is None
    assert list(inspect.signature(costagg.cost_agg).parameters)[:3] == ["features", "proj_matrices", "depth_values"]
    assert set(costagg.launch_counts) == set(costagg.det_launch_counts) == {"bwd_ref", "bwd_src_views"}
    assert costagg.det_launch_counts is not costagg.launch_counts
    assert not hasattr(dmvsnet_amd, "det_launch_counts") and not hasattr(dmvsnet_amd, "warp_corr_backward_det")
    assert costagg.DiffCostAgg("variance", 8, deterministic=True).deterministic is True
