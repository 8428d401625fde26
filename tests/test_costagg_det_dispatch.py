"""CPU: the boundary of K1b's deterministic mode -- the two C entries are declared and exported under the unchanged ABI version, the
workspace size is the int64 sums and nothing else, and the Python wrapper refuses what it cannot launch with ``DmvsError`` (no GPU
is touched: every refusal happens before a launch)."""
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


def test_wrapper_refuses_cpu_tensors():
    from dmvsnet_amd import ops
    from dmvsnet_amd._lib import DmvsError
    with pytest.raises(DmvsError, match="HIP device"):
        ops.warp_corr_backward_det(**_args())


@pytest.mark.parametrize("field,shape", [("gsim", (2, 4, 9, 33)), ("gsim", (1, 3, 9, 33)), ("proj12", (3, 12)), ("proj12", (2, 9)),
                                         ("depth_dhw", (1, 3, 9, 33)), ("gref", (4, 9, 33)), ("ref_q4", (9, 33, 8)),
                                         ("ref_q4", (2, 9, 32, 4))])
def test_wrapper_refuses_wrong_shapes(field, shape):
    from dmvsnet_amd import ops
    from dmvsnet_amd._lib import DmvsError
    a = _args()
    a[field] = torch.zeros(shape)
    with pytest.raises(DmvsError, match="warp_corr_backward_det"):
        ops.warp_corr_backward_det(**a)


def test_wrapper_refuses_wrong_lists_and_workspaces():
    from dmvsnet_amd import ops
    from dmvsnet_amd._lib import DmvsError
    a = _args()
    a["gsrc"] = a["gsrc"][:1]
    with pytest.raises(DmvsError, match="warp_corr_backward_det"):
        ops.warp_corr_backward_det(**a)
    a = _args()
    a["gsrc"][1] = torch.zeros((8, 9, 32))
    with pytest.raises(DmvsError, match="warp_corr_backward_det"):
        ops.warp_corr_backward_det(**a)
    a = _args()
    a["src_q4"][0] = torch.zeros((2, 9, 34, 4))
    with pytest.raises(DmvsError, match="warp_corr_backward_det"):
        ops.warp_corr_backward_det(**a)


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
