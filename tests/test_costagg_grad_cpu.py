"""CPU: the gradient yardsticks of the differentiable cost aggregation, and its boundary.

tests/golden/op_costagg_grad.npz holds the gradients the REFERENCE's CostAgg gives under autograd
(tests/golden/make_golden_costagg_grad.py).  The oracle under autograd must reproduce them -- which makes it a valid gradient
oracle on the GPU machine, where the reference does not exist -- and the float64 restatement (tests/costagg_grad_ref.py) must
agree with them at the fp32 level; that distance is each case's ``e_oracle``, the unit of the GPU parity bound."""
import os
import re

import numpy as np
import pytest
import torch

import costagg_grad_ref as R
from oracle import dmvs_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy


@pytest.fixture(scope="module")
def grad_golden(golden):
    return golden("op_costagg_grad.npz")


def load_case(g, name):
    V = R.GOLDEN_CASES[name]["V"]
    feats = [T(g[f"{name}.feat{v}"]) for v in range(V)]
    grads = [g[f"{name}.grad{v}"] for v in range(V)]
    return feats, T(g[f"{name}.proj"]), T(g[f"{name}.depth"]), T(g[f"{name}.gsim"]), g[f"{name}.sim"], grads


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_golden_inputs_are_the_synthetic_cases(grad_golden, name):
    """The stored inputs are make_case's (the GPU tests may regenerate them), the share of samples with a tap outside the
    image is in the 5-50 % band, and train and eval mode of the reference gave the same bits."""
    feats, cams, depth, gsim, _, _ = load_case(grad_golden, name)
    f2, c2, d2, g2 = R.make_case(**R.GOLDEN_CASES[name])
    assert all(torch.equal(a, b) for a, b in zip(feats, f2)) and torch.equal(cams, c2)
    assert torch.equal(depth, d2) and torch.equal(gsim, g2)
    share = float(grad_golden[f"{name}.outside_share"])
    assert 0.05 <= share <= 0.50
    assert abs(R.outside_share(cams, depth) - share) < 1e-3
    assert bool(grad_golden[f"{name}.train_eq_eval"])


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_oracle_gradients_equal_the_reference(grad_golden, name):
    """Bit for bit where the goldens were generated; a few ulp of the largest gradient elsewhere (other CPUs pick other
    vector kernels), the slack test_oracle.py allows on the same operator's forward (1e-6 at magnitude ~1)."""
    feats, cams, depth, gsim, sim_want, grads_want = load_case(grad_golden, name)
    sim, grads = R.grads_of(O.warp_corr, feats, cams, depth, gsim)
    np.testing.assert_allclose(sim.numpy(), sim_want, atol=1e-6 * max(1.0, np.abs(sim_want).max()), rtol=0)
    for v, (got, want) in enumerate(zip(grads, grads_want)):
        d = np.abs(got.numpy() - want).max()
        print(f"{name} grad{v}: max |oracle - reference| = {d:.3e} (|grad| max {np.abs(want).max():.3f})")
        assert d <= 1e-6 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_float64_restatement_agrees_at_fp32_level(grad_golden, name):
    """e_oracle = max |reference fp32 gradient - float64 restatement| per gradient tensor, recorded in the npz.  It is the
    reference's own rounding error (fp32 inverse, fp32 coordinates, fp32 sums): a few 1e-6 for cameras outside the sampled
    volume, up to a few 1e-5 for the turned camera inside it, where a coordinate is a ratio of numbers of magnitude 1e4 over
    a denominator of magnitude 10.  Checked: the recorded figure is reproduced (the float64 side moves by far less than the
    fp32 side's error between CPUs), and it is at the fp32 level -- below 1e-4 of the largest gradient."""
    feats, cams, depth, gsim, sim_want, grads_want = load_case(grad_golden, name)
    sim64, g64 = R.grads_f64(feats, cams, depth, gsim)
    assert sim64.dtype == torch.float64 and all(x.dtype == torch.float64 for x in g64)
    e_rec = grad_golden[f"{name}.e_oracle"]
    for v, (want, hi) in enumerate(zip(grads_want, g64)):
        e = np.abs(want.astype(np.float64) - hi.numpy()).max()
        print(f"{name} grad{v}: e_oracle = {e:.3e} (recorded {e_rec[v]:.3e}; |grad| max {np.abs(want).max():.3f})")
        assert abs(e - e_rec[v]) <= 0.05 * e_rec[v]
        assert e <= 1e-4 * np.abs(want).max()


def test_new_symbols_are_declared_exported_and_bound():
    from dmvsnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "dmvs.h")).read()
    lib = _lib.load()
    for name in ("dmvs_warp_corr_backward", "dmvs_nchw_to_q4"):
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/dmvs.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1]
    assert lib.dmvs_version() == 140   # additive: the ABI version does not move
    # argument checks run on the host, before any launch
    assert lib.dmvs_warp_corr_backward(None, None, 1, None, None, None, None, None, 8, 4, 8, 8, None) == _lib.EINVAL
    assert lib.dmvs_nchw_to_q4(None, 64, 0, 8, 8, 8, None, None) == _lib.EINVAL


def test_diff_cost_agg_boundary():
    """Reference constructor and forward signature, no parameters, 'adaptive' refused as in mvsnet.CostAgg, CPU tensors
    refused with DmvsError (there is no fallback) -- and so are fp16 features and unsupported channel counts."""
    import inspect
    import dmvsnet_amd
    from dmvsnet_amd._lib import DmvsError
    agg = dmvsnet_amd.DiffCostAgg("variance", [32, 16, 8])
    assert list(inspect.signature(agg.forward).parameters)[:4] == ["features", "proj_matrices", "depth_values", "stage_idx"]
    assert list(agg.parameters()) == [] and list(agg.buffers()) == []
    agg.train()
    agg.eval()
    with pytest.raises(NotImplementedError):
        dmvsnet_amd.DiffCostAgg("adaptive", [32, 16, 8])
    with pytest.raises(AssertionError):
        dmvsnet_amd.DiffCostAgg("bogus")
    feats, cams, depth, _ = R.make_case(**R.GOLDEN_CASES["c8_v3_d4"])
    with pytest.raises(DmvsError):
        agg([f.requires_grad_(True) for f in feats], cams, depth, 0)
    with pytest.raises(DmvsError):
        dmvsnet_amd.cost_agg(feats, cams, depth)


def test_training_stays_out_of_the_product_model():
    from dmvsnet_amd import MVSNet
    with pytest.raises(NotImplementedError):
        MVSNet([8], [4], verbose=False).train()
    import dmvsnet_amd.costagg as ca
    src = open(ca.__file__).read()
    assert not re.search(r"^\s*(from|import)\s+oracle", src, re.M)
