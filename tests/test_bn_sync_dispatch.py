"""CPU (-m "not gpu"): what the four sync wrappers of K5 (ops.bn_sync_moments / _forward / _backward_sums / _backward_apply), the autograd
Function behind ``DiffSyncBatchNormReLU*`` and the modules themselves launch, without a GPU and without a process group -- on the
recording library, timer and stubs of tests/test_train_dispatch.py (imported, not copied).  Pinned: the C entry and its integer arguments,
the launch_log families (one per dispatch), the timer record, nothing logged or timed when the launch fails, the refusals before any
launch, and the order moments -> all-gather -> apply in both directions, with the second collective if and only if the input needs a
gradient.  ``torch.distributed.all_gather_into_tensor`` is replaced by a stub that records itself among the launches."""
import contextlib
import types

import pytest
import torch

from dmvsnet_amd import _lib, bn, ops
from dmvsnet_amd.ops import BN_TRAIN, RELU
from test_train_dispatch import EINVAL, _ok, _refused, _ws, fake  # noqa: F401  (``fake`` is the fixture)

B, C, SP = 2, 8, (3, 5)
V = 15
NV = B * C * V


def _vec():
    return [torch.zeros(C) for _ in range(4)]


def _x():
    return torch.zeros(B, C, *SP)


def _ws5():
    return _ws("dmvs_bn_workspace", C, B, V)


def test_moments(fake):
    lib = fake()
    m = ops.bn_sync_moments(_x(), workspace=_ws5())
    assert m.dtype == torch.float64 and tuple(m.shape) == (C, 3)
    _ok(lib, [("dmvs_bn_sync_moments", (B, C, V))], ["batchnorm"] * 2, ("batchnorm", "bn8", 3.0 * NV, 4.0 * NV, 3.0 * NV))


@pytest.mark.parametrize("R", [1, 3, 16])
@pytest.mark.parametrize("relu", [True, False])
def test_forward(fake, relu, R):
    lib = fake()
    y, mean, invstd, N = ops.bn_sync_forward(_x(), *_vec(), torch.zeros(R, C, 3, dtype=torch.float64), 0.1, 1e-5, relu)
    assert y.shape == _x().shape and mean.shape == invstd.shape == (C,) and N == 0   # (the count is the library's to write)
    _ok(lib, [("dmvs_bn_sync_forward", (B, C, V, R, RELU if relu else 0))], ["batchnorm"], ("batchnorm", "bn8", 5.0 * NV, 8.0 * NV, 5.0 * NV))


def test_backward_sums(fake):
    lib = fake()
    sums, gg, gb = ops.bn_sync_backward_sums(_x(), _x(), *_vec(), True, workspace=_ws5())
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (C, 2) and gg.shape == gb.shape == (C,) and gg.dtype == torch.float32
    _ok(lib, [("dmvs_bn_sync_backward_sums", (B, C, V, RELU))], ["batchnorm"] * 2, ("batchnorm", "bn8", 7.0 * NV, 8.0 * NV, 7.0 * NV))


def test_backward_apply(fake):
    lib = fake()
    gx = ops.bn_sync_backward_apply(_x(), _x(), *_vec(), torch.zeros(3, C, 2, dtype=torch.float64), 4 * V, False)
    assert gx.shape == _x().shape
    _ok(lib, [("dmvs_bn_sync_backward_apply", (B, C, V, 3, 4 * V, 0))], ["batchnorm"], ("batchnorm", "bn8", 8.0 * NV, 12.0 * NV, 8.0 * NV))


def test_launch_fails(fake):
    g3, g2 = torch.zeros(2, C, 3, dtype=torch.float64), torch.zeros(2, C, 2, dtype=torch.float64)
    calls = {"dmvs_bn_sync_moments": (lambda: ops.bn_sync_moments(_x(), workspace=_ws5()), (B, C, V)),
             "dmvs_bn_sync_forward": (lambda: ops.bn_sync_forward(_x(), *_vec(), g3, 0.1, 1e-5, True), (B, C, V, 2, RELU)),
             "dmvs_bn_sync_backward_sums": (lambda: ops.bn_sync_backward_sums(_x(), _x(), *_vec(), True, workspace=_ws5()), (B, C, V, RELU)),
             "dmvs_bn_sync_backward_apply": (lambda: ops.bn_sync_backward_apply(_x(), _x(), *_vec(), g2, 2 * B * V, True),
                                             (B, C, V, 2, 2 * B * V, RELU))}
    for entry, (call, ints) in calls.items():
        lib = fake({entry: EINVAL})
        with pytest.raises(_lib.DmvsError):
            call()
        _refused(lib, [(entry, ints)])


def test_refusals(fake):
    lib = fake()
    x, ws = _x(), _ws5()
    with pytest.raises(_lib.DmvsError, match="workspace too small"):
        ops.bn_sync_moments(x, workspace=ws[1:])
    with pytest.raises(_lib.DmvsError, match="workspace too small"):
        ops.bn_sync_backward_sums(x, x, *_vec(), True, workspace=ws[1:])
    with pytest.raises(_lib.DmvsError, match="per-channel vector"):
        ops.bn_sync_forward(x, torch.zeros(C + 1), *_vec()[1:], torch.zeros(2, C, 3, dtype=torch.float64), 0.1, 1e-5, True)
    with pytest.raises(_lib.DmvsError, match="same shape"):
        ops.bn_sync_backward_sums(x, torch.zeros(B, C, V), *_vec(), True, workspace=ws)
    with pytest.raises(_lib.DmvsError, match="same shape"):
        ops.bn_sync_backward_apply(x, torch.zeros(B, C, V), *_vec(), torch.zeros(2, C, 2, dtype=torch.float64), 60, True)
    for bad in (torch.zeros(2, C, 3), torch.zeros(2, C, 2, dtype=torch.float64), torch.zeros(2 * C, 3, dtype=torch.float64),
                torch.zeros(2, 3, C, dtype=torch.float64).transpose(1, 2), torch.zeros(0, C, 3, dtype=torch.float64),
                torch.zeros(ops.BN_MAX_RANKS + 1, C, 3, dtype=torch.float64)):
        with pytest.raises(_lib.DmvsError, match="gathered buffer|ranks"):
            ops.bn_sync_forward(x, *_vec(), bad, 0.1, 1e-5, True)
    with pytest.raises(_lib.DmvsError, match="gathered buffer"):
        ops.bn_sync_backward_apply(x, x, *_vec(), torch.zeros(2, C, 3, dtype=torch.float64), 60, True)
    x24 = torch.zeros(B, 24, *SP)   # the default workspace's size query refuses, before any device is asked for
    with pytest.raises(_lib.DmvsError, match="not covered by the BatchNorm kernels"):
        ops.bn_sync_moments(x24)
    _refused(lib)


# ------------------------------------------------------------------------------------------ the autograd Function and the modules
@pytest.fixture
def gathers(monkeypatch):
    """torch.distributed.all_gather_into_tensor -> a stub that files ("all_gather", shape of the receive buffer) among ``lib.calls``."""
    import torch.distributed as dist
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    box = {}

    def stub(recv, send, group=None):
        assert recv.dtype == send.dtype == torch.float64 and recv.dim() == 2 and recv.shape[0] % send.shape[0] == 0   # rank-major rows
        assert recv.shape[1] == send.shape[1] and recv.is_contiguous() and group is box.get("group")
        recv.zero_()
        box["lib"].calls.append(("all_gather", tuple(recv.shape)))
    monkeypatch.setattr(dist, "all_gather_into_tensor", stub)
    return box


def _delta(before):
    return {k: bn.sync_launch_counts[k] - before[k] for k in before}


@pytest.mark.parametrize("x_grad", [True, False])
def test_function_order(fake, gathers, x_grad):
    lib = gathers["lib"] = fake()
    x = torch.zeros(B, C, *SP, requires_grad=x_grad)
    w, b = torch.ones(C, requires_grad=True), torch.zeros(C, requires_grad=True)
    before, plain = dict(bn.sync_launch_counts), dict(bn.launch_counts)
    y = bn._SyncBnReluFn.apply(x, w, b, torch.zeros(C), torch.ones(C), 0.1, 1e-5, True, None, 3)
    fwd = [("dmvs_bn_sync_moments", (B, C, V)), ("all_gather", (3 * C, 3)), ("dmvs_bn_sync_forward", (B, C, V, 3, RELU))]
    assert lib.calls == fwd and _delta(before) == {"moments": 1, "sums": 0, "apply": 0, "gather": 1}
    grads = torch.autograd.grad(y, [t for t in (x, w, b) if t.requires_grad], torch.zeros_like(y))
    assert [tuple(g.shape) for g in grads] == ([tuple(x.shape)] if x_grad else []) + [(C,), (C,)]
    bwd = [("dmvs_bn_sync_backward_sums", (B, C, V, RELU))]
    if x_grad:   # the second collective if and only if the input needs a gradient (N = 0: the recording library writes no count)
        bwd += [("all_gather", (3 * C, 2)), ("dmvs_bn_sync_backward_apply", (B, C, V, 3, 0, RELU))]
    assert lib.calls == fwd + bwd
    assert _delta(before) == {"moments": 1, "sums": 1, "apply": int(x_grad), "gather": 1 + int(x_grad)}
    assert bn.launch_counts == plain   # the plain path's counters are the plain path's
    assert ops.launch_log == ["batchnorm"] * (5 + int(x_grad)) and ops.timer.held()


@pytest.mark.parametrize("nd", [3, 2])
def test_module_picks_its_path(fake, gathers, monkeypatch, nd):
    """Train mode under a group of more than one rank: the sync launches; eval mode, or a group of one: K5's plain entry and no
    collective.  Stubs beyond the fixture's: bn._check_input (accepts CPU tensors) and bn._sync_world."""
    import dmvsnet_amd as da
    monkeypatch.setattr(bn, "_check_input", lambda *a: None)
    world = {"n": 2}
    monkeypatch.setattr(bn, "_sync_world", lambda group: world["n"])
    group = gathers["group"] = object()
    m = (da.DiffSyncBatchNormReLU3d if nd == 3 else da.DiffSyncBatchNormReLU2d)(C, relu=False, process_group=group)
    x = torch.zeros((1, C, 1, 1, 1) if nd == 3 else (1, C, 1, 1))   # one value per channel on this rank: fine under a group
    lib = gathers["lib"] = fake()
    y = m.train()(x.clone().requires_grad_(True))
    assert lib.calls == [("dmvs_bn_sync_moments", (1, C, 1)), ("all_gather", (2 * C, 3)), ("dmvs_bn_sync_forward", (1, C, 1, 2, 0))]
    assert int(m.num_batches_tracked) == 1 and y.grad_fn is not None and len(y.grad_fn.saved_tensors) == 5
    lib = gathers["lib"] = fake()
    m.eval()(x)
    assert lib.calls == [("dmvs_bn_relu_forward", (1, C, 1, 0))] and int(m.num_batches_tracked) == 1
    world["n"] = 1
    lib = gathers["lib"] = fake()
    x2 = torch.zeros((2, C, 1, 1, 1) if nd == 3 else (2, C, 1, 1))
    m.train()(x2)
    assert lib.calls == [("dmvs_bn_relu_forward", (2, C, 1, BN_TRAIN))] and int(m.num_batches_tracked) == 2
