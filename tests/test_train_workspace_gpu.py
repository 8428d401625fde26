"""GPU (-m gpu, no kernel launch): the cached workspaces of K3g, K3h, K2g, K3k, K3f and K5 are one buffer per device however the device is
spelled -- "cuda", the current device with its index, a tensor's ``.device`` -- at the smallest shape each kernel covers, and another
buffer for another size (K2g's size is the same for both of its shapes and every volume) or another kernel."""
import pytest
import torch

from dmvsnet_amd import ops

pytestmark = pytest.mark.gpu

# (getter, smallest covered shape, a shape whose workspace has another size)
GETTERS = [
    (ops.conv3d_wgrad_workspace, (16, 1, 1, 1, 3), (32, 1, 1, 1, 3)),      # C, D, H, W, kdepth
    (ops.conv3d_wgrad_s2_workspace, (16, 1, 1, 1, 3), (32, 1, 1, 1, 3)),   # Ca, Dc, Hc, Wc, kdepth
    (ops.conv3d_wgrad_c2_workspace, (2, 8, 1, 1, 1), None),                # Cin, Cout, D, H, W
    (ops.conv2d_k5s2_wgrad_workspace, (16, 1, 1, 1), (32, 1, 1, 1)),       # Ca, D, Hf, Wf
    (ops.conv2d_wgrad_fpn_workspace, (3, 8, 3, 1, 1, 1), (8, 8, 3, 1, 1, 1)),   # Cin, Cout, kernel, D, H, W
    (ops.bn_workspace, (8, 1, 2), (16, 1, 2)),                             # C, B, V
]


@pytest.mark.parametrize("getter,shape,other", GETTERS, ids=[g[0].__name__ for g in GETTERS])
def test_one_workspace_per_device_however_spelled(getter, shape, other):
    x = torch.empty(1, device="cuda")
    ws = getter(*shape, "cuda")
    assert ws.is_cuda and ws.dtype == torch.float32 and ws.device == x.device
    assert getter(*shape, torch.device("cuda", torch.cuda.current_device())) is ws
    assert getter(*shape, x.device) is ws
    if other is not None:
        ws2 = getter(*other, x.device)
        assert ws2.numel() != ws.numel() and ws2 is not ws
        assert getter(*other, "cuda") is ws2 and getter(*shape, x.device) is ws


def test_kernels_of_one_size_keep_separate_workspaces():
    a, b = ops.conv3d_wgrad_workspace(32, 1, 1, 1, 3, "cuda"), ops.conv3d_wgrad_s2_workspace(64, 1, 1, 1, 3, "cuda")
    assert a.numel() == b.numel() and a is not b and a.data_ptr() != b.data_ptr()
