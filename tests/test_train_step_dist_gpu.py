"""GPU (-m gpu): T8, two ranks train ``convert_sync_batchnorm(DiffMVSNet(...))`` under ``DistributedDataParallel``.

Launcher and process hygiene of tests/test_bn_sync_dist_gpu.py: fresh child processes (spawn), gloo, every rank on cuda:0 (one MI355X,
and RCCL refuses two ranks on one GPU), a 60 s timeout on the process group (a mismatched collective errors instead of hanging),
``q.get(timeout=...)``, the parent terminates its children in a ``finally``, ``pytest.mark.timeout``.

Each rank takes one sample of the batch of two of case ``b2_32x64`` and runs two ``train_step``s with Adam; ``find_unused_parameters`` is
False, so a parameter the loss does not reach would raise in the second step.  Asserted: the losses are finite, and every parameter and
every BatchNorm buffer is bitwise equal across the ranks afterwards (DDP averages the gradients; the sync BatchNorm blends the running
buffers with the global statistics)."""
import datetime
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import train_step_ref as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = "b2_32x64"
STEPS = 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _job(rank, world, sd, sample):
    import dmvsnet_amd as da
    from dmvsnet_amd import bn
    from torch.nn.parallel import DistributedDataParallel
    net = da.DiffMVSNet(list(T.NDEPTHS), list(T.RATIOS), deterministic=True)
    net.load_state_dict(sd, strict=True)
    net = da.convert_sync_batchnorm(net.cuda()).train()
    n_sync = sum(isinstance(m, bn._DiffSyncBatchNormReLU) for m in net.modules())
    ddp = DistributedDataParallel(net, device_ids=[0], find_unused_parameters=False)
    opt = torch.optim.Adam(ddp.parameters(), lr=1e-3)
    mine = {k: ({s: t[rank:rank + 1].cuda() for s, t in v.items()} if isinstance(v, dict) else v[rank:rank + 1].cuda()) for k, v in sample.items()}
    scalars = [{k: float(v) for k, v in da.train_step(ddp, opt, mine, T.DLOSSW).items()} for _ in range(STEPS)]
    torch.cuda.synchronize()
    return dict(scalars=scalars, n_sync=n_sync, state={k: v.detach().cpu().numpy() for k, v in net.state_dict().items()})


def _worker(rank, world, port, q, args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    try:
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
        res = _job(rank, world, *args)
        q.put({"rank": rank, "res": res})   # (numpy arrays and floats: by value)
    except Exception as e:   # noqa: BLE001 -- report to the parent instead of hanging its queue
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc() + repr(e)})
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def _run(world, args):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, args)) for r in range(world)]
    try:
        for p in procs:
            p.start()
        res = [q.get(timeout=180) for _ in range(world)]
        for p in procs:
            p.join(60)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    for r in res:
        assert "error" not in r, r.get("error")
    res.sort(key=lambda r: r["rank"])
    return [r["res"] for r in res]


@pytest.mark.timeout(300)
def test_two_ranks_train_in_step():
    import numpy as np
    kw = T.CASES[CASE]
    assert kw["B"] == 2
    imgs, proj, dv = T.make_inputs(**kw)
    gt, mask = T.make_ground_truth(**kw)
    sample = {"imgs": imgs, "proj_matrices": proj, "depth_values": dv, "depth": gt, "mask": mask}
    a, b = _run(2, (T.make_state_dict(0), sample))
    print(f"TRAINSTEP T8: {a['n_sync']} sync BatchNorm modules; losses rank 0 {[s['loss'] for s in a['scalars']]}, rank 1 {[s['loss'] for s in b['scalars']]}")
    assert a["n_sync"] == 8 + 12 * 10 and len(a["scalars"]) == len(b["scalars"]) == STEPS
    for r in (a, b):
        assert all(np.isfinite(v) for s in r["scalars"] for v in s.values()), r["scalars"]
    assert set(a["state"]) == set(b["state"]) and len(a["state"]) == 787
    assert [k for k in a["state"] if not np.array_equal(a["state"][k], b["state"][k])] == []
    sd = T.make_state_dict(0)
    assert any(not np.array_equal(a["state"][k], sd[k].numpy()) for k in a["state"] if k.endswith("prob.weight"))   # the steps moved the weights
    assert all(int(a["state"][k]) == STEPS * (kw["V"] if k.startswith("feature.") else 1) for k in a["state"] if k.endswith("num_batches_tracked"))
