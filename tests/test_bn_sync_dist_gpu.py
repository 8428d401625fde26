"""GPU (-m gpu): the synchronised BatchNorm + ReLU under real process groups -- gloo, every rank on cuda:0 (the harness of
tests/test_dist_gpu.py: one MI355X, and RCCL refuses two ranks on one GPU).  What runs is what runs over RCCL on a node: the module's
two all-gathers on the current stream around K5's sync launches.

  module   ``DiffSyncBatchNormReLU3d`` at worlds 2 and 3 with batches (1, 1) and (2, 1, 1): every rank's tensors against float64 on the
           concatenated batch (criterion and norms of tests/test_bn_sync_gpu.py), statistics and running buffers torch.equal across the
           ranks, each rank torch.equal to the single-process emulation of the same pieces, the distance to stock
           ``torch.nn.SyncBatchNorm`` + ReLU printed.
  network  ``convert_sync_batchnorm(DiffCostRegNetPart / ...Refine)`` on the two stored cases of tests/golden/op_regnet_grad.npz, one
           sample per rank: concatenated outputs and summed parameter gradients against the float64 restatement and the reference's
           recorded batch-2 results -- tensors and criterion of tests/test_regnet_grad_gpu.py
           ``test_network_against_the_reference_and_float64``; the same network with per-rank BatchNorm misses the criterion.
  DDP      the converted refine part inside DistributedDataParallel: gradients and running buffers torch.equal across the ranks, two
           collectives per BatchNorm and step.

Hang protection: a 60 s timeout on the process group (a mismatched collective errors), ``q.get(timeout=120)``, the parent terminates its
children in a ``finally``, ``pytest.mark.timeout(300)``.  Figures are printed before they are asserted.  No test provokes a fault."""
import datetime
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import bn_grad_ref as G
import bn_sync_ref as S
import regnet_grad_ref as RG
from test_bn_sync_gpu import KEYS, compare, running_init
from test_regnet_grad_gpu import net_refs  # noqa: F401  (the fixture: inputs, weights, float64 / fp32 / recorded results per stored case)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPATIAL = (2, 5, 9)
MOMENTUM = 0.1


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ------------------------------------------------------------------------------------------------ what the ranks run
def _job_module(rank, world, pieces, channels):
    import dmvsnet_amd as da
    from dmvsnet_amd import bn, ops
    res = {}
    for C in channels:
        case, _ = S.first_clean_pieces(C, pieces, SPATIAL)
        xs, gys = (S.split(case[k].cuda(), pieces) for k in ("x", "gy"))
        running = running_init(C)

        def load(m):
            with torch.no_grad():
                m.weight.copy_(case["gamma"]), m.bias.copy_(case["beta"])
                m.running_mean.copy_(running[0]), m.running_var.copy_(running[1])
            return m.train()

        m = load(da.DiffSyncBatchNormReLU3d(C, momentum=MOMENTUM).cuda())
        before = dict(bn.sync_launch_counts)
        xin = xs[rank].clone().requires_grad_(True)
        y = m(xin)
        mean, invstd = (t.clone() for t in y.grad_fn.saved_tensors[3:5])
        y.backward(gys[rank])
        got = dict(y=y.detach(), g_x=xin.grad, g_gamma=m.weight.grad, g_beta=m.bias.grad, mean=mean, invstd=invstd,
                   running_mean=m.running_mean, running_var=m.running_var)
        emu = S.emulate(ops, xs, gys, case["gamma"].cuda(), case["beta"].cuda(), MOMENTUM, m.eps, True, running=running)[rank]
        out = {k: v.detach().cpu() for k, v in got.items()}
        out["equals_emulation"] = {k: bool(torch.equal(got[k], emu[k])) for k in KEYS}
        out["num_batches_tracked"] = int(m.num_batches_tracked)
        out["counts"] = {k: bn.sync_launch_counts[k] - before[k] for k in before}
        try:   # stock SyncBatchNorm + ReLU in the same ranks: a distance to print, nothing more
            stock = load(torch.nn.SyncBatchNorm(C, momentum=MOMENTUM).cuda())
            xs_in = xs[rank].clone().requires_grad_(True)
            ys = torch.relu(stock(xs_in))
            ys.backward(gys[rank])
            out["stock"] = {k: G.rel_dist(a, b) for k, a, b in (("y", got["y"], ys), ("g_x", got["g_x"], xs_in.grad),
                                                                  ("g_gamma", got["g_gamma"], stock.weight.grad),
                                                                  ("running_var", got["running_var"], stock.running_var))}
        except Exception as e:   # noqa: BLE001 -- the stock module may refuse the backend; that is not this test's subject
            out["stock"] = repr(e)
        res[C] = out
    return res


def _run_net(net, x, gy):
    post, hooks = {}, []
    for blk in RG.BLOCKS:
        hooks.append(getattr(net, blk).register_forward_hook(lambda mod, inp, out, blk=blk: post.__setitem__(blk, (out.detach() > 0).cpu())))
    xin = x.cuda().clone().requires_grad_(True)
    out = net(xin)
    for h in hooks:
        h.remove()
    out.backward(gy.cuda())
    return out.detach().cpu(), xin.grad.cpu(), post


def _diff_part(name, sd):
    import dmvsnet_amd as da
    net = (da.DiffCostRegNetPartRefine if RG.GOLDEN_NETS[name]["refine"] else da.DiffCostRegNetPart)(2, 8)
    net.load_state_dict(sd, strict=True)
    return net.cuda().train()


def _job_nets(rank, world, cases):
    import dmvsnet_amd as da
    res = {}
    for name, (x, gy, sd) in cases.items():
        net = da.convert_sync_batchnorm(_diff_part(name, sd)).train()
        out, gx, post = _run_net(net, x[rank:rank + 1], gy[rank:rank + 1])
        res[name] = dict(out=out, g_x=gx, post=post, grads={n: p.grad.cpu() for n, p in net.named_parameters()},
                         tracked=[int(m.num_batches_tracked) for m in net.modules() if hasattr(m, "num_batches_tracked")],
                         buffers={n: b.cpu() for n, b in net.named_buffers()})
    return res


def _job_ddp(rank, world, case):
    import dmvsnet_amd as da
    from dmvsnet_amd import bn
    from torch.nn.parallel import DistributedDataParallel
    x, gy, sd = case
    net = da.convert_sync_batchnorm(_diff_part("refine", sd)).train()
    n_bn = sum(isinstance(m, bn._DiffSyncBatchNormReLU) for m in net.modules())
    ddp = DistributedDataParallel(net, device_ids=[0])
    before = dict(bn.sync_launch_counts)
    out = ddp(x[rank:rank + 1].cuda())
    out.backward(gy[rank:rank + 1].cuda())
    torch.cuda.synchronize()
    return dict(grads={n: p.grad.cpu() for n, p in net.named_parameters()}, buffers={n: b.cpu() for n, b in net.named_buffers()},
                counts={k: bn.sync_launch_counts[k] - before[k] for k in before}, n_bn=n_bn)


JOBS = {"module": _job_module, "nets": _job_nets, "ddp": _job_ddp}


def _map(obj, kind, fn):
    """``fn`` on every ``kind`` inside nested dicts, lists and tuples."""
    if isinstance(obj, kind):
        return fn(obj)
    if isinstance(obj, dict):
        return {k: _map(v, kind, fn) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_map(v, kind, fn) for v in obj)
    return obj


def _worker(rank, world, port, q, job, args):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    try:
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
        res = JOBS[job](rank, world, *args)
        torch.cuda.synchronize()
        # (results travel as numpy arrays, by value: a tensor's shared-memory handle would need this process alive when it is read)
        q.put({"rank": rank, "res": _map(res, torch.Tensor, lambda t: t.detach().cpu().numpy())})
    except Exception as e:   # noqa: BLE001 -- report to the parent instead of hanging its queue
        import traceback
        q.put({"rank": rank, "error": traceback.format_exc() + repr(e)})
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def _run(world, job, args):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, job, args)) for r in range(world)]
    try:
        for p in procs:
            p.start()
        res = [q.get(timeout=120) for _ in range(world)]
        for p in procs:
            p.join(60)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    for r in res:
        assert "error" not in r, r.get("error")
    res.sort(key=lambda r: r["rank"])
    import numpy as np
    return [_map(r["res"], np.ndarray, torch.from_numpy) for r in res]


# ------------------------------------------------------------------------------------------------ module
@pytest.mark.timeout(300)
@pytest.mark.parametrize("pieces", [(1, 1), (2, 1, 1)])
def test_module_under_a_process_group(pieces):
    channels = (8, 64)
    res = _run(len(pieces), "module", (pieces, channels))
    for C in channels:
        ranks = [r[C] for r in res]
        case, seed = S.first_clean_pieces(C, pieces, SPATIAL)
        assert G.kink_violations(case) == 0
        tag = f"DIST C {C} world {len(pieces)} B {pieces}"
        print(f"{tag} seed {seed}: stock SyncBatchNorm + ReLU distance per rank {[r['stock'] for r in ranks]}")
        print(f"{tag}: equals the single-process emulation {[r['equals_emulation'] for r in ranks]}; launches {[r['counts'] for r in ranks]}")
        compare(tag, ranks, case, pieces, MOMENTUM, running_init(C))
        for r in ranks:
            assert all(torch.equal(r[k], ranks[0][k]) for k in ("mean", "invstd", "running_mean", "running_var"))
            assert all(r["equals_emulation"].values()), r["equals_emulation"]   # the collective adds nothing to the arithmetic
            assert r["num_batches_tracked"] == 1 and r["counts"] == {"moments": 1, "sums": 1, "apply": 1, "gather": 2}


# ------------------------------------------------------------------------------------------------ whole networks
def _criterion(name, c, out, ghip):
    """The rows of test_network_against_the_reference_and_float64: (tensor, yardstick, e_hip, e_ref)."""
    (o64, g64, _), (_, g32, _) = c["f64"], c["f32"]
    assert set(ghip) == set(g64)
    rows = [("out", "recorded", RG.rel_dist(out, o64), RG.rel_dist(c["out"], o64))]
    for k in sorted(g64):
        ref, what = (c["stored"][k], "recorded") if k in c["stored"] else (g32[k], "stock fp32")
        rows.append((k, what, RG.rel_dist(ghip[k], g64[k]), RG.rel_dist(ref, g64[k])))
    return rows


@pytest.mark.timeout(300)
def test_converted_networks_reproduce_the_batch_of_two(net_refs):  # noqa: F811
    """Two ranks with one sample each reproduce what the reference computed on a batch of two (the fixture's float64 run has no
    BatchNorm output within 1e-4 of the kink); per-rank BatchNorm on one sample misses by orders of magnitude."""
    cases = {name: (c["x"], c["gy"], c["sd"]) for name, c in net_refs.items()}
    assert set(cases) == set(RG.GOLDEN_NETS) and all(c["x"].shape[0] == 2 for c in net_refs.values())
    res = _run(2, "nets", (cases,))
    failed = []
    for name, c in net_refs.items():
        (o64, g64, pre64), (_, _, pre32) = c["f64"], c["f32"]
        assert RG.kink_violations(pre64) == 0 and RG.same_masks(pre32, pre64)
        ranks = [r[name] for r in res]
        flips = {blk: int((torch.cat([r["post"][blk] for r in ranks]) != (pre64[blk] > 0)).sum()) for blk in RG.BLOCKS}
        print(f"DISTNET {name} mask flips per block: {flips}")
        assert not any(flips.values()), flips
        out = torch.cat([r["out"] for r in ranks])
        ghip = {"x": torch.cat([r["g_x"] for r in ranks]), **{n: ranks[0]["grads"][n] + ranks[1]["grads"][n] for n in ranks[0]["grads"]}}
        rows = _criterion(name, c, out, ghip)
        for k, what, e_hip, e_ref in rows:
            print(f"DISTNET {name} {k}: e_hip {e_hip:.3e}  e_ref ({what}) {e_ref:.3e}  bound {RG.bound_of(e_ref):.3e}")
        failed += [(name, k, e_hip, e_ref) for k, what, e_hip, e_ref in rows if not e_hip <= RG.bound_of(e_ref)]
        assert all(t == 1 for r in ranks for t in r["tracked"])
        assert all(torch.equal(ranks[0]["buffers"][n], ranks[1]["buffers"][n]) for n in ranks[0]["buffers"])
    assert not failed, failed
    # the counter-test: the same networks with plain DiffBatchNormReLU*, one sample per "rank" (no group needed: nothing is exchanged)
    for name, c in net_refs.items():
        outs = []
        for r in range(2):
            with torch.no_grad():
                outs.append(_diff_part(name, c["sd"])(c["x"][r:r + 1].cuda()).cpu())
        e_hip, e_ref = RG.rel_dist(torch.cat(outs), c["f64"][0]), RG.rel_dist(c["out"], c["f64"][0])
        print(f"DISTNET {name} per-rank BatchNorm, out: e_hip {e_hip:.3e}  e_ref {e_ref:.3e}  bound {RG.bound_of(e_ref):.3e}")
        assert e_hip > 100 * RG.bound_of(e_ref), "per-rank statistics must miss the criterion: the test above can fail"


# ------------------------------------------------------------------------------------------------ DDP
@pytest.mark.timeout(300)
def test_ddp_wraps_the_converted_network(net_refs):  # noqa: F811
    c = net_refs["refine"]
    a, b = _run(2, "ddp", ((c["x"], c["gy"], c["sd"]),))
    print(f"DDP refine: {a['n_bn']} BatchNorm modules, launches per rank {a['counts']} / {b['counts']}")
    assert set(a["grads"]) == set(b["grads"]) and len(a["grads"]) > 0
    for n in a["grads"]:
        assert torch.equal(a["grads"][n], b["grads"][n]), n
    for n in a["buffers"]:
        assert torch.equal(a["buffers"][n], b["buffers"][n]), n
    for r in (a, b):   # hooks and custom Functions coexist: two collectives per BatchNorm and step, neither more nor fewer
        assert r["counts"] == {"moments": r["n_bn"], "sums": r["n_bn"], "apply": r["n_bn"], "gather": 2 * r["n_bn"]}
    # DDP averages: each rank holds half the sum over the batch of two (halving is exact), which is held as the network test holds it
    rows = [r for r in _criterion("refine", c, c["out"], {"x": c["f64"][1]["x"], **{n: 2.0 * g for n, g in a["grads"].items()}}) if r[0] in a["grads"]]
    for k, what, e_hip, e_ref in rows:
        print(f"DDP refine 2 x {k}: e_hip {e_hip:.3e}  e_ref ({what}) {e_ref:.3e}  bound {RG.bound_of(e_ref):.3e}")
    assert all(e_hip <= RG.bound_of(e_ref) for k, what, e_hip, e_ref in rows)
