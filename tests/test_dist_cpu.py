"""CPU, world_size 2, gloo: the multi-GPU contracts of the path.

(1) source-view sharding: every rank warps only its own source views, the partial similarity volumes are
    summed with all_reduce (RCCL on the GPUs, gloo here) and every rank then holds the single-process result.
    There is no GPU in this container and the product has no CPU path, so the COMPUTE here is the oracle's: this
    test checks the ALGORITHM of the shard (the product's partition function + a SUM reduce reproduce the unsharded
    result) and bench.py's rank bookkeeping.  The product's own sharded forward (MVSNet.set_view_shard, v1 and the
    H-slab v2) executes in tests/test_dist_gpu.py (-m gpu, two ranks on cuda:0).
(1b) the product's row-gather (MVSNet._gather_rows: padded slabs -> all_gather -> full planes) on CPU tensors.
(1c) the product's row-slab collective (MVSNet._reduce_rows): reduce_scatter along H + point-to-point halo exchange
    against all_reduce + slice, world 4 (slabs shorter than the halo: several neighbours; a rank with an EMPTY slab).
(2) replica mode: ranks process different reference views with no collective; the aggregate count is world x steps.
"""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _work(rank, world, q)
    except Exception:   # noqa: BLE001 -- report to the parent instead of leaving its queue empty
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def _work(rank, world, q):
    if True:
        from dmvsnet_amd import MVSNet, shard_source_views, synth
        from oracle import dmvs_oracle as O

        H, W, V = 64, 96, 4
        ndepths, ratios = [8, 8, 8], [3, 2, 1]
        net = MVSNet(ndepths, ratios, verbose=False)
        sd = synth.synth_state_dict(net.state_dict(), 5)
        imgs, proj, dv = synth.synth_inputs(H, W, V, 5)
        mine = shard_source_views(V, world, rank)

        def reduce_fn(sim):  # what CostAgg.forward does on the GPUs (RCCL); gloo here
            dist.all_reduce(sim, op=dist.ReduceOp.SUM)
            return sim

        sharded = O.mvsnet_forward(sd, ndepths, ratios, imgs, proj, dv, views=mine, reduce_fn=reduce_fn)
        full = O.mvsnet_forward(sd, ndepths, ratios, imgs, proj, dv)
        rel = ((sharded["depth"] - full["depth"]).abs().mean() / full["depth"].abs().mean()).item()
        # replica bookkeeping: every rank did `steps` maps; aggregate = world * steps
        t = torch.tensor([3.0])
        dist.all_reduce(t)
        # (1b) the product's gather of regression outputs over H-slabs (pure torch + the process group)
        net.set_view_shard(dist.group.WORLD, rank, world, shard_rows=True)
        ok = True
        for h in (24, 40, 64):
            truth = torch.arange(3 * h * 5, dtype=torch.float32).view(3, h, 5)
            slabs, per = MVSNet.row_slabs(h, world)
            r0, r1 = slabs[rank]
            e0, e1 = max(0, r0 - 8), min(h, r1 + 8)
            mine_rows = truth[:, e0:e1].clone()
            mine_rows[:, :r0 - e0] = -1.0                   # halo rows must never reach the result
            mine_rows[:, r1 - e0:] = -1.0
            got = net._gather_rows(mine_rows, r0, r1, e0, h, per)
            ok = ok and torch.equal(got, truth)
        q.put((rank, mine, rel, float(t.item()), ok))


def _rows_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from dmvsnet_amd import MVSNet
        net = MVSNet([8, 8, 8], [3, 2, 1], verbose=False)
        net.return_prob_volume = False
        res = []
        for h in (16, 24, 72, 104, 296):      # 16 / 24: ranks with empty slabs; 72: the c3 quarter-size stage-1 volume
            g = torch.Generator().manual_seed(100 + h)
            parts = [torch.randint(-50, 50, (2, 3, h, 5), generator=g).float() for _ in range(world)]  # exact sums
            total = sum(parts)
            slabs, per = MVSNet.row_slabs(h, world)
            r0, r1 = slabs[rank]
            e0, e1 = MVSNet.row_extent(h, r0, r1)
            out = {}
            for mode in ("reduce_scatter", "all_reduce"):
                net.set_view_shard(dist.group.WORLD, rank, world, shard_rows=True, row_collective=mode)
                out[mode] = net._reduce_rows(parts[rank].clone(), h)
            ok = tuple(out["all_reduce"].shape) == tuple(out["reduce_scatter"].shape) == (2, 3, e1 - e0, 5)
            if r1 > r0:   # (an empty slab's dummy block carries no promise: its results are never gathered)
                ok = ok and torch.equal(out["reduce_scatter"], out["all_reduce"]) and torch.equal(out["reduce_scatter"], total[:, :, e0:e1])
            res.append((h, r1 - r0, bool(ok)))
        q.put((rank, res))
    except Exception:   # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_row_collective_reduce_scatter_equals_allreduce_world4():
    world = 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rows_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    empty = 0
    for rank, r in res:
        assert isinstance(r, list), r
        for h, rows, ok in r:
            assert ok, (rank, h, rows)
            empty += rows == 0
    assert empty > 0, "the cases must include a rank with an empty slab"


def _subgroup_worker(rank, world, port, q):
    """Two view groups of two ranks inside one job of four: the halo exchange addresses its peers by GLOBAL rank
    (dist.P2POp), the slabs by the rank INSIDE the view group."""
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from dmvsnet_amd import MVSNet
        groups = [dist.new_group([0, 1]), dist.new_group([2, 3])]   # every rank creates every group
        gi, grank = rank // 2, rank % 2
        net = MVSNet([8, 8, 8], [3, 2, 1], verbose=False)
        net.return_prob_volume = False
        res = []
        for h in (72, 104, 296):
            gen = torch.Generator().manual_seed(7 * h + gi)          # the two groups sum DIFFERENT volumes
            parts = [torch.randint(-50, 50, (2, 3, h, 5), generator=gen).float() for _ in range(2)]
            total = parts[0] + parts[1]
            slabs, per = MVSNet.row_slabs(h, 2)
            r0, r1 = slabs[grank]
            e0, e1 = MVSNet.row_extent(h, r0, r1)
            ok = True
            for mode in ("reduce_scatter", "all_reduce"):
                net.set_view_shard(groups[gi], grank, 2, shard_rows=True, row_collective=mode)
                got = net._reduce_rows(parts[grank].clone(), h)
                ok = ok and torch.equal(got, total[:, :, e0:e1])
            res.append((h, bool(ok)))
        q.put((rank, res))
    except Exception:   # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_row_collective_inside_a_sub_group():
    world = 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_subgroup_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, r in res:
        assert isinstance(r, list), r
        assert all(ok for _, ok in r), (rank, r)


@pytest.mark.timeout(300)
def test_row_collective_world8():
    """BASELINE configs[3] / [4] name 8 GPUs: the row collective with 8 ranks -- slabs of 16 rows (shorter than the
    32-row halo: up to four neighbours per side) and, for the small volumes, trailing ranks with EMPTY slabs."""
    world = 8
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rows_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    empty = 0
    for rank, r in res:
        assert isinstance(r, list), r
        for h, rows, ok in r:
            assert ok, (rank, h, rows)
            empty += rows == 0
    assert empty > 0


def test_view_partition_eight_ranks():
    """north_star's partition {v : (v - 1) mod G == g} at G = 8: 11 views -> 2/2/1/1/1/1/1/1 source views, 5 views ->
    ranks 4..7 own NO source view (they still compute the reference features and contribute zeros to the sum)."""
    from dmvsnet_amd import shard_source_views
    s11 = [shard_source_views(11, 8, g) for g in range(8)]
    assert [len(x) for x in s11] == [2, 2, 1, 1, 1, 1, 1, 1] and s11[0] == [1, 9] and s11[1] == [2, 10]
    assert sorted(v for x in s11 for v in x) == list(range(1, 11))
    s5 = [shard_source_views(5, 8, g) for g in range(8)]
    assert s5 == [[1], [2], [3], [4], [], [], [], []]
    s7 = [shard_source_views(7, 8, g) for g in range(8)]       # configs[4]: 7 views on 8 GPUs
    assert [len(x) for x in s7] == [1, 1, 1, 1, 1, 1, 0, 0]


@pytest.mark.timeout(300)
def test_view_shard_allreduce_matches_single_process():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for r in res:
        assert len(r) == 5, r[1]
    res.sort()
    assert res[0][1] == [1, 3] and res[1][1] == [2]          # {v : (v-1) % G == g}
    for _, _, rel, total, gather_ok in res:
        assert rel < 1e-6, rel                                   # sum order differs only
        assert total == 6.0
        assert gather_ok


def test_costagg_uses_allreduce_sum():
    """The product's reduce step is a SUM all_reduce on the similarity volume (checked on its source: the kernel
    itself needs a GPU)."""
    import inspect
    from dmvsnet_amd.mvsnet import CostAgg
    src = inspect.getsource(CostAgg.forward)
    assert "all_reduce" in src and "ReduceOp.SUM" in src


def test_hybrid_partition_leaves_no_rank_without_a_view():
    """config 2 (5 views) on 8 GPUs = 2 view groups x 4 ranks -- inside a group of 4 every rank owns exactly one
    source view, where the 8-way shard leaves four ranks empty; config 3 / 4 (11 views) as 2 x 4: 3/3/2/2 per group."""
    from dmvsnet_amd import shard_source_views
    assert [shard_source_views(5, 8, r) for r in range(8)][4:] == [[], [], [], []]
    assert [shard_source_views(5, 4, r) for r in range(4)] == [[1], [2], [3], [4]]
    assert [len(shard_source_views(11, 4, r)) for r in range(4)] == [3, 3, 2, 2]
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    old = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "8", "--mode", "view-shard-rows", "--view-group", "4", "--full-outputs"]
        a = bench.parse()
        assert (a.gpus, a.mode, a.view_group, a.full_outputs) == (8, "view-shard-rows", 4, True)
    finally:
        sys.argv = old


def test_bench_contract_cli():
    """bench.py parses the driver's flags and defaults to N=1."""
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    old = sys.argv
    try:
        sys.argv = ["bench.py"]
        a = bench.parse()
        assert a.gpus == 1 and a.steps > 0 and a.warmup >= 0
        sys.argv = ["bench.py", "--gpus", "8", "--steps", "5", "--warmup", "2"]
        a = bench.parse()
        assert (a.gpus, a.steps, a.warmup) == (8, 5, 2)
        # the driver's multi-GPU command carries no --mode: the default is the line with BOTH the replicas rate (`value`) and
        # north_star's partition (`latency_mode`, the hybrid view shard) -- VERDICT r05 item 2
        assert a.mode == "auto" and a.view_group == 0
        # ranks per view group = the largest divisor of N that is <= V - 1 source views
        assert [bench.default_view_group(n, 5) for n in (2, 4, 8)] == [2, 4, 4]
        assert [bench.default_view_group(n, 11) for n in (2, 4, 8)] == [2, 4, 8]
        assert bench.default_view_group(8, 3) == 2 and bench.default_view_group(6, 5) == 3 and bench.default_view_group(4, 2) == 1
        # a plain run times only the headline; the context legs and the output dump are opt-in
        assert a.full is False and a.dump_outputs is None
        sys.argv = ["bench.py", "--full", "--dump-outputs", "outs"]
        a = bench.parse()
        assert a.full is True and a.dump_outputs == "outs"
    finally:
        sys.argv = old


def test_bench_dump_outputs(tmp_path):
    """bench.py --dump-outputs: every tensor of the forward's output dict once (the top-level aliases of the last stage are
    not written twice), float32 / float64 only, under 64 MB in all, and an oversized array sampled at the same positions
    in every run."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import importlib
    bench = importlib.import_module("bench")
    g = torch.Generator().manual_seed(0)
    big = torch.rand(1, 4, 2048, 2048, generator=g)
    small = torch.rand(1, 32, 40, generator=g, dtype=torch.float64)
    out = {"stage1": {"depth": small, "mask": small > 0.5}, "stage2": {"depth_sub_plus": big}}
    out.update(out["stage2"])
    names = bench.dump_outputs(out, str(tmp_path / "a"))
    bench.dump_outputs(out, str(tmp_path / "b"))
    assert names == ["stage1.depth", "stage1.mask", "stage2.depth_sub_plus"]
    assert sorted(os.listdir(tmp_path / "a")) == [n + ".npy" for n in names]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    d = np.load(tmp_path / "a" / "stage1.depth.npy")
    assert d.dtype == np.float64 and np.array_equal(d, small.numpy())
    m = np.load(tmp_path / "a" / "stage1.mask.npy")
    assert m.dtype == np.float32 and np.array_equal(m, (small > 0.5).float().numpy())
    s = np.load(tmp_path / "a" / "stage2.depth_sub_plus.npy")
    assert s.dtype == np.float32 and 0 < s.size < big.numel() and np.isin(s, big.numpy()).all()
    assert np.array_equal(s, np.load(tmp_path / "b" / "stage2.depth_sub_plus.npy"))
