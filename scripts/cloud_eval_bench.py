#!/usr/bin/env python
"""Time the DTU point-cloud evaluation (dmvsnet_amd.cloud_eval) on a synthetic scan and compare it with the CPU restatement.

One JSON line: wall time per phase between device synchronisations (sort / cell tables, thinning rounds, each of the two
searches, classification + statistics), the thinning round count, points examined per query and the share of queries that
left the first grid level, and the same searches through tests/cloud_eval_ref.py (cKDTree with --workers threads where scipy
is importable) on the same thinned cloud, with the distances compared in the same run.

Default size: a data cloud of 20 M points before thinning (49 views x ~0.4 M fused pixels, the order of a DTU scan at
864 x 1152) against a 4 M-point reference cloud of the same surface at 0.2 mm.  Not real DTU data.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def spread(ts):
    return dict(min=min(ts), median=float(np.median(ts)), max=max(ts), n=len(ts))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n-data", type=int, default=20_000_000)
    ap.add_argument("--n-stl", type=int, default=4_000_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--nn-cell0", type=float, default=None, help="finest search grid in mm (A/B; default cloud_eval.NN_CELL0)")
    ap.add_argument("--nn-grow", type=float, default=None, help="cell growth per search level (A/B; default cloud_eval.NN_GROW)")
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU restatement")
    ap.add_argument("--cpu-unbounded", action="store_true", help="cKDTree queries without distance_upper_bound = 60 (the slower baseline)")
    ap.add_argument("--cpu-thinning", action="store_true", help="also run the sequential thinning loop on the CPU and compare the kept set")
    args = ap.parse_args()

    from dmvsnet_amd import cloud_eval, synth
    import cloud_eval_ref as ref
    assert torch.cuda.is_available(), "the benchmark needs the MI355X"
    cloud_eval.NN_CELL0 = args.nn_cell0 or cloud_eval.NN_CELL0
    cloud_eval.NN_GROW = args.nn_grow or cloud_eval.NN_GROW
    dev = torch.device("cuda:0")
    t0 = time.perf_counter()
    s = synth.synth_cloud_scene(args.seed, args.n_data, args.n_stl)
    order = np.random.Generator(np.random.PCG64(args.seed + 1)).permutation(len(s["data"]))
    gen_s = time.perf_counter() - t0
    data, stl = torch.from_numpy(s["data"]).to(dev), torch.from_numpy(s["stl"]).to(dev)
    order_d = torch.from_numpy(order).to(dev)

    def run(timing, count):
        info = dict(timing=timing, count_examined=count)
        torch.cuda.synchronize()
        t = time.perf_counter()
        be = cloud_eval.point_compare(data, stl, s["ObsMask"], s["BB"], s["Res"], s["P"], order=order_d, info=info)
        torch.cuda.synchronize()
        t_pc = time.perf_counter() - t
        st = cloud_eval.scan_stats(be)
        torch.cuda.synchronize()
        return be, st, info, t_pc, time.perf_counter() - t

    be, st, info0, _, _ = run(False, True)          # warm-up of every shape + the instrumented (counting) run
    phases, totals, three = [], [], []
    for _ in range(max(args.reps, 3)):
        be, st, info, t_pc, t_all = run(True, False)
        th, d2s, s2d = info["thinning"]["seconds"], info["data_to_stl"]["seconds"], info["stl_to_data"]["seconds"]
        ph = dict(thin_sort_and_cell_tables=th["sort_and_cell_tables"], thin_rounds=th["rounds"], thin_scatter=th["scatter"],
                  data_to_stl_sort=d2s["sort_and_cell_tables"], data_to_stl_search=d2s["search"],
                  stl_to_data_sort=s2d["sort_and_cell_tables"], stl_to_data_search=s2d["search"])
        ph["classification_and_statistics"] = t_all - sum(ph.values())
        phases.append(ph)
        totals.append(t_all)
        three.append(sum(th.values()) + sum(d2s.values()) + sum(s2d.values()))
    # un-instrumented wall time (no synchronisation inside)
    plain = [run(False, False)[4] for _ in range(max(args.reps, 3))]

    def level_share(i):
        lv = i["levels"]
        return dict(queries=i["queries"], examined_per_query=(i["examined"] or 0) / max(i["queries"], 1),
                    left_first_level=(lv[1]["queries"] / max(i["queries"], 1)) if len(lv) > 1 else 0.0,
                    level_queries=[l["queries"] for l in lv])

    out = dict(bench="cloud_eval", n_data=len(s["data"]), n_stl=len(s["stl"]), kept=int(be["Qdata"].shape[0]),
               rounds=info["thinning"]["rounds"], undecided_after_round=info["thinning"]["undecided_after_round"],
               thin_cells=info["thinning"]["cells"], scene_generation_s=gen_s,
               phase_seconds={k: spread([p[k] for p in phases]) for k in phases[0]},
               thinning_plus_searches_s=spread(three), scan_total_s=spread(totals), scan_total_unsynchronised_s=spread(plain),
               data_to_stl=level_share(info0["data_to_stl"]), stl_to_data=level_share(info0["stl_to_data"]), stats=st,
               nn_levels=cloud_eval.nn_levels(60.0), device=torch.cuda.get_device_name(0))
    if not args.no_cpu:
        q = be["Qdata"].cpu().numpy()
        cpu = {}
        t = time.perf_counter()
        d_cpu = ref.bounded_nn(s["stl"], q, s["BB"], 60.0) if not ref.HAVE_CKDTREE else None
        if ref.HAVE_CKDTREE:
            # two tree builds and two 16-thread queries bounded at max_dist, nothing else: the floor the device path is held to
            from scipy.spatial import cKDTree
            qs, ss = q.astype(np.float64), s["stl"].astype(np.float64)
            t = time.perf_counter()
            tree_s, tree_q = cKDTree(ss), cKDTree(qs)
            cpu["build_s"] = time.perf_counter() - t
            t1 = time.perf_counter()
            ub = np.inf if args.cpu_unbounded else 60.0   # bounded: misses come back as inf and are capped below
            dd = tree_s.query(qs, k=1, workers=args.workers, distance_upper_bound=ub)[0]
            ds = tree_q.query(ss, k=1, workers=args.workers, distance_upper_bound=ub)[0]
            cpu["query_s"] = time.perf_counter() - t1
            cpu["two_searches_s"] = time.perf_counter() - t
            dom_d, dom_s = ref.in_domain(q, s["BB"], 60.0), ref.in_domain(s["stl"], s["BB"], 60.0)
            want_d = np.where(dom_d, np.minimum(dd, 60.0), 60.0)
            want_s = np.where(dom_s, np.minimum(ds, 60.0), 60.0)
        else:
            want_d, want_s = d_cpu, ref.bounded_nn(q, s["stl"], s["BB"], 60.0)
            cpu["two_searches_s"] = time.perf_counter() - t
        cpu["kdtree"] = ref.HAVE_CKDTREE
        cpu["query_upper_bound"] = None if args.cpu_unbounded else 60.0
        cpu["workers"] = args.workers
        for k, want in (("Ddata", want_d), ("Dstl", want_s)):
            got = be[k].cpu().numpy()
            rel = np.abs(got - want) / np.maximum(want, 1e-300)
            cpu[k + "_max_rel_diff"] = float(rel.max()) if len(rel) else 0.0
            cpu[k + "_capped_equal"] = bool(np.array_equal(got == 60.0, want == 60.0))
        in_mask, _ = ref.data_in_mask(q, s["ObsMask"], s["BB"], s["Res"])
        cpu["DataInMask_equal"] = bool(np.array_equal(in_mask, be["DataInMask"].cpu().numpy()))
        cpu["StlAbovePlane_equal"] = bool(np.array_equal(ref.stl_above_plane(s["stl"], s["P"]), be["StlAbovePlane"].cpu().numpy()))
        if args.cpu_thinning:
            t = time.perf_counter()
            kept = ref.reduce_points_sequential(s["data"], 0.2, order)
            cpu["thinning_s"] = time.perf_counter() - t
            cpu["kept_equal"] = bool(np.array_equal(kept, be["Qdata_kept"].cpu().numpy()))
        out["cpu_restatement"] = cpu
        out["device_over_cpu_searches"] = out["thinning_plus_searches_s"]["median"] / cpu["two_searches_s"]
        out["floor_holds"] = bool(out["thinning_plus_searches_s"]["median"] < cpu["two_searches_s"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
