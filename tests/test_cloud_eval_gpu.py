"""N5 (DTU point-cloud evaluation) on the MI355X: every comparison is against the CPU restatement (cloud_eval_ref), never
against another run of the code under test.  The equality tests rest on conditions on the INPUTS, asserted here on the
restatement's own values: no point pair within 1e-7 of dst, no restated distance within 1e-6 of the outlier threshold or of
max_dist, no mask coordinate within 1e-9 of a rounding boundary."""
import os

import numpy as np
import pytest
import torch

import cloud_eval_ref as ref

pytestmark = pytest.mark.gpu

DST, MAXD, OUTLIER = 0.2, 60.0, 20.0


def rng_of(seed):
    return np.random.Generator(np.random.PCG64(seed))


def assert_distance_conditions(*dists):
    """No restated distance within 1e-6 of the outlier threshold or of max_dist (capped values are exactly max_dist)."""
    for d in dists:
        assert not np.any(np.abs(d - OUTLIER) < 1e-6)
        assert not np.any((np.abs(d - MAXD) < 1e-6) & (d != MAXD))


def assert_scan_conditions(data, want):
    """Every input condition of a whole-scan comparison, on the restatement's own values."""
    assert not np.any(np.abs(ref.adjacency(data, DST)[2] - DST) < 1e-7)
    assert_distance_conditions(want["Ddata"], want["Dstl"])
    frac = want["mask_arg"] - np.floor(want["mask_arg"])
    assert not np.any(np.abs(frac - 0.5) < 1e-9)


def thin_clouds():
    r = rng_of(11)
    n = 20011                                                   # not a multiple of the workgroup
    surface = np.stack([r.uniform(0, 25, n), r.uniform(0, 25, n), r.normal(0, 0.05, n)], 1)
    dup = np.stack([r.uniform(0, 10, 6000), r.uniform(0, 10, 6000), r.normal(0, 0.05, 6000)], 1)
    dup[4000:] = dup[:2000]                                     # exact duplicate points
    one_cell = 5.0 + r.uniform(0.01, 0.19, (700, 3))            # all points in a single 0.2 mm cell
    clump = np.concatenate([np.stack([r.uniform(0, 12, 5000), r.uniform(0, 12, 5000), r.normal(0, 0.05, 5000)], 1),
                            np.array([6.0, 6.0, 0.0]) + r.normal(0, 0.45, (10000, 3))])   # a 10 000-point clump
    volume = rng_of(15).uniform(-3, 3, (30001, 3)) * np.array([1.0, 1.0, 0.2])   # seed chosen for the input condition below
    return dict(surface=surface, duplicates=dup, one_cell=one_cell, clump=clump, volume=volume, single=np.array([[1.0, 2.0, 3.0]]))


@pytest.mark.parametrize("name", ["surface", "duplicates", "one_cell", "clump", "volume", "single"])
def test_reduce_points_equals_sequential(name):
    from dmvsnet_amd import cloud_eval
    p = thin_clouds()[name].astype(np.float32)
    adj = ref.adjacency(p, DST)
    near = int(np.sum(np.abs(adj[2] - DST) < 1e-7))
    print(f"{name}: {len(p)} points, {len(adj[1]) // 2} neighbour pairs, {near} within 1e-7 of dst")
    assert near == 0
    for seed in (0, 7):                                         # two visit orders, each against its own restatement
        order = rng_of(1000 + seed).permutation(len(p))
        want = ref.reduce_points_sequential(p, DST, order, adj)
        info = {}
        got = cloud_eval.reduce_points(p, DST, order=order, info=info)
        again = cloud_eval.reduce_points(torch.from_numpy(p).cuda(), DST, order=torch.from_numpy(order).cuda())
        print(f"  order {seed}: kept {int(want.sum())} (device {info['kept']}), rounds {info['rounds']}, cells {info['cells']}")
        assert got.dtype == torch.bool and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want)
        assert torch.equal(got, again)                          # same input twice: bit-identical
        assert 1 <= info["rounds"] < 64 and info["kept"] == int(want.sum())
    # the default order is the seeded host permutation
    want = ref.reduce_points_sequential(p, DST, rng_of(3).permutation(len(p)), adj)
    assert np.array_equal(cloud_eval.reduce_points(p, DST, seed=3).cpu().numpy(), want)


def check_max_dist_cp(to, frm, bb, subset=None, label=""):
    from dmvsnet_amd import cloud_eval
    info = {"count_examined": True}
    got, idx = cloud_eval.max_dist_cp(to, frm, bb, MAXD, info=info, return_index=True)
    assert got.dtype == torch.float64 and got.is_cuda and got.shape == (len(frm),)
    got, idx = got.cpu().numpy(), idx.cpu().numpy()
    sel = np.arange(len(frm)) if subset is None else subset
    want = np.minimum(ref.max_dist_cp_blocks(to, np.asarray(frm)[sel], bb, MAXD), MAXD)
    assert_distance_conditions(want)
    below = want < MAXD
    rel = np.abs(got[sel][below] - want[below]) / np.maximum(want[below], 1e-300)
    rel[want[below] == got[sel][below]] = 0.0
    print(f"{label}: {len(sel)} checked, {int(below.sum())} below max_dist, max rel diff {rel.max() if len(rel) else 0.0:.3e}, "
          f"levels {[(l['cell'], l['queries']) for l in info['levels']]}, examined/query "
          f"{(info['examined'] or 0) / max(info['queries'], 1):.1f}")
    assert np.all(rel <= 1e-12)
    assert np.all(got[sel][~below] == MAXD)
    # the reported neighbour is at the reported distance
    has = idx[sel] >= 0
    assert np.all(has[below])
    d = np.asarray(to, np.float32).astype(np.float64)[idx[sel][has]] - np.asarray(frm, np.float32).astype(np.float64)[sel][has]
    dn = np.minimum(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]), MAXD)
    assert np.all(np.abs(dn - got[sel][has]) <= 1e-12 * np.maximum(dn, 1e-300))
    return info


def test_max_dist_cp_scene_both_directions():
    from test_cloud_eval_cpu import nn_scene
    to, frm, bb = nn_scene(21, n_to=30000, n_from=20000)
    i1 = check_max_dist_cp(to, frm, bb, label="data->stl")
    i2 = check_max_dist_cp(frm, to, bb, label="stl->data")
    assert len(i1["levels"]) == 3 and len(i2["levels"]) >= 2      # queries that need every grid level


def test_max_dist_cp_edge_shapes():
    from dmvsnet_amd import cloud_eval
    r = rng_of(22)
    bb = np.array([[-10.0, -10.0, -10.0], [135.0, 100.0, 77.0]])  # not a multiple of max_dist: domain = [-10, 170) x [-10, 110) x [-10, 110)
    frm = r.uniform(-10, 100, (5000, 3)).astype(np.float32)
    # to-cloud empty
    assert torch.all(cloud_eval.max_dist_cp(np.zeros((0, 3), np.float32), frm, bb) == MAXD)
    assert cloud_eval.max_dist_cp(frm, np.zeros((0, 3), np.float32), bb).numel() == 0
    # from-points outside the domain on every face (and exactly on the faces), to-points right next to them
    faces = np.array([[-10.0, 0, 0], [-10.001, 0, 0], [170.0, 0, 0], [169.99, 0, 0], [0, -10.0, 0], [0, -10.001, 0], [0, 110.0, 0],
                      [0, 109.99, 0], [0, 0, -10.0], [0, 0, -10.001], [0, 0, 110.0], [0, 0, 109.99], [np.nan, 0, 0]], dtype=np.float32)
    to = np.concatenate([faces[:12] + np.float32(0.25), r.uniform(-10, 100, (2000, 3)).astype(np.float32)])
    got = cloud_eval.max_dist_cp(to, faces, bb).cpu().numpy()
    want = np.minimum(ref.max_dist_cp_blocks(to, faces[:12], bb, MAXD), MAXD)
    assert_distance_conditions(want)
    assert np.array_equal(want == MAXD, [False, True, True, False] * 3)
    assert np.all(np.abs(got[:12] - want) <= 1e-12 * want) and got[12] == MAXD
    # a to-point exactly on a cell boundary of the two finer grids (origins -70.5 / -74 mm, cells 0.5 / 4 mm) and queries around it
    to_b = np.array([[22.0, 22.0, 22.0], [54.0, 22.0, 22.0], [22.5, 22.0, 22.0]], dtype=np.float32)
    q_b = (to_b[0] + r.uniform(-1.2, 1.2, (4000, 3))).astype(np.float32)
    check_max_dist_cp(to_b, q_b, bb, label="boundary")
    # neighbours only beyond 60 mm
    far_to = np.array([[100.0, 100.0, 100.0]], dtype=np.float32)
    q_far = r.uniform(-10, 30, (3000, 3)).astype(np.float32)
    assert torch.all(cloud_eval.max_dist_cp(far_to, q_far, bb) == MAXD)
    assert np.all(ref.max_dist_cp_blocks(far_to, q_far, bb, MAXD) >= MAXD)
    # a non-empty to-cloud that lies entirely more than max_dist outside the domain (a cloud in another frame): no cell of any
    # level's grid is occupied; every distance is max_dist and no neighbour is reported (MaxDistCP.m:28-29)
    away = (np.array([900.0, -700.0, 400.0]) + r.uniform(-5, 5, (500, 3))).astype(np.float32)
    got, idx = cloud_eval.max_dist_cp(away, q_far, bb, return_index=True)
    assert torch.all(got == MAXD) and torch.all(idx == -1) and got.shape == (len(q_far),)
    assert np.all(ref.max_dist_cp_blocks(away, q_far, bb, MAXD) == MAXD)
    # ... and one that is outside the finest grid but inside the coarsest one's one-cell margin (75 mm off the domain)
    edge = (np.array([245.0, 50.0, 50.0]) + r.uniform(-2, 2, (300, 3))).astype(np.float32)
    q_edge = r.uniform([150.0, 40.0, 40.0], [169.9, 60.0, 60.0], (2000, 3)).astype(np.float32)   # the nearest queries of the domain
    got, idx = cloud_eval.max_dist_cp(edge, q_edge, bb, return_index=True)
    assert torch.all(got == MAXD) and torch.all(idx == -1) and got.shape == (len(q_edge),)
    assert np.all(ref.max_dist_cp_blocks(edge, q_edge, bb, MAXD) >= MAXD)
    # queries that need every grid level: distances spread from 0.01 mm to beyond 60 mm off a dense plane
    plane = np.stack([r.uniform(0, 90, 40000), r.uniform(0, 90, 40000), np.zeros(40000)], 1).astype(np.float32)
    q = np.stack([r.uniform(0, 90, 6000), r.uniform(0, 90, 6000), np.exp(r.uniform(np.log(0.01), np.log(90.0), 6000))], 1).astype(np.float32)
    info = check_max_dist_cp(plane, q, bb, label="all levels")
    assert len(info["levels"]) == 3 and all(l["queries"] > 0 for l in info["levels"])


def test_max_dist_cp_one_million():
    r = rng_of(23)
    n = 1_000_000
    side = 300.0                                                 # 1 M points on 300 x 300 mm: 11 per mm^2, as a 0.3 mm cloud
    bb = np.array([[-20.0, -15.0, -50.0], [200.0, 190.0, 60.0]])   # 4 x 4 x 2 blocks: the domain ends inside the cloud at 220 / 225 mm
    h = lambda x, y: 12.0 * np.sin(x / 40.0) * np.cos(y / 55.0)
    tx, ty = r.uniform(0, side, n), r.uniform(0, side, n)
    to = np.stack([tx, ty, h(tx, ty)], 1).astype(np.float32)
    fx, fy = r.uniform(-10, side + 10, n), r.uniform(-10, side + 10, n)
    fz = h(fx, fy) + r.normal(0, 0.2, n)
    out = r.uniform(0, 1, n) < 0.04
    fz[out] += r.choice([-1.0, 1.0], int(out.sum())) * r.uniform(3, 100, int(out.sum()))
    frm = np.stack([fx, fy, fz], 1).astype(np.float32)
    subset = None if ref.HAVE_CKDTREE else np.sort(r.choice(n, 1500, replace=False))   # brute force: a seeded subset, not a skip
    check_max_dist_cp(to, frm, bb, subset=subset, label="1M x 1M")


def scene_and_restatement(seed, n_data, n_stl, order_seed):
    from dmvsnet_amd import synth
    s = synth.synth_cloud_scene(seed, n_data, n_stl)
    order = rng_of(order_seed).permutation(len(s["data"]))
    want = ref.point_compare(s["data"], s["stl"], s["ObsMask"], s["BB"], s["Res"], s["P"], DST, MAXD, order, OUTLIER)
    assert_scan_conditions(s["data"], want)
    return s, order, want


def close(a, b, rel):
    return abs(a - b) <= rel * abs(b)


def test_point_compare_and_scan_stats_on_synth_scene():
    from dmvsnet_amd import cloud_eval
    s, order, want = scene_and_restatement(31, 120000, 40000, 32)
    info = {}
    be = cloud_eval.point_compare(torch.from_numpy(s["data"]).cuda(), s["stl"], s["ObsMask"], s["BB"], s["Res"], s["P"], DST, MAXD,
                                  order=order, info=info)
    assert np.array_equal(be["Qdata_kept"].cpu().numpy(), want["kept"])
    assert np.array_equal(be["DataInMask"].cpu().numpy(), want["DataInMask"])
    assert np.array_equal(be["StlAbovePlane"].cpu().numpy(), want["StlAbovePlane"])
    # the scene exercises every branch of the classification and both tails of the distances
    assert 0.2 < want["kept"].mean() < 0.9 and 0.05 < want["DataInMask"].mean() < 0.95 and 0.05 < want["StlAbovePlane"].mean() < 0.95
    assert (want["Ddata"] == MAXD).any() and (want["Ddata"] > OUTLIER).any() and (want["Dstl"] > 1.0).any()
    for k in ("Ddata", "Dstl"):
        g, w = be[k].cpu().numpy(), want[k]
        assert np.all(np.abs(g - w) <= 1e-12 * w) and np.array_equal(g == MAXD, w == MAXD)
    st, ws = cloud_eval.scan_stats(be, OUTLIER), want["stats"]
    print("device", st)
    print("restatement", ws)
    assert st["nData"] == ws["nData"] > 1000 and st["nStl"] == ws["nStl"] > 1000
    for k in ("MeanData", "MeanStl", "VarData", "VarStl"):
        assert close(st[k], ws[k], 1e-9), k
    for k in ("MedData", "MedStl"):
        assert close(st[k], ws[k], 1e-12), k
    assert info["thinning"]["rounds"] < 64


def test_evaluate_dtu_on_a_synthetic_dataset(tmp_path):
    from dmvsnet_amd import cloud_eval, eval_io, fusion, synth
    data_path, ply_dir, out_dir = tmp_path / "MVSData", tmp_path / "out" / "pcd", tmp_path / "results"
    os.makedirs(data_path / "Points" / "stl")
    os.makedirs(data_path / "ObsMask")
    os.makedirs(ply_dir)
    scans, want = (4, 114), {}
    for k, scan in enumerate(scans):
        s = synth.synth_cloud_scene(40 + k, 30000 + 5000 * k, 12000)
        name = eval_io.ply_path(str(tmp_path / "out"), "scan%d" % scan)
        assert name == str(ply_dir / ("mvsnet%03d_l3.ply" % scan))
        fusion.write_ply(name, s["data"], np.zeros((len(s["data"]), 3), np.uint8))
        fusion.write_ply(str(data_path / "Points" / "stl" / ("stl%03d_total.ply" % scan)), s["stl"], np.zeros((len(s["stl"]), 3), np.uint8))
        np.savez(data_path / "ObsMask" / ("ObsMask%d_10.npz" % scan), ObsMask=s["ObsMask"], BB=s["BB"], Res=s["Res"])
        np.savez(data_path / "ObsMask" / ("Plane%d.npz" % scan), P=s["P"])
        order = rng_of(5).permutation(len(s["data"]))           # evaluate_dtu(seed=5): the default seeded host permutation
        want[scan] = ref.point_compare(s["data"], s["stl"], s["ObsMask"], s["BB"], s["Res"], s["P"], DST, MAXD, order, OUTLIER)
        assert_scan_conditions(s["data"], want[scan])
    tot = cloud_eval.evaluate_dtu(str(ply_dir), str(data_path), str(out_dir), scans=scans, seed=5)
    acc = [want[s]["stats"]["MeanData"] for s in scans]
    comp = [want[s]["stats"]["MeanStl"] for s in scans]
    text = (out_dir / "TotalStat_mvsnet_Eval_.txt").read_bytes()
    print(text.decode())
    assert text == ref.total_stat_text(scans, acc, comp)
    assert close(tot["acc"], np.mean(acc), 1e-9) and close(tot["comp"], np.mean(comp), 1e-9)
    assert close(tot["overall"], (np.mean(acc) + np.mean(comp)) / 2, 1e-9)
    for s in scans:
        assert tot["scans"][s]["nData"] == want[s]["stats"]["nData"] and tot["scans"][s]["nStl"] == want[s]["stats"]["nStl"]
        assert tot["scans"][s]["kept"] == int(want[s]["kept"].sum())
        assert (out_dir / ("mvsnet_Eval_%d.json" % s)).exists()
