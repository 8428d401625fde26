"""N5 (DTU point-cloud evaluation) without a GPU: the ABI surface, the restatement against itself, the host-side I/O and text."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cloud_eval_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("dmvs_cloud_cell_keys", "dmvs_cloud_cell_runs", "dmvs_cloud_thin_round", "dmvs_cloud_nn", "dmvs_cloud_in_mask",
                "dmvs_cloud_above_plane", "dmvs_cloud_in_box")


def test_entry_points_declared_bound_and_exported():
    import dmvsnet_amd
    from dmvsnet_amd import _lib, cloud_eval
    header = open(os.path.join(ROOT, "include", "dmvs.h")).read()
    declared = set(re.findall(r"\b(dmvs_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    for fn in ("reduce_points", "max_dist_cp", "point_compare", "scan_stats", "evaluate_dtu"):
        assert callable(getattr(cloud_eval, fn)) and getattr(dmvsnet_amd, fn) is getattr(cloud_eval, fn)
    assert cloud_eval.DTU_TEST_SETS == (1, 4, 9, 10, 11, 12, 13, 15, 23, 24, 29, 32, 33, 34, 48, 49, 62, 75, 77, 110, 114, 118)
    # the kernels live in a header that fusion.hip includes (the set of .hip files is pinned by test_boundary)
    assert '#include "cloud_eval.h"' in open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "fusion.hip")).read()
    assert "cloud_eval.h" in open(os.path.join(ROOT, "dmvsnet_amd", "csrc", "Makefile")).read()


def nn_scene(seed, n_to=4000, n_from=3000):
    """A surface patch + noisy queries with far outliers, queries outside the domain on every face, and a far corner of the box
    with no to-point within max_dist.  BB is not a multiple of max_dist."""
    rng = np.random.Generator(np.random.PCG64(seed))
    bb = np.array([[-30.0, -20.0, -50.0], [175.0, 131.0, 95.0]])
    to = np.stack([rng.uniform(0, 90, n_to), rng.uniform(0, 80, n_to), rng.uniform(-2, 2, n_to)], 1)
    frm = np.stack([rng.uniform(0, 90, n_from), rng.uniform(0, 80, n_from), rng.normal(0, 0.3, n_from)], 1)
    k = n_from // 10
    frm[:k, 2] += rng.choice([-1.0, 1.0], k) * rng.uniform(5, 75, k)          # far outliers, some beyond 60 mm
    frm[k:2 * k] = rng.uniform([-80, -80, -120], [260, 220, 200], (k, 3))     # anywhere, incl. outside the domain on every face
    frm[2 * k:2 * k + 20] = rng.uniform([190, 140, 100], [209, 159, 129], (20, 3))  # in the domain, nothing within 60 mm
    to[:50] = rng.uniform([-89, -79, -109], [-31, -21, -51], (50, 3))         # to-points outside BB but inside the grown box
    return to.astype(np.float32), frm.astype(np.float32), bb


def test_block_form_equals_bounded_nn_with_domain_rule():
    for seed in (1, 2):
        to, frm, bb = nn_scene(seed)
        for a, b in ((to, frm), (frm, to)):
            blocks = ref.max_dist_cp_blocks(a, b, bb, 60.0)
            dom = ref.in_domain(b, bb, 60.0)
            assert 0 < dom.sum() < len(b)
            assert np.array_equal(np.minimum(blocks, 60.0), ref.bounded_nn(a, b, bb, 60.0))
            assert np.all(blocks[~dom] == 60.0)
        blocks = ref.max_dist_cp_blocks(to, frm, bb, 60.0)
        assert (blocks[ref.in_domain(frm, bb, 60.0)] >= 60.0).any()       # the empty neighbourhood
        assert np.all(ref.max_dist_cp_blocks(np.zeros((0, 3), np.float32), frm, bb, 60.0) == 60.0)


def thin_cloud(seed, n=3000):
    rng = np.random.Generator(np.random.PCG64(seed))
    p = np.stack([rng.uniform(0, 8, n), rng.uniform(0, 8, n), rng.normal(0, 0.05, n)], 1).astype(np.float32)
    p[n - 40:] = p[:40]                                   # exact duplicates
    p[100:400] = p[100] + rng.uniform(0, 0.15, (300, 3)).astype(np.float32)   # a clump
    return p


def test_fixed_point_schedule_keeps_the_sequential_points():
    for seed in (3, 4):
        p = thin_cloud(seed)
        rng = np.random.Generator(np.random.PCG64(100 + seed))
        order = rng.permutation(len(p))
        adj = ref.adjacency(p, 0.2)
        assert not np.any(np.abs(adj[2] - 0.2) < 1e-7)
        want = ref.reduce_points_sequential(p, 0.2, order, adj)
        assert 0 < want.sum() < len(p)
        # maximal independent set: no two kept points are neighbours, every removed point has a kept neighbour
        start, nbr, _ = adj
        for i in range(len(p)):
            nb = nbr[start[i]:start[i + 1]]
            assert (not want[nb].any()) if want[i] else want[nb].any()
        got_sync, rounds = ref.reduce_points_fixed_point(p, 0.2, order, in_place=False, adj=adj)
        assert np.array_equal(got_sync, want) and 1 < rounds < 64
        for visit in (np.arange(len(p))[::-1], rng.permutation(len(p))):
            got, r2 = ref.reduce_points_fixed_point(p, 0.2, order, in_place=True, visit=visit, adj=adj)
            assert np.array_equal(got, want) and r2 <= rounds


def test_ply_reader(tmp_path):
    from dmvsnet_amd import cloud_eval, fusion
    rng = np.random.Generator(np.random.PCG64(5))
    xyz = rng.normal(0, 100, (257, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (257, 3)).astype(np.uint8)
    f = str(tmp_path / "a.ply")
    fusion.write_ply(f, xyz, rgb)
    assert np.array_equal(cloud_eval.read_ply_xyz(f), xyz)
    # ASCII with normals in front of the positions, a comment and a face element behind the vertices
    g = str(tmp_path / "b.ply")
    with open(g, "w") as fh:
        fh.write("ply\nformat ascii 1.0\ncomment made by a test\nelement vertex 5\nproperty float nx\nproperty float ny\nproperty float nz\n"
                 "property float x\nproperty float y\nproperty float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n")
        for r in xyz[:5]:
            fh.write("0 0 1 %r %r %r\n" % (float(r[0]), float(r[1]), float(r[2])))
        fh.write("3 0 1 2\n")
    assert np.array_equal(cloud_eval.read_ply_xyz(g), xyz[:5])
    # binary with extra properties (double positions, normals, colour)
    h = str(tmp_path / "c.ply")
    v = np.zeros(7, dtype=[("x", "<f8"), ("nx", "<f4"), ("y", "<f8"), ("z", "<f8"), ("red", "u1")])
    v["x"], v["y"], v["z"], v["nx"] = xyz[:7, 0], xyz[:7, 1], xyz[:7, 2], 0.5
    with open(h, "wb") as fh:
        fh.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty double x\nproperty float nx\nproperty double y\n"
                 b"property double z\nproperty uchar red\nend_header\n")
        fh.write(v.tobytes())
    assert np.array_equal(cloud_eval.read_ply_xyz(h), xyz[:7])
    with open(h, "r+b") as fh:
        fh.truncate(os.path.getsize(h) - 3)
    with pytest.raises(cloud_eval._lib.DmvsError):
        cloud_eval.read_ply_xyz(h)


def test_mask_and_plane_loaders_npz(tmp_path):
    from dmvsnet_amd import cloud_eval
    mask = (np.arange(4 * 5 * 6).reshape(4, 5, 6) % 3 == 0)
    bb = np.array([[-1.5, 2.0, 3.0], [10.0, 20.0, 30.0]])
    np.savez(tmp_path / "ObsMask7_10.npz", ObsMask=mask, BB=bb, Res=np.array([[0.25]]))
    np.savez(tmp_path / "Plane7.npz", P=np.array([[0.1], [0.2], [0.3], [-4.0]]))
    m, b, r = cloud_eval.load_obs_mask(str(tmp_path / "ObsMask7_10.npz"))
    assert m.dtype == np.uint8 and m.flags.c_contiguous and np.array_equal(m, mask.astype(np.uint8))
    assert np.array_equal(b, bb) and r == 0.25
    assert np.array_equal(cloud_eval.load_plane(str(tmp_path / "Plane7.npz")), [0.1, 0.2, 0.3, -4.0])
    np.savez(tmp_path / "bad.npz", BB=bb)
    with pytest.raises(cloud_eval._lib.DmvsError):
        cloud_eval.load_obs_mask(str(tmp_path / "bad.npz"))
    (tmp_path / "v73.mat").write_bytes(b"MATLAB 7.3 MAT-file, Platform: GLNXA64" + b"\0" * 200)
    with pytest.raises(cloud_eval._lib.DmvsError, match="7.3"):
        cloud_eval.load_plane(str(tmp_path / "v73.mat"))


def test_mask_and_plane_loaders_mat(tmp_path):
    sio = pytest.importorskip("scipy.io")
    from dmvsnet_amd import cloud_eval
    mask = (np.arange(3 * 4 * 5).reshape(3, 4, 5) % 2 == 0)
    bb = np.array([[-1.0, -2.0, -3.0], [4.0, 5.0, 6.0]])
    sio.savemat(str(tmp_path / "ObsMask3_10.mat"), dict(ObsMask=mask, BB=bb, Res=0.5))
    sio.savemat(str(tmp_path / "Plane3.mat"), dict(P=np.array([[0.0], [0.0], [1.0], [-2.0]])))
    m, b, r = cloud_eval.load_obs_mask(str(tmp_path / "ObsMask3_10.mat"))
    assert m.shape == (3, 4, 5) and np.array_equal(m, mask.astype(np.uint8)) and np.array_equal(b, bb) and r == 0.5
    assert np.array_equal(cloud_eval.load_plane(str(tmp_path / "Plane3.mat")), [0.0, 0.0, 1.0, -2.0])


def test_total_stat_text_and_statistics():
    from dmvsnet_amd import cloud_eval
    got = cloud_eval.total_stat_text([1, 114], [0.35, 0.4512349], [0.3, 0.25])
    assert got == (b"mean acc:0.400617\tmean comp:0.275000\tmean overall:0.337809\r\n"
                   b"scans\tacc  \tcmop  \r\n"
                   b"scan1\t0.3500\t0.3000\r\n"
                   b"scan114\t0.4512\t0.2500\r\n")
    assert got == ref.total_stat_text([1, 114], [0.35, 0.4512349], [0.3, 0.25])
    # median rule for odd and even n, variance with N - 1, the outlier threshold is strict
    be = dict(Ddata=torch.tensor([3.0, 1.0, 20.0, 2.0, 7.0, 60.0], dtype=torch.float64),
              DataInMask=torch.tensor([True, True, True, True, False, True]),
              Dstl=torch.tensor([4.0, 1.0, 3.0, 2.0, 19.999], dtype=torch.float64),
              StlAbovePlane=torch.tensor([True, True, True, True, False]))
    st = cloud_eval.scan_stats(be, outlier=20.0)
    assert (st["nData"], st["MeanData"], st["VarData"], st["MedData"]) == (3, 2.0, 1.0, 2.0)
    assert (st["nStl"], st["MeanStl"], st["MedStl"]) == (4, 2.5, 2.5) and abs(st["VarStl"] - 5.0 / 3.0) < 1e-15
    assert ref.stats([4.0, 1.0, 3.0, 2.0]) == (4, 2.5, st["VarStl"], 2.5)
    assert cloud_eval.nn_levels(60.0) == [(0.5, 4), (4.0, 4), (32.0, 2)]


def test_refusals():
    from dmvsnet_amd import _lib, cloud_eval
    lib = _lib.load()
    # a grid axis beyond 2^21 cells is refused by the entry point before anything is launched (the pointers are never followed)
    fake = ctypes.c_void_p(256)
    origin = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    assert lib.dmvs_cloud_cell_keys(fake, 10, origin, 0.2, (ctypes.c_int * 3)(1 << 21, 4, 2 ** 21 + 1), fake, None) == _lib.EINVAL
    assert lib.dmvs_cloud_cell_keys(fake, 10, origin, 0.0, (ctypes.c_int * 3)(4, 4, 4), fake, None) == _lib.EINVAL
    assert lib.dmvs_cloud_cell_keys(None, 10, origin, 0.2, (ctypes.c_int * 3)(4, 4, 4), fake, None) == _lib.EINVAL
    assert lib.dmvs_cloud_nn(fake, fake, fake, 1, origin, 0.5, (ctypes.c_int * 3)(4, 2 ** 21 + 1, 4), fake, None, 1, 4, 60.0, fake, None,
                             fake, fake, None, None) == _lib.EINVAL
    with pytest.raises(_lib.DmvsError, match="2\\^21"):
        cloud_eval.check_grid([10, (1 << 21) + 1, 10])
    cloud_eval.check_grid([1 << 21, 1, 1])
    if not torch.cuda.is_available():
        pts = np.zeros((4, 3), np.float32)
        for call in (lambda: cloud_eval.reduce_points(pts), lambda: cloud_eval.max_dist_cp(pts, pts, np.array([[0, 0, 0], [1, 1, 1.0]])),
                     lambda: cloud_eval.point_compare(pts, pts, np.ones((2, 2, 2), np.uint8), np.zeros((2, 3)), 1.0, np.ones(4))):
            with pytest.raises(_lib.DmvsError, match="no CPU fallback"):
                call()
