"""GPU (-m gpu): scan-level fusion on device-resident maps (fusion.fuse_view / ScanFusion, run_test(resident_fusion=True)).

* The fused per-view pass against ViewFilter + the per-pair kernels on the same inputs: masks and averaged depth
  bit-identical, the same points in the same (row-major) order, xyz within 1 fp32 ulp -- static and dynamic filters,
  1..16 sources, stage confidences or a scalar conf, zero depths, sizes that are not a multiple of the workgroup.
* ScanFusion against fuse_scene on the files of the same scene (incl. the colour subsampling of 1- / 2-stage nets) and
  against the reference's filters (tests/golden/fusion_scene.npz, the tolerances of test_fuse_scene_vs_reference).
* run_test(feature_cache=True, resident_fusion=True) against run_test(feature_cache=True): the same files (mask PNGs: the
  same pixels), the same PLY up to 1 ulp of xyz, the same return value.
xyz: where an fp64 sum cancels to ~1e-15 its sign depends on the reduction order (torch.mm vs the emit kernel's fma
chain); such values are allowed within fp64 rounding of the point's scale (_check_xyz).
* The refusals.
"""
import io
import os

import numpy as np
import pytest
import torch

from dmvsnet_amd import MVSNet, eval_io, synth
from dmvsnet_amd._lib import DmvsError
from dmvsnet_amd.fusion import ScanFusion, ViewFilter, fuse_scene, fuse_view, read_camera_parameters
from fusion_ref import _check_xyz, _ulps  # noqa: F401  (the 1-ulp rule, shared with test_fusion_ref_gpu.py)
from test_fusion import CONF, PAIRS, _plane_depths, _scene
from test_scan_cpu import dtu_like_pairs, write_scene

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _check_view(depths, confs, cam, ref, srcs, conf, thres_view, dynamic, stages):
    """fuse_view vs ViewFilter on one reference view; -> number of points."""
    c2 = confs[ref][1] if stages else None
    c1 = confs[ref][0] if stages else None
    vf = ViewFilter(depths[ref], cam(ref), confs[ref][2], conf, c2, c1, dynamic)
    for s in srcs:
        vf.add_source(depths[s], cam(s))
    H, W = depths[ref].shape
    want = vf.finish(np.zeros((H, W, 3), np.float32), thres_view)
    scalar = np.isscalar(conf)
    th = (conf,) * 3 if scalar else conf
    out = fuse_view(_dev(depths[ref]), cam(ref), [_dev(depths[s]) for s in srcs], [cam(s) for s in srcs],
                    _dev(confs[ref][2]), None if (scalar or not stages) else _dev(c2),
                    None if (scalar or not stages) else _dev(c1), th, thres_view, dynamic)
    m = out["masks"].cpu().numpy()
    for k, w in enumerate((want.photo_mask, want.geo_mask, want.final_mask)):
        assert np.array_equal(m[k] != 0, w), (ref, k, int(((m[k] != 0) != w).sum()))
        assert set(np.unique(m[k]).tolist()) <= {0, 255}
    assert out["depth_avg"].cpu().numpy().tobytes() == want.depth_averaged.tobytes(), ref
    n = int(out["count"].item())
    assert n == len(want.xyz) == int(want.final_mask.sum())
    return n, _check_xyz(out["xyz"][:n].cpu().numpy(), want.xyz)


@pytest.mark.parametrize("dynamic,nsrc", [(False, 1), (False, 4), (False, 10), (False, 16), (True, 1), (True, 4), (True, 10)])
def test_fuse_view_equals_view_filter(dynamic, nsrc):
    H, W, V = 37, 53, nsrc + 1
    cams, depths, confs, _ = synth.synth_fusion_scene(H, W, V, seed=nsrc)
    depths[0][0, :] = 0.0                         # zero reference depths: the static filter's 1e-4 patch
    cam = lambda v: (cams[v, 1, :3, :3].copy(), cams[v, 0].copy())   # noqa: E731
    srcs = list(range(1, V))
    tv = min(2, nsrc)
    npts = 0
    for conf, stages in (((0.1, 0.2, 0.3), True), ((0.05, 0.1, 0.2), False), (0.4, True)):
        n, _ = _check_view(depths, confs, cam, 0, srcs, conf, tv, dynamic, stages)
        npts += n
    # and a second reference view with the sources in another order
    n, _ = _check_view(depths, confs, cam, V - 1, list(range(V - 1))[::-1], (0.1, 0.2, 0.3), tv, dynamic, True)
    # (one source: the dynamic filter's gates start at two views, nothing passes -- in the reference as well)
    assert (npts + n > 0) == (not dynamic or nsrc > 1)


@pytest.mark.parametrize("dynamic", [False, True])
def test_fuse_view_on_exact_plane(dynamic):
    H, W, V = 96, 128, 5
    cams, depths = _plane_depths(H, W, V, z0=650.0)
    cam = lambda v: (cams[v, 1, :3, :3], cams[v, 0])   # noqa: E731
    conf = np.full((H, W), 0.9, np.float32)
    conf[:, :10] = 0.0
    confs = [(conf, conf, conf)] * V
    n, _ = _check_view(depths, confs, cam, 0, [1, 2, 3, 4], 0.1, 2, dynamic, False)
    assert n > 0.3 * H * W


# ------------------------------------------------------------------------------------------ ScanFusion vs fuse_scene
def _ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n")
    v = np.frombuffer(body, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
    return head, v


def _same_outputs(a, b, dynamic, refs):
    """Folders a (file path) and b (resident path): the mask PNGs decode to the same pixels, the averaged depth PFMs
    (dynamic filter) are byte-equal."""
    from PIL import Image
    for r in refs:
        for kind in ("photo", "geo", "final"):
            p = "mask/{:0>8}_{}.png".format(r, kind)
            assert np.array_equal(np.array(Image.open(os.path.join(a, p))), np.array(Image.open(os.path.join(b, p)))), p
        if dynamic:
            p = "depth_est/{:0>8}_averaged.pfm".format(r)
            assert open(os.path.join(a, p), "rb").read() == open(os.path.join(b, p), "rb").read(), p


def _compare_ply(pa, pb):
    ha, va = _ply(pa)
    hb, vb = _ply(pb)
    assert ha == hb and len(va) == len(vb)
    for c in ("r", "g", "b"):
        assert np.array_equal(va[c], vb[c])
    return len(va), _check_xyz(np.stack([va[c] for c in "xyz"], 1), np.stack([vb[c] for c in "xyz"], 1))


def _write_folder(root, depths, confs, cams, imgs, stages):
    from PIL import Image
    for sub in ("cams", "images", "depth_est", "confidence"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for v in range(len(depths)):
        eval_io.write_cam(os.path.join(root, "cams/{:0>8}_cam.txt".format(v)), cams[v])
        Image.fromarray(imgs[v]).save(os.path.join(root, "images/{:0>8}.jpg".format(v)))
        eval_io.save_pfm(os.path.join(root, "depth_est/{:0>8}.pfm".format(v)), depths[v])
        eval_io.save_pfm(os.path.join(root, "confidence/{:0>8}.pfm".format(v)), confs[v][2])
        if stages:
            eval_io.save_pfm(os.path.join(root, "confidence/{:0>8}_stage2.pfm".format(v)), confs[v][1])
            eval_io.save_pfm(os.path.join(root, "confidence/{:0>8}_stage1.pfm".format(v)), confs[v][0])


@pytest.mark.parametrize("num_stage,dynamic,stages,conf", [(3, False, True, (0.1, 0.2, 0.3)), (3, True, False, 0.2),
                                                           (2, False, False, (0.1, 0.1, 0.2)), (1, True, True, (0.1, 0.2, 0.3))])
def test_scan_fusion_equals_fuse_scene(tmp_path, num_stage, dynamic, stages, conf):
    """Maps at 1 / (2 ** (3 - num_stage)) of the image size: the colours are the image's [1::step, 1::step] pixels."""
    from PIL import Image
    H, W, V = 37, 53, 7
    step = 2 ** (3 - num_stage)
    cams, depths, confs, _ = synth.synth_fusion_scene(H, W, V, seed=11)
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (H * step, W * step, 3), dtype=np.uint8) for _ in range(V)]
    pairs = [(v, srcs) for v, srcs in dtu_like_pairs(V, 4).items()][::-1]     # the last views first
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _write_folder(a, depths, confs, cams, imgs, stages)
    os.makedirs(os.path.join(b, "depth_est"))
    sa = fuse_scene(pairs, a, os.path.join(a, "out.ply"), conf=conf, thres_view=2, dynamic=dynamic, num_stage=num_stage)
    fz = ScanFusion(pairs, conf=conf, thres_view=2, dynamic=dynamic, num_stage=num_stage)
    for v in np.random.default_rng(3).permutation(V):
        cam = read_camera_parameters(os.path.join(a, "cams/{:0>8}_cam.txt".format(v)))
        with Image.open(os.path.join(a, "images/{:0>8}.jpg".format(v))) as im:
            img = np.asarray(im)
        fz.add(v, _dev(depths[v]), _dev(confs[v][2]), cam, img, _dev(confs[v][1]) if stages else None,
               _dev(confs[v][0]) if stages else None)
    assert fz.fused_views() == V and not fz.depth and not fz.conf     # every map released
    sb = fz.write(b, os.path.join(b, "out.ply"))
    assert sa == sb
    _same_outputs(a, b, dynamic, range(V))
    n, nd = _compare_ply(os.path.join(a, "out.ply"), os.path.join(b, "out.ply"))
    print(f"points {n}, xyz values 1 ulp apart: {nd}")
    assert n > 0


def test_scan_fusion_vs_reference(golden, tmp_path):
    """ScanFusion on the scene the reference's filters were run on (tolerances of test_fuse_scene_vs_reference)."""
    g = golden("fusion_scene.npz")
    cams, depths, confs, _, cam = _scene()
    for tag, dynamic in (("pcd", False), ("dy", True)):
        out = tmp_path / tag
        (out / "depth_est").mkdir(parents=True)
        fz = ScanFusion(PAIRS, conf=CONF, thres_view=2, dynamic=dynamic)
        for v in (4, 3, 2, 1, 0):
            fz.add(v, _dev(depths[v]), _dev(confs[v][2]), cam(v), g[f"img.{v}"], _dev(confs[v][1]), _dev(confs[v][0]))
        fz.write(str(out), str(out / "out.ply"))
        from PIL import Image
        for r, _ in PAIRS:
            for kind in ("photo", "geo", "final"):
                got = np.array(Image.open(out / "mask/{:0>8}_{}.png".format(r, kind))) > 0
                want = g[f"{tag}.mask.{r}.{kind}"]
                assert (got != want).sum() <= (0 if kind == "photo" else 12), (tag, r, kind, int((got != want).sum()))
        _, pts = _ply(str(out / "out.ply"))
        v = g[f"{tag}.vertex"]
        assert abs(len(pts) - len(v)) <= 36
        key = lambda x, y, z: set(zip(np.round(x, 1).tolist(), np.round(y, 1).tolist(), np.round(z, 1).tolist()))   # noqa: E731
        a, b = key(pts["x"], pts["y"], pts["z"]), key(v["x"], v["y"], v["z"])
        assert len(a & b) > 0.99 * len(b)


# ------------------------------------------------------------------------------------------ run_test end to end
def _net(ndepths, ratios, inverse=False, seed=1):
    net = MVSNet(ndepths, ratios, inverse_depth=inverse, verbose=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed))
    net.return_prob_volume = False
    return net.cuda()


def _files(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _compare_run_test(net, data, scans, tmp, nv, mh, mw, **kw):
    a, b = str(tmp / "a"), str(tmp / "b")
    ra = eval_io.run_test(net, data, scans, a, nv, mh, mw, feature_cache=True, **kw)
    stats = {}
    rb = eval_io.run_test(net, data, scans, b, nv, mh, mw, feature_cache=True, resident_fusion=True, stats=stats, **kw)
    assert ra == rb
    fa, fb = _files(a), _files(b)
    assert sorted(fa) == sorted(fb)
    from PIL import Image
    npts = 0
    for k in fa:
        if k.endswith(".png"):
            assert np.array_equal(np.array(Image.open(io.BytesIO(fa[k]))), np.array(Image.open(io.BytesIO(fb[k])))), k
        elif k.endswith(".ply"):
            n, nd = _compare_ply(os.path.join(a, k), os.path.join(b, k))
            print(f"{k}: {n} points, xyz values 1 ulp apart: {nd}")
            npts += n
        else:
            assert fa[k] == fb[k], k
    assert stats["fused_views"] == stats["maps"] and stats["fusion_peak_bytes"] > 0
    assert stats["phases_s"]["fuse"] > 0 and stats["phases_s"]["fuse_write"] > 0
    return npts


def test_run_test_resident_fusion_equals_file_path(tmp_path):
    net = _net([16, 8, 8], [3, 2, 1])
    data = str(tmp_path / "data")
    write_scene(data, "scan3", [(64, 96)] * 6, pairs=dtu_like_pairs(6, 4))
    # the first views wait for the last ones
    write_scene(data, "late", [(64, 96)] * 5, pairs={0: [4, 3], 1: [4, 2], 2: [4, 3], 3: [4, 0], 4: [3, 2]})
    cfg = {"scan3": {"conf": (0.0, 0.0, 0.05)}, "late": {"conf": 0.05}}
    for method in ("pcd", "dypcd"):
        _compare_run_test(net, data, ["scan3", "late"], tmp_path / method, 3, 1200, 1600, thres_view=2,
                          filter_method=method, scene_cfg=cfg)


def test_run_test_resident_fusion_fix_res(tmp_path):
    net = _net([16, 8, 8], [3, 2, 1])
    data = str(tmp_path / "data")
    write_scene(data, "scan5", [(64, 96), (64, 96), (96, 64), (64, 96), (64, 96)], pairs=dtu_like_pairs(5, 3))
    _compare_run_test(net, data, ["scan5"], tmp_path / "f", 3, 1200, 1600, conf=(0.0, 0.0, 0.0), thres_view=2,
                      fix_res=True)


def test_run_test_resident_fusion_dtu_recipe(tmp_path):
    """8 synthetic 1600x1200 JPEGs -> 864x1152, 5 views, 48/32/8, inverse depth (scripts/dtu_test.sh's recipe)."""
    net = _net([48, 32, 8], [4, 2, 1], inverse=True)
    data = str(tmp_path / "data")
    write_scene(data, "scan1", [(1200, 1600)] * 8, pairs=dtu_like_pairs(8, 7))
    _compare_run_test(net, data, ["scan1"], tmp_path / "d", 5, 864, 1152, numdepth=192, inverse_depth=True,
                      conf=(0.0, 0.0, 0.0), thres_view=2)


# ------------------------------------------------------------------------------------------ refusals
def test_refusals(tmp_path):
    net = _net([16, 8, 8], [3, 2, 1])
    with pytest.raises(DmvsError):
        eval_io.run_test(net, str(tmp_path), ["x"], str(tmp_path / "o"), 3, 64, 96, resident_fusion=True)
    with pytest.raises(DmvsError):
        ScanFusion([(0, list(range(1, 18)))])                      # 17 sources
    with pytest.raises(DmvsError):
        ScanFusion([(0, list(range(1, 12)))], dynamic=True)       # 11 sources, nine gates
    H, W = 37, 53
    cams, depths, confs, _ = synth.synth_fusion_scene(H, W, 4, seed=2)
    cam = lambda v: (cams[v, 1, :3, :3].copy(), cams[v, 0].copy())   # noqa: E731
    img = np.zeros((H, W, 3), np.uint8)
    # maps of different sizes in one scene
    fz = ScanFusion([(0, [1]), (1, [0])])
    fz.add(0, _dev(depths[0]), _dev(confs[0][2]), cam(0), img)
    with pytest.raises(DmvsError):
        fz.add(1, _dev(depths[1][:, :-1]), _dev(confs[1][2][:, :-1]), cam(1), img)
    fz.close()
    # a source that never gets a map; write() before every view is fused
    fz = ScanFusion([(0, [1, 3]), (1, [0]), (2, [0, 1])])
    for v in (0, 1, 2):
        fz.add(v, _dev(depths[v]), _dev(confs[v][2]), cam(v), img)
    with pytest.raises(DmvsError, match="3"):
        fz.write(str(tmp_path), str(tmp_path / "x.ply"))
    fz.close()
    assert not os.path.exists(tmp_path / "x.ply")
    with pytest.raises(DmvsError):
        fuse_view(_dev(depths[0]), cam(0), [_dev(depths[1][:-1])], [cam(1)], _dev(confs[0][2]))
