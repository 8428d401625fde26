"""GPU (-m gpu): the scan-level eval path (dmvsnet_amd/scan.py) against the default per-sample path.

* dmvs_image_ingest equals eval_io.MVSDataset's host images bit for bit (identity, downscale, odd / base-32 sizes, the
  chained fp32 pass, stack-slot and HWC outputs).
* MVSNet.encode_views + forward_features gives the same bits as forward on every output key, and refuses what it must.
* save_depth_maps / run_test with feature_cache write byte-identical files.
"""
import os

import numpy as np
import pytest
import torch

from dmvsnet_amd import MVSNet, eval_io, ops, synth
from dmvsnet_amd._lib import DmvsError
from dmvsnet_amd.scan import ScanPlan, _Tables, ingest_chain
from test_scan_cpu import dtu_like_pairs, write_scene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
pytestmark = pytest.mark.gpu


def _net(ndepths, ratios, inverse=False, seed=1):
    net = MVSNet(ndepths, ratios, inverse_depth=inverse, verbose=False)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), seed))
    return net.cuda()


def _equal_dicts(a, b, path=""):
    assert sorted(a) == sorted(b), (path, sorted(a), sorted(b))
    for k in a:
        if isinstance(a[k], dict):
            _equal_dicts(a[k], b[k], path + k + ".")
        else:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (path + k)
            assert torch.equal(a[k], b[k]), path + k


# ------------------------------------------------------------------------------------------ ingest kernel
def test_ingest_equals_loader_images(tmp_path):
    from PIL import Image
    root = str(tmp_path)
    write_scene(root, "sM", [(150, 200), (200, 150), (157, 211), (200, 150)])
    tables = _Tables(torch.device("cuda"))
    cases = [(os.path.join(GOLDEN, "eval_scene"), "scanA", 3, (1200, 1600), False),   # identity (base-32 sized images)
             (root, "sM", 4, (96, 128), False),                                       # downscale + chained resize
             (root, "sM", 4, (96, 128), True),                                        # fix_res
             (root, "sM", 3, (1200, 1600), False)]                                    # rounding down to base 32 only
    n_chained = 0
    for datapath, scan, nv, (mh, mw), fix in cases:
        ds = eval_io.MVSDataset(datapath, [scan], "test", nv, 192, 1.06, max_h=mh, max_w=mw, fix_res=fix)
        plan = ScanPlan(datapath, scan, nv, 192, 1.06, False, mh, mw, fix)
        for i, p in enumerate(plan.samples):
            want = torch.from_numpy(ds[i]["imgs"])
            stack = torch.full((len(p.view_ids) + 1, 3) + p.size, -1.0, device="cuda")
            for k, (vid, chain) in enumerate(zip(p.view_ids, p.chains)):
                u8 = torch.from_numpy(np.array(Image.open(plan.image_path(vid)))).cuda()
                ingest_chain(u8, chain, tables, stack[k + 1])          # into a slot of a FeatureNet input stack
                n_chained += chain[1] != chain[2]
            torch.cuda.synchronize()
            assert torch.equal(stack[1:].cpu(), want), (scan, i, p.chains)
            assert (stack[0] == -1.0).all()                             # nothing written outside the slot
    assert n_chained > 0


@pytest.mark.parametrize("src_hw,dst_hw", [((37, 53), (20, 31)), ((64, 96), (64, 96)), ((150, 200), (96, 128)),
                                           ((31, 45), (31, 60)), ((120, 160), (33, 17))])
def test_ingest_odd_sizes_hwc_and_float_input(src_hw, dst_hw):
    rng = np.random.default_rng(sum(src_hw + dst_hw))
    u8 = rng.integers(0, 256, src_hw + (3,), dtype=np.uint8)
    f = np.array(u8, dtype=np.float32) / 255.0
    want = eval_io.resize_linear(f, *dst_hw)                            # [H,W,3]
    tables = _Tables(torch.device("cuda"))
    taps = tables.taps(src_hw, dst_hw)
    chw = ops.image_ingest(torch.from_numpy(u8).cuda(), *dst_hw, tables.lut, taps)
    hwc = ops.image_ingest(torch.from_numpy(u8).cuda(), *dst_hw, tables.lut, taps, hwc=True)
    fin = ops.image_ingest(torch.from_numpy(f).cuda(), *dst_hw, None, taps, hwc=True)   # the chained pass's fp32 input
    torch.cuda.synchronize()
    assert torch.equal(hwc.cpu(), torch.from_numpy(np.ascontiguousarray(want)))
    assert torch.equal(chw.cpu(), torch.from_numpy(np.ascontiguousarray(want.transpose(2, 0, 1))))
    assert torch.equal(fin.cpu(), torch.from_numpy(np.ascontiguousarray(want)))


# ------------------------------------------------------------------------------------------ encode + forward_features
@pytest.mark.parametrize("cfg,inverse,fdt,two_streams", [("c1", False, "f32", True), ("c1", True, "f16", False),
                                                         ("c1s3", False, "f32", True), ("c1s3", True, "f32", False),
                                                         ("c1s3", False, "f16", True)])
def test_forward_features_equals_forward(cfg, inverse, fdt, two_streams):
    c = synth.CONFIGS[cfg]
    net = _net(c["ndepths"], c["ratios"], inverse)
    net.feature_dtype, net.two_streams = fdt, two_streams
    imgs, proj, dv = synth.synth_inputs(c["H"], c["W"], c["V"], seed=2)
    imgs, proj, dv = imgs.cuda(), {k: v.cuda() for k, v in proj.items()}, dv.cuda()
    ref = net(imgs, proj, dv)
    ref = {k: (v if not isinstance(v, dict) else dict(v)) for k, v in ref.items()}
    # encode out of order and in another grouping: FeatureNet's output depends on the image only
    views = net.encode_views(imgs[0].flip(0).contiguous())[::-1]
    assert all(v.size == (c["H"], c["W"]) and v.dtype == fdt for v in views)
    assert views[0].nbytes == (2 if fdt == "f16" else 4) * 28 * c["H"] * c["W"]
    got = net.forward_features(views, proj, dv)
    torch.cuda.synchronize()
    _equal_dicts(got, ref)


def test_forward_features_refusals():
    c = synth.CONFIGS["c1"]
    net = _net(c["ndepths"], c["ratios"])
    imgs, proj, dv = synth.synth_inputs(c["H"], c["W"], c["V"], seed=2)
    imgs, proj, dv = imgs.cuda(), {k: v.cuda() for k, v in proj.items()}, dv.cuda()
    views = net.encode_views(imgs[0])
    net.forward_features(views, proj, dv)
    small = net.encode_views(imgs[0][..., :64, :96].contiguous())
    with pytest.raises(DmvsError):          # mixed sizes
        net.forward_features([views[0], small[1], views[2]], proj, dv)
    with pytest.raises(DmvsError):          # batch > 1
        net.forward_features(views, {k: v.repeat(2, 1, 1, 1, 1) for k, v in proj.items()}, dv.repeat(2, 1))
    net.set_view_shard(object(), 0, 2)
    with pytest.raises(DmvsError):          # view sharding
        net.forward_features(views, proj, dv)
    net.set_view_shard(None, 0, 1)
    net.forward_features(views, proj, dv)
    net.load_state_dict(synth.synth_state_dict(net.state_dict(), 5))
    with pytest.raises(DmvsError):          # stale fingerprint: other weights
        net.forward_features(views, proj, dv)
    net.forward_features(net.encode_views(imgs[0]), proj, dv)


# ------------------------------------------------------------------------------------------ save_depth_maps / run_test
def _files(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _compare_runs(net, datapath, scans, tmp, nv, mh, mw, **kw):
    a = eval_io.save_depth_maps(net, datapath, scans, str(tmp / "a"), nv, mh, mw, **kw)
    outs = []
    for tag, fc in (("b", True), ("c", 1)):   # default budget; a 1-byte budget (every entry evicted at once)
        stats = {}
        b = eval_io.save_depth_maps(net, datapath, scans, str(tmp / tag), nv, mh, mw, feature_cache=fc, stats=stats, **kw)
        assert [os.path.relpath(p, str(tmp / tag)) for p in b] == [os.path.relpath(p, str(tmp / "a")) for p in a]
        fa, fb = _files(str(tmp / "a")), _files(str(tmp / tag))
        assert sorted(fa) == sorted(fb)
        for k in fa:
            assert fa[k] == fb[k], (tag, k)
        outs.append(stats)
    big, tiny = outs
    assert big["encodes"] == big["images"] and big["evictions"] == 0 and big["maps"] == len(a)
    assert tiny["encodes"] > tiny["images"] and tiny["evictions"] > 0
    return big


def test_save_depth_maps_cached_is_byte_identical(tmp_path):
    net = _net([16, 8, 8], [3, 2, 1])
    net.return_prob_volume = False
    data = str(tmp_path / "data")
    write_scene(data, "scan7", [(150, 200), (150, 200), (200, 150), (150, 200), (150, 200), (200, 150)],
                pairs=dtu_like_pairs(6, 5))
    st = _compare_runs(net, data, ["scan7"], tmp_path / "s", 4, 96, 128)
    assert st["images"] > 6                  # portrait views are also needed at the landscape size (chained resize)
    _compare_runs(net, os.path.join(GOLDEN, "eval_scene"), ["scanA", "scanB"], tmp_path / "g", 3, 1200, 1600,
                  inverse_depth=True)
    _compare_runs(net, data, ["scan7"], tmp_path / "f", 4, 96, 128, fix_res=True, scene_cfg={"scan7": {"max_h": 64, "max_w": 96}})


def test_run_test_cached_same_ply(tmp_path):
    net = _net([16, 8, 8], [3, 2, 1])
    net.return_prob_volume = False
    data = str(tmp_path / "data")
    write_scene(data, "scan9", [(64, 96)] * 5)
    for method in ("pcd", "dypcd"):
        res = {}
        for tag, fc in (("a", None), ("b", True)):
            out = str(tmp_path / (method + tag))
            res[tag] = (eval_io.run_test(net, data, ["scan9"], out, 4, 1200, 1600, conf=(0.0, 0.0, 0.0),
                                         filter_method=method, feature_cache=fc),
                        open(os.path.join(out, "pcd", "mvsnet009_l3.ply"), "rb").read())
        assert res["a"][0] == res["b"][0] and res["a"][1] == res["b"][1], method


def test_dtu_recipe_size_cached_is_byte_identical(tmp_path):
    """8 synthetic 1600x1200 JPEGs -> 864x1152, 5 views, 48/32/8, inverse depth (scripts/dtu_test.sh's recipe)."""
    net = _net([48, 32, 8], [4, 2, 1], inverse=True)
    net.return_prob_volume = False
    data = str(tmp_path / "data")
    write_scene(data, "scan1", [(1200, 1600)] * 8, pairs=dtu_like_pairs(8, 7))
    a = eval_io.save_depth_maps(net, data, ["scan1"], str(tmp_path / "a"), 5, 864, 1152, numdepth=192, inverse_depth=True)
    stats = {}
    b = eval_io.save_depth_maps(net, data, ["scan1"], str(tmp_path / "b"), 5, 864, 1152, numdepth=192, inverse_depth=True,
                                feature_cache=True, stats=stats)
    assert len(a) == len(b) == 8 and stats["encodes"] == stats["images"] == 8
    fa, fb = _files(str(tmp_path / "a")), _files(str(tmp_path / "b"))
    assert sorted(fa) == sorted(fb) and all(fa[k] == fb[k] for k in fa)
    d, _ = eval_io.read_pfm(b[0])
    assert d.shape == (864, 1152)
