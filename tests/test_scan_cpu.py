"""CPU (-m "not gpu"): the scan-level eval path's host side (dmvsnet_amd/scan.py).

* ScanPlan restates eval_io.MVSDataset without pixels: view ids, resize chains, proj_matrices, depth_values and filenames
  must equal the loader's bit for bit (committed eval_scene fixture and scenes that hit the resize / chained-resize /
  fix_res / per-scene-override branches).
* The ingest kernel's tables (resize taps, uint8 table) applied with NumPy fp32 in the kernel's order reproduce the loader's
  images exactly: a CPU restatement of dmvs_image_ingest that pins its arithmetic.
* FeatureCache bookkeeping with a fake encoder: one encode per image under a large budget, LRU under a small one, counters.
"""
import os

import numpy as np
import pytest

from dmvsnet_amd import eval_io, synth
from dmvsnet_amd.scan import FeatureCache, ScanPlan

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def write_scene(root, scan, sizes, pairs=None, depth_line="425.0 2.5", seed=3):
    """Scene with one image per entry of ``sizes`` ((h, w) each; mixed sizes and orientations allowed), synthetic cams and
    either ``pairs`` ({ref: [src, ...]}) or every other view as a source."""
    from PIL import Image
    os.makedirs(os.path.join(root, scan, "cams"))
    os.makedirs(os.path.join(root, scan, "images"))
    V = len(sizes)
    for v, (h, w) in enumerate(sizes):
        cams = synth.synth_cameras(h, w, V)["stage3"][0].numpy()        # intrinsics of this image's own size
        img = synth.synth_images(h, w, 1, seed=seed + v)[0, 0]
        Image.fromarray((img.permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(
            os.path.join(root, scan, "images", f"{v:08d}.jpg"), quality=90)
        with open(os.path.join(root, scan, "cams", f"{v:08d}_cam.txt"), "w") as f:
            f.write("extrinsic\n")
            for r in range(4):
                f.write(" ".join(repr(float(x)) for x in cams[v, 0, r]) + "\n")
            f.write("\nintrinsic\n")
            for r in range(3):
                f.write(" ".join(repr(float(x)) for x in cams[v, 1, r, :3]) + "\n")
            f.write("\n" + depth_line + "\n")
    pairs = pairs or {v: [u for u in range(V) if u != v] for v in range(V)}
    with open(os.path.join(root, scan, "pair.txt"), "w") as f:
        f.write(f"{len(pairs)}\n")
        for v, srcs in pairs.items():
            f.write(f"{v}\n{len(srcs)} " + " ".join(f"{u} {10.0 - i}" for i, u in enumerate(srcs)) + "\n")


def dtu_like_pairs(n, k=10):
    """The k nearest other views along the camera path, nearest first (DTU's pair.txt lists 10 per view)."""
    return {v: sorted((u for u in range(n) if u != v), key=lambda u: (abs(u - v), u))[:k] for v in range(n)}


def assert_same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a, b), what


def check_plan(datapath, scan, nviews, max_h, max_w, ndepths=192, interval_scale=1.06, inverse=False, fix_res=False):
    ds = eval_io.MVSDataset(datapath, [scan], "test", nviews, ndepths, interval_scale, inverse_depth=inverse,
                            max_h=max_h, max_w=max_w, fix_res=fix_res)
    plan = ScanPlan(datapath, scan, nviews, ndepths, interval_scale, inverse, max_h, max_w, fix_res)
    assert len(plan.samples) == len(ds)
    for i, p in enumerate(plan.samples):
        s = ds[i]
        assert p.filename == s["filename"]
        assert p.view_ids == [ds.metas[i][1]] + ds.metas[i][2][: nviews - 1]
        assert all(c[2] == tuple(s["imgs"].shape[-2:]) for c in p.chains), (p.chains, s["imgs"].shape)
        for c, vid in zip(p.chains, p.view_ids):
            assert c[0] == plan.image_size(vid) and c[1] == ds.policy.target(*c[0])
        assert_same(p.depth_values, s["depth_values"], "depth_values")
        assert sorted(p.proj_matrices) == sorted(s["proj_matrices"])
        for k in s["proj_matrices"]:
            assert_same(p.proj_matrices[k], s["proj_matrices"][k], k)
    return ds, plan


@pytest.mark.parametrize("scan,nviews,inverse", [("scanA", 3, False), ("scanA", 3, True), ("scanB", 5, False)])
def test_plan_equals_dataset_on_fixture(scan, nviews, inverse):
    ds, plan = check_plan(os.path.join(GOLDEN, "eval_scene"), scan, nviews, 1200, 1600, inverse=inverse)
    if scan == "scanB":   # the short source list is padded with the best source view
        assert any(len(set(p.view_ids)) < len(p.view_ids) for p in plan.samples)


def test_plan_resize_chain_fix_res_and_override(tmp_path):
    root = str(tmp_path)
    write_scene(root, "sR", [(150, 200)] * 4, depth_line="400.0 2.0 100 700.0")             # resize branch
    ds, plan = check_plan(root, "sR", 3, 96, 128)
    assert plan.samples[0].chains[0] == ((150, 200), (96, 128), (96, 128))
    # mixed orientations: portrait views are resized to the policy size, then again to the reference's size (chained)
    write_scene(root, "sM", [(150, 200), (200, 150), (150, 200), (200, 150)])
    for inverse in (False, True):
        ds, plan = check_plan(root, "sM", 4, 96, 128, inverse=inverse)
    assert ((200, 150), (96, 64), (96, 128)) in plan.samples[0].chains
    assert ((150, 200), (96, 128), (96, 64)) in plan.samples[1].chains
    # fix_res: the first image ever loaded fixes the size of every later sample (portrait references included)
    ds, plan = check_plan(root, "sM", 3, 96, 128, fix_res=True)
    assert all(p.size == (96, 128) for p in plan.samples)
    assert plan.samples[1].chains[0] == ((200, 150), (96, 64), (96, 128))
    # per-scene override of the policy size (save_depth_maps' scene_cfg) and a per-scene interval scale
    check_plan(root, "sR", 4, 64, 64, interval_scale={"sR": 0.8})
    check_plan(root, "sR", 2, 1200, 1600, ndepths=48)


def restated_ingest(u8, chain):
    """dmvs_image_ingest in NumPy fp32, the kernel's order: LUT, then per resize step (identity steps skipped) the row pass
    a*(1-fx) + b*fx for the two source rows, then the column pass r0*(1-fy) + r1*fy."""
    img = eval_io.u8_to_float_table()[u8]
    sizes = [chain[0]] + [s for a, s in zip(chain, chain[1:]) if s != a]
    for (h, w), (H, W) in zip(sizes, sizes[1:]):
        x0, x1, fx = eval_io.resize_taps(W, w)
        y0, y1, fy = eval_io.resize_taps(H, h)
        wx0, wy0 = np.float32(1.0) - fx, np.float32(1.0) - fy
        r0 = img[y0][:, x0] * wx0[None, :, None] + img[y0][:, x1] * fx[None, :, None]
        r1 = img[y1][:, x0] * wx0[None, :, None] + img[y1][:, x1] * fx[None, :, None]
        img = r0 * wy0[:, None, None] + r1 * fy[:, None, None]
    return np.ascontiguousarray(img.transpose(2, 0, 1))


def test_tables_restate_the_loader_images(tmp_path):
    from PIL import Image
    # the uint8 table is the loader's own expression, value by value
    u = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    assert_same(eval_io.u8_to_float_table()[u], np.array(u, dtype=np.float32) / 255.0, "lut")
    # resize_taps is what resize_linear applies
    a = np.random.default_rng(0).random((37, 53, 3)).astype(np.float32)
    assert_same(restated_ingest_float(a, (37, 53), (20, 31)), eval_io.resize_linear(a, 20, 31).transpose(2, 0, 1), "taps")
    root = str(tmp_path)
    write_scene(root, "sM", [(150, 200), (200, 150), (157, 211), (200, 150)])
    for max_hw, fix_res in (((96, 128), False), ((96, 128), True), ((1200, 1600), False), ((64, 64), False)):
        ds = eval_io.MVSDataset(root, ["sM"], "test", 4, 192, 1.06, max_h=max_hw[0], max_w=max_hw[1], fix_res=fix_res)
        plan = ScanPlan(root, "sM", 4, 192, 1.06, False, *max_hw, fix_res)
        for i, p in enumerate(plan.samples):
            imgs = ds[i]["imgs"]
            for k, (vid, chain) in enumerate(zip(p.view_ids, p.chains)):
                u8 = np.asarray(Image.open(plan.image_path(vid)))
                assert_same(restated_ingest(u8, chain), imgs[k], (max_hw, fix_res, i, k, chain))


def restated_ingest_float(a, src, dst):
    x0, x1, fx = eval_io.resize_taps(dst[1], src[1])
    y0, y1, fy = eval_io.resize_taps(dst[0], src[0])
    r0 = a[y0][:, x0] * (np.float32(1.0) - fx)[None, :, None] + a[y0][:, x1] * fx[None, :, None]
    r1 = a[y1][:, x0] * (np.float32(1.0) - fx)[None, :, None] + a[y1][:, x1] * fx[None, :, None]
    return (r0 * (np.float32(1.0) - fy)[:, None, None] + r1 * fy[:, None, None]).transpose(2, 0, 1)


class _Val:
    def __init__(self, key, nbytes):
        self.key, self.nbytes = key, nbytes


class _FakeEncoder:
    def __init__(self, nbytes=100):
        self.calls, self.nbytes = [], nbytes

    def __call__(self, keys):
        self.calls.append(list(keys))
        return [_Val(k, self.nbytes) for k in keys]


def _samples(n=49, nviews=5):
    pairs = dtu_like_pairs(n)
    return [[v] + pairs[v][: nviews - 1] for v in range(n)]


def test_cache_encodes_every_image_once_under_a_large_budget():
    samples = _samples()
    for lookahead in (0, 16):
        enc = _FakeEncoder()
        cache = FeatureCache(enc, max_bytes=10 ** 9)
        for i, keys in enumerate(samples):
            look = [k for ks in samples[i + 1:] for k in ks][:lookahead]
            vals = cache.fetch(keys, look)
            assert [v.key for v in vals] == keys
        distinct = {k for ks in samples for k in ks}
        assert cache.stats["encodes"] == len(distinct) == sum(len(c) for c in enc.calls)
        assert cache.stats["evictions"] == 0 and cache.stats["peak_bytes"] == 100 * len(distinct)
        assert cache.stats["hits"] + cache.stats["misses"] == sum(len(set(ks)) for ks in samples)
        if lookahead:   # batches are filled from the following samples
            assert max(len(c) for c in enc.calls) > 5 and len(enc.calls) < len(samples)


def test_cache_lru_under_a_small_budget():
    samples = _samples()
    enc = _FakeEncoder(nbytes=100)
    cache = FeatureCache(enc, max_bytes=350)          # three entries: less than one sample's five views
    seen_max = 0
    for keys in samples:
        vals = cache.fetch(keys)
        assert [v.key for v in vals] == keys           # values stay valid after eviction
        assert cache.bytes <= 350
        seen_max = max(seen_max, cache.bytes)
    assert cache.stats["peak_bytes"] == seen_max <= 350
    assert cache.stats["evictions"] == cache.stats["encodes"] - len(cache)
    assert cache.stats["encodes"] > len({k for ks in samples for k in ks})
    # least recently used goes first
    enc = _FakeEncoder(nbytes=100)
    cache = FeatureCache(enc, max_bytes=300)
    cache.fetch(["a", "b", "c"])
    cache.fetch(["a"])                                 # a is now the most recent
    cache.fetch(["d"])                                 # evicts b
    assert "b" not in cache and all(k in cache for k in "acd")
    assert cache.stats == dict(encodes=4, hits=1, misses=4, evictions=1, peak_bytes=300)
    cache.fetch(["b", "b"])                            # a duplicate key is one miss, one encode
    assert cache.stats["misses"] == 5 and cache.stats["encodes"] == 5 and "c" not in cache


def test_cache_key_includes_fingerprint_and_dtype():
    enc = _FakeEncoder()
    cache = FeatureCache(enc, max_bytes=10 ** 6)
    k = ("scan1", 3, ((1200, 1600), (864, 1152), (864, 1152)))
    cache.fetch([k + (111, "f32")])
    cache.fetch([k + (111, "f32")])
    cache.fetch([k + (222, "f32")])                    # other weights
    cache.fetch([k + (111, "f16")])                    # other feature dtype
    assert cache.stats["hits"] == 1 and cache.stats["misses"] == 3 and cache.stats["encodes"] == 3
