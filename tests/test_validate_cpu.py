"""CPU (-m "not gpu"): validation mode (N6) -- the restatement against the reference's recorded values, the DTU training-format
loader against the reference loader's recorded sample dicts, the ABI surface, the refusals and the averaging order."""
import ctypes
import hashlib
import json
import os
import re

import numpy as np
import pytest
import torch

import validate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GOLDEN_REL = ref.GOLDEN_REL   # 4 x the measured worst gap restatement vs reference (validate_ref.py)


def rel_gap(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


@pytest.fixture(scope="module")
def loss_golden(golden):
    return golden("validate_loss.npz")


@pytest.mark.parametrize("name", list(ref.CASES))
def test_restatement_matches_the_reference(loss_golden, name):
    case = ref.loss_case(name)
    assert ref.case_digest(case) == str(loss_golden[name + ".digest"]), "the seeded inputs are not the ones the reference saw"
    want = float(loss_golden[name + ".loss"])
    got = float(ref.mvs_loss_ref(case["inputs"], case["depth_gt"], case["mask"], case["dlossw"]))
    last = "stage{}".format(len(case["inputs"]))
    met = ref.metrics_ref(case["depth"], case["depth_gt"][last], case["mask"][last])
    print(f"{name}: reference {want!r} restatement {got!r} metrics {met.tolist()} reference {loss_golden[name + '.metrics'].tolist()}")
    if "empty" in name and "one" not in name:
        assert np.isnan(want) and np.isnan(got)
        assert np.array_equal(met, np.zeros(4, dtype=np.float32))
    else:
        assert rel_gap(got, want) <= GOLDEN_REL
    # the rates are ratios of exact counts: equal; the abs error differs by the summation (fp32 there, fp64 here)
    assert np.array_equal(met[1:], loss_golden[name + ".metrics"][1:])
    assert abs(float(met[0]) - float(loss_golden[name + ".metrics"][0])) <= GOLDEN_REL * abs(float(met[0]))


def test_measured_gap_is_the_recorded_one(loss_golden):
    assert float(loss_golden["gap.rel"].max()) <= ref.MEASURED_GAP_REL
    # the sizes the tests compare at keep every all-valid cell in the reference
    sizes = loss_golden["cells.sizes"]
    assert np.array_equal(sizes[:, 2], sizes[:, 3])
    used = {tuple(s) for v in ref.STAGE_SIZES.values() for s in v} | {(32, 40), (128, 160), (296, 400), (512, 640), (1184, 1600)}
    assert used <= {(int(h), int(w)) for h, w in sizes[:, :2]}


def test_nonfinite_values_under_the_mask_change_nothing():
    clean = ref.loss_case("s3_b2_nonfinite")
    poisoned = ref.loss_case("s3_b2_nonfinite")
    for k in clean["inputs"]:
        bad = clean["mask"][k] <= 0.5
        for t in (clean["inputs"][k]["depth_sub_plus"], clean["inputs"][k]["depth_sub_plus_refine"]):
            assert not torch.isfinite(t[bad[:, None].expand_as(t)]).all()
            t[bad[:, None].expand_as(t)] = 0.0
        clean["depth_gt"][k][bad] = 0.0
    a = ref.mvs_loss_ref(clean["inputs"], clean["depth_gt"], clean["mask"], clean["dlossw"])
    b = ref.mvs_loss_ref(poisoned["inputs"], poisoned["depth_gt"], poisoned["mask"], poisoned["dlossw"])
    assert torch.isfinite(a) and a.item() == b.item()


# ------------------------------------------------------------------------------------------ loader
@pytest.fixture(scope="module")
def val_scene(tmp_path_factory):
    from dmvsnet_amd import synth
    root = str(tmp_path_factory.mktemp("val_scene"))
    return root, synth.synth_val_scene(root, seed=0)


def test_loader_matches_the_reference_loader(golden, val_scene):
    from dmvsnet_amd.validate import DTUValDataset
    g = golden("validate_dataset.npz")
    root, info = val_scene
    nviews = int(g["nviews"])
    full = DTUValDataset(root, info["listfile"], "val", nviews)
    assert len(full) == info["views"] * 7                                   # 7 lights per view, as the reference
    ds = DTUValDataset(root, info["listfile"], "val", nviews, lights=info["lights"])
    assert len(ds) == info["views"] * info["lights"]
    for view, light in g["index"]:
        tag = f"v{view}_l{light}"
        s = ds[view * info["lights"] + light]
        assert full.metas[view * 7 + light] == ds.metas[view * info["lights"] + light]
        assert list(s) == ["imgs", "proj_matrices", "depth", "depth_values", "mask"]
        flat = {"imgs": s["imgs"], "depth_values": s["depth_values"]}
        for group in ("proj_matrices", "depth", "mask"):
            assert list(s[group]) == ["stage1", "stage2", "stage3"]
            for k, a in s[group].items():
                flat[f"{group}.{k}"] = a
        meta = json.loads(str(g[tag + ".meta"]))
        assert set(meta) == set(flat)
        for k, a in flat.items():
            a = np.ascontiguousarray(a)
            assert list(a.shape) == meta[k]["shape"] and str(a.dtype) == meta[k]["dtype"], k
            assert hashlib.sha256(a.tobytes()).hexdigest() == meta[k]["sha256"], (tag, k)
        assert np.array_equal(s["depth"]["stage1"], g[tag + ".depth.stage1"])
        assert np.array_equal(s["mask"]["stage1"], g[tag + ".mask.stage1"])
        assert np.array_equal(s["depth_values"], g[tag + ".depth_values"])
        assert np.array_equal(s["proj_matrices"]["stage1"], g[tag + ".proj_matrices.stage1"])
        # the scene exercises the mask: holes, a band through the crop, pixels exactly at the threshold
        m = s["mask"]["stage3"]
        assert 0.5 < m.mean() < 0.95 and s["depth"]["stage3"][m > 0.5].min() > 400


def test_loader_refuses_what_it_cannot_restate(val_scene):
    from dmvsnet_amd._lib import DmvsError
    from dmvsnet_amd.validate import DTUValDataset, nearest_resize
    a = np.arange(30, dtype=np.float32).reshape(5, 6)
    assert np.array_equal(nearest_resize(np.arange(32, dtype=np.float32).reshape(4, 8), 4, 2), [[0, 2, 4, 6], [16, 18, 20, 22]])
    with pytest.raises(DmvsError, match="integer ratio"):
        nearest_resize(a, 3, 2)            # 5 rows -> 2: ratio 2.5
    with pytest.raises(DmvsError, match="integer ratio"):
        nearest_resize(a, 4, 5)            # 6 columns -> 4
    root, info = val_scene
    with pytest.raises(DmvsError, match="training is out of scope"):
        DTUValDataset(root, info["listfile"], "train", 3)


# ------------------------------------------------------------------------------------------ ABI and refusals
def test_abi_surface():
    from dmvsnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "dmvs.h")).read()
    lib = _lib.load()
    for name in ("dmvs_dual_depth_loss", "dmvs_dual_depth_loss_workspace"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["dmvs_dual_depth_loss"][1]) == 17
    assert lib.dmvs_version() == _lib.ABI_VERSION == 140
    # the comment of the entry cites the reference lines it replaces
    doc = header[header.index("/* N6:"):header.index("long dmvs_dual_depth_loss_workspace")]
    assert "loss.py:5-80" in doc and "loss.py:106-159" in doc and "tools.py:159-201" in doc
    # one fp64 row of 24 per workgroup (63 columns x 32 rows); bad sizes are refused without touching a device
    ws = lib.dmvs_dual_depth_loss_workspace
    assert ws(1, 512, 640) == 16 * 11 * 24 and ws(2, 128, 160) == 2 * 4 * 3 * 24 and ws(1, 2, 2) == 24
    assert ws(1, 1, 640) == _lib.EINVAL and ws(1, 512, 1) == _lib.EINVAL and ws(0, 512, 640) == _lib.EINVAL
    one = ctypes.c_void_p(64)   # a non-null pointer that is never followed: the argument checks come first
    call = lib.dmvs_dual_depth_loss
    assert call(one, one, one, one, None, 1, 1, 8, 1.0, None, one, one, None, None, None, None, None) == _lib.EINVAL   # h < 2
    assert call(one, one, one, one, None, 1, 8, 1, 1.0, None, one, one, None, None, None, None, None) == _lib.EINVAL   # w < 2
    assert call(one, one, None, one, None, 1, 8, 8, 1.0, None, one, one, None, None, None, None, None) == _lib.EINVAL  # gt
    assert call(one, None, one, one, None, 1, 8, 8, 1.0, None, one, one, None, None, None, None, None) == _lib.EINVAL  # refine
    assert call(one, one, one, one, None, 1, 8, 8, 1.0, None, None, one, None, None, None, None, None) == _lib.EINVAL  # workspace
    assert call(one, one, one, one, None, 1, 8, 8, 1.0, None, one, None, None, None, None, None, None) == _lib.EINVAL  # no output
    assert call(None, None, one, one, one, 1, 8, 8, 1.0, None, one, None, None, None, None, one, None) == _lib.EINVAL  # thresholds


def test_refusals():
    from dmvsnet_amd import MVSNet, mvs_loss, validate
    from dmvsnet_amd._lib import DmvsError
    case = ref.loss_case("s1_b1_default_n03")
    for mode in ("classification", "gfocal", "unification"):
        with pytest.raises(NotImplementedError, match=mode):
            mvs_loss(case["inputs"], case["depth_gt"], case["mask"], mode)
    with pytest.raises(DmvsError, match="CPU"):
        mvs_loss(case["inputs"], case["depth_gt"], case["mask"], "regression")
    gt, mask = case["depth_gt"]["stage1"], case["mask"]["stage1"]
    with pytest.raises(DmvsError, match="CPU"):
        validate.AbsDepthError_metrics(case["depth"], gt, mask > 0.5)
    with pytest.raises(DmvsError, match="CPU"):
        validate.Thres_metrics(case["depth"], gt, mask > 0.5, 2)
    with pytest.raises(DmvsError, match="HIP device"):
        validate.run_validate(None, "/nonexistent", "/nonexistent", device="cpu")
    with pytest.raises(NotImplementedError):   # not training
        MVSNet([8], [4], verbose=False).train(True)


def test_average_is_the_reference_meters():
    """DictAverageMeter (tools.py:18-37): Python floats, added in batch order, divided by the count -- not a mean in fp32,
    not a pairwise sum."""
    from dmvsnet_amd.validate import SCALARS, average_scalars
    rows = [[float(np.float32(v)) for v in r] for r in
            ([0.1, 1e17, 3.0, 0.25, 0.5], [0.2, 1.0, 1e-3, 0.5, 0.25], [0.7, -1e17, 2.0, 0.125, 1.0], [1e-9, 3.0, 5.0, 0.0, 0.0])]
    got = average_scalars(rows)
    assert list(got) == list(SCALARS) == ["loss", "abs_depth_error", "thres2mm_error", "thres4mm_error", "thres8mm_error"]
    for k, name in enumerate(SCALARS):
        acc = rows[0][k]
        for r in rows[1:]:
            acc += r[k]
        assert got[name] == acc / len(rows)
    assert got == ref.average_meter(rows)
    assert got["abs_depth_error"] != float(np.mean([r[1] for r in rows][::-1]))   # the order matters on this data
    assert average_scalars(rows[:1]) == dict(zip(SCALARS, rows[0]))
