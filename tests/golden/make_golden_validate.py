#!/usr/bin/env python3
"""Golden vectors for validation mode (row N6) by RUNNING THE REFERENCE's loss.py, tools.py and datasets/dtu_yao.py
(build container only; /root/reference is never copied).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_validate.py

loss.py needs torch and numpy only and is imported as it is.  tools.py imports torchvision (for TensorBoard image grids) and
dtu_yao.py imports torchvision and cv2, none of which this image has and none of which is on the arithmetic path pinned
here except ``cv2.resize``: the generator registers placeholder modules -- an empty ``torchvision`` and a ``cv2`` whose
``resize`` handles ``INTER_NEAREST`` at EXACT INTEGER shrink ratios by slicing (source index floor(dst * ratio), OpenCV's
published nearest rule) and asserts everything else away.  That rule is restated, not executed: the unpinned detail of the
loader.

Writes
  validate_loss.npz     for every case of tests/validate_ref.py::CASES (1 and 3 stages, B = 1 and 2, default and
                        (0.5, 1, 2) stage weights, 0.3 mm and 3 mm noise, masks with holes, an empty mask, one empty image
                        of two, NaN / inf under the mask): the SHA-256 of the seeded inputs (the tests regenerate them with
                        the same generator), the reference's ``mvs_loss`` value, its ``AbsDepthError_metrics`` and three
                        ``Thres_metrics``; the restatement's value and the measured gap; and per size used anywhere in the
                        tests the number of all-valid 2x2 cells against the number the reference's
                        ``grid_sample(mask) >= 1`` keeps (asserted equal: the tests use only such sizes)
  validate_dataset.npz  the reference loader on dmvsnet_amd.synth.synth_val_scene (written to a temp dir): the stage-1 depth
                        and mask of every sample in full, shape / dtype / SHA-256 of every other array of the sample dict
"""
import contextlib
import hashlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")

from dmvsnet_amd import synth  # noqa: E402
import validate_ref as vr  # noqa: E402


def _cv2_resize(img, dsize, interpolation=None):
    assert interpolation == sys.modules["cv2"].INTER_NEAREST, interpolation
    new_w, new_h = dsize
    h, w = img.shape[:2]
    assert h % new_h == 0 and w % new_w == 0, (img.shape, dsize)
    return np.ascontiguousarray(img[::h // new_h, ::w // new_w])


cv2 = types.ModuleType("cv2")
cv2.INTER_NEAREST, cv2.INTER_LINEAR, cv2.resize = 0, 1, _cv2_resize
sys.modules["cv2"] = cv2
for name in ("torchvision", "torchvision.utils", "torchvision.transforms"):
    sys.modules[name] = types.ModuleType(name)
sys.modules["torchvision"].utils = sys.modules["torchvision.utils"]
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
# datasets/__init__.py pulls in every loader: expose the package directory without running it
sys.modules["datasets"] = types.ModuleType("datasets")
sys.modules["datasets"].__path__ = ["/root/reference/datasets"]

import loss as ref_loss  # noqa: E402
import tools as ref_tools  # noqa: E402
with contextlib.redirect_stdout(io.StringIO()):
    from datasets import dtu_yao as ref_dtu  # noqa: E402

# every (h, w) at which a validate test compares with the reference or runs the kernel on seeded planes.  (The run_validate
# tests also meet 256 x 320, the middle stage of a 512 x 640 sample; they compare with the restatement, which counts the all-valid
# cells at any size.  There the reference drops one all-valid cell: recorded below, not asserted.)
TEST_SIZES = [(32, 40), (96, 128), (128, 160), (296, 400), (512, 640), (1184, 1600)]
DROPPING_SIZES = [(64, 80), (256, 320)]


def reference_cells(h, w, valid=None):
    """(all-valid cells, cells the reference keeps) on a full mask (or ``valid`` [B,h,w] bool): Monte_Carlo_sampling_loss's grid and its
    ``grid_sample(mask) >= 1`` (loss.py:111-130), restated call for call."""
    y, x = torch.meshgrid([torch.arange(0, h - 1, dtype=torch.float32), torch.arange(0, w - 1, dtype=torch.float32)], indexing="ij")
    y, x = y.contiguous().unsqueeze(0) + 0.5, x.contiguous().unsqueeze(0) + 0.5
    x = x / ((w - 1) / 2) - 1
    y = y / ((h - 1) / 2) - 1
    if valid is None:
        valid = torch.ones(1, h, w, dtype=torch.bool)
    B = valid.shape[0]
    grid = torch.stack((x.repeat(B, 1, 1), y.repeat(B, 1, 1)), dim=3)
    m = F.grid_sample(valid.float().unsqueeze(1), grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    cells = int((valid[:, :-1, :-1] & valid[:, :-1, 1:] & valid[:, 1:, :-1] & valid[:, 1:, 1:]).sum())
    return cells, int((m >= 1.0).sum())


def loss_goldens():
    out, gaps = {}, {}
    for name in vr.CASES:
        case = vr.loss_case(name)
        inputs = {k: dict(v, prob_volume=None, depth_values=None, interval=None) for k, v in case["inputs"].items()}
        kw = {} if case["dlossw"] is None else {"dlossw": list(case["dlossw"])}
        with torch.no_grad():
            ref = ref_loss.mvs_loss(inputs, case["depth_gt"], case["mask"], "regression", **kw)
            last = "stage{}".format(len(inputs))
            gt, mask = case["depth_gt"][last], case["mask"][last] > 0.5
            met = [ref_tools.AbsDepthError_metrics(case["depth"], gt, mask)] + \
                  [ref_tools.Thres_metrics(case["depth"], gt, mask, t) for t in (2, 4, 8)]
        mine = vr.mvs_loss_ref(case["inputs"], case["depth_gt"], case["mask"], case["dlossw"])
        out[name + ".digest"] = np.array(vr.case_digest(case))
        out[name + ".loss"] = np.array(ref.item(), dtype=np.float32)
        out[name + ".metrics"] = np.array([m.item() for m in met], dtype=np.float32)
        out[name + ".restatement"] = np.array(mine.item(), dtype=np.float32)
        if np.isnan(ref.item()):
            assert np.isnan(mine.item()), name
            gaps[name] = 0.0
        else:
            gaps[name] = abs(float(mine) - float(ref)) / abs(float(ref))
        # the masks of the case lose no all-valid cell in the reference either
        for k, m in case["mask"].items():
            cells, kept = reference_cells(m.shape[1], m.shape[2], m > 0.5)
            assert cells == kept, (name, k, cells, kept)
        print(f"{name:22s} reference {ref.item():.9g}  restatement {mine.item():.9g}  rel gap {gaps[name]:.3e}  metrics "
              + " ".join(f"{m.item():.7g}" for m in met))
    out["gap.names"] = np.array(list(gaps))
    out["gap.rel"] = np.array([gaps[k] for k in gaps], dtype=np.float64)
    sizes = []
    for h, w in TEST_SIZES:
        full, kept = reference_cells(h, w)
        assert full == kept, (h, w, full, kept)   # no all-valid cell is dropped by grid_sample(mask) >= 1 at this size
        sizes.append((h, w, full, kept))
    out["cells.sizes"] = np.array(sizes, dtype=np.int64)
    out["cells.dropping_sizes"] = np.array([(h, w) + reference_cells(h, w) for h, w in DROPPING_SIZES], dtype=np.int64)
    print("sizes where the reference drops all-valid cells (h, w, all-valid, kept):", out["cells.dropping_sizes"].tolist())
    print("worst relative gap restatement vs reference:", max(gaps.values()))
    np.savez_compressed(os.path.join(HERE, "validate_loss.npz"), **out)


def dataset_goldens():
    out = {}
    with tempfile.TemporaryDirectory() as root:
        info = synth.synth_val_scene(root, seed=0)
        nviews = 3
        with contextlib.redirect_stdout(io.StringIO()):
            ds = ref_dtu.MVSDataset(root, info["listfile"], "val", nviews, None, 192, 1.06)
        assert len(ds) == info["views"] * 7
        index = []
        for view in range(info["views"]):
            for light in range(info["lights"]):
                idx = view * 7 + light          # metas: views x 7 lights (dtu_yao.py:46-51); the scene has `lights` of them
                s = ds[idx]
                tag = f"v{view}_l{light}"
                flat = {"imgs": s["imgs"], "depth_values": s["depth_values"]}
                for group in ("proj_matrices", "depth", "mask"):
                    for k, a in s[group].items():
                        flat[f"{group}.{k}"] = a
                meta = {}
                for k, a in flat.items():
                    a = np.ascontiguousarray(a)
                    meta[k] = {"shape": list(a.shape), "dtype": str(a.dtype), "sha256": hashlib.sha256(a.tobytes()).hexdigest()}
                out[tag + ".meta"] = np.array(json.dumps(meta))
                out[tag + ".depth.stage1"] = s["depth"]["stage1"]
                out[tag + ".mask.stage1"] = s["mask"]["stage1"]
                out[tag + ".depth_values"] = s["depth_values"]
                out[tag + ".proj_matrices.stage1"] = s["proj_matrices"]["stage1"]
                index.append((view, light))
        out["index"] = np.array(index, dtype=np.int64)
        out["nviews"] = np.array(nviews)
    np.savez_compressed(os.path.join(HERE, "validate_dataset.npz"), **out)


if __name__ == "__main__":
    loss_goldens()
    dataset_goldens()
    for f in ("validate_loss.npz", "validate_dataset.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")
