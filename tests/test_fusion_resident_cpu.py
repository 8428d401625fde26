"""CPU (-m "not gpu"): the host side of scan-level fusion (fusion.ScanFusion, scan.save_depth_maps_cached's resident path).

* FusionSchedule: every reference view is fused once, right after the last of its maps arrives; every depth map is released
  once, right after the last view that reads it; a view that never arrives keeps the scene from completing.
* The inputs the resident path hands over equal what fuse_scene reads back from the files: cams (write_cam's text of fp32
  parses back to the same bits) and colours (``float32(u8) / 255 * 255 -> uint8`` is the identity).
* The zlib PNG writer's files decode to their input.
* The new kernels use no scratch and spill nothing (scripts/kernel_regs.py over the built library's code object notes).
"""
import io
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from dmvsnet_amd import eval_io
from dmvsnet_amd._lib import DmvsError
from dmvsnet_amd.fusion import FusionSchedule, png_gray8, read_camera_parameters
from dmvsnet_amd.scan import as_written_cam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dtu_like(n, k=10):
    return [(v, sorted((u for u in range(n) if u != v), key=lambda u: (abs(u - v), u))[:k]) for v in range(n)]


def ring(n, k=2):
    return [(v, [(v + i) % n for i in range(1, k + 1)]) for v in range(n)]


def sources_last(n, k=3):
    """The first views wait for the last ones (each view's sources are the k views at the end of the list)."""
    return [(v, [u for u in range(n - 1, -1, -1) if u != v][:k]) for v in range(n)]


def _simulate(pairs, order):
    sch = FusionSchedule(pairs)
    fused, released, arrived = [], {}, set()
    srcs = dict(pairs)
    for step, v in enumerate(order):
        arrived.add(v)
        for r in sch.arrive(v):
            assert r not in fused, r
            assert r in arrived and all(s in arrived for s in srcs[r]), r
            # fused right at the arrival of its last map
            assert v == r or v in srcs[r]
            fused.append(r)
            for u in sch.fuse(r):
                assert u not in released, u
                released[u] = len(fused)
    return sch, fused, released


@pytest.mark.parametrize("pairs", [dtu_like(13), dtu_like(6, 3), ring(9), ring(5, 4), sources_last(8)],
                         ids=["dtu13", "dtu6", "ring9", "ring5", "sources_last"])
def test_schedule_fuses_once_and_releases_after_last_use(pairs):
    rng = np.random.default_rng(0)
    views = sorted({r for r, _ in pairs} | {s for _, ss in pairs for s in ss})
    for trial in range(6):
        order = list(views) if trial == 0 else list(views[::-1]) if trial == 1 else list(rng.permutation(views))
        sch, fused, released = _simulate(pairs, order)
        assert sorted(fused) == sorted(r for r, _ in pairs) and sch.done() and sch.missing() == []
        # every depth map released exactly once, at the fusion of the last view that reads it
        for v in views:
            users = [i + 1 for i, r in enumerate(fused) if r == v or v in dict(pairs)[r]]
            assert released[v] == max(users), (v, released[v], users)
        # every reference fused no earlier than needed: when its last map arrived
        pos = {v: i for i, v in enumerate(order)}
        srcs = dict(pairs)
        last = {r: max(pos[u] for u in [r] + srcs[r]) for r, _ in pairs}
        assert sorted(fused, key=lambda r: (last[r], [p[0] for p in pairs].index(r))) == fused


def test_schedule_missing_view_and_refusals():
    pairs = [(0, [1, 2]), (1, [0, 7]), (2, [0, 1])]     # view 7 is a source that never gets a map
    sch = FusionSchedule(pairs)
    for v in (0, 1, 2):
        for r in sch.arrive(v):
            sch.fuse(r)
    assert not sch.done() and sch.missing() == [7]
    with pytest.raises(DmvsError):
        sch.arrive(0)            # twice
    with pytest.raises(DmvsError):
        sch.arrive(42)           # not in the pair list
    with pytest.raises(DmvsError):
        FusionSchedule([(0, [1]), (0, [2])])


def test_write_cam_text_round_trips_fp32(tmp_path):
    rng = np.random.default_rng(1)
    for trial in range(20):
        cam = np.zeros((2, 4, 4), np.float32)
        scale = 10.0 ** rng.integers(-6, 6)
        cam[0] = (rng.standard_normal((4, 4)) * scale).astype(np.float32)
        cam[1, :3, :3] = (rng.random((3, 3)) * 3000).astype(np.float32)
        cam[1, 3] = rng.random(4).astype(np.float32) * 1000
        K, E = as_written_cam(cam)
        path = str(tmp_path / "c.txt")
        eval_io.write_cam(path, cam)
        Kf, Ef = read_camera_parameters(path)
        assert K.dtype == E.dtype == np.float32
        assert K.tobytes() == Kf.tobytes() and E.tobytes() == Ef.tobytes()
        # and str() of fp32 round-trips exactly, so the resident cams are the step-1 cams themselves
        assert K.tobytes() == cam[1, :3, :3].tobytes() and E.tobytes() == cam[0].tobytes()


def test_colour_identity():
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal((u.astype(np.float32) / 255.0 * 255).astype(np.uint8), u)
    img = np.random.default_rng(2).integers(0, 256, (9, 11, 3), dtype=np.uint8)
    f = np.array(img, dtype=np.float32) / 255.0      # fuse_scene's decode
    assert np.array_equal((f * 255).astype(np.uint8), img)


@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (37, 53), (96, 128)])
def test_png_writer_decodes_to_its_input(hw):
    from PIL import Image
    rng = np.random.default_rng(hw[0] * 1000 + hw[1])
    for m in (np.zeros(hw, np.uint8), np.full(hw, 255, np.uint8), (rng.random(hw) < 0.3).astype(np.uint8) * 255,
              rng.integers(0, 256, hw, dtype=np.uint8)):
        got = np.array(Image.open(io.BytesIO(png_gray8(m))))
        assert got.dtype == np.uint8 and got.shape == m.shape and np.array_equal(got, m)
    with pytest.raises(ValueError):
        png_gray8(np.zeros((2, 3, 3), np.uint8))


def test_fused_kernels_use_no_scratch_and_do_not_spill():
    lib = os.path.join(ROOT, "dmvsnet_amd", "csrc", "libdmvs_hip.so")
    bindir = "/opt/rocm/lib/llvm/bin"
    objdump = os.path.join(bindir, "llvm-objdump") if os.path.exists(os.path.join(bindir, "llvm-objdump")) else shutil.which("llvm-objdump")
    readelf = os.path.join(bindir, "llvm-readelf") if os.path.exists(os.path.join(bindir, "llvm-readelf")) else shutil.which("llvm-readelf")
    if not os.path.exists(lib) or not objdump or not readelf:
        pytest.skip("needs the built library and llvm-objdump / llvm-readelf")
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib, os.path.join(tmp, "lib.so"))
        subprocess.run([objdump, "--offloading", "lib.so"], cwd=tmp, check=True, capture_output=True)
        for f in sorted(os.listdir(tmp)):
            if "amdgcn" not in f:
                continue
            notes = subprocess.run([readelf, "--notes", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
            out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "kernel_regs.py")], input=notes,
                                 check=True, capture_output=True, text=True).stdout
            rows += [line for line in out.splitlines() if line.startswith(("fuse_view_kernel", "fuse_scan_kernel", "fuse_emit_kernel"))]
    assert len(rows) == 4, rows       # view <static>, view <dynamic>, scan, emit
    for line in rows:
        f = line.split()
        assert f[f.index("spill") + 1] == "0" and f[f.index("scratch") + 1] == "0", line
