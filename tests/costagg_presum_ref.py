"""What the two test files of K1b's pre-summed scatter share (``warp_corr_bwd_src_presum_kernel`` of csrc/warp_corr_bwd_presum.h;
test_costagg_presum_cpu.py, test_costagg_presum_gpu.py): the literal tables the new decomposition needs, built on the helpers of
tests/warp_corr_ref.py / warp_corr_grad_ref.py, and a CPU restatement of the kernel's path decision.  A plain module: no tests, no
fixtures, no pytest settings; no product code runs here.

  SEAMS     (D, H, W) = (9, 9, 130), C = 8 and 32, the identity and the offset (-0.5, 0.5): 130 columns are two full 64-column tiles
            and a 2-pixel one, 9 rows two tile rows and one row, 9 planes a full 8-plane chunk and a 1-plane one.  The boxes of
            neighbouring workgroups overlap by a column and a row, those of the two chunks coincide: several workgroups flush into the
            same texels, and the partial tiles hold lanes outside the map at the barriers.  (W - 1) / 2 = 64.5 is no power of two, so
            the reference's coordinate round trip is inexact here: against float64 the GPU file asserts the mean bound on every
            tensor and the plain max bound on the identity cases' dSrc, prints the max elsewhere (the WINDOWS rule) and holds every
            max to the fp32 op-order restatement within the any-order allowance (test_costagg_presum_gpu.py::test_seams_atomic).
  CAPACITY  two cases on a map of W = cap + 1 columns on which ONE tile column owns a box of exactly ``cap`` and of ``cap + 1`` texels:
            sy = 0 and oy = H - 1 send every sample to the last row (y1 = H is outside: a one-row box), ix = sx x + ox with
            sx = cap / 64 + 1 makes tile 0 span more columns than the map has, so the box ends at the map's last column; it starts at
            column ox = 1 (``cap`` texels) or 0 (``cap + 1``).  Every other tile column samples beyond the map: empty.  (W - 1) / 2 is a
            power of two, so the reference's normalise / un-normalise round trip is exact and the coordinates are integers in fp32 too.
            15 samples per destination column: criterion CONTENTION's (the any-order allowance).

``predict`` restates the decision: per workgroup (64 x 4 tile, chunk of ``dch`` planes) the bounding box of every in-image tap -- the
taps of ``warp_corr_grad_ref._taps(..., ref_order=True)`` in fp32, which on exact-coordinate tables are the kernel's -- is empty, at
most ``cap`` texels (windowed) or more (direct).  A tap is in the image on its range tests alone, whatever its weight."""
import torch

import warp_corr_grad_ref as GR
import warp_corr_ref as R

TX, TY = 64, 4                     # the scatter's tile: one wave per row
SEAM_SHAPE = (9, 9, 130)           # (D, H, W)
SEAM_OFFSETS = ((0, 0), (-0.5, 0.5))
CAP_SHAPE_DH = (3, 5)              # (D, H) of the capacity maps: one chunk, a full tile row and a one-row one


def seam_name(C, ox, oy):
    return f"seam-c{C}-{ox:g}_{oy:g}"


def _with_gsim(case):
    case["gsim"] = GR.gsim_of(case["name"], *case["depth"].shape)
    return case


def seam_cases():
    """name -> case.  The table key is AFFINE's (unit scale, literal projection); the criterion is the one the module's text names."""
    out = {}
    for C in (8, 32):
        for ox, oy in SEAM_OFFSETS:
            name = seam_name(C, ox, oy)
            out[name] = _with_gsim(GR._literal_case("AFFINE", name, C, SEAM_SHAPE, R.affine_p12(1.0, ox, 1.0, oy)))
    return out


def capacity_cases(cap, C=8):
    """(at, over): tile column 0 owns a one-row box of exactly ``cap`` / ``cap + 1`` texels, every other tile column none."""
    assert cap % TX == 0 and cap >= 2 * TX
    D, H = CAP_SHAPE_DH
    sx, W = cap // TX + 1, cap + 1   # the samples reach column W - 1 or beyond (the CPU file asserts the boxes)
    out = []
    for side, ox in (("at", 1.0), ("over", 0.0)):
        name = f"capacity-c{C}-{side}"
        out.append(_with_gsim(GR._literal_case("CONTENTION", name, C, (D, H, W), R.affine_p12(float(sx), ox, 0.0, float(H - 1)))))
    return tuple(out)


def boxes(p12_v, depth, dch):
    """{(tile x, tile y, chunk): (x0, x1, y0, y1) or None} of one view: the bounding box of the in-image taps of the workgroup's
    samples.  fp32, the reference's op order."""
    D, H, W = depth.shape
    taps = GR._taps(p12_v.to(R.F32), depth.to(R.F32), None, True)
    inside = torch.stack([t[1].expand(D, H, W) for t in taps])                  # [4,D,H,W]
    idx = torch.stack([t[2].view(D, H, W) for t in taps])
    tx, ty = idx % W, idx // W
    out = {}
    for c in range((D + dch - 1) // dch):
        for by in range((H + TY - 1) // TY):
            for bx in range((W + TX - 1) // TX):
                sl = (slice(None), slice(c * dch, (c + 1) * dch), slice(by * TY, (by + 1) * TY), slice(bx * TX, (bx + 1) * TX))
                m = inside[sl]
                if not m.any():
                    out[(bx, by, c)] = None
                    continue
                xs, ys = tx[sl][m], ty[sl][m]
                out[(bx, by, c)] = (int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max()))
    return out


def texels(box):
    return 0 if box is None else (box[1] - box[0] + 1) * (box[3] - box[2] + 1)


def path_of(box, cap):
    return 2 if box is None else 0 if texels(box) <= cap else 1


def predict(p12, depth, C, cap, variant=0, views=None):
    """[windowed, direct, empty] workgroups of a launch that asks for ``views`` (None: all): one workgroup per (wanted view, group of
    two channel quads, chunk, tile)."""
    dch = 4 if variant & 1 else 8
    counts = [0, 0, 0]
    for v in range(p12.shape[0]) if views is None else views:
        for box in boxes(p12[v], depth, dch).values():
            counts[path_of(box, cap)] += C // 8
    return counts
