"""DTU point-cloud evaluation on the device: accuracy / completeness of a fused cloud (kernels: csrc/cloud_eval.h, "N5").

The counterpart of the reference's MATLAB scripts under scripts/evaluation_dtu (BaseEvalMain_web.m, PointCompareMain.m,
reducePts_haa.m, MaxDistCP.m, ComputeStat_web.m):

* ``reduce_points``  -- the 0.2 mm thinning: visit the points in a random order, a point that is still alive removes every
  point within ``dst`` of it.  That is the lexicographically first maximal independent set of the "closer than dst" graph
  under the visit order, computed here by a fixed-point iteration with the same result (one kernel launch per round).
  MATLAB's ``randperm`` stream cannot be reproduced: the order is an input (a seeded permutation by default), so the result
  is one draw from the same distribution as MATLAB's, not MATLAB's own draw.
* ``max_dist_cp``    -- ``min(d_nn, max_dist)`` for from-points inside the block grid of MaxDistCP.m, ``max_dist`` outside it.
  The block-by-block form can return values above ``max_dist`` (a neighbour in the far corner of the 27-block
  neighbourhood); everything downstream keeps only distances below 20, so those values are never looked at and are not
  reproduced.
* ``point_compare`` / ``scan_stats`` / ``evaluate_dtu`` -- the two MATLAB drivers.

All distance arithmetic is float64 on float32 coordinates.  There is no CPU fallback: host arrays are uploaded, a missing
device raises ``DmvsError``.  No real ``ObsMask*.mat`` / ``stl*_total.ply`` has been read by this code (the dataset is not
available to the project); the loaders are tested on files written by the tests.
"""
from __future__ import annotations

import ctypes
import json
import math
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .eval_io import ply_path

__all__ = ["reduce_points", "max_dist_cp", "point_compare", "scan_stats", "evaluate_dtu", "read_ply_xyz", "load_obs_mask",
           "load_plane", "total_stat_text", "DTU_TEST_SETS"]

# UsedSets of BaseEvalMain_web.m / ComputeStat_web.m
DTU_TEST_SETS = (1, 4, 9, 10, 11, 12, 13, 15, 23, 24, 29, 32, 33, 34, 48, 49, 62, 75, 77, 110, 114, 118)

MAX_AXIS_CELLS = 1 << 21     # csrc/cloud_eval.h CLOUD_MAX_AXIS
_NO_CELL = (1 << 63) - 1
_SLACK = 1.0 + 1e-6          # thinning cell = dst * _SLACK: neighbours closer than dst always sit in adjacent cells
NN_CELL0 = 0.5               # mm, finest search grid; NN_GROW x coarser per level (0.5 / 4 / 32 mm reach 60 mm)
NN_GROW = 8.0
NN_RINGS = 4                 # rings per pass: at most 9^3 cells per query and level
MAX_ROUNDS = 4096


def _device(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.DmvsError("cloud evaluation kernels need a HIP device (no CPU fallback)")
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _cloud(a, device, what) -> torch.Tensor:
    """[N,3] float32 contiguous on the device (host input is uploaded)."""
    t = torch.as_tensor(a)
    if t.dim() != 2 or t.shape[1] != 3:
        raise _lib.DmvsError(f"{what}: expected an [N,3] cloud, got {tuple(t.shape)}")
    if t.shape[0] >= 2 ** 31 - 256:
        raise _lib.DmvsError(f"{what}: {t.shape[0]} points; the kernels index with 32 bits")
    return t.to(device=device, dtype=torch.float32).contiguous()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _d3(v):
    return (ctypes.c_double * len(v))(*[float(x) for x in v])


def _i3(v):
    return (ctypes.c_int * 3)(*[int(x) for x in v])


class _Clock:
    """Wall time per phase between device synchronisations, into info["seconds"]; off (no synchronisation) unless asked for."""

    def __init__(self, dev, info):
        self.on = info is not None and bool(info.get("timing"))
        self.dev, self.t = dev, {}
        if self.on:
            import time
            self.now = time.perf_counter
            torch.cuda.synchronize(dev)
            self.last = self.now()

    def lap(self, name):
        if self.on:
            torch.cuda.synchronize(self.dev)
            t = self.now()
            self.t[name] = self.t.get(name, 0.0) + t - self.last
            self.last = t


def check_grid(dims) -> None:
    if any(int(d) < 1 or int(d) > MAX_AXIS_CELLS for d in dims):
        raise _lib.DmvsError(f"grid of {tuple(int(d) for d in dims)} cells: an axis needs more than 2^21 cells (64-bit key)")


class _Grid:
    """A cloud sorted by the cell keys of one uniform grid: the points inside it, their permutation, the occupied cells."""

    def __init__(self, xyz: torch.Tensor, origin, cell: float, dims, need_inverse=False):
        check_grid(dims)
        self.origin, self.cell, self.dims = [float(o) for o in origin], float(cell), [int(d) for d in dims]
        dev = xyz.device
        n = xyz.shape[0]
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        _lib.check(_lib.load().dmvs_cloud_cell_keys(_ptr(xyz), n, _d3(self.origin), self.cell, _i3(self.dims), _ptr(keys),
                                                    _stream(dev)), "dmvs_cloud_cell_keys")
        skeys, perm = torch.sort(keys)
        n_in = int(torch.searchsorted(skeys, torch.tensor([_NO_CELL], dtype=torch.int64, device=dev)).item())
        self.perm = perm[:n_in]                      # sorted position -> index into xyz
        self.xyz = xyz[self.perm].contiguous()
        self.n = n_in
        if n_in:
            out = torch.unique_consecutive(skeys[:n_in], return_inverse=need_inverse, return_counts=True)
            self.ukeys, counts = out[0].contiguous(), out[-1]
            self.cell_of = out[1].to(torch.int32).contiguous() if need_inverse else None
            self.ustart = torch.zeros(self.ukeys.numel() + 1, dtype=torch.int32, device=dev)
            self.ustart[1:] = torch.cumsum(counts, 0).to(torch.int32)
            self.M = self.ukeys.numel()
        else:
            self.ukeys = self.ustart = self.cell_of = None
            self.M = 0


def reduce_points(xyz, dst: float = 0.2, order=None, seed: int = 0, info: Optional[dict] = None, device=None) -> torch.Tensor:
    """reducePts_haa(pts, dst): bool mask [N] (device) of the points that survive the thinning.

    ``order``: the visit order, a permutation of 0..N-1 (``order[k]`` is the k-th point visited); default: a permutation drawn
    on the host from ``numpy.random.Generator(PCG64(seed))``, so that a run is reproducible anywhere.  ``info`` (a dict)
    receives ``rounds`` (kernel sweeps until nothing was undecided), ``cells`` and ``kept``."""
    dev = _device(device)
    pts = _cloud(xyz, dev, "reduce_points")
    n = pts.shape[0]
    if n == 0:
        if info is not None:
            info.update(rounds=0, cells=0, kept=0)
        return torch.zeros(0, dtype=torch.bool, device=dev)
    if not bool(torch.isfinite(pts).all()):
        raise _lib.DmvsError("reduce_points: the cloud holds non-finite coordinates")
    if not dst >= 0:
        raise _lib.DmvsError(f"reduce_points: dst = {dst}")
    if order is None:
        order = np.random.Generator(np.random.PCG64(seed)).permutation(n)
    order = torch.as_tensor(order).to(device=dev, dtype=torch.int64).reshape(-1)
    if order.numel() != n:
        raise _lib.DmvsError(f"reduce_points: order has {order.numel()} entries for {n} points")
    prio0 = torch.full((n,), -1, dtype=torch.int32, device=dev)
    prio0[order] = torch.arange(n, dtype=torch.int32, device=dev)
    if bool((prio0 < 0).any()):
        raise _lib.DmvsError("reduce_points: order is not a permutation of 0..N-1")
    clock = _Clock(dev, info)
    lo = pts.amin(0).double().cpu().numpy()
    hi = pts.amax(0).double().cpu().numpy()
    cell = max(float(dst), 1e-30) * _SLACK
    dims = np.floor((hi - lo) / cell).astype(np.int64) + 2
    g = _Grid(pts, lo, cell, dims, need_inverse=True)
    assert g.n == n
    lib = _lib.load()
    st = _stream(dev)
    prio = prio0[g.perm].contiguous()
    runs = torch.empty((g.M, 9, 2), dtype=torch.int32, device=dev)
    _lib.check(lib.dmvs_cloud_cell_runs(_ptr(g.ukeys), _ptr(g.ustart), g.M, _i3(g.dims), _ptr(runs), st), "dmvs_cloud_cell_runs")
    state = torch.zeros(n, dtype=torch.uint8, device=dev)
    remaining = torch.zeros(1, dtype=torch.int32, device=dev)
    todo, n_todo, rounds, undecided = None, n, 0, []
    clock.lap("sort_and_cell_tables")
    while True:
        remaining.zero_()
        _lib.check(lib.dmvs_cloud_thin_round(_ptr(g.xyz), _ptr(prio), _ptr(g.cell_of), _ptr(runs), _ptr(state), _ptr(todo), n_todo,
                                             float(dst), _ptr(remaining), st), "dmvs_cloud_thin_round")
        rounds += 1
        left = int(remaining.item())
        undecided.append(left)
        if left == 0:
            break
        if rounds >= MAX_ROUNDS:
            raise _lib.DmvsError(f"reduce_points: {left} points undecided after {rounds} rounds")
        # compact the undecided points (plumbing); every round decides at least the earliest undecided point
        todo = (torch.nonzero(state == 0).reshape(-1) if todo is None else todo[state[todo.long()] == 0]).to(torch.int32).contiguous()
        n_todo = todo.numel()
    clock.lap("rounds")
    kept = torch.empty(n, dtype=torch.bool, device=dev)
    kept[g.perm] = state == 1
    if info is not None:
        info.update(rounds=rounds, cells=g.M, kept=int(kept.sum().item()), undecided_after_round=undecided)
        clock.lap("scatter")
        if clock.on:
            info["seconds"] = clock.t
    return kept


def domain_box(bb, max_dist: float):
    """The block grid of MaxDistCP.m:5-15: blocks 0..Range per axis from BB(1,:); (lo, hi) of the from-points it searches."""
    bb = np.asarray(bb, dtype=np.float64).reshape(2, 3)
    rng = np.floor((bb[1] - bb[0]) / max_dist)
    return bb[0].copy(), (bb[0] + rng * max_dist) + max_dist


def nn_levels(max_dist: float, cell0: Optional[float] = None, grow: Optional[float] = None, rings: Optional[int] = None):
    """[(cell, rings)] of the search passes: the last one reaches max_dist (rings * cell * (1 - 1e-6) >= max_dist)."""
    cell0, grow, rings = cell0 or NN_CELL0, grow or NN_GROW, rings or NN_RINGS
    levels, cell = [], float(cell0)
    while True:
        need = int(math.ceil(max_dist / (cell * (1.0 - 1e-6))))
        if need <= rings:
            levels.append((cell, need))
            return levels
        levels.append((cell, rings))
        cell *= grow


def max_dist_cp(q_to, q_from, bb, max_dist: float = 60.0, info: Optional[dict] = None, return_index: bool = False, device=None):
    """MaxDistCP(Qto, Qfrom, BB, MaxDist) as the code downstream uses it: float64 [N_from] (device) = min(d_nn, max_dist) for
    from-points in the domain ``BB(1,:) <= q < BB(1,:) + (floor((BB(2,:) - BB(1,:)) / MaxDist) + 1) * MaxDist``, max_dist
    outside it.  Worst-case work per query: (2 * NN_RINGS + 1)^3 cells per level, len(nn_levels(max_dist)) levels.
    ``return_index``: also the index of the nearest to-point (-1 where none was found within reach)."""
    dev = _device(device)
    to, frm = _cloud(q_to, dev, "max_dist_cp: q_to"), _cloud(q_from, dev, "max_dist_cp: q_from")
    nf = frm.shape[0]
    max_dist = float(max_dist)
    if not max_dist > 0:
        raise _lib.DmvsError(f"max_dist_cp: max_dist = {max_dist}")
    lib = _lib.load()
    st = _stream(dev)
    dist = torch.full((nf,), max_dist, dtype=torch.float64, device=dev)
    nn = torch.full((nf,), -1, dtype=torch.int64, device=dev) if return_index else None
    stats = dict(queries=0, levels=[], examined=None)
    lo, hi = domain_box(bb, max_dist)
    levels = nn_levels(max_dist)
    clock = _Clock(dev, info)
    if nf and to.shape[0]:
        dom = torch.empty(nf, dtype=torch.uint8, device=dev)
        _lib.check(lib.dmvs_cloud_in_box(_ptr(frm), nf, _d3(lo), _d3(hi), _ptr(dom), st), "dmvs_cloud_in_box")

        def grid_of(cell):
            origin = lo - max_dist - cell
            return origin, cell, np.ceil((hi - lo + 2 * max_dist + 2 * cell) / cell).astype(np.int64) + 1

        # the queries in the cell order of the finest grid: the lanes of a wave then walk the same few cells
        qkeys = torch.empty(nf, dtype=torch.int64, device=dev)
        o0, c0, d0 = grid_of(levels[0][0])
        check_grid(d0)
        _lib.check(lib.dmvs_cloud_cell_keys(_ptr(frm), nf, _d3(o0), c0, _i3(d0), _ptr(qkeys), st), "dmvs_cloud_cell_keys")
        qkeys[dom == 0] = _NO_CELL
        skeys, qperm = torch.sort(qkeys)
        nq = int(torch.searchsorted(skeys, torch.tensor([_NO_CELL], dtype=torch.int64, device=dev)).item())
        q_idx = qperm[:nq].to(torch.int32).contiguous()
        stats["queries"] = nq
        best2 = torch.full((nf,), float("inf"), dtype=torch.float64, device=dev)
        nn_lvl = torch.full((nf,), -1, dtype=torch.int32, device=dev) if return_index else None
        examined = torch.zeros(1, dtype=torch.int64, device=dev) if info is not None and info.get("count_examined") else None
        for cell, rings in levels:
            if q_idx.numel() == 0:
                break
            g = _Grid(to, *grid_of(cell))
            clock.lap("sort_and_cell_tables")
            if g.M == 0:
                # no to-point within max_dist (+ one cell) of the domain, e.g. a cloud in another frame: nobody has a neighbour
                # within reach, every distance stays max_dist and every index -1 (MaxDistCP.m:28-29)
                q_idx = q_idx[:0]
                break
            nq = q_idx.numel()
            resolved = torch.empty(nq, dtype=torch.uint8, device=dev)
            if return_index:  # the best point so far was found on another level's sorted cloud: keep it as an original index
                nn_lvl.fill_(-1)
            _lib.check(lib.dmvs_cloud_nn(_ptr(g.xyz), _ptr(g.ukeys), _ptr(g.ustart), g.M, _d3(g.origin), g.cell, _i3(g.dims), _ptr(frm),
                                         _ptr(q_idx), nq, rings, max_dist, _ptr(best2), _ptr(nn_lvl), _ptr(dist), _ptr(resolved),
                                         _ptr(examined), st), "dmvs_cloud_nn")
            if return_index:
                qi = q_idx.long()
                found = nn_lvl[qi] >= 0
                nn[qi[found]] = g.perm[nn_lvl[qi[found]].long()]
            stats["levels"].append(dict(cell=cell, rings=rings, queries=nq, to_points=g.n, cells=g.M))
            clock.lap("search")
            q_idx = q_idx[resolved == 0].contiguous()
        if q_idx.numel():
            raise _lib.DmvsError(f"max_dist_cp: {q_idx.numel()} queries unresolved after the last level")
        if examined is not None:
            stats["examined"] = int(examined.item())
        clock.lap("sort_and_cell_tables")
    if info is not None:
        info.update(stats)
        if clock.on:
            info["seconds"] = clock.t
    return (dist, nn) if return_index else dist


def _host_f64(a, n, what):
    v = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float64).reshape(-1)
    if v.size != n:
        raise _lib.DmvsError(f"{what}: expected {n} values, got {v.size}")
    return v


def data_in_mask(xyz, obs_mask, bb, res, device=None) -> torch.Tensor:
    """DataInMask of PointCompareMain.m:33-42: bool [N] (device)."""
    dev = _device(device)
    pts = _cloud(xyz, dev, "data_in_mask")
    m = torch.as_tensor(obs_mask)
    if m.dim() != 3:
        raise _lib.DmvsError(f"data_in_mask: ObsMask must be a 3-D volume, got {tuple(m.shape)}")
    m = (m != 0).to(device=dev, dtype=torch.uint8).contiguous()
    bb0 = _host_f64(bb, 6, "BB")[:3]
    res = float(_host_f64(res, 1, "Res")[0])
    out = torch.zeros(pts.shape[0], dtype=torch.uint8, device=dev)
    if pts.shape[0]:
        _lib.check(_lib.load().dmvs_cloud_in_mask(_ptr(pts), pts.shape[0], _d3(bb0), res, _ptr(m), _i3(m.shape), _ptr(out),
                                                  _stream(dev)), "dmvs_cloud_in_mask")
    return out.bool()


def stl_above_plane(xyz, plane, device=None) -> torch.Tensor:
    """StlAbovePlane of PointCompareMain.m:54: bool [N] (device)."""
    dev = _device(device)
    pts = _cloud(xyz, dev, "stl_above_plane")
    out = torch.zeros(pts.shape[0], dtype=torch.uint8, device=dev)
    if pts.shape[0]:
        _lib.check(_lib.load().dmvs_cloud_above_plane(_ptr(pts), pts.shape[0], _d3(_host_f64(plane, 4, "P")), _ptr(out), _stream(dev)),
                   "dmvs_cloud_above_plane")
    return out.bool()


def point_compare(data_xyz, stl_xyz, obs_mask, bb, res, plane, dst: float = 0.2, max_dist: float = 60.0, order=None, seed: int = 0,
                  info: Optional[dict] = None, device=None) -> Dict[str, torch.Tensor]:
    """PointCompareMain: the fields of BaseEval that the statistics use, as device tensors.  ``Qdata_kept`` is the thinning
    mask over the input cloud; ``Qdata`` the thinned cloud that ``Ddata`` and ``DataInMask`` refer to."""
    dev = _device(device)
    data, stl = _cloud(data_xyz, dev, "point_compare: data"), _cloud(stl_xyz, dev, "point_compare: stl")
    bb = _host_f64(bb, 6, "BB").reshape(2, 3)
    flags = {} if info is None else {k: info[k] for k in ("timing", "count_examined") if k in info}
    i_thin, i_d, i_s = dict(flags), dict(flags), dict(flags)
    kept = reduce_points(data, dst, order, seed, info=i_thin, device=dev)
    qdata = data[kept].contiguous()
    out = dict(Qdata_kept=kept, Qdata=qdata,
               Ddata=max_dist_cp(stl, qdata, bb, max_dist, info=i_d, device=dev),
               Dstl=max_dist_cp(qdata, stl, bb, max_dist, info=i_s, device=dev),
               DataInMask=data_in_mask(qdata, obs_mask, bb, res, device=dev),
               StlAbovePlane=stl_above_plane(stl, plane, device=dev))
    if info is not None:
        info.update(thinning=i_thin, data_to_stl=i_d, stl_to_data=i_s)
    return out


def _stats(d: torch.Tensor):
    """n, mean, var (N - 1), median with MATLAB's rule (mean of the two middle values for even n); float64 on the device."""
    n = d.numel()
    if n == 0:
        return 0, float("nan"), float("nan"), float("nan")
    s = torch.sort(d).values
    med = s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2
    mean = d.sum() / n
    var = ((d - mean) ** 2).sum() / (n - 1) if n > 1 else torch.zeros((), dtype=d.dtype)
    return n, float(mean), float(var), float(med)


def scan_stats(base_eval: Dict[str, torch.Tensor], outlier: float = 20.0) -> Dict[str, float]:
    """ComputeStat_web.m:57-73 for one scan: distances inside the mask / above the plane and below the outlier threshold."""
    dd = torch.as_tensor(base_eval["Ddata"], dtype=torch.float64)[torch.as_tensor(base_eval["DataInMask"]).bool()]
    ds = torch.as_tensor(base_eval["Dstl"], dtype=torch.float64)[torch.as_tensor(base_eval["StlAbovePlane"]).bool()]
    nd, md, vd, qd = _stats(dd[dd < outlier])
    ns, ms, vs, qs = _stats(ds[ds < outlier])
    return dict(nData=nd, nStl=ns, MeanData=md, MeanStl=ms, VarData=vd, VarStl=vs, MedData=qd, MedStl=qs)


def total_stat_text(scans: Sequence[int], mean_data: Sequence[float], mean_stl: Sequence[float]) -> bytes:
    """The bytes of TotalStat_<method>_Eval_.txt (ComputeStat_web.m:92-107)."""
    acc, comp = float(np.mean(mean_data)), float(np.mean(mean_stl))
    text = "mean acc:%f\tmean comp:%f\tmean overall:%f\r\n" % (acc, comp, (acc + comp) / 2)
    text += "scans\tacc  \tcmop  \r\n"
    for s, a, c in zip(scans, mean_data, mean_stl):
        text += "scan%d\t%.4f\t%.4f\r\n" % (s, a, c)
    return text.encode("ascii")


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply_xyz(filename: str) -> np.ndarray:
    """Vertex positions [N,3] float32 of a PLY file (binary little / big endian or ASCII; any scalar property list that has
    x, y, z; the vertex element must come first).  The counterpart of fusion.write_ply; needs no third-party reader."""
    with open(filename, "rb") as f:
        if f.readline().strip() != b"ply":
            raise _lib.DmvsError(f"{filename}: not a PLY file")
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise _lib.DmvsError(f"{filename}: PLY header without end_header")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == "property":
                if not elements:
                    raise _lib.DmvsError(f"{filename}: property before any element")
                elements[-1][2].append((tok[-1], None if tok[1] == "list" else _PLY_TYPES.get(tok[1])))
            elif tok[0] == "end_header":
                break
        if not elements or elements[0][0] != "vertex":
            raise _lib.DmvsError(f"{filename}: the first element must be `vertex`")
        _, n, props = elements[0]
        names = [p[0] for p in props]
        if any(p[1] is None for p in props) or not all(a in names for a in "xyz"):
            raise _lib.DmvsError(f"{filename}: vertex needs scalar properties including x, y, z (has {names})")
        if fmt == "ascii":
            rows = np.loadtxt(f, dtype=np.float64, max_rows=n, ndmin=2) if n else np.zeros((0, len(names)))
            if rows.shape != (n, len(names)):
                raise _lib.DmvsError(f"{filename}: expected {n} vertex rows of {len(names)} values, got {rows.shape}")
            return np.stack([rows[:, names.index(a)] for a in "xyz"], 1).astype(np.float32)
        if fmt not in ("binary_little_endian", "binary_big_endian"):
            raise _lib.DmvsError(f"{filename}: unknown PLY format {fmt!r}")
        dt = np.dtype([(nm, ("<" if fmt == "binary_little_endian" else ">") + t) for nm, t in props])
        raw = f.read(n * dt.itemsize)
        if len(raw) != n * dt.itemsize:
            raise _lib.DmvsError(f"{filename}: truncated vertex data ({len(raw)} of {n * dt.itemsize} bytes)")
        v = np.frombuffer(raw, dtype=dt, count=n)
        return np.stack([v[a].astype(np.float32) for a in "xyz"], 1)


def _load_vars(path: str):
    if path.endswith(".npz"):
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    with open(path, "rb") as f:
        if f.read(19) == b"MATLAB 7.3 MAT-file":
            raise _lib.DmvsError(f"{path} is a MATLAB v7.3 (HDF5) file; save it with -v7 or convert it to .npz")
    try:
        from scipy.io import loadmat
    except ImportError as e:
        raise _lib.DmvsError(f"reading {path} needs scipy (scipy.io.loadmat); convert the file to .npz with the same names") from e
    return loadmat(path)


def load_obs_mask(path: str):
    """(ObsMask uint8 [nx][ny][nz] C-order, BB float64 [2,3], Res float) from ObsMask<scan>_10.mat or a .npz with the same names."""
    v = _load_vars(path)
    for k in ("ObsMask", "BB", "Res"):
        if k not in v:
            raise _lib.DmvsError(f"{path}: no variable {k}")
    mask = np.ascontiguousarray(np.asarray(v["ObsMask"]) != 0, dtype=np.uint8)
    if mask.ndim != 3:
        raise _lib.DmvsError(f"{path}: ObsMask has shape {mask.shape}")
    return mask, np.asarray(v["BB"], dtype=np.float64).reshape(2, 3), float(np.asarray(v["Res"], dtype=np.float64).reshape(-1)[0])


def load_plane(path: str) -> np.ndarray:
    """P float64 [4] from Plane<scan>.mat or a .npz with the same name."""
    v = _load_vars(path)
    if "P" not in v:
        raise _lib.DmvsError(f"{path}: no variable P")
    return np.asarray(v["P"], dtype=np.float64).reshape(4)


def _first_existing(*paths):
    for p in paths:
        if os.path.exists(p):
            return p
    raise _lib.DmvsError("none of these files exists: " + ", ".join(paths))


def evaluate_dtu(ply_dir: str, data_path: str, out_dir: str, scans: Sequence[int] = DTU_TEST_SETS, method: str = "mvsnet",
                 light: str = "l3", dst: float = 0.2, max_dist: float = 60.0, outlier: float = 20.0, seed: int = 0, device=None):
    """BaseEvalMain_web.m + ComputeStat_web.m in one call.  Per scan: ``<ply_dir>/<method>NNN_<light>.ply`` (the name run_test
    writes), ``<data_path>/Points/stl/stlNNN_total.ply``, ``<data_path>/ObsMask/ObsMask<scan>_10.mat`` and ``Plane<scan>.mat``
    (or ``.npz`` files with the same names).  Writes ``<out_dir>/<method>_Eval_<scan>.json`` per scan and
    ``TotalStat_<method>_Eval_.txt`` in the reference's text format; returns the totals and the per-scan statistics."""
    dev = _device(device)
    os.makedirs(out_dir, exist_ok=True)
    per_scan = {}
    for scan in scans:
        scan = int(scan)
        name = ply_path(ply_dir, "scan%d" % scan, pcd_dir="")
        if (method, light) != ("mvsnet", "l3"):
            name = os.path.join(ply_dir, "%s%03d_%s.ply" % (method.lower(), scan, light))
        data = read_ply_xyz(name)
        stl = read_ply_xyz(os.path.join(data_path, "Points", "stl", "stl%03d_total.ply" % scan))
        obs = os.path.join(data_path, "ObsMask")
        mask, bb, res = load_obs_mask(_first_existing(os.path.join(obs, "ObsMask%d_10.mat" % scan), os.path.join(obs, "ObsMask%d_10.npz" % scan)))
        plane = load_plane(_first_existing(os.path.join(obs, "Plane%d.mat" % scan), os.path.join(obs, "Plane%d.npz" % scan)))
        info = {}
        be = point_compare(data, stl, mask, bb, res, plane, dst=dst, max_dist=max_dist, seed=seed, info=info, device=dev)
        st = scan_stats(be, outlier)
        st.update(scan=scan, points=int(data.shape[0]), kept=int(be["Qdata"].shape[0]), rounds=info["thinning"]["rounds"], dst=dst,
                  seed=seed)
        per_scan[scan] = st
        with open(os.path.join(out_dir, "%s_Eval_%d.json" % (method, scan)), "w") as f:
            json.dump(st, f, indent=1)
    ids = list(per_scan)
    acc = [per_scan[s]["MeanData"] for s in ids]
    comp = [per_scan[s]["MeanStl"] for s in ids]
    with open(os.path.join(out_dir, "TotalStat_%s_Eval_.txt" % method), "wb") as f:
        f.write(total_stat_text(ids, acc, comp))
    a, c = float(np.mean(acc)), float(np.mean(comp))
    return dict(acc=a, comp=c, overall=(a + c) / 2, scans=per_scan)
