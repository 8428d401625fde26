"""CPU restatement of the DTU point-cloud evaluation in NumPy float64 (helper for test_cloud_eval_*.py and the benchmark; not
collected).  What the MATLAB scripts compute, written from their description: the block-by-block nearest neighbour, the
sequential thinning loop, the mask / plane tests and the statistics.  Runs with NumPy alone; scipy's cKDTree is used for the
nearest-neighbour search when it is importable, chunked brute force otherwise."""
import numpy as np

try:
    from scipy.spatial import cKDTree
    HAVE_CKDTREE = True
except ImportError:  # pragma: no cover
    cKDTree = None
    HAVE_CKDTREE = False


def _f64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32), dtype=np.float64).reshape(-1, 3)


def nn_dist(to, frm, workers=-1):
    """Distance from every row of frm to its nearest row of to (both float64 [n,3], to non-empty)."""
    if len(frm) == 0:
        return np.zeros(0)
    if HAVE_CKDTREE:
        return cKDTree(to).query(frm, k=1, workers=workers)[0]
    out = np.empty(len(frm))
    chunk = max(1, int(4e6 // max(len(to), 1)))
    for s in range(0, len(frm), chunk):
        d = frm[s:s + chunk, None, :] - to[None, :, :]
        out[s:s + chunk] = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]).min(1))
    return out


def max_dist_cp_blocks(q_to, q_from, bb, max_dist=60.0):
    """The block-by-block form: a grid of max_dist-sized blocks from bb[0]; the from-points of a block are searched against the
    to-points of the block grown by max_dist on every side; from-points in no block keep max_dist.  Values above max_dist
    can come out (a neighbour in the far corner of the grown block)."""
    to, frm = _f64(q_to), _f64(q_from)
    bb = np.asarray(bb, dtype=np.float64).reshape(2, 3)
    dist = np.full(len(frm), float(max_dist))
    rng = np.floor((bb[1] - bb[0]) / max_dist).astype(int)

    def axis_masks(pts, grow):
        # per axis and block index: low <= p < high (the block, or the block grown by max_dist), compared once per axis
        out = []
        for a in range(3):
            low = [bb[0, a] + float(i) * max_dist for i in range(rng[a] + 1)]
            out.append([(pts[:, a] >= (lo - max_dist if grow else lo)) & (pts[:, a] < ((lo + max_dist) + max_dist if grow else lo + max_dist))
                        for lo in low])
        return out

    mf, mt = axis_masks(frm, False), axis_masks(to, True)
    for x in range(rng[0] + 1):
        for y in range(rng[1] + 1):
            for z in range(rng[2] + 1):
                idx_f = np.nonzero(mf[0][x] & mf[1][y] & mf[2][z])[0]
                if len(idx_f) == 0:
                    continue
                idx_t = np.nonzero(mt[0][x] & mt[1][y] & mt[2][z])[0]
                dist[idx_f] = max_dist if len(idx_t) == 0 else nn_dist(to[idx_t], frm[idx_f])
    return dist


def in_domain(q_from, bb, max_dist=60.0):
    frm = _f64(q_from)
    bb = np.asarray(bb, dtype=np.float64).reshape(2, 3)
    rng = np.floor((bb[1] - bb[0]) / max_dist)
    hi = (bb[0] + rng * max_dist) + max_dist
    return np.all(frm >= bb[0], 1) & np.all(frm < hi, 1)


def bounded_nn(q_to, q_from, bb, max_dist=60.0):
    """min(d_nn, max_dist) inside the domain, max_dist outside it: the form the product computes."""
    to, frm = _f64(q_to), _f64(q_from)
    dist = np.full(len(frm), float(max_dist))
    dom = in_domain(q_from, bb, max_dist)
    if len(to) and dom.any():
        dist[dom] = np.minimum(nn_dist(to, frm[dom]), max_dist)
    return dist


def neighbour_pairs(xyz, r):
    """All pairs i != j (each once) with distance <= r, by a NumPy cell sort: (i, j, d)."""
    p = _f64(xyz)
    n = len(p)
    e = np.zeros(0, dtype=np.int64)
    if n < 2:
        return e, e, np.zeros(0)
    c = np.floor((p - p.min(0)) / r).astype(np.int64) + 1
    dims = c.max(0) + 2
    key = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    o = np.argsort(key, kind="stable")
    ks = key[o]
    ps = p[o]
    oi, oj, od = [], [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                off = (dz * dims[1] + dy) * dims[0] + dx
                if off < 0:
                    continue
                b = np.searchsorted(ks, ks + off, "right")
                a = np.arange(n) + 1 if off == 0 else np.searchsorted(ks, ks + off, "left")
                cnt = b - a
                tot = int(cnt.sum())
                if tot == 0:
                    continue
                ii = np.repeat(np.arange(n), cnt)
                jj = np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(a, cnt)
                d = ps[jj] - ps[ii]
                dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
                m = dist <= r
                oi.append(o[ii[m]])
                oj.append(o[jj[m]])
                od.append(dist[m])
    if not oi:
        return e, e, np.zeros(0)
    return np.concatenate(oi), np.concatenate(oj), np.concatenate(od)


def adjacency(xyz, dst):
    """CSR neighbour lists (distance <= dst) and the distances of all pairs within dst + 1e-6 (for the input conditions)."""
    i, j, d = neighbour_pairs(xyz, dst + 1e-6)
    n = len(np.asarray(xyz).reshape(-1, 3))
    m = d <= dst
    a = np.concatenate([i[m], j[m]])
    b = np.concatenate([j[m], i[m]])
    o = np.argsort(a, kind="stable")
    start = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(a, minlength=n), out=start[1:])
    return start, b[o], d


def reduce_points_sequential(xyz, dst, order, adj=None):
    """The visit loop: a point that is still alive when it is visited removes every point within dst of it."""
    start, nbr, _ = adj if adj is not None else adjacency(xyz, dst)
    alive = np.ones(len(start) - 1, dtype=bool)
    for i in np.asarray(order).tolist():
        if alive[i]:
            alive[nbr[start[i]:start[i + 1]]] = False
            alive[i] = True
    return alive


def reduce_points_fixed_point(xyz, dst, order, in_place, visit=None, adj=None):
    """The parallel schedule restated: undecided / kept / removed; an undecided point is removed when an earlier neighbour is
    kept, kept when all earlier neighbours are removed.  in_place: a sweep sees the decisions made earlier in the same sweep,
    points visited in the order `visit` (a permutation); otherwise every sweep works on a snapshot.  (kept mask, rounds)."""
    start, nbr, _ = adj if adj is not None else adjacency(xyz, dst)
    n = len(start) - 1
    prio = np.empty(n, dtype=np.int64)
    prio[np.asarray(order)] = np.arange(n)
    visit = np.arange(n) if visit is None else np.asarray(visit)
    state = np.zeros(n, dtype=np.int8)
    rounds = 0
    while (state == 0).any():
        rounds += 1
        src = state if in_place else state.copy()
        for i in visit.tolist():
            if state[i]:
                continue
            nb = nbr[start[i]:start[i + 1]]
            nb = nb[prio[nb] < prio[i]]
            s = src[nb]
            if (s == 1).any():
                state[i] = 2
            elif (s == 2).all():
                state[i] = 1
        assert rounds <= n + 1
    return state == 1, rounds


def data_in_mask(xyz, obs_mask, bb, res):
    """round((q - bb[0]) / res + 1) (half away from zero) inside the volume and the voxel set; also the rounding arguments."""
    q = _f64(xyz)
    bb = np.asarray(bb, dtype=np.float64).reshape(2, 3)
    v = (q - bb[0]) / float(res) + 1.0
    qv = np.sign(v) * np.floor(np.abs(v) + 0.5)
    shape = np.array(obs_mask.shape, dtype=np.float64)
    inside = np.all(qv > 0, 1) & np.all(qv <= shape, 1)
    out = np.zeros(len(q), dtype=bool)
    idx = qv[inside].astype(np.int64) - 1
    out[inside] = np.asarray(obs_mask)[idx[:, 0], idx[:, 1], idx[:, 2]] != 0
    return out, v


def stl_above_plane(xyz, plane):
    q = _f64(xyz)
    p = np.asarray(plane, dtype=np.float64).reshape(4)
    return p[0] * q[:, 0] + p[1] * q[:, 1] + p[2] * q[:, 2] + p[3] > 0


def stats(d):
    """n, mean, variance (N - 1), median (mean of the two middle values for even n)."""
    d = np.asarray(d, dtype=np.float64)
    n = len(d)
    if n == 0:
        return 0, float("nan"), float("nan"), float("nan")
    s = np.sort(d)
    med = s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2
    mean = d.sum() / n
    var = ((d - mean) ** 2).sum() / (n - 1) if n > 1 else 0.0
    return n, float(mean), float(var), float(med)


def point_compare(data, stl, obs_mask, bb, res, plane, dst=0.2, max_dist=60.0, order=None, outlier=20.0):
    """The whole scan on the CPU: thinning, both searches (block form, capped at max_dist), classification, statistics."""
    kept = reduce_points_sequential(data, dst, order)
    qdata = np.asarray(data, dtype=np.float32)[kept]
    ddata = np.minimum(max_dist_cp_blocks(stl, qdata, bb, max_dist), max_dist)
    dstl = np.minimum(max_dist_cp_blocks(qdata, stl, bb, max_dist), max_dist)
    in_mask, v = data_in_mask(qdata, obs_mask, bb, res)
    above = stl_above_plane(stl, plane)
    dd, ds = ddata[in_mask], dstl[above]
    nd, md, vd, qd = stats(dd[dd < outlier])
    ns, ms, vs, qs = stats(ds[ds < outlier])
    st = dict(nData=nd, nStl=ns, MeanData=md, MeanStl=ms, VarData=vd, VarStl=vs, MedData=qd, MedStl=qs)
    return dict(kept=kept, Ddata=ddata, Dstl=dstl, DataInMask=in_mask, StlAbovePlane=above, mask_arg=v, stats=st)


def total_stat_text(scans, acc, comp):
    a, c = float(np.mean(acc)), float(np.mean(comp))
    lines = ["mean acc:%f\tmean comp:%f\tmean overall:%f" % (a, c, (a + c) / 2), "scans\tacc  \tcmop  "]
    lines += ["scan%d\t%.4f\t%.4f" % (s, x, y) for s, x, y in zip(scans, acc, comp)]
    return ("\r\n".join(lines) + "\r\n").encode("ascii")
