// N5: DTU point-cloud evaluation (accuracy / completeness) -- device code, included at the end of fusion.hip.
//
// Replaces the arithmetic of the reference's scripts/evaluation_dtu: reducePts_haa.m (greedy thinning), MaxDistCP.m (bounded
// nearest neighbour) and the mask / plane classification of PointCompareMain.m:31-54.  Sorting, compaction and the statistics are
// host plumbing (dmvsnet_amd/cloud_eval.py); the kernels below are the gathers.
//
// Arithmetic: coordinates are fp32, every difference and distance is formed in fp64 (the differences are then exact):
// dx * dx + dy * dy + dz * dz in that order, unfused (-ffp-contract=off), compared squared, one sqrt at the end.
//
// Grid: a point's cell is floor((p - origin) / cell) per axis in fp64, key (iz * ny + iy) * nx + ix (x fastest), so the
// x-neighbours of a cell are one contiguous run of the key-sorted cloud.  The cloud is sparse in the key space: the occupied
// cells are the sorted unique keys `ukeys` [M] with `ustart` [M + 1] their first points; a run is found by one binary search.
// The quotient is off by at most 2^-29 cells (|t| < 2^21, a few ulp), so two points whose cell indices differ by m on an axis
// are more than (m - 1) * cell * (1 - 1e-6) apart on it: every distance bound below uses the shrunk cell size `hb`.
#pragma once
#include "common.h"

constexpr int CLOUD_WG = 256;
constexpr int CLOUD_MAX_AXIS = 1 << 21;  // 3 x 21 bits: the key stays below 2^63
constexpr long long CLOUD_NO_CELL = 0x7fffffffffffffffLL;

struct CloudGrid {
    double ox, oy, oz, cell;
    int nx, ny, nz;
};

static inline bool cloud_grid_ok(const double* origin3, double cell, const int* dims3) {
    if (!origin3 || !dims3 || !(cell > 0.0)) return false;
    for (int i = 0; i < 3; ++i)
        if (dims3[i] < 1 || dims3[i] > CLOUD_MAX_AXIS || !(origin3[i] == origin3[i])) return false;
    return true;
}

static inline CloudGrid cloud_grid(const double* origin3, double cell, const int* dims3) {
    return CloudGrid{origin3[0], origin3[1], origin3[2], cell, dims3[0], dims3[1], dims3[2]};
}

// cell index on one axis, or -1 outside [0, n) (NaN included)
__device__ __forceinline__ int cloud_axis_cell(double p, double o, double cell, int n) {
    const double t = floor((p - o) / cell);
    return (t >= 0.0 && t < (double)n) ? (int)t : -1;
}

__global__ __launch_bounds__(CLOUD_WG) void cloud_cell_keys_kernel(const float* __restrict__ xyz, int n, const CloudGrid g,
                                                                  long long* __restrict__ keys) {
    const int i = blockIdx.x * CLOUD_WG + threadIdx.x;
    if (i >= n) return;
    const int ix = cloud_axis_cell((double)xyz[3 * (size_t)i], g.ox, g.cell, g.nx);
    const int iy = cloud_axis_cell((double)xyz[3 * (size_t)i + 1], g.oy, g.cell, g.ny);
    const int iz = cloud_axis_cell((double)xyz[3 * (size_t)i + 2], g.oz, g.cell, g.nz);
    keys[i] = (ix < 0 || iy < 0 || iz < 0) ? CLOUD_NO_CELL : ((long long)iz * g.ny + iy) * g.nx + ix;
}

// first j in [0, M) with ukeys[j] >= key (M when there is none)
__device__ __forceinline__ int cloud_lower_bound(const long long* __restrict__ ukeys, int M, long long key) {
    int lo = 0, hi = M;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ukeys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The nine x-runs of every occupied cell's 27-cell neighbourhood as point ranges [begin, end) of the key-sorted cloud:
// one binary search per run and OCCUPIED CELL, once, instead of one per point and thinning round.
__global__ __launch_bounds__(CLOUD_WG) void cloud_cell_runs_kernel(const long long* __restrict__ ukeys,
                                                                  const int* __restrict__ ustart, int M, int nx, int ny, int nz,
                                                                  int* __restrict__ runs) {
    const int j = blockIdx.x * CLOUD_WG + threadIdx.x;
    if (j >= M) return;
    const long long key = ukeys[j];
    const int ix = (int)(key % nx), iy = (int)((key / nx) % ny), iz = (int)(key / ((long long)nx * ny));
    for (int t = 0; t < 9; ++t) {
        const int y = iy + t % 3 - 1, z = iz + t / 3 - 1;
        int b = 0, e = 0;
        if (y >= 0 && y < ny && z >= 0 && z < nz) {
            const long long base = ((long long)z * ny + y) * nx;
            const long long lo = base + (ix > 0 ? ix - 1 : 0), hi = base + (ix < nx - 1 ? ix + 1 : nx - 1);
            int j0 = cloud_lower_bound(ukeys, M, lo), j1 = j0;
            while (j1 < M && ukeys[j1] <= hi) ++j1;
            b = ustart[j0];
            e = ustart[j1];
        }
        runs[((size_t)j * 9 + t) * 2] = b;
        runs[((size_t)j * 9 + t) * 2 + 1] = e;
    }
}

// One thinning round (reducePts_haa.m:23-29 as a fixed-point iteration).  state: 0 undecided, 1 kept, 2 removed; prio = position
// in the visit order.  An undecided point becomes removed when a neighbour (distance <= dst) that comes earlier is kept, kept
// when every earlier neighbour is removed.  States only move from 0 to the value the order fixes, so reading a neighbour's
// state while its owner writes it is harmless: a stale 0 leaves this point undecided for one more round.
__global__ __launch_bounds__(CLOUD_WG) void cloud_thin_round_kernel(const float* __restrict__ xyz, const int* __restrict__ prio,
                                                                   const int* __restrict__ cell_of,
                                                                   const int* __restrict__ runs, unsigned char* state,
                                                                   const int* __restrict__ todo, int n_todo, double dst2,
                                                                   int* remaining) {
    const int k = blockIdx.x * CLOUD_WG + threadIdx.x;
    bool still = false;
    if (k < n_todo) {
        const int i = todo ? todo[k] : k;
        if (__hip_atomic_load(&state[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
            const int pi = prio[i];
            const double x = (double)xyz[3 * (size_t)i], y = (double)xyz[3 * (size_t)i + 1], z = (double)xyz[3 * (size_t)i + 2];
            const int* r = runs + (size_t)cell_of[i] * 18;
            bool removed = false, pending = false;
            for (int t = 0; t < 9 && !removed; ++t) {
                const int e = r[2 * t + 1];
                for (int j = r[2 * t]; j < e; ++j) {
                    if (prio[j] >= pi) continue;  // later in the order (or the point itself)
                    const unsigned char sj = __hip_atomic_load(&state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (sj == 2) continue;
                    const double dx = (double)xyz[3 * (size_t)j] - x, dy = (double)xyz[3 * (size_t)j + 1] - y,
                                 dz = (double)xyz[3 * (size_t)j + 2] - z;
                    if (dx * dx + dy * dy + dz * dz > dst2) continue;
                    if (sj == 1) { removed = true; break; }
                    pending = true;
                }
            }
            if (removed)
                __hip_atomic_store(&state[i], (unsigned char)2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else if (!pending)
                __hip_atomic_store(&state[i], (unsigned char)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else
                still = true;
        }
    }
    const int n = __syncthreads_count(still);
    if (threadIdx.x == 0 && n) atomicAdd(remaining, n);  // one integer atomic per workgroup
}

struct CloudNNArgs {
    const float* to_xyz;       // key-sorted to-points of this level's grid
    const long long* ukeys;    // [M] occupied cells
    const int* ustart;         // [M + 1]
    int M;
    CloudGrid g;
    const float* q_xyz;        // from-points (original order)
    const int* q_idx;          // [nq] the queries of this pass, in cell order; NULL: 0 .. nq - 1
    int nq, rings;
    double max_dist;
    double* best2;             // [N_from] in / out: smallest squared distance seen so far (+inf at the start)
    int* nn;                   // [N_from] in / out or NULL: its point (index into to_xyz of the level that found it)
    double* dist;              // [N_from] out, written when resolved: min(sqrt(best2), max_dist)
    unsigned char* resolved;   // [nq] out
    unsigned long long* examined;  // NULL or one counter: distances evaluated (instrumentation)
};

// Bounded nearest neighbour, one pass on one grid level (MaxDistCP.m:31-33 without the blocks).  Rings of cells outwards from the
// query's cell; after rings 0..r every unexamined point is more than r * hb away, so the search stops when the best distance is
// no larger, or when r * hb reaches max_dist.  At most `rings` rings per pass: (2 * rings + 1)^3 cells; a query that is still open
// goes to the next, coarser level with its best distance, which prunes every cell that cannot beat it.
__global__ __launch_bounds__(CLOUD_WG) void cloud_nn_kernel(const CloudNNArgs a) {
    const int k = blockIdx.x * CLOUD_WG + threadIdx.x;
    if (k >= a.nq) return;
    const int qi = a.q_idx ? a.q_idx[k] : k;
    const double qx = (double)a.q_xyz[3 * (size_t)qi], qy = (double)a.q_xyz[3 * (size_t)qi + 1], qz = (double)a.q_xyz[3 * (size_t)qi + 2];
    const CloudGrid g = a.g;
    const int cx = cloud_axis_cell(qx, g.ox, g.cell, g.nx), cy = cloud_axis_cell(qy, g.oy, g.cell, g.ny),
              cz = cloud_axis_cell(qz, g.oz, g.cell, g.nz);
    if (cx < 0 || cy < 0 || cz < 0) {  // outside the grid: the bounds below do not hold; the host never sends such a query
        a.resolved[k] = 1;
        a.dist[qi] = a.max_dist;
        return;
    }
    const double hb = g.cell * (1.0 - 1e-6), hb2 = hb * hb;
    double best2 = a.best2[qi];
    int bi = a.nn ? a.nn[qi] : -1;
    unsigned long long cnt = 0;
    bool done = false;
    for (int r = 0; r <= a.rings && !done; ++r) {
        for (int dz = -r; dz <= r; ++dz) {
            const int z = cz + dz;
            if (z < 0 || z >= g.nz) continue;
            const int mz = abs(dz) > 1 ? abs(dz) - 1 : 0;
            for (int dy = -r; dy <= r; ++dy) {
                const int y = cy + dy;
                if (y < 0 || y >= g.ny) continue;
                const int my = abs(dy) > 1 ? abs(dy) - 1 : 0;
                const double row2 = (double)(my * my + mz * mz) * hb2;
                if (row2 > best2) continue;
                const long long base = ((long long)z * g.ny + y) * g.nx;
                const bool face = abs(dz) == r || abs(dy) == r;  // the whole x-run lies on the shell; else only its two ends
                for (int seg = 0; seg < (face ? 1 : 2); ++seg) {
                    int xlo = face ? cx - r : (seg ? cx + r : cx - r), xhi = face ? cx + r : xlo;
                    xlo = xlo < 0 ? 0 : xlo;
                    xhi = xhi > g.nx - 1 ? g.nx - 1 : xhi;
                    if (xlo > xhi) continue;
                    for (int j = cloud_lower_bound(a.ukeys, a.M, base + xlo); j < a.M; ++j) {
                        const long long key = a.ukeys[j];
                        if (key > base + xhi) break;
                        const int ax = abs((int)(key - base) - cx), mx = ax > 1 ? ax - 1 : 0;
                        if ((double)(mx * mx) * hb2 + row2 > best2) continue;
                        const int e = a.ustart[j + 1];
                        for (int p = a.ustart[j]; p < e; ++p) {
                            const double dx = (double)a.to_xyz[3 * (size_t)p] - qx, dy2 = (double)a.to_xyz[3 * (size_t)p + 1] - qy,
                                         dz2 = (double)a.to_xyz[3 * (size_t)p + 2] - qz;
                            const double d2 = dx * dx + dy2 * dy2 + dz2 * dz2;
                            if (d2 < best2) { best2 = d2; bi = p; }
                        }
                        cnt += (unsigned long long)(e - a.ustart[j]);
                    }
                }
            }
        }
        const double rb = (double)r * hb;
        done = best2 <= rb * rb || rb >= a.max_dist;
    }
    a.best2[qi] = best2;
    if (a.nn) a.nn[qi] = bi;
    a.resolved[k] = done ? 1 : 0;
    if (done) {
        const double d = sqrt(best2);
        a.dist[qi] = d < a.max_dist ? d : a.max_dist;
    }
    if (a.examined) atomicAdd(a.examined, cnt);
}

// PointCompareMain.m:33-42: Qv = round((Q - BB(1,:)) / Res + 1), inside size(ObsMask) and ObsMask(Qv) set.  MATLAB's round is
// half away from zero; floor(v + 0.5) agrees with it on every v > -0.5, i.e. on every value that can land in 1..size.
struct CloudMaskArgs {
    const float* xyz;
    int n;
    double bx, by, bz, res;
    const unsigned char* mask;  // [mx][my][mz], z fastest (the C-order array loadmat returns)
    int mx, my, mz;
    unsigned char* out;
};

__global__ __launch_bounds__(CLOUD_WG) void cloud_in_mask_kernel(const CloudMaskArgs a) {
    const int i = blockIdx.x * CLOUD_WG + threadIdx.x;
    if (i >= a.n) return;
    const double vx = floor(((double)a.xyz[3 * (size_t)i] - a.bx) / a.res + 1.0 + 0.5);
    const double vy = floor(((double)a.xyz[3 * (size_t)i + 1] - a.by) / a.res + 1.0 + 0.5);
    const double vz = floor(((double)a.xyz[3 * (size_t)i + 2] - a.bz) / a.res + 1.0 + 0.5);
    bool in = vx >= 1.0 && vx <= (double)a.mx && vy >= 1.0 && vy <= (double)a.my && vz >= 1.0 && vz <= (double)a.mz;
    if (in) in = a.mask[((size_t)((int)vx - 1) * a.my + ((int)vy - 1)) * a.mz + ((int)vz - 1)] != 0;
    a.out[i] = in ? 1 : 0;
}

// PointCompareMain.m:54: P' * [Q; 1] > 0
__global__ __launch_bounds__(CLOUD_WG) void cloud_above_plane_kernel(const float* __restrict__ xyz, int n, double p0, double p1,
                                                                    double p2, double p3, unsigned char* __restrict__ out) {
    const int i = blockIdx.x * CLOUD_WG + threadIdx.x;
    if (i >= n) return;
    const double s = p0 * (double)xyz[3 * (size_t)i] + p1 * (double)xyz[3 * (size_t)i + 1] + p2 * (double)xyz[3 * (size_t)i + 2] + p3;
    out[i] = s > 0.0 ? 1 : 0;
}

// MaxDistCP.m:10-18: a from-point is searched at all only when lo <= q < hi on every axis (hi = the end of the last block)
__global__ __launch_bounds__(CLOUD_WG) void cloud_in_box_kernel(const float* __restrict__ xyz, int n, double lx, double ly, double lz,
                                                               double hx, double hy, double hz, unsigned char* __restrict__ out) {
    const int i = blockIdx.x * CLOUD_WG + threadIdx.x;
    if (i >= n) return;
    const double x = (double)xyz[3 * (size_t)i], y = (double)xyz[3 * (size_t)i + 1], z = (double)xyz[3 * (size_t)i + 2];
    out[i] = (x >= lx && y >= ly && z >= lz && x < hx && y < hy && z < hz) ? 1 : 0;
}

extern "C" int dmvs_cloud_cell_keys(const float* xyz, int n, const double* origin3, double cell, const int* dims3,
                                    long long* keys, dmvs_stream_t stream) {
    if (!xyz || !keys || n < 1 || !cloud_grid_ok(origin3, cell, dims3)) return DMVS_EINVAL;
    cloud_cell_keys_kernel<<<ceil_div(n, CLOUD_WG), CLOUD_WG, 0, (hipStream_t)stream>>>(xyz, n, cloud_grid(origin3, cell, dims3), keys);
    DMVS_LAUNCH_CHECK();
}

extern "C" int dmvs_cloud_cell_runs(const long long* ukeys, const int* ustart, int M, const int* dims3, int* runs,
                                    dmvs_stream_t stream) {
    const double zero3[3] = {0.0, 0.0, 0.0};
    if (!ukeys || !ustart || !runs || M < 1 || !cloud_grid_ok(zero3, 1.0, dims3)) return DMVS_EINVAL;
    cloud_cell_runs_kernel<<<ceil_div(M, CLOUD_WG), CLOUD_WG, 0, (hipStream_t)stream>>>(ukeys, ustart, M, dims3[0], dims3[1], dims3[2], runs);
    DMVS_LAUNCH_CHECK();
}

extern "C" int dmvs_cloud_thin_round(const float* xyz, const int* prio, const int* cell_of, const int* runs, unsigned char* state,
                                     const int* todo, int n_todo, double dst, int* remaining, dmvs_stream_t stream) {
    if (!xyz || !prio || !cell_of || !runs || !state || !remaining || n_todo < 1 || !(dst >= 0.0)) return DMVS_EINVAL;
    cloud_thin_round_kernel<<<ceil_div(n_todo, CLOUD_WG), CLOUD_WG, 0, (hipStream_t)stream>>>(xyz, prio, cell_of, runs, state, todo, n_todo,
                                                                                             dst * dst, remaining);
    DMVS_LAUNCH_CHECK();
}

extern "C" int dmvs_cloud_nn(const float* to_xyz, const long long* ukeys, const int* ustart, int M, const double* origin3,
                             double cell, const int* dims3, const float* q_xyz, const int* q_idx, int nq, int rings,
                             double max_dist, double* best2, int* nn, double* dist, unsigned char* resolved,
                             unsigned long long* examined, dmvs_stream_t stream) {
    if (!to_xyz || !ukeys || !ustart || !q_xyz || !best2 || !dist || !resolved || M < 1 || nq < 1 || rings < 0 || rings > 64 ||
        !(max_dist > 0.0) || !cloud_grid_ok(origin3, cell, dims3))
        return DMVS_EINVAL;
    CloudNNArgs a;
    a.to_xyz = to_xyz;
    a.ukeys = ukeys;
    a.ustart = ustart;
    a.M = M;
    a.g = cloud_grid(origin3, cell, dims3);
    a.q_xyz = q_xyz;
    a.q_idx = q_idx;
    a.nq = nq;
    a.rings = rings;
    a.max_dist = max_dist;
    a.best2 = best2;
    a.nn = nn;
    a.dist = dist;
    a.resolved = resolved;
    a.examined = examined;
    cloud_nn_kernel<<<ceil_div(nq, CLOUD_WG), CLOUD_WG, 0, (hipStream_t)stream>>>(a);
    DMVS_LAUNCH_CHECK();
}

extern "C" int dmvs_cloud_in_mask(const float* xyz, int n, const double* bb0, double res, const unsigned char* mask,
                                  const int* mask_dims3, unsigned char* out, dmvs_stream_t stream) {
    if (!xyz || !bb0 || !mask || !mask_dims3 || !out || n < 1 || !(res > 0.0) || mask_dims3[0] < 1 || mask_dims3[1] < 1 ||
        mask_dims3[2] < 1)
        return DMVS_EINVAL;
    const CloudMaskArgs a{xyz, n, bb0[0], bb0[1], bb0[2], res, mask, mask_dims3[0], mask_dims3[1], mask_dims3[2], out};
    cloud_in_mask_kernel<<<ceil_div(n, CLOUD_WG), CLOUD_WG, 0, (hipStream_t)stream>>>(a);
    DMVS_LAUNCH_CHECK();
}

extern "C" int dmvs_cloud_above_plane(const float* xyz, int n, const double* plane4, unsigned char* out, dmvs_stream_t stream) {
    if (!xyz || !plane4 || !out || n < 1) return DMVS_EINVAL;
    cloud_above_plane_kernel<<<ceil_div(n, CLOUD_WG), CLOUD_WG, 0, (hipStream_t)stream>>>(xyz, n, plane4[0], plane4[1], plane4[2], plane4[3], out);
    DMVS_LAUNCH_CHECK();
}

extern "C" int dmvs_cloud_in_box(const float* xyz, int n, const double* lo3, const double* hi3, unsigned char* out,
                                 dmvs_stream_t stream) {
    if (!xyz || !lo3 || !hi3 || !out || n < 1) return DMVS_EINVAL;
    cloud_in_box_kernel<<<ceil_div(n, CLOUD_WG), CLOUD_WG, 0, (hipStream_t)stream>>>(xyz, n, lo3[0], lo3[1], lo3[2], hi3[0], hi3[1], hi3[2], out);
    DMVS_LAUNCH_CHECK();
}
