// The share scheme of the weight-gradient kernels (K3g, K3h, K2g, K3k, K3f; K3d walks its tiles the same way), written once: the tile
// grid, the shares, the walk, the partials' sum and the two launches.  Plain functions and one POD struct; no kernel lives here.
//
//   grid     persistent: at most 256 workgroups (one per CU) = `blocks` operand blocks of the family x S voxel shares,
//            S = min(tiles, 256 / blocks).  The tile list runs x fastest, then y, then z (or the plane); share s walks its contiguous
//            range [s * tiles / S, (s + 1) * tiles / S), so every tile -- and with it every voxel -- is in exactly one share and no
//            share is empty.  The launch is padded to xcd_grid (common.h) and un-mapped again: workgroup blockIdx.x takes the place
//            wg = (blockIdx.x & 7) * per + (blockIdx.x >> 3), per = ceil(nwg / 8), so XCD k gets the k-th eighth of the places; a place
//            past nwg is idle, the others are wg = s * blocks + block.  A tile is tile % a.nx, (tile / a.nx) % a.ny, tile / (a.nx * a.ny)
//            of the family's own `Args a`.
//   sums     three levels, all in a fixed order: a tile is ONE chain from zero; the tiles of a share are added to the share's running
//            sum one after the other in walk order; the S partials go to a workspace of FIXED size (256 / blocks partials, whatever the
//            volume) and a second kernel adds them in the order s = 0 .. S - 1 (and then onto the gradient with `accumulate`).
//            No atomics anywhere: the result is bitwise reproducible.
//   plan     the host-only `_plan` entries return tiles * 512 + xcd_grid(nwg): the tile count must stay below 2^22.
#pragma once
#include "common.h"

namespace wshare {

constexpr int kMaxWg = 256;   // one workgroup per CU

struct Grid {
    int nx, ny, ntiles;   // tile grid: nx * ny * D tiles
    int S, nwg;           // voxel shares; workgroups with work = S * blocks
};

// the tile grid of ty x tx tiles over D planes of rows x cols and its shares; false: an extent < 1 or 2^22 tiles and more
inline bool grid(int D, int rows, int cols, int ty, int tx, int blocks, Grid& g) {
    if (D < 1 || rows < 1 || cols < 1) return false;
    g.nx = ceil_div(cols, tx); g.ny = ceil_div(rows, ty);
    const long nt = (long)g.nx * g.ny * D;
    if (nt >= (1L << 22)) return false;   // the plan packs the tile count into 22 bits (indices are 64-bit throughout)
    g.ntiles = (int)nt;
    const int smax = kMaxWg / blocks;
    g.S = g.ntiles < smax ? g.ntiles : smax;
    g.nwg = g.S * blocks;
    return true;
}

inline int plan(const Grid& g) { return g.ntiles * 512 + (int)xcd_grid(g.nwg); }
inline long workspace(int blocks, long n) { return (long)(kMaxWg / blocks) * n; }   // one partial of n floats per share

// the place of workgroup `bid` of the xcd_grid launch: s * blocks + block, or -1 for an idle one
__host__ __device__ inline int place(const Grid& g, unsigned bid) {
    const int per = (g.nwg + 7) >> 3;
    const int wg = (bid & 7) * per + (bid >> 3);
    return wg < g.nwg ? wg : -1;
}

// share s walks the tiles [first_tile(g, s), first_tile(g, s + 1))
__host__ __device__ inline int first_tile(const Grid& g, int s) { return (int)((long)s * g.ntiles / g.S); }

struct Tile { int bx, by, z; };
__host__ __device__ inline Tile decode(const Grid& g, int tile) {
    const int rr = tile / g.nx;
    return {tile % g.nx, rr % g.ny, rr / g.ny};
}

// dst[c][TY][TX] (channel stride `stride`) = src[c0 + c][z][y0 ..][x0 ..] of a tensor [.][.][H][W], zeros outside the plane and for
// c >= cmax: the dY / coarse tile of K3g, K3h, K3k and K3f.  Walks x fastest; no global address is formed outside the tensor.
template <int ROWS, int TY, int TX>
__device__ __forceinline__ void stage_rows(float* dst, int stride, const float* src, int c0, int cmax, size_t vol, size_t plane, int z,
                                           int y0, int x0, int H, int W, int tid) {
    for (int i = tid; i < ROWS * TY * TX; i += 256) {
        const int c = i / (TY * TX), r = i % (TY * TX), y = y0 + r / TX, x = x0 + r % TX;
        float v = 0.f;
        if (c < cmax && y < H && x < W) v = src[(size_t)(c0 + c) * vol + z * plane + (size_t)y * W + x];
        dst[c * stride + r] = v;
    }
}

// out (+)= sum_{s = 0 .. S-1} ws[s][e], s ascending, for element e = this thread of the n in a partial; map(e) is where it goes, or null
template <class Map>
__device__ __forceinline__ void reduce(const float* __restrict__ ws, int n, int S, int accumulate, Map map) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float sum = ws[e];
    for (int s = 1; s < S; ++s) sum += ws[(size_t)s * n + e];
    if (float* o = map(e)) *o = accumulate ? *o + sum : sum;
}

// the map of K3g, K3h and K3k: ws[tap][a][b] -> gw[a][b][tap]
__device__ __forceinline__ float* tap_last(float* gw, int e, int A, int B, int NT) {
    const int t = e / (A * B), ca = (e / B) % A, cb = e % B;
    return gw + ((size_t)ca * B + cb) * NT + t;
}

// the two launches: the partials on the padded grid (lds bytes of dynamic LDS, 0: none), then the reduce over n elements
template <class Args, class... RP, class... RA>
int launch(void (*kernel)(Args), const Args& a, size_t lds, hipStream_t st, void (*reduce_kernel)(RP...), int n, RA... ra) {
    if (lds)
        if (int e = dmvs_ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), lds)) return e;
    kernel<<<dim3(xcd_grid(a.g.nwg)), 256, lds, st>>>(a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    reduce_kernel<<<dim3(ceil_div(n, 256)), 256, 0, st>>>(ra...);
    DMVS_LAUNCH_CHECK();
}

}  // namespace wshare
