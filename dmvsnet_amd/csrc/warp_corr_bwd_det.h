// K1b, deterministic mode: the dSrc scatter of warp_corr_bwd.h with FIXED-POINT accumulation (included by warp_corr.hip, after
// warp_corr_bwd.h).  A sum of integers does not depend on its order, so the source-view gradients become a pure function of the
// inputs: independent of the arrival order of the atomics, of the grid decomposition and of which other views are asked for.
//
// The contract (docs/kernels/K1b_warp_corr_backward.md, "Deterministic mode"; tests/costagg_det_ref.py restates it on the CPU):
//   addend    t = w_tap * ((gsim * inv) * ref): the fp32 addend of warp_corr_bwd_src_kernel, same two fp32 products, no FMA
//   quantum   q = rint(t * 2^k) (int64): the product is exact in fp64 (a power of two), rint rounds to nearest even
//   sum       no-return 64-bit integer atomic add into an int64 workspace [nact][C][H][W], cleared on the stream by the entry
//   result    finalize WRITES every element of every wanted gsrc: (float)((double)sum * 2^-k) -- no zero fill by the caller
//   k         one per launch (= per sample):  eg = floor(log2(max |gsim|)) over [2][D][H][W], er the same over the reference
//             feature map; E = eg + er + 2 + log2(2 / C), so every |t| <= 2^E (rounding cannot cross a power of two);
//             L = ceil(log2(D H W)) (an element receives at most one tap per sample); k = min(62 - L, 50) - E.
//             No sum reaches 2^63, every |q| <= 2^50, the resolution is 2^-50 of the addend bound or better.
//   zero      a maximum of zero: k = 0, every element 0
//   NaN       a maximum that is not finite (or E > 127: an addend may overflow fp32): every element of every wanted gsrc is NaN
// The two maxima come from a pre-pass that takes max |x| on the unsigned bit patterns with the integer atomic max (order-free as
// well; the pattern of a NaN is above that of infinity, so the maximum tells both).  They live in the first two words of the
// first wanted gsrc, which is scratch until finalize writes it: no device state outside the caller's buffers, no host
// read-back, no synchronisation -- the path can be captured in a graph.  Finalize therefore runs as two launches of one
// kernel: every element but those two words (every workgroup still reads them), then the two.
#pragma once
#include <algorithm>

constexpr unsigned kDetInfBits = 0x7f800000u;

struct DetScale {
    int k;
    bool zero, bad;   // a maximum of zero / not finite
};

// floor(log2(x)) of a positive finite float given as its bit pattern (subnormals: bits * 2^-149)
__device__ __forceinline__ int det_floor_log2(unsigned bits) {
    return bits >= 0x00800000u ? (int)(bits >> 23) - 127 : (31 - __clz(bits)) - 149;
}

// mx: the pre-pass's two maxima (bit patterns, read as floats so that no load is typed differently from finalize's stores);
// kcap = min(62 - L, 50), lc = log2(2 / C)
__device__ __forceinline__ DetScale det_scale(const float* mx, int kcap, int lc) {
    const unsigned mg = __float_as_uint(mx[0]), mr = __float_as_uint(mx[1]);
    DetScale s;
    s.zero = mg == 0u || mr == 0u;
    s.bad = mg >= kDetInfBits || mr >= kDetInfBits;
    s.k = 0;
    if (!s.zero && !s.bad) {
        const int E = det_floor_log2(mg) + det_floor_log2(mr) + 2 + lc;
        s.k = kcap - E;
        s.bad = E > 127;
    }
    return s;
}

// max |x| of gsim (blockIdx.y = 0) and of the reference feature map (1) as unsigned bits: one integer atomic max per workgroup.
__global__ __launch_bounds__(256) void warp_corr_det_absmax_kernel(const float* gsim, size_t ng, const float* ref, size_t nr,
                                                                    unsigned* mx) {
    __shared__ unsigned part[4];
    const float* p = blockIdx.y ? ref : gsim;
    const size_t n = blockIdx.y ? nr : ng;
    unsigned m = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        m = max(m, __float_as_uint(p[i]) & 0x7fffffffu);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(part[0], part[1]), max(part[2], part[3]));
        if (m) atomicMax(mx + blockIdx.y, m);
    }
}

// The scatter: warp_corr_bwd_src_kernel's structure, tile and template parameters, addends formed the same way, added as int64.
// REV (variant 1): planes of a chunk walked in reverse and blockIdx.z mapped in reverse -- with another DCH a different
// decomposition of the same addends.
template <int NQ, int QPT, int DCH, bool REV>
__global__ __launch_bounds__(kBwdTX * kBwdTY) void warp_corr_det_src_kernel(WarpBwdArgs a, int nqg, int nch, long long* ws,
                                                                            const float* mx, int kcap, int lc) {
    const int x = blockIdx.x * kBwdTX + threadIdx.x, y = blockIdx.y * kBwdTY + threadIdx.y;
    const int z = REV ? (int)(gridDim.z - 1 - blockIdx.z) : (int)blockIdx.z;
    const int chunk = z % nch, qg = (z / nch) % nqg, i = z / (nch * nqg);
    const int W = a.W, H = a.H;
    if (x >= W || y >= H) return;
    const DetScale sc = det_scale(mx, kcap, lc);
    if (sc.zero || sc.bad) return;   // all zeros (the cleared workspace) / all NaN (finalize)
    const int v = a.view[i], q0 = qg * QPT;
    const size_t plane = (size_t)H * W, pix = (size_t)y * W + x;
    const float fx = (float)x, fy = (float)y;
    const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
    const float half_w = wm1 / 2.0f, half_h = hm1 / 2.0f;
    const float inv = 2.0f / (float)(NQ * 4);
    const float* P = a.proj + v * 12;
    float4_t r[QPT];
#pragma unroll
    for (int q = 0; q < QPT; ++q) r[q] = reinterpret_cast<const float4_t*>(a.ref)[(size_t)(q0 + q) * plane + pix];
    unsigned long long* const Gs = reinterpret_cast<unsigned long long*>(ws) + ((size_t)i * (NQ * 4) + (size_t)q0 * 4) * plane;
    const int dbeg = chunk * DCH, dend = min((chunk + 1) * DCH, a.D);
    for (int s = dbeg; s < dend; ++s) {
        const int d = REV ? dbeg + dend - 1 - s : s;
        const float depth = a.depth[(size_t)d * plane + pix];
        const float g0 = a.gsim[(size_t)d * plane + pix] * inv, g1 = a.gsim[(size_t)(a.D + d) * plane + pix] * inv;
        const RefTaps t = ref_order_taps(P, fx, fy, depth, wm1, hm1, half_w, half_h);
        const bool in00 = t.x0in && t.y0in, in01 = t.x1in && t.y0in, in10 = t.x0in && t.y1in, in11 = t.x1in && t.y1in;
        unsigned long long* const p00 = Gs + t.y0 * W + t.x0;
        unsigned long long* const p01 = Gs + t.y0 * W + t.x1;
        unsigned long long* const p10 = Gs + t.y1 * W + t.x0;
        unsigned long long* const p11 = Gs + t.y1 * W + t.x1;
#pragma unroll
        for (int q = 0; q < QPT; ++q) {
            const float gw[4] = {g0 * r[q].x, g1 * r[q].y, g0 * r[q].z, g1 * r[q].w};   // dL/dwarped of the quad
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t c = (size_t)(q * 4 + j) * plane;
                // t * 2^k is exact in fp64; |q| <= 2^50 by the choice of k
                if (in00) atomicAdd(p00 + c, (unsigned long long)__double2ll_rn(ldexp((double)(t.w00 * gw[j]), sc.k)));
                if (in01) atomicAdd(p01 + c, (unsigned long long)__double2ll_rn(ldexp((double)(t.w01 * gw[j]), sc.k)));
                if (in10) atomicAdd(p10 + c, (unsigned long long)__double2ll_rn(ldexp((double)(t.w10 * gw[j]), sc.k)));
                if (in11) atomicAdd(p11 + c, (unsigned long long)__double2ll_rn(ldexp((double)(t.w11 * gw[j]), sc.k)));
            }
        }
    }
}

// gsrc[view0 + blockIdx.y][e] = (float)((double)sum * 2^-k) for e in [lo, hi), lo = lo0 on the first wanted view and 0 on the
// others (the first launch leaves out the two words every workgroup reads, the second one writes them).
__global__ __launch_bounds__(256) void warp_corr_det_finalize_kernel(WarpBwdArgs a, const long long* ws, size_t per_view,
                                                                      size_t lo0, size_t hi, const float* mx, int kcap, int lc) {
    const int i = blockIdx.y;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x + (i == 0 ? lo0 : 0);
    const DetScale sc = det_scale(mx, kcap, lc);   // read before any store of this thread
    if (e >= hi) return;
    float out;
    if (sc.bad) out = __uint_as_float(0x7fc00000u);
    else out = (float)ldexp((double)ws[(size_t)i * per_view + e], -sc.k);
    a.gsrc[i][e] = out;
}

static int det_ceil_log2(unsigned long long n) {
    int l = 0;
    while ((1ull << l) < n) ++l;
    return l;
}

template <int NQ>
static int launch_warp_bwd_det(const WarpBwdArgs& a, long long* ws, int variant, hipStream_t st) {
    constexpr int QPT = 2, C = NQ * 4;
    const dim3 block(kBwdTX, kBwdTY);
    const int gx = ceil_div(a.W, kBwdTX), gy = ceil_div(a.H, kBwdTY), nqg = NQ / QPT;
    if (a.gref) {
        warp_corr_bwd_ref_kernel<NQ, QPT><<<dim3(gx, gy, nqg), block, 0, st>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    if (a.nact > 0) {
        const int nch = ceil_div(a.D, variant ? 4 : 8);
        if ((long)a.nact * nqg * nch > 65535) return DMVS_EUNSUPPORTED;
        const size_t plane = (size_t)a.H * a.W, per_view = (size_t)C * plane, ng = 2 * (size_t)a.D * plane;
        const int kcap = std::min(62 - det_ceil_log2((unsigned long long)a.D * plane), 50);
        const int lc = C == 8 ? -2 : C == 16 ? -3 : -4;
        float* const mx = a.gsrc[0];   // scratch until the last launch below
        hipError_t e = hipMemsetAsync(mx, 0, 2 * sizeof(unsigned), st);
        if (e == hipSuccess) e = hipMemsetAsync(ws, 0, (size_t)a.nact * per_view * sizeof(long long), st);
        if (e != hipSuccess) return (int)e;
        const unsigned nb = (unsigned)std::min((size_t)256, (std::max(ng, per_view) + 2047) / 2048);
        warp_corr_det_absmax_kernel<<<dim3(nb, 2), 256, 0, st>>>(a.gsim, ng, a.ref, per_view, reinterpret_cast<unsigned*>(mx));
        const dim3 grid(gx, gy, a.nact * nqg * nch);
        if (variant) warp_corr_det_src_kernel<NQ, QPT, 4, true><<<grid, block, 0, st>>>(a, nqg, nch, ws, mx, kcap, lc);
        else warp_corr_det_src_kernel<NQ, QPT, 8, false><<<grid, block, 0, st>>>(a, nqg, nch, ws, mx, kcap, lc);
        const unsigned fb = (unsigned)((per_view + 255) / 256);   // < 2^21: per_view < 2^29
        warp_corr_det_finalize_kernel<<<dim3(fb, a.nact), 256, 0, st>>>(a, ws, per_view, 2, per_view, mx, kcap, lc);
        warp_corr_det_finalize_kernel<<<dim3(1, 1), 256, 0, st>>>(a, ws, per_view, 0, 2, mx, kcap, lc);
    }
    DMVS_LAUNCH_CHECK();
}

extern "C" long dmvs_warp_corr_backward_det_workspace(int C, int H, int W, int nact) {
    if ((C != 8 && C != 16 && C != 32) || H < 1 || W < 1 || nact < 0 || nact > DMVS_MAX_SRC_VIEWS) return 0;
    return (long)sizeof(long long) * nact * C * H * W;
}

extern "C" int dmvs_warp_corr_backward_det(const float* ref_q4, const float* const* src_q4, int nsrc, const float* proj12,
                                           const float* depth_dhw, const float* gsim_2dhw, float* gref_chw,
                                           float* const* gsrc_chw, int C, int D, int H, int W, void* workspace,
                                           size_t workspace_bytes, int variant, dmvs_stream_t stream) {
    if (!ref_q4 || !src_q4 || !proj12 || !depth_dhw || !gsim_2dhw) return DMVS_EINVAL;
    if (nsrc < 1 || nsrc > DMVS_MAX_SRC_VIEWS || D < 1 || H < 1 || W < 1) return DMVS_EINVAL;
    if (variant != 0 && variant != 1) return DMVS_EINVAL;
    if (C != 8 && C != 16 && C != 32) return DMVS_EUNSUPPORTED;
    if ((long)H * W * C >= (1L << 29)) return DMVS_EUNSUPPORTED;   // 32-bit tap offsets
    WarpBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.ref = ref_q4;
    for (int v = 0; v < nsrc; ++v) {
        if (!src_q4[v]) return DMVS_EINVAL;
        a.src[v] = src_q4[v];
        if (gsrc_chw && gsrc_chw[v]) { a.gsrc[a.nact] = gsrc_chw[v]; a.view[a.nact] = v; ++a.nact; }
    }
    if (a.nact > 0) {
        if (!workspace || ((uintptr_t)workspace & 7)) return DMVS_EINVAL;
        if (workspace_bytes < (size_t)dmvs_warp_corr_backward_det_workspace(C, H, W, a.nact)) return DMVS_EINVAL;
    }
    a.proj = proj12; a.depth = depth_dhw; a.gsim = gsim_2dhw; a.gref = gref_chw;
    a.nsrc = nsrc; a.D = D; a.H = H; a.W = W;
    hipStream_t st = (hipStream_t)stream;
    long long* ws = static_cast<long long*>(workspace);
    switch (C) {
        case 8: return launch_warp_bwd_det<2>(a, ws, variant, st);
        case 16: return launch_warp_bwd_det<4>(a, ws, variant, st);
        default: return launch_warp_bwd_det<8>(a, ws, variant, st);
    }
}
