// K1b, deterministic mode: the dSrc scatter of warp_corr_bwd.h with FIXED-POINT accumulation (included by warp_corr_bwd.h, between
// its kernels and its launcher; the scatter loop, the launcher and the entry are there).  A sum of integers does not depend on its order, so the source-view gradients become a pure function of the
// inputs: independent of the arrival order of the atomics, of the grid decomposition and of which other views are asked for.
//
// The contract (docs/kernels/K1b_warp_corr_backward.md, "Deterministic mode"; tests/costagg_det_ref.py restates it on the CPU):
//   addend    t = w_tap * ((gsim * inv) * ref): formed once in the body of warp_corr_bwd_src_kernel, which hands the same fp32
//             number to the default sink and to this one (two fp32 products, no FMA)
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

// The order-free sink of warp_corr_bwd_src_kernel: the shared body's fp32 addend t joins an int64 workspace [nact][C][H][W] as
// rint(t * 2^k).  t * 2^k is exact in fp64; |q| <= 2^50 by the choice of k.
struct FixedSink {
    long long* ws;
    const float* mx;
    int kcap, lc;
    using Scale = DetScale;
    __device__ __forceinline__ Scale scale() const { return det_scale(mx, kcap, lc); }
    // all zeros (the cleared workspace) / all NaN (finalize)
    __device__ __forceinline__ static bool idle(const Scale& sc) { return sc.zero || sc.bad; }
    __device__ __forceinline__ unsigned long long* dest(const WarpBwdArgs&, int i, size_t per_view) const {
        return reinterpret_cast<unsigned long long*>(ws) + (size_t)i * per_view;
    }
    // the pre-summed scatter (warp_corr_bwd_presum.h) sums the SAME q in LDS first and adds each sum once
    using Acc = unsigned long long;
    __device__ __forceinline__ static Acc quant(float t, const Scale& sc) {
        return (unsigned long long)__double2ll_rn(ldexp((double)t, sc.k));
    }
    __device__ __forceinline__ static void add(unsigned long long* p, float t, const Scale& sc) { atomicAdd(p, quant(t, sc)); }
    __device__ __forceinline__ static void flush(unsigned long long* p, Acc s, const Scale&) { atomicAdd(p, s); }
};

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

extern "C" long dmvs_warp_corr_backward_det_workspace(int C, int H, int W, int nact) {
    if ((C != 8 && C != 16 && C != 32) || H < 1 || W < 1 || nact < 0 || nact > DMVS_MAX_SRC_VIEWS) return 0;
    return (long)sizeof(long long) * nact * C * H * W;
}
