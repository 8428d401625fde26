// K1b: backward of the fused warp + correlation (included by warp_corr.hip, after ref_order_taps).
//
// Differentiates CostAgg.forward (networks/mvsnet.py:111-153) over homo_warping (networks/module.py:212-251) with
// respect to the FEATURE MAPS only: the reference builds the sampling grid under torch.no_grad() (module.py:222-243), so
// no gradient reaches the cameras or the depth hypotheses.  With G = dL/dsim [2][D][H][W] and W_v = source view v
// sampled bilinearly (zeros padding, align_corners=True):
//   dRef[c][y][x]          = (2/C) sum_v sum_d G[c & 1][d][y][x] * W_v[c][d][y][x]           -- a gather
//   dSrc_v[c][tap(yy,xx)] += w_tap * (2/C) * G[c & 1][d][y][x] * Ref[c][y][x]                -- a scatter over 4 taps
// Neither the [C][D][H][W] warped volume nor the [D][H][W][2] grid that autograd keeps per source view exists here: both
// kernels recompute the taps with the generic forward's routine (ref_order_taps, the reference's op order).
//
// Features are read quad-planar [C/4][H][W][4] (what the differentiable forward saved), gradients are written planar
// [C][H][W] (what autograd hands to the feature maps' producers).  A lane owns a pixel, 64 lanes along x: in the planar
// gradient one wave instruction per (channel, tap) touches ~256 contiguous bytes -- the shape the float atomics want.
#pragma once

struct WarpBwdArgs {
    const float* ref;                        // [C/4][H][W][4]
    const float* src[DMVS_MAX_SRC_VIEWS];    // [C/4][H][W][4] each
    const float* proj;                       // [nsrc][12]
    const float* depth;                      // [D][H][W]
    const float* gsim;                       // [2][D][H][W]
    float* gref;                             // [C][H][W], every element written
    float* gsrc[DMVS_MAX_SRC_VIEWS];         // [C][H][W] each, zero-initialised by the caller; compacted: entry i belongs
    int view[DMVS_MAX_SRC_VIEWS];            //   to source view view[i] (views whose gradient is not wanted are left out)
    int nsrc, nact, D, H, W;
};

constexpr int kBwdTX = 64, kBwdTY = 4;   // one wave per tile row

// dRef: registers accumulate QPT channel quads of one pixel over every (view, plane); plain stores, no atomics ->
// bitwise reproducible.  blockIdx.z = quad group.
template <int NQ, int QPT>
__global__ __launch_bounds__(kBwdTX * kBwdTY) void warp_corr_bwd_ref_kernel(WarpBwdArgs a) {
    const int x = blockIdx.x * kBwdTX + threadIdx.x, y = blockIdx.y * kBwdTY + threadIdx.y;
    const int q0 = blockIdx.z * QPT;
    const int W = a.W, H = a.H;
    if (x >= W || y >= H) return;
    const size_t plane = (size_t)H * W, pix = (size_t)y * W + x;
    const float fx = (float)x, fy = (float)y;
    const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
    const float half_w = wm1 / 2.0f, half_h = hm1 / 2.0f;
    const float inv = 2.0f / (float)(NQ * 4);   // mean over the C/2 channels of a group (a power of two: exact)
    float4_t acc[QPT];
#pragma unroll
    for (int q = 0; q < QPT; ++q) acc[q] = float4_t{0.f, 0.f, 0.f, 0.f};
    for (int v = 0; v < a.nsrc; ++v) {
        const float* P = a.proj + v * 12;   // uniform -> scalar loads
        const float4_t* S = reinterpret_cast<const float4_t*>(a.src[v]) + (size_t)q0 * plane;
        for (int d = 0; d < a.D; ++d) {
            const float depth = a.depth[(size_t)d * plane + pix];
            const float g0 = a.gsim[(size_t)d * plane + pix] * inv, g1 = a.gsim[(size_t)(a.D + d) * plane + pix] * inv;
            const RefTaps t = ref_order_taps(P, fx, fy, depth, wm1, hm1, half_w, half_h);
            const int o00 = t.y0 * W + t.x0, o01 = t.y0 * W + t.x1, o10 = t.y1 * W + t.x0, o11 = t.y1 * W + t.x1;
#pragma unroll
            for (int q = 0; q < QPT; ++q) {
                const float4_t* Sq = S + (size_t)q * plane;
                const float4_t s00 = Sq[o00], s01 = Sq[o01], s10 = Sq[o10], s11 = Sq[o11];
                // the warped feature, taps in ATen's order (nw, ne, sw, se)
                const float4_t wv = {fmaf(t.w11, s11.x, fmaf(t.w10, s10.x, fmaf(t.w01, s01.x, t.w00 * s00.x))),
                                     fmaf(t.w11, s11.y, fmaf(t.w10, s10.y, fmaf(t.w01, s01.y, t.w00 * s00.y))),
                                     fmaf(t.w11, s11.z, fmaf(t.w10, s10.z, fmaf(t.w01, s01.z, t.w00 * s00.z))),
                                     fmaf(t.w11, s11.w, fmaf(t.w10, s10.w, fmaf(t.w01, s01.w, t.w00 * s00.w)))};
                acc[q].x = fmaf(g0, wv.x, acc[q].x);   // even channels -> group 0, odd channels -> group 1
                acc[q].y = fmaf(g1, wv.y, acc[q].y);
                acc[q].z = fmaf(g0, wv.z, acc[q].z);
                acc[q].w = fmaf(g1, wv.w, acc[q].w);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < QPT; ++q) {
        float* o = a.gref + (size_t)(q0 + q) * 4 * plane + pix;
        o[0] = acc[q].x;
        o[plane] = acc[q].y;
        o[2 * plane] = acc[q].z;
        o[3 * plane] = acc[q].w;
    }
}

// dSrc: every sample adds t = w_tap * (2/C) G Ref to its four taps through a sink policy, which says whether the thread has
// anything to do, where active view i's destination starts and how one fp32 addend joins it.  The addend is formed HERE, once,
// from two fp32 products (no FMA): both sinks accumulate the same numbers.  blockIdx.z = (active view, quad group, chunk of
// DCH planes).  A tap outside the image is skipped, as ATen's grid_sample backward skips it; the clamped coordinates keep every
// address inside the destination.  REV: planes of a chunk walked in reverse and blockIdx.z mapped in reverse (a different
// decomposition of the same addends, for the order-free sink's tests).
template <int NQ, int QPT, int DCH, bool REV, class Sink>
__global__ __launch_bounds__(kBwdTX * kBwdTY) void warp_corr_bwd_src_kernel(WarpBwdArgs a, int nqg, int nch, Sink sink) {
    const int x = blockIdx.x * kBwdTX + threadIdx.x, y = blockIdx.y * kBwdTY + threadIdx.y;
    const int z = REV ? (int)(gridDim.z - 1 - blockIdx.z) : (int)blockIdx.z;
    const int chunk = z % nch, qg = (z / nch) % nqg, i = z / (nch * nqg);
    const int W = a.W, H = a.H;
    if (x >= W || y >= H) return;
    const typename Sink::Scale sc = sink.scale();
    if (Sink::idle(sc)) return;
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
    auto* const Gs = sink.dest(a, i, (size_t)(NQ * 4) * plane) + (size_t)q0 * 4 * plane;
    const int dbeg = chunk * DCH, dend = min((chunk + 1) * DCH, a.D);
    for (int s = dbeg; s < dend; ++s) {
        const int d = REV ? dbeg + dend - 1 - s : s;
        const float depth = a.depth[(size_t)d * plane + pix];
        const float g0 = a.gsim[(size_t)d * plane + pix] * inv, g1 = a.gsim[(size_t)(a.D + d) * plane + pix] * inv;
        const RefTaps t = ref_order_taps(P, fx, fy, depth, wm1, hm1, half_w, half_h);
        const bool in00 = t.x0in && t.y0in, in01 = t.x1in && t.y0in, in10 = t.x0in && t.y1in, in11 = t.x1in && t.y1in;
        auto* const p00 = Gs + t.y0 * W + t.x0;
        auto* const p01 = Gs + t.y0 * W + t.x1;
        auto* const p10 = Gs + t.y1 * W + t.x0;
        auto* const p11 = Gs + t.y1 * W + t.x1;
#pragma unroll
        for (int q = 0; q < QPT; ++q) {
            const float gw[4] = {g0 * r[q].x, g1 * r[q].y, g0 * r[q].z, g1 * r[q].w};   // dL/dwarped of the quad
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t c = (size_t)(q * 4 + j) * plane;
                if (in00) Sink::add(p00 + c, t.w00 * gw[j], sc);
                if (in01) Sink::add(p01 + c, t.w01 * gw[j], sc);
                if (in10) Sink::add(p10 + c, t.w10 * gw[j], sc);
                if (in11) Sink::add(p11 + c, t.w11 * gw[j], sc);
            }
        }
    }
}

// The default sink: fp32 global atomics (return value unused: the no-return form) into the caller's zero-initialised gsrc.  The
// order in which the atomics of different waves arrive is not fixed: the result is reproducible to fp32 rounding only
// (FixedSink, warp_corr_bwd_det.h, is the order-free one).
struct AtomicSink {
    struct Scale {};
    __device__ __forceinline__ Scale scale() const { return {}; }
    __device__ __forceinline__ static bool idle(Scale) { return false; }
    __device__ __forceinline__ float* dest(const WarpBwdArgs& a, int i, size_t) const { return a.gsrc[i]; }
    __device__ __forceinline__ static void add(float* p, float t, Scale) { atomicAdd(p, t); }
    // the pre-summed scatter (warp_corr_bwd_presum.h): what a window element holds, what an addend joins it as, one sum's global add
    using Acc = float;
    __device__ __forceinline__ static Acc quant(float t, Scale) { return t; }
    __device__ __forceinline__ static void flush(float* p, Acc s, Scale) { atomicAdd(p, s); }
};

// the deterministic mode's scale, pre-pass, sink and finalize; needs WarpBwdArgs, needed by the launcher
#include "warp_corr_bwd_det.h"
// the pre-summed form of the scatter; needs both sinks, needed by the launcher
#include "warp_corr_bwd_presum.h"

// ws: null for the default mode, else the deterministic mode's workspace (variant bit 0: its decomposition).  ps: null for the plain
// scatter, else the pre-summed one in the same mode (variant bit 1: its test capacity).
template <int NQ>
static int launch_warp_bwd(const WarpBwdArgs& a, long long* ws, int variant, const WarpBwdPresum* ps, hipStream_t st) {
    constexpr int QPT = 2, C = NQ * 4;
    const dim3 block(kBwdTX, kBwdTY);
    const int gx = ceil_div(a.W, kBwdTX), gy = ceil_div(a.H, kBwdTY), nqg = NQ / QPT;
    if (a.gref) {
        warp_corr_bwd_ref_kernel<NQ, QPT><<<dim3(gx, gy, nqg), block, 0, st>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    if (a.nact > 0) {
        const int nch = ceil_div(a.D, (variant & 1) ? 4 : 8);
        if ((long)a.nact * nqg * nch > 65535) return DMVS_EUNSUPPORTED;
        const dim3 grid(gx, gy, a.nact * nqg * nch);
        if (!ws) {
            if (ps) launch_presum_scatter<NQ, QPT>(a, grid, block, nqg, nch, AtomicSink{}, variant, *ps, st);
            else warp_corr_bwd_src_kernel<NQ, QPT, 8, false><<<grid, block, 0, st>>>(a, nqg, nch, AtomicSink{});
        } else {
            const size_t plane = (size_t)a.H * a.W, per_view = (size_t)C * plane, ng = 2 * (size_t)a.D * plane;
            const int kcap = std::min(62 - det_ceil_log2((unsigned long long)a.D * plane), 50);
            const int lc = C == 8 ? -2 : C == 16 ? -3 : -4;
            float* const mx = a.gsrc[0];   // scratch until the last launch below
            hipError_t e = hipMemsetAsync(mx, 0, 2 * sizeof(unsigned), st);
            if (e == hipSuccess) e = hipMemsetAsync(ws, 0, (size_t)a.nact * per_view * sizeof(long long), st);
            if (e != hipSuccess) return (int)e;
            const unsigned nb = (unsigned)std::min((size_t)256, (std::max(ng, per_view) + 2047) / 2048);
            warp_corr_det_absmax_kernel<<<dim3(nb, 2), 256, 0, st>>>(a.gsim, ng, a.ref, per_view, reinterpret_cast<unsigned*>(mx));
            const FixedSink sink{ws, mx, kcap, lc};
            if (ps) launch_presum_scatter<NQ, QPT>(a, grid, block, nqg, nch, sink, variant, *ps, st);
            else if (variant) warp_corr_bwd_src_kernel<NQ, QPT, 4, true><<<grid, block, 0, st>>>(a, nqg, nch, sink);
            else warp_corr_bwd_src_kernel<NQ, QPT, 8, false><<<grid, block, 0, st>>>(a, nqg, nch, sink);
            const unsigned fb = (unsigned)((per_view + 255) / 256);   // < 2^21: per_view < 2^29
            warp_corr_det_finalize_kernel<<<dim3(fb, a.nact), 256, 0, st>>>(a, ws, per_view, 2, per_view, mx, kcap, lc);
            warp_corr_det_finalize_kernel<<<dim3(1, 1), 256, 0, st>>>(a, ws, per_view, 0, 2, mx, kcap, lc);
        }
    }
    DMVS_LAUNCH_CHECK();
}

// The public entries.  det: the deterministic mode, which needs an 8-byte aligned workspace of
// dmvs_warp_corr_backward_det_workspace() bytes once a source gradient is wanted, and a variant of 0 or 1.  ps: the pre-summed
// scatter in either mode (variant 0..3), null for the plain one.
static int warp_corr_bwd_entry(bool det, const WarpBwdPresum* ps, const float* ref_q4, const float* const* src_q4, int nsrc,
                               const float* proj12, const float* depth_dhw, const float* gsim_2dhw, float* gref_chw,
                               float* const* gsrc_chw, int C, int D, int H, int W, void* workspace, size_t workspace_bytes, int variant,
                               dmvs_stream_t stream) {
    if (!ref_q4 || !src_q4 || !proj12 || !depth_dhw || !gsim_2dhw) return DMVS_EINVAL;
    if (nsrc < 1 || nsrc > DMVS_MAX_SRC_VIEWS || D < 1 || H < 1 || W < 1) return DMVS_EINVAL;
    if (ps ? (variant < 0 || variant > 3) : (det && variant != 0 && variant != 1)) return DMVS_EINVAL;
    if (C != 8 && C != 16 && C != 32) return DMVS_EUNSUPPORTED;
    if ((long)H * W * C >= (1L << 29)) return DMVS_EUNSUPPORTED;   // 32-bit tap offsets
    WarpBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.ref = ref_q4;
    if (!copy_view_ptrs(a.src, src_q4, nsrc)) return DMVS_EINVAL;
    for (int v = 0; v < nsrc; ++v)   // compaction: views whose gradient is not wanted are left out
        if (gsrc_chw && gsrc_chw[v]) { a.gsrc[a.nact] = gsrc_chw[v]; a.view[a.nact] = v; ++a.nact; }
    if (det && a.nact > 0) {
        if (!workspace || ((uintptr_t)workspace & 7)) return DMVS_EINVAL;
        if (workspace_bytes < (size_t)dmvs_warp_corr_backward_det_workspace(C, H, W, a.nact)) return DMVS_EINVAL;
    }
    a.proj = proj12; a.depth = depth_dhw; a.gsim = gsim_2dhw; a.gref = gref_chw;
    a.nsrc = nsrc; a.D = D; a.H = H; a.W = W;
    hipStream_t st = (hipStream_t)stream;
    long long* ws = det && a.nact > 0 ? static_cast<long long*>(workspace) : nullptr;
    switch (C) {
        case 8: return launch_warp_bwd<2>(a, ws, variant, ps, st);
        case 16: return launch_warp_bwd<4>(a, ws, variant, ps, st);
        default: return launch_warp_bwd<8>(a, ws, variant, ps, st);
    }
}

extern "C" int dmvs_warp_corr_backward(const float* ref_q4, const float* const* src_q4, int nsrc, const float* proj12,
                                       const float* depth_dhw, const float* gsim_2dhw, float* gref_chw,
                                       float* const* gsrc_chw, int C, int D, int H, int W, dmvs_stream_t stream) {
    return warp_corr_bwd_entry(false, nullptr, ref_q4, src_q4, nsrc, proj12, depth_dhw, gsim_2dhw, gref_chw, gsrc_chw, C, D, H, W,
                               nullptr, 0, 0, stream);
}

extern "C" int dmvs_warp_corr_backward_det(const float* ref_q4, const float* const* src_q4, int nsrc, const float* proj12,
                                           const float* depth_dhw, const float* gsim_2dhw, float* gref_chw,
                                           float* const* gsrc_chw, int C, int D, int H, int W, void* workspace,
                                           size_t workspace_bytes, int variant, dmvs_stream_t stream) {
    return warp_corr_bwd_entry(true, nullptr, ref_q4, src_q4, nsrc, proj12, depth_dhw, gsim_2dhw, gref_chw, gsrc_chw, C, D, H, W,
                               workspace, workspace_bytes, variant, stream);
}

// K1b with the pre-summed scatter (warp_corr_bwd_presum.h) in place of the plain one: the same part of the reference as the two
// entries above -- the backward autograd records for CostAgg.forward (mvsnet.py:111-153) over homo_warping (module.py:212-251).
extern "C" int dmvs_warp_corr_backward_presum(const float* ref_q4, const float* const* src_q4, int nsrc, const float* proj12,
                                              const float* depth_dhw, const float* gsim_2dhw, float* gref_chw,
                                              float* const* gsrc_chw, int C, int D, int H, int W, int det, void* workspace,
                                              size_t workspace_bytes, int variant, unsigned* path_counts, dmvs_stream_t stream) {
    const WarpBwdPresum ps{path_counts};
    return warp_corr_bwd_entry(det != 0, &ps, ref_q4, src_q4, nsrc, proj12, depth_dhw, gsim_2dhw, gref_chw, gsrc_chw, C, D, H, W,
                               workspace, workspace_bytes, variant, stream);
}
