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

// dSrc: every sample adds w_tap * (2/C) G Ref to its four taps with fp32 global atomics (return value unused: the
// no-return form).  blockIdx.z = (active view, quad group, chunk of DCH planes).  A tap outside the image is skipped,
// as ATen's grid_sample backward skips it; the clamped coordinates keep every address inside the gradient.  The order
// in which the atomics of different waves arrive is not fixed: the result is reproducible to fp32 rounding only
// (warp_corr_bwd_det.h is the order-free form of this kernel).
template <int NQ, int QPT, int DCH>
__global__ __launch_bounds__(kBwdTX * kBwdTY) void warp_corr_bwd_src_kernel(WarpBwdArgs a, int nqg, int nch) {
    const int x = blockIdx.x * kBwdTX + threadIdx.x, y = blockIdx.y * kBwdTY + threadIdx.y;
    const int z = blockIdx.z;
    const int chunk = z % nch, qg = (z / nch) % nqg, i = z / (nch * nqg);
    const int W = a.W, H = a.H;
    if (x >= W || y >= H) return;
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
    float* const Gs = a.gsrc[i] + (size_t)q0 * 4 * plane;
    const int dend = min((chunk + 1) * DCH, a.D);
    for (int d = chunk * DCH; d < dend; ++d) {
        const float depth = a.depth[(size_t)d * plane + pix];
        const float g0 = a.gsim[(size_t)d * plane + pix] * inv, g1 = a.gsim[(size_t)(a.D + d) * plane + pix] * inv;
        const RefTaps t = ref_order_taps(P, fx, fy, depth, wm1, hm1, half_w, half_h);
        const bool in00 = t.x0in && t.y0in, in01 = t.x1in && t.y0in, in10 = t.x0in && t.y1in, in11 = t.x1in && t.y1in;
        float* const p00 = Gs + t.y0 * W + t.x0;
        float* const p01 = Gs + t.y0 * W + t.x1;
        float* const p10 = Gs + t.y1 * W + t.x0;
        float* const p11 = Gs + t.y1 * W + t.x1;
#pragma unroll
        for (int q = 0; q < QPT; ++q) {
            const float gw[4] = {g0 * r[q].x, g1 * r[q].y, g0 * r[q].z, g1 * r[q].w};   // dL/dwarped of the quad
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t c = (size_t)(q * 4 + j) * plane;
                if (in00) atomicAdd(p00 + c, t.w00 * gw[j]);
                if (in01) atomicAdd(p01 + c, t.w01 * gw[j]);
                if (in10) atomicAdd(p10 + c, t.w10 * gw[j]);
                if (in11) atomicAdd(p11 + c, t.w11 * gw[j]);
            }
        }
    }
}

template <int NQ>
static int launch_warp_bwd(const WarpBwdArgs& a, hipStream_t st) {
    constexpr int QPT = 2, DCH = 8;
    const dim3 block(kBwdTX, kBwdTY);
    const int gx = ceil_div(a.W, kBwdTX), gy = ceil_div(a.H, kBwdTY), nqg = NQ / QPT;
    if (a.gref) {
        warp_corr_bwd_ref_kernel<NQ, QPT><<<dim3(gx, gy, nqg), block, 0, st>>>(a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    if (a.nact > 0) {
        const int nch = ceil_div(a.D, DCH);
        if ((long)a.nact * nqg * nch > 65535) return DMVS_EUNSUPPORTED;
        warp_corr_bwd_src_kernel<NQ, QPT, DCH><<<dim3(gx, gy, a.nact * nqg * nch), block, 0, st>>>(a, nqg, nch);
    }
    DMVS_LAUNCH_CHECK();
}

extern "C" int dmvs_warp_corr_backward(const float* ref_q4, const float* const* src_q4, int nsrc, const float* proj12,
                                       const float* depth_dhw, const float* gsim_2dhw, float* gref_chw,
                                       float* const* gsrc_chw, int C, int D, int H, int W, dmvs_stream_t stream) {
    if (!ref_q4 || !src_q4 || !proj12 || !depth_dhw || !gsim_2dhw) return DMVS_EINVAL;
    if (nsrc < 1 || nsrc > DMVS_MAX_SRC_VIEWS || D < 1 || H < 1 || W < 1) return DMVS_EINVAL;
    if ((long)H * W * C >= (1L << 29)) return DMVS_EUNSUPPORTED;   // 32-bit tap offsets
    WarpBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.ref = ref_q4;
    for (int v = 0; v < nsrc; ++v) {
        if (!src_q4[v]) return DMVS_EINVAL;
        a.src[v] = src_q4[v];
        if (gsrc_chw && gsrc_chw[v]) { a.gsrc[a.nact] = gsrc_chw[v]; a.view[a.nact] = v; ++a.nact; }
    }
    a.proj = proj12; a.depth = depth_dhw; a.gsim = gsim_2dhw; a.gref = gref_chw;
    a.nsrc = nsrc; a.D = D; a.H = H; a.W = W;
    hipStream_t st = (hipStream_t)stream;
    switch (C) {
        case 8: return launch_warp_bwd<2>(a, st);
        case 16: return launch_warp_bwd<4>(a, st);
        case 32: return launch_warp_bwd<8>(a, st);
        default: return DMVS_EUNSUPPORTED;
    }
}
