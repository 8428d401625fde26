// K4b: backward of the dual-depth regression (K4, depth_regress.hip) -- device code, included at the end of depth_regress.hip.
//
// Replaces what autograd runs behind DepthNet.forward / .refine (mvsnet.py:15-100, module.py:454-460): a kept softmax volume
// [4][D][H][W], the product p * depth of the same size and ~60 plane-sized intermediates per pass.  Nothing is kept here: the
// softmax is recomputed from the logits in the forward kernel's operation order (max, exp, sum in plane order, e / s), and the
// min / max routing is taken from the forward's dsp, so forward and backward agree on the selected channel bit for bit.
//
//   G[c]        = g_dsp[c] + what g_sel sends to expectation c through (min, max) of its pair and the checkerboard cases
//   g_logits    = alpha * p[c][d] * (hyp[d] - E[c]) * G[c]
//   g_hyp[d]    = ((p[0][d] G[0] + p[1][d] G[1]) + p[2][d] G[2]) + p[3][d] G[3]
//
// HBM-bound: one read and one write of [4][D][H][W].  Same shapes as the forward (docs/kernels/K4_depth_regress.md): lane = pixel
// along x, one thread per pixel with the logits in registers for D = 4 / 8, channel-per-wave for D = 32 / 48 / 64 (the main
// passes, which need no g_hyp: their hypotheses come from a detached depth).  Plain stores, one writer per element.
#pragma once
#include "common.h"

// Upstream gradient on the four expectations of a pixel.  The six-stack of mode 0 is (3 - t) lo + (t - 2) hi for t = 0..5
// (3lo-2hi, 2lo-hi, lo, hi, 2hi-lo, 3hi-2lo); rows with y % 4 >= 2 use lo' = 2 lo - hi, hi' = 2 hi - lo.  min / max: the channel
// fminf / fmaxf returned in regress_tail (a tie sends both to channel 0 of the pair, as torch's min / max over a dim do).
__device__ __forceinline__ void regress_bwd_fold(const float (&e4)[4], const float* __restrict__ g_dsp, const float* __restrict__ g_sel,
                                                 int mode, int x, int y, size_t plane, size_t pix, float (&G)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c) G[c] = g_dsp ? g_dsp[c * plane + pix] : 0.f;
    if (!g_sel) return;
    float glo = 0.f, ghi = 0.f;
    int pair;
    if (mode == 1) {
        // (row%2, col%2): (0,0) small_min, (0,1) small_max, (1,0) huge_max, (1,1) huge_min
        const int r = y & 1, c = x & 1;
        const float g = g_sel[pix];
        pair = r;
        if ((r ^ c) == 0) glo = g; else ghi = g;
    } else {
        const int q = y & 3;
        pair = q & 1;
        const int off = ((y + x) & 1) ? 2 : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float g = g_sel[k * plane + pix];
            const int t = k + off;
            glo += g * (float)(3 - t);
            ghi += g * (float)(t - 2);
        }
        if (q >= 2) { const float l2 = 2.f * glo - ghi, h2 = 2.f * ghi - glo; glo = l2; ghi = h2; }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (pair != p) continue;
        const bool min1 = e4[2 * p + 1] < e4[2 * p], max1 = e4[2 * p + 1] > e4[2 * p];
        G[2 * p] += (min1 ? 0.f : glo) + (max1 ? 0.f : ghi);
        G[2 * p + 1] += (min1 ? glo : 0.f) + (max1 ? ghi : 0.f);
    }
}

// One thread per pixel, all four channels.  DREG > 0: D == DREG, the logits of a channel stay in registers; DREG == 0: any D,
// three sweeps as the forward's generic kernel (the re-reads hit L2).
template <int DREG>
__global__ __launch_bounds__(256) void depth_regress_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ hyp,
                                                                float alpha, int mode, int D, int H, int W,
                                                                const float* __restrict__ dsp, const float* __restrict__ g_dsp,
                                                                const float* __restrict__ g_sel, float* __restrict__ g_logits,
                                                                float* __restrict__ g_hyp) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= W) return;
    const size_t plane = (size_t)H * W;
    const size_t pix = (size_t)y * W + x;
    const size_t cstride = (size_t)D * plane;
    const float e4[4] = {dsp[pix], dsp[plane + pix], dsp[2 * plane + pix], dsp[3 * plane + pix]};
    float G[4];
    regress_bwd_fold(e4, g_dsp, g_sel, mode, x, y, plane, pix, G);

    if constexpr (DREG > 0) {
        float dep[DREG], gh[DREG];
#pragma unroll
        for (int d = 0; d < DREG; ++d) { dep[d] = hyp[d * plane + pix]; gh[d] = 0.f; }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float v[DREG];
#pragma unroll
            for (int d = 0; d < DREG; ++d) v[d] = logits[c * cstride + d * plane + pix] * alpha;
            float m = -INFINITY, s = 0.f;
#pragma unroll
            for (int d = 0; d < DREG; ++d) m = fmaxf(m, v[d]);
#pragma unroll
            for (int d = 0; d < DREG; ++d) { v[d] = expf(v[d] - m); s += v[d]; }
#pragma unroll
            for (int d = 0; d < DREG; ++d) {
                const float p = v[d] / s;
                g_logits[c * cstride + d * plane + pix] = alpha * p * (dep[d] - e4[c]) * G[c];
                gh[d] += p * G[c];
            }
        }
        if (g_hyp) {
#pragma unroll
            for (int d = 0; d < DREG; ++d) g_hyp[d * plane + pix] = gh[d];
        }
    } else {
        float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        for (int d = 0; d < D; ++d) {
#pragma unroll
            for (int c = 0; c < 4; ++c) m[c] = fmaxf(m[c], logits[c * cstride + d * plane + pix] * alpha);
        }
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int d = 0; d < D; ++d) {
#pragma unroll
            for (int c = 0; c < 4; ++c) s[c] += expf(logits[c * cstride + d * plane + pix] * alpha - m[c]);
        }
        for (int d = 0; d < D; ++d) {
            const float dep = hyp[d * plane + pix];
            float gh = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float p = expf(logits[c * cstride + d * plane + pix] * alpha - m[c]) / s[c];
                g_logits[c * cstride + d * plane + pix] = alpha * p * (dep - e4[c]) * G[c];
                gh += p * G[c];
            }
            if (g_hyp) g_hyp[d * plane + pix] = gh;
        }
    }
}

// Channel-per-wave form of the large-D main passes (no g_hyp): a workgroup owns 64 pixels, wave c owns channel c of them with its
// D logits in registers, every load and store a 256-byte run.  The channels are independent once G is known; each wave folds the
// pixel's G from the twelve planes itself (the other three waves' reads of the same lines hit the cache) and keeps its own.
template <int DREG>
__global__ __launch_bounds__(256) void depth_regress_bwd_split_kernel(const float* __restrict__ logits, const float* __restrict__ hyp,
                                                                      float alpha, int mode, int H, int W,
                                                                      const float* __restrict__ dsp, const float* __restrict__ g_dsp,
                                                                      const float* __restrict__ g_sel, float* __restrict__ g_logits) {
    const int lane = threadIdx.x & 63, c = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + lane, y = blockIdx.y;
    if (x >= W) return;
    const size_t plane = (size_t)H * W;
    const size_t pix = (size_t)y * W + x;
    const size_t base = (size_t)c * DREG * plane + pix;
    const float e4[4] = {dsp[pix], dsp[plane + pix], dsp[2 * plane + pix], dsp[3 * plane + pix]};
    float G[4];
    regress_bwd_fold(e4, g_dsp, g_sel, mode, x, y, plane, pix, G);
    const float Gc = c == 0 ? G[0] : (c == 1 ? G[1] : (c == 2 ? G[2] : G[3]));
    const float Ec = c == 0 ? e4[0] : (c == 1 ? e4[1] : (c == 2 ? e4[2] : e4[3]));
    float v[DREG];
#pragma unroll
    for (int d = 0; d < DREG; ++d) v[d] = logits[base + d * plane] * alpha;
    float m = -INFINITY, s = 0.f;
#pragma unroll
    for (int d = 0; d < DREG; ++d) m = fmaxf(m, v[d]);
#pragma unroll
    for (int d = 0; d < DREG; ++d) { v[d] = expf(v[d] - m); s += v[d]; }
#pragma unroll
    for (int d = 0; d < DREG; ++d) g_logits[base + d * plane] = alpha * (v[d] / s) * (hyp[d * plane + pix] - Ec) * Gc;
}

extern "C" int dmvs_depth_regress_backward(const float* logits, const float* hyp, float alpha, int mode, int D, int H, int W,
                                           const float* dsp, const float* g_dsp, const float* g_sel, float* g_logits,
                                           float* g_hyp, dmvs_stream_t stream) {
    if (!logits || !hyp || !dsp || !g_logits || (!g_dsp && !g_sel)) return DMVS_EINVAL;
    if (D < 1 || H < 1 || W < 1 || (mode != 0 && mode != 1)) return DMVS_EINVAL;
    if (D > 64) return DMVS_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(ceil_div(W, 256), H), split(ceil_div(W, 64), H);
    if (D == 4)
        depth_regress_bwd_kernel<4><<<grid, 256, 0, st>>>(logits, hyp, alpha, mode, D, H, W, dsp, g_dsp, g_sel, g_logits, g_hyp);
    else if (D == 8)
        depth_regress_bwd_kernel<8><<<grid, 256, 0, st>>>(logits, hyp, alpha, mode, D, H, W, dsp, g_dsp, g_sel, g_logits, g_hyp);
    else if (D == 32 && !g_hyp)
        depth_regress_bwd_split_kernel<32><<<split, 256, 0, st>>>(logits, hyp, alpha, mode, H, W, dsp, g_dsp, g_sel, g_logits);
    else if (D == 48 && !g_hyp)
        depth_regress_bwd_split_kernel<48><<<split, 256, 0, st>>>(logits, hyp, alpha, mode, H, W, dsp, g_dsp, g_sel, g_logits);
    else if (D == 64 && !g_hyp)
        depth_regress_bwd_split_kernel<64><<<split, 256, 0, st>>>(logits, hyp, alpha, mode, H, W, dsp, g_dsp, g_sel, g_logits);
    else
        depth_regress_bwd_kernel<0><<<grid, 256, 0, st>>>(logits, hyp, alpha, mode, D, H, W, dsp, g_dsp, g_sel, g_logits, g_hyp);
    DMVS_LAUNCH_CHECK();
}
