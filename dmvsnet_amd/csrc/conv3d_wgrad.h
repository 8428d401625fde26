// K3g: weight gradient of the stride-1 3x3(x3) pad-1 square convolutions (C -> C, C in {16, 32, 64}; kdepth 3 or 1) on the fp32
// matrix cores -- device code and launcher, included at the end of conv3d_direct.hip.
//
// Replaces what autograd runs behind the reference's Conv3d / Conv2d blocks (networks/module.py:28-70, 142) for the weight of
// conv2 / conv4 / conv6, the 2D conv6 and FeatureNet's conv1.1 / 1.2 / 2.1 / 2.2:
//
//   dW[co][ci][kz][ky][kx] = sum_{z,y,x} dY[co][z][y][x] * X[ci][z + kz - 1][y + ky - 1][x + kx - 1]     (zero outside the volume)
//
// GEMM view: M = Cout, N = taps * Cin, reduction over the D * H * W voxels.
//   MFMA     v_mfma_f32_16x16x4_f32 (C = 16) / v_mfma_f32_32x32x2_f32 (C >= 32), exact fp32 (a k-ordered fmaf chain).
//            A = dY[co = lane % M][voxel = lane / M], B = tap-shifted X[ci = lane % M][voxel]; D[co][ci], one accumulator block per tap.
//   tile     one z plane x TY = 4 rows x TX = 32 columns of voxels.  LDS holds dY[M][TY][TX] and X[M][kd][TY + 2][TX + 2] (one-voxel
//            halo, staged as zeros outside the volume: the zero padding; no global load is formed outside the two tensors).  The
//            channel strides are padded so the M channels x KK voxels of an operand read fall on 64 different banks.
//   waves    the 4 waves of a workgroup split the TAPS (7 + 7 + 7 + 6 of 27, 3 + 3 + 3 + 0 of 9): every wave walks all voxels of the
//            tile and owns TPW accumulator blocks (TPW * 16 = 112 registers on the 32-row MFMA, where 27 blocks would not fit).  One
//            dY fragment feeds TPW MFMAs; a tap is a wave-uniform LDS offset.
//   blocks   C = 64 has 2 x 2 (co, ci) blocks of 32: a workgroup owns ONE block pair.
//   grid, sums   wgrad_share.h, with NBP block pairs as the blocks: a tile's 128 voxels are ONE MFMA chain from zero (128 fmaf), the
//            running sum is VALU adds, the partials are [S][tap][co][ci].
#pragma once
#include "wgrad_share.h"

namespace wgrad {

typedef float acc16_t __attribute__((ext_vector_type(16)));
typedef float acc4_t __attribute__((ext_vector_type(4)));

template <int M> struct Frag;
template <> struct Frag<32> {
    static constexpr int KK = 2, ACC = 16;
    typedef acc16_t acc_t;
    static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int r, int lk) { return (r & 3) + 8 * (r >> 2) + 4 * lk; }
};
template <> struct Frag<16> {
    static constexpr int KK = 4, ACC = 4;
    typedef acc4_t acc_t;
    static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int r, int lk) { return lk * 4 + r; }
};

constexpr int kTY = 4, kTX = 32;   // voxel tile (one z plane); dmvs_conv3d_wgrad_plan counts these

constexpr int pad_to(int n, int want) { return n + ((want - n % 64) + 64) % 64; }   // smallest n' >= n with n' % 64 == want

template <int M, int KD>
struct Geom {
    static constexpr int KK = Frag<M>::KK;
    static constexpr int NT = 9 * KD, TPW = (NT + 3) / 4;   // taps, taps per wave
    static constexpr int IY = kTY + 2, IXP = kTX + 2;
    static constexpr int BANK = M == 16 ? 4 : 2;            // M channels x KK consecutive voxels -> 64 banks
    static constexpr int XS = pad_to(KD * IY * IXP, BANK);  // channel stride of the X tile
    static constexpr int DYS = pad_to(kTY * kTX, BANK);     // ... of the dY tile
    static constexpr int LDS_F = M * (XS + DYS);
};

struct Args {
    const float* x;
    const float* gy;
    float* ws;
    int C, D, H, W;
    wshare::Grid g;   // blocks = (C / M)^2
};

template <int M, int KD>
__global__ __launch_bounds__(256, 1) void conv_wgrad_kernel(Args a) {
    typedef Frag<M> F;
    typedef typename F::acc_t acc_t;
    typedef Geom<M, KD> G;
    constexpr int NT = G::NT, TPW = G::TPW, IY = G::IY, IXP = G::IXP, XS = G::XS, DYS = G::DYS, KK = G::KK;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* xs = smem;
    float* dys = smem + M * XS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ln = lane % M, lk = lane / M;
    const int wg = wshare::place(a.g, blockIdx.x);
    if (wg < 0) return;
    const int NB = a.C / M, NBP = NB * NB;
    const int bp = wg % NBP, s = wg / NBP;
    const int co0 = (bp / NB) * M, ci0 = (bp % NB) * M;
    const int t0 = wshare::first_tile(a.g, s), t1 = wshare::first_tile(a.g, s + 1);
    const size_t plane = (size_t)a.H * a.W, vol = plane * a.D;

    // the wave's taps wave * TPW + j; a tap past the end repeats the last one (computed, never written)
    int toff[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int t = min(wave * TPW + j, NT - 1);
        toff[j] = ((t / 9) * IY + (t / 3) % 3) * IXP + t % 3;
    }
    const bool live = wave * TPW < NT;

    acc_t run[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int r = 0; r < F::ACC; ++r) run[j][r] = 0.f;

    for (int tile = t0; tile < t1; ++tile) {
        const wshare::Tile t = wshare::decode(a.g, tile);
        const int x0 = t.bx * kTX, y0 = t.by * kTY, z = t.z;
        __syncthreads();   // every wave is done reading the previous tile
        wshare::stage_rows<M, kTY, kTX>(dys, DYS, a.gy, co0, M, vol, plane, z, y0, x0, a.H, a.W, tid);
        for (int i = tid; i < M * KD * IY * IXP; i += 256) {
            const int c = i / (KD * IY * IXP), r = i % (KD * IY * IXP);
            const int pz = r / (IY * IXP), py = (r / IXP) % IY, px = r % IXP;
            const int gz = KD == 3 ? z + pz - 1 : z, y = y0 + py - 1, x = x0 + px - 1;
            float v = 0.f;
            if (gz >= 0 && gz < a.D && y >= 0 && y < a.H && x >= 0 && x < a.W)
                v = a.x[(size_t)(ci0 + c) * vol + gz * plane + (size_t)y * a.W + x];
            xs[c * XS + r] = v;
        }
        __syncthreads();
        if (live) {
            acc_t acc[TPW];
#pragma unroll
            for (int j = 0; j < TPW; ++j)
#pragma unroll
                for (int r = 0; r < F::ACC; ++r) acc[j][r] = 0.f;
            const float* pa = dys + ln * DYS + lk;
            const float* pb = xs + ln * XS + lk;
#pragma unroll 1
            for (int y = 0; y < kTY; ++y) {
#pragma unroll
                for (int g = 0; g < kTX / KK; ++g) {
                    const float av = pa[y * kTX + g * KK];
#pragma unroll
                    for (int j = 0; j < TPW; ++j) acc[j] = F::mfma(av, pb[y * IXP + g * KK + toff[j]], acc[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < TPW; ++j) run[j] += acc[j];
        }
    }

    // partial of this share: ws[s][tap][co][ci]; the 16 / 32 lanes of a row write 64 / 128 contiguous bytes
    if (live) {
        float* w = a.ws + (size_t)s * NT * a.C * a.C;
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            const int t = wave * TPW + j;
            if (t < NT) {
#pragma unroll
                for (int r = 0; r < F::ACC; ++r)
                    w[((size_t)t * a.C + co0 + F::row(r, lk)) * a.C + ci0 + ln] = run[j][r];
            }
        }
    }
}

// gw[co][ci][tap] (+)= sum_{s = 0 .. S-1} ws[s][tap][co][ci], s ascending.  One thread per element, in workspace order.
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ gw, int C, int NT, int S,
                                                                 int accumulate) {
    wshare::reduce(ws, NT * C * C, S, accumulate, [=](int e) { return wshare::tap_last(gw, e, C, C, NT); });
}

inline bool shape_ok(int C, int kdepth) { return (C == 16 || C == 32 || C == 64) && (kdepth == 1 || kdepth == 3); }
inline int blocks_of(int C) { return C == 64 ? 4 : 1; }   // (co, ci) block pairs: M = 16 for C = 16, else 32

// the launch geometry, one source of truth for the launcher, the workspace size and the plan
inline bool geometry(int C, int D, int H, int W, Args& a) {
    a.C = C; a.D = D; a.H = H; a.W = W;
    return wshare::grid(D, H, W, kTY, kTX, blocks_of(C), a.g);
}

template <int M, int KD>
int launch(const Args& a, float* gw, int accumulate, hipStream_t st) {
    typedef Geom<M, KD> G;
    constexpr size_t lds = (size_t)G::LDS_F * sizeof(float);
    static_assert(lds <= 160 * 1024, "the two tiles must fit the 160 KB LDS");
    return wshare::launch(conv_wgrad_kernel<M, KD>, a, lds, st, conv_wgrad_reduce_kernel, G::NT * a.C * a.C, a.ws, gw, a.C, G::NT, a.g.S,
                          accumulate);
}

}  // namespace wgrad

extern "C" long dmvs_conv3d_wgrad_workspace(int C, int D, int H, int W, int kdepth) {
    wgrad::Args a;
    if (!wgrad::shape_ok(C, kdepth) || !wgrad::geometry(C, D, H, W, a)) return 0;
    return wshare::workspace(wgrad::blocks_of(C), 9L * kdepth * C * C);
}

extern "C" int dmvs_conv3d_wgrad_plan(int C, int D, int H, int W, int kdepth) {
    wgrad::Args a;
    if (!wgrad::shape_ok(C, kdepth)) return DMVS_EUNSUPPORTED;
    if (!wgrad::geometry(C, D, H, W, a)) return DMVS_EINVAL;
    return wshare::plan(a.g);
}

extern "C" int dmvs_conv3d_wgrad(const float* x, const float* gy, float* gw, float* workspace, int C, int D, int H, int W, int kdepth,
                                 int accumulate, dmvs_stream_t stream) {
    if (!x || !gy || !gw || !workspace || D < 1 || H < 1 || W < 1) return DMVS_EINVAL;
    if (!wgrad::shape_ok(C, kdepth)) return DMVS_EUNSUPPORTED;
    wgrad::Args a;
    if (!wgrad::geometry(C, D, H, W, a)) return DMVS_EINVAL;
    a.x = x; a.gy = gy; a.ws = workspace;
    hipStream_t st = (hipStream_t)stream;
    const int acc = accumulate ? 1 : 0;
    if (C == 16) return kdepth == 3 ? wgrad::launch<16, 3>(a, gw, acc, st) : wgrad::launch<16, 1>(a, gw, acc, st);
    return kdepth == 3 ? wgrad::launch<32, 3>(a, gw, acc, st) : wgrad::launch<32, 1>(a, gw, acc, st);
}
