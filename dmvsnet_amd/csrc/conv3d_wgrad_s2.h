// K3h: weight gradient of the stride-2 and the transposed 3x3(x3) convolutions (kernel 3, stride 2, padding 1; transposed:
// output_padding 1) on the fp32 matrix cores -- device code and launcher, included at the end of conv3d_direct.hip after K3g.
//
// Replaces what autograd runs behind the reference's Conv3d / Deconv3d / Conv2d / Deconv2d blocks (networks/module.py) for the
// weight of conv1 / 3 / 5 and conv7 / 9 / 11 of the regularisation U-Nets and the 2D conv5 / conv7 of the refine net.  Both layer
// forms are one formula.  A is the COARSE tensor [Ca][Dc][Hc][Wc], B the FINE one [Cb][Df][2 Hc][2 Wc], Ca = 2 Cb,
// Df = 2 Dc (kdepth 3) or Dc (kdepth 1):
//
//   G[a][b][kz][ky][kx] = sum_{z,y,x over the coarse grid} A[a][z][y][x] * B[b][2z + kz - 1][2y + ky - 1][2x + kx - 1]   (zero outside B;
//                                                                                                        kdepth 1: plane z, no kz)
//   stride-2 conv:  A = dY, B = X, dW = G.       transposed conv:  A = X, B = dY, dWt = G.       G is the layer's own weight layout.
//
// GEMM view: M = Ca, N = taps * Cb, reduction over the coarse voxels.
//   MFMA     v_mfma_f32_16x16x4_f32 (Ca = 16) / v_mfma_f32_32x32x2_f32 (Ca >= 32), exact fp32.  A = A[a = lane % MF][voxel = lane / MF].
//            Cb = MF / 2 (16 -> 8, 32 -> 16): the N columns hold TWO taps side by side, column n = tap n / Cb, channel n % Cb -- 14 slots
//            for 27 taps, the second half of the last slot is computed and never written.  Cb = MF (64 -> 32): one tap per slot and a
//            workgroup owns one 32-row block of a.
//   tile     one coarse z plane x TY rows x TX = 32 columns (TY = 4; 2 for 64 / 32 / kdepth 3, whose fine tile would not fit).  LDS
//            holds A[MF][TY][TX] and the fine halo B[Cb][kd planes][2 TY + 1 rows], every row SPLIT BY x PARITY: the even columns
//            2x (tap kx = 1) at [0, TX), the odd columns 2x - 1 (kx = 0; kx = 2 is the next one) at [OB, OB + TX].  A tap is then a
//            unit-stride read at a per-lane offset.  Outside the fine tensor the halo is staged as zeros: the zero padding; no global
//            address is formed outside the two tensors.
//   banks    ds_read_b32: 32 banks, the two 32-lane halves of a wave are served separately.  docs/kernels/K3h_conv_wgrad_s2.md
//            derives the strides (FS, AS, RS, OB below) that put the 32 lanes of a half on 32 different banks for every slot.
//   waves    the 4 waves of a workgroup split the slots (4 + 4 + 4 + 2 of 14, 7 + 7 + 7 + 6 of 27, 3 + 3 + 3 + 0 of 9).
//   grid, sums   wgrad_share.h, with the NB a-blocks as the blocks; a tile is one MFMA chain from zero, the partials are [S][tap][a][b].
//            The chain and the partial store (tile_chain, store_partial) are K3k's too.
#pragma once
#include "conv3d_wgrad.h"
#include "wgrad_share.h"

namespace wgrad_s2 {

using wgrad::Frag;

constexpr int kTX = 32;

constexpr int pad32(int n, int want) { return n + ((want - n % 32) + 32) % 32; }   // smallest n' >= n with n' % 32 == want

// MF: the MFMA's M = N (rows of a per workgroup); CB: channels of the fine tensor; KD: kdepth
template <int MF, int CB, int KD>
struct Geom {
    static constexpr int KK = Frag<MF>::KK;
    static constexpr int TPN = MF / CB;                       // taps side by side in N: 2 or 1
    static constexpr int NT = 9 * KD;                         // taps
    static constexpr int NP = (NT + TPN - 1) / TPN;           // slots
    static constexpr int SPW = (NP + 3) / 4;                  // slots per wave
    static constexpr int TY = (CB == 32 && KD == 3) ? 2 : 4;  // coarse rows of a tile
    static constexpr int IY = 2 * TY + 1;                     // fine rows of the halo
    // row of the fine halo: even columns at [0, TX), odd columns at [OB, OB + TX]; see the doc for the residues
    static constexpr int OB = CB == 8 ? kTX + 2 : CB == 16 ? kTX + 1 : kTX;
    static constexpr int RS = CB == 8 ? 2 * kTX + 6 : CB == 16 ? 2 * kTX + 3 : 2 * kTX + 1;
    static constexpr int FS = pad32(KD * IY * RS, CB == 8 ? 4 : CB == 16 ? 2 : 1);   // channel stride of the fine halo
    static constexpr int AS = pad32(TY * kTX, MF == 16 ? 2 : 1);                     // ... of the coarse tile
    static constexpr int LDS_F = CB * FS + MF * AS;
    static_assert(OB + kTX + 1 <= RS, "the odd sub-plane must fit the row");
    static_assert(TPN == 1 || KD == 3, "the tap pairs are laid out for 27 taps");
};

// the tap (kz * 9 + ky * 3 + kx) in half q of slot s, or -1.  One tap per slot: the identity.  Two taps per slot (27 taps, 14 slots):
//   s 0 .. 8   (kz, ky) = (s / 3, s % 3): kx = 0 | kx = 1             offsets differ by OB
//   s 9 .. 11  kz = s - 9: (ky, kx) = (0, 2) | (1, 2)                 ... by RS
//   s 12       (kz, ky, kx) = (0, 2, 2) | (1, 2, 2)                   ... by IY * RS
//   s 13       (2, 2, 2) | nothing
template <int TPN>
__host__ __device__ inline int slot_tap(int s, int q) {
    if (TPN == 1) return s;
    if (s < 9) return s * 3 + q;
    if (s < 12) return (s - 9) * 9 + q * 3 + 2;
    if (s == 12) return q * 9 + 8;
    return q == 0 ? 26 : -1;
}

struct Args {
    const float* coarse;
    const float* fine;
    float* ws;
    int Ca, Cb, Dc, Hc, Wc;
    wshare::Grid g;   // blocks = Ca / MF
};

// one tile of K3h / K3k: an MFMA chain from zero over its TY x 32 coarse voxels per slot, then added to the share's running sums.
// pa: the lane's A fragment in the coarse tile; pb[j]: the lane's tap of slot j in the parity-split fine halo (row stride RS)
template <int MF, int SPW, int TY, int RS>
__device__ __forceinline__ void tile_chain(const float* pa, const float* (&pb)[SPW], typename Frag<MF>::acc_t (&run)[SPW]) {
    typedef Frag<MF> F;
    constexpr int KK = F::KK, TX = kTX;
    typename F::acc_t acc[SPW];
#pragma unroll
    for (int j = 0; j < SPW; ++j)
#pragma unroll
        for (int r = 0; r < F::ACC; ++r) acc[j][r] = 0.f;
#pragma unroll 1
    for (int y = 0; y < TY; ++y) {
#pragma unroll
        for (int g = 0; g < TX / KK; ++g) {
            const float av = pa[y * TX + g * KK];
#pragma unroll
            for (int j = 0; j < SPW; ++j) acc[j] = F::mfma(av, pb[j][2 * y * RS + g * KK], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < SPW; ++j) run[j] += acc[j];
}

// partial of a share: w[tap][a][b]; the CB lanes of a tap's row write CB contiguous floats
template <int MF, int CB, int SPW>
__device__ __forceinline__ void store_partial(float* w, int Ca, int a0, int lk, int lb, const int (&tap)[SPW],
                                              const typename Frag<MF>::acc_t (&run)[SPW]) {
    typedef Frag<MF> F;
#pragma unroll
    for (int j = 0; j < SPW; ++j) {
        if (tap[j] >= 0) {
#pragma unroll
            for (int r = 0; r < F::ACC; ++r) w[((size_t)tap[j] * Ca + a0 + F::row(r, lk)) * CB + lb] = run[j][r];
        }
    }
}

template <int MF, int CB, int KD>
__global__ __launch_bounds__(256, 1) void conv_wgrad_s2_kernel(Args a) {
    typedef Frag<MF> F;
    typedef typename F::acc_t acc_t;
    typedef Geom<MF, CB, KD> G;
    constexpr int NT = G::NT, NP = G::NP, SPW = G::SPW, TPN = G::TPN, TY = G::TY, IY = G::IY, OB = G::OB, RS = G::RS, FS = G::FS,
                  AS = G::AS, TX = kTX;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* fs = smem;
    float* as = smem + CB * FS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ln = lane % MF, lk = lane / MF;
    const int lq = ln / CB, lb = ln % CB;   // this lane's half of the slot and its fine channel
    const int wg = wshare::place(a.g, blockIdx.x);
    if (wg < 0) return;
    const int NB = a.Ca / MF;
    const int blk = wg % NB, s = wg / NB;
    const int a0 = blk * MF;
    const int t0 = wshare::first_tile(a.g, s), t1 = wshare::first_tile(a.g, s + 1);
    const int Hf = 2 * a.Hc, Wf = 2 * a.Wc, Df = KD == 3 ? 2 * a.Dc : a.Dc;
    const size_t cplane = (size_t)a.Hc * a.Wc, cvol = cplane * a.Dc;
    const size_t fplane = (size_t)Hf * Wf, fvol = fplane * Df;

    // the lane's taps of the wave's slots wave * SPW + j; a slot past the end repeats the last one, an empty half repeats the
    // slot's first tap (both computed, never written)
    int tap[SPW];
    const float* pb[SPW];
#pragma unroll
    for (int j = 0; j < SPW; ++j) {
        const int sl = min(wave * SPW + j, NP - 1);
        const int t = slot_tap<TPN>(sl, lq);
        tap[j] = wave * SPW + j < NP ? t : -1;
        const int tt = t < 0 ? slot_tap<TPN>(sl, 0) : t;
        const int kz = tt / 9, ky = (tt / 3) % 3, kx = tt % 3;
        pb[j] = fs + lb * FS + (kz * IY + ky) * RS + (kx == 1 ? 0 : kx == 0 ? OB : OB + 1) + lk;
    }
    const bool live = wave * SPW < NP;

    acc_t run[SPW];
#pragma unroll
    for (int j = 0; j < SPW; ++j)
#pragma unroll
        for (int r = 0; r < F::ACC; ++r) run[j][r] = 0.f;

    for (int tile = t0; tile < t1; ++tile) {
        const wshare::Tile t = wshare::decode(a.g, tile);
        const int x0 = t.bx * TX, y0 = t.by * TY, z = t.z;
        __syncthreads();   // every wave is done reading the previous tile
        wshare::stage_rows<MF, TY, TX>(as, AS, a.coarse, a0, MF, cvol, cplane, z, y0, x0, a.Hc, a.Wc, tid);
        // the fine halo: columns 2 x0 - 1 .. 2 x0 + 2 TX - 1 of rows 2 y0 - 1 .. 2 y0 + 2 TY - 1 of planes 2z - 1 .. 2z + 1 (kdepth 1: z),
        // read along x and written split by parity: column 2 (x0 + i) -> [i], column 2 (x0 + i) - 1 -> [OB + i]
        constexpr int FW = 2 * TX + 1;
        for (int i = tid; i < CB * KD * IY * FW; i += 256) {
            const int c = i / (KD * IY * FW), r = i % (KD * IY * FW);
            const int pz = r / (IY * FW), py = (r / FW) % IY, f = r % FW;
            const int gz = KD == 3 ? 2 * z + pz - 1 : z, gy = 2 * y0 + py - 1, gx = 2 * x0 + f - 1;
            float v = 0.f;
            if (gz >= 0 && gz < Df && gy >= 0 && gy < Hf && gx >= 0 && gx < Wf)
                v = a.fine[(size_t)c * fvol + gz * fplane + (size_t)gy * Wf + gx];
            fs[c * FS + (pz * IY + py) * RS + ((f & 1) ? (f >> 1) : OB + (f >> 1))] = v;
        }
        __syncthreads();
        if (live) tile_chain<MF, SPW, TY, RS>(as + ln * AS + lk, pb, run);
    }
    if (live) store_partial<MF, CB, SPW>(a.ws + (size_t)s * NT * a.Ca * CB, a.Ca, a0, lk, lb, tap, run);
}

// gw[a][b][tap] (+)= sum_{s = 0 .. S-1} ws[s][tap][a][b], s ascending.  One thread per element, in workspace order.
__global__ __launch_bounds__(256) void conv_wgrad_s2_reduce_kernel(const float* __restrict__ ws, float* __restrict__ gw, int Ca, int Cb,
                                                                    int NT, int S, int accumulate) {
    wshare::reduce(ws, NT * Ca * Cb, S, accumulate, [=](int e) { return wshare::tap_last(gw, e, Ca, Cb, NT); });
}

inline bool shape_ok(int Ca, int kdepth) { return kdepth == 3 ? (Ca == 16 || Ca == 32 || Ca == 64) : (kdepth == 1 && Ca == 64); }
inline int blocks_of(int Ca) { return Ca == 64 ? 2 : 1;   /* 32-row blocks of a */ }
inline int tile_rows(int Ca, int kdepth) { return Ca == 64 && kdepth == 3 ? 2 : 4; }

// the launch geometry, one source of truth for the launcher, the workspace size and the plan
inline bool geometry(int Ca, int Dc, int Hc, int Wc, int kdepth, Args& a) {
    if (Hc > (1 << 20) || Wc > (1 << 20) || Dc > (1 << 20)) return false;   // 2 * extent stays an int
    a.Ca = Ca; a.Cb = Ca / 2; a.Dc = Dc; a.Hc = Hc; a.Wc = Wc;
    return wshare::grid(Dc, Hc, Wc, tile_rows(Ca, kdepth), kTX, blocks_of(Ca), a.g);
}

template <int MF, int CB, int KD>
int launch(const Args& a, float* gw, int accumulate, hipStream_t st) {
    typedef Geom<MF, CB, KD> G;
    constexpr size_t lds = (size_t)G::LDS_F * sizeof(float);
    static_assert(lds <= 160 * 1024, "the two tiles must fit the 160 KB LDS");
    return wshare::launch(conv_wgrad_s2_kernel<MF, CB, KD>, a, lds, st, conv_wgrad_s2_reduce_kernel, G::NT * a.Ca * a.Cb, a.ws, gw, a.Ca,
                          a.Cb, G::NT, a.g.S, accumulate);
}

}  // namespace wgrad_s2

extern "C" long dmvs_conv3d_wgrad_s2_workspace(int Ca, int Dc, int Hc, int Wc, int kdepth) {
    wgrad_s2::Args a;
    if (!wgrad_s2::shape_ok(Ca, kdepth) || !wgrad_s2::geometry(Ca, Dc, Hc, Wc, kdepth, a)) return 0;
    return wshare::workspace(wgrad_s2::blocks_of(Ca), 9L * kdepth * Ca * (Ca / 2));
}

extern "C" int dmvs_conv3d_wgrad_s2_plan(int Ca, int Dc, int Hc, int Wc, int kdepth) {
    wgrad_s2::Args a;
    if (!wgrad_s2::shape_ok(Ca, kdepth)) return DMVS_EUNSUPPORTED;
    if (!wgrad_s2::geometry(Ca, Dc, Hc, Wc, kdepth, a)) return DMVS_EINVAL;
    return wshare::plan(a.g);
}

extern "C" int dmvs_conv3d_wgrad_s2(const float* coarse, const float* fine, float* gw, float* workspace, int Ca, int Dc, int Hc, int Wc,
                                    int kdepth, int accumulate, dmvs_stream_t stream) {
    if (!coarse || !fine || !gw || !workspace || Dc < 1 || Hc < 1 || Wc < 1) return DMVS_EINVAL;
    if (!wgrad_s2::shape_ok(Ca, kdepth)) return DMVS_EUNSUPPORTED;
    wgrad_s2::Args a;
    if (!wgrad_s2::geometry(Ca, Dc, Hc, Wc, kdepth, a)) return DMVS_EINVAL;
    a.coarse = coarse; a.fine = fine; a.ws = workspace;
    hipStream_t st = (hipStream_t)stream;
    const int acc = accumulate ? 1 : 0;
    if (Ca == 16) return wgrad_s2::launch<16, 8, 3>(a, gw, acc, st);
    if (Ca == 32) return wgrad_s2::launch<32, 16, 3>(a, gw, acc, st);
    return kdepth == 3 ? wgrad_s2::launch<32, 32, 3>(a, gw, acc, st) : wgrad_s2::launch<32, 32, 1>(a, gw, acc, st);
}
