// K3k / K3d: weight and data gradient of the 5x5 stride-2 pad-2 2D convolutions of FeatureNet (conv1.0: 8 -> 16, conv2.0: 16 -> 32;
// networks/module.py:289, :295) on the fp32 matrix cores -- device code and launchers, included at the end of conv3d_direct.hip after
// K3h.  docs/kernels/K3k_conv_wgrad_k5s2.md.
//
// One sample is a stack of D independent planes, K3's kdepth-1 layout: the fine tensor X / dX is [Cb][D][Hf][Wf], the coarse one
// Y / dY is [Ca][D][Hc][Wc] with Ca = 2 Cb, Hc = (Hf + 1) / 2, Wc = (Wf + 1) / 2 (even and odd fine extents), W is [Ca][Cb][5][5]:
//
//   wgrad (K3k)  dW[a][b][ky][kx]  = sum_{z,y,x coarse} dY[a][z][y][x] * X[b][z][2y + ky - 2][2x + kx - 2]                (X zero outside)
//   dgrad (K3d)  dX[b][z][2j + py][2i + px] = sum_{a, ty, tx : 2ty + py <= 4, 2tx + px <= 4}
//                                              dY[a][z][j + 1 - ty][i + 1 - tx] * W[a][b][2ty + py][2tx + px]            (dY zero outside)
//
// K3k is K3h (conv3d_wgrad_s2.h) carried to 25 taps.  GEMM view: M = Ca, N = 25 taps * Cb, reduction over the coarse pixels.
//   MFMA     v_mfma_f32_16x16x4_f32 (Ca = 16) / v_mfma_f32_32x32x2_f32 (Ca = 32), exact fp32.  Cb = MF / 2: the N columns hold TWO taps
//            side by side -- 13 slots for 25 taps, the second half of the last slot is computed and never written.
//   tile     one plane x TY = 4 rows x TX = 32 coarse columns.  LDS holds dY[MF][TY][TX] and the fine rows 2 y0 - 2 .. 2 y0 + 2 TY
//            (2 TY + 3 rows) x columns 2 x0 - 2 .. 2 x0 + 64, every row SPLIT BY x PARITY: the even columns (kx = 0, 2, 4 at entries
//            i, i + 1, i + 2) at [0, 34), the odd ones (kx = 1, 3 at OB + i, OB + i + 1) at [OB, OB + 33).  A tap is then a unit-stride
//            read at a per-lane offset.  Loads are checked against Hf, Wf; outside the tensor zeros are staged: no global address is
//            formed outside the two tensors, on ragged tiles and on the missing last row / column of an odd extent alike.
//   banks    K3h's rule: the paired taps differ by an offset that is 2 mod 4 (MF 16) resp. odd (MF 32); derivation in the doc.
//   grid, sums   wgrad_share.h, one block; the tile's MFMA chain and the store of the partial [S][tap][a][b] are K3h's own functions.
//
// K3d is a gather: every fine pixel is written exactly once, by the lane that owns (b, z, j, i, py, px).
//   MFMA     v_mfma_f32_16x16x4_f32 for both shapes: M = 16 fine-channel rows, N = 16 coarse pixels of a row, K = 4 coarse channels of
//            one tap.  Cb = 16: one parity class (py, px) per accumulator, 9 + 6 + 6 + 4 = 25 taps, none wasted.  Cb = 8: the two x
//            parities share the 16 rows (row = px * 8 + b); the tap tx = 2 of px = 1 does not exist and is a zero row.
//   weights  the A operand, staged once per workgroup from the raw nn.Conv2d layout into LDS as [ky][kx][a][16] (Cb = 8:
//            [ky][tx][a][px * 8 + b], kx = 2 tx + px, zeros at kx = 5): a k-step is 64 consecutive floats.  No host packing.
//   tile     8 rows x 32 columns of (j, i) = 16 x 64 fine pixels, the coarse tile with a one-pixel halo in LDS (zeros outside the
//            coarse grid), channel stride 16 mod 32.  A wave owns 2 rows x 2 column blocks of 16 and all four parity classes: a dY
//            fragment is read once per tap and k-step and feeds every class that has the tap.
//   grid     the shares' walk (wgrad_share.h) without their sums: every workgroup stages the weights once.
#pragma once
#include "conv3d_wgrad_s2.h"
#include "wgrad_share.h"

namespace k5s2 {

using wgrad::Frag;
using wgrad_s2::store_partial;
using wgrad_s2::tile_chain;

constexpr int kTX = 32;
constexpr int kTY = 4;   // coarse rows of a K3k tile; dmvs_conv2d_k5s2_wgrad_plan counts kTY x kTX tiles
constexpr int kNT = 25;  // taps
constexpr int kNP = 13;  // slots of two taps

constexpr int pad32(int n, int want) { return n + ((want - n % 32) + 32) % 32; }   // smallest n' >= n with n' % 32 == want

// ------------------------------------------------------------------------------------------------------------------ K3k
// MF: the MFMA's M = N = Ca; CB = MF / 2: channels of the fine tensor
template <int MF>
struct Geom {
    static constexpr int CB = MF / 2;
    static constexpr int KK = Frag<MF>::KK;
    static constexpr int SPW = (kNP + 3) / 4;          // slots per wave: 4 + 4 + 4 + 1
    static constexpr int IY = 2 * kTY + 3;             // fine rows of the halo
    static constexpr int NE = kTX + 2, NO = kTX + 1;   // even / odd columns staged per row
    // row of the fine halo: even columns at [0, NE), odd columns at [OB, OB + NO); see the doc for the residues
    static constexpr int OB = MF == 16 ? NE : NE + 1;            // 34 (2 mod 4) / 35 (odd)
    static constexpr int RS = MF == 16 ? OB + NO + 3 : OB + NO + 1;   // 70 (2 mod 4) / 69 (odd)
    static constexpr int FS = pad32(IY * RS, MF == 16 ? 4 : 2);  // channel stride of the fine halo
    static constexpr int AS = pad32(kTY * kTX, MF == 16 ? 2 : 1);   // ... of the coarse tile
    static constexpr int LDS_F = CB * FS + MF * AS;
    static_assert(OB >= NE && OB + NO <= RS, "the two sub-planes must fit the row");
    static_assert(MF == 16 ? (OB % 4 == 2 && RS % 4 == 2) : (OB % 2 == 1 && RS % 2 == 1), "the paired taps must fall on other banks");
};

// the tap (ky * 5 + kx) in half q of slot s, or -1:
//   s 0 .. 9   ky = s / 2, kx = 2 (s % 2) + q: kx = 0 | 1 and kx = 2 | 3     offsets differ by OB
//   s 10, 11   kx = 4, ky = 2 (s - 10) + q: ky = 0 | 1 and ky = 2 | 3         ... by RS
//   s 12       (4, 4) | nothing
__host__ __device__ inline int slot_tap(int s, int q) {
    if (s < 10) return (s >> 1) * 5 + 2 * (s & 1) + q;
    if (s < 12) return (2 * (s - 10) + q) * 5 + 4;
    return q == 0 ? 24 : -1;
}

struct Args {
    const float* gy;    // coarse [Ca][D][Hc][Wc]
    const float* x;     // fine   [Cb][D][Hf][Wf]
    float* ws;
    int Ca, D, Hf, Wf, Hc, Wc;
    wshare::Grid g;   // one block
};

template <int MF>
__global__ __launch_bounds__(256, 1) void conv_wgrad_k5s2_kernel(Args a) {
    typedef Frag<MF> F;
    typedef typename F::acc_t acc_t;
    typedef Geom<MF> G;
    constexpr int CB = G::CB, SPW = G::SPW, IY = G::IY, OB = G::OB, RS = G::RS, FS = G::FS, AS = G::AS, TX = kTX, TY = kTY;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* fs = smem;
    float* as = smem + CB * FS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ln = lane % MF, lk = lane / MF;
    const int lq = ln / CB, lb = ln % CB;   // this lane's half of the slot and its fine channel
    const int s = wshare::place(a.g, blockIdx.x);
    if (s < 0) return;
    const int t0 = wshare::first_tile(a.g, s), t1 = wshare::first_tile(a.g, s + 1);
    const size_t cplane = (size_t)a.Hc * a.Wc, cvol = cplane * a.D;
    const size_t fplane = (size_t)a.Hf * a.Wf, fvol = fplane * a.D;

    // the lane's taps of the wave's slots wave * SPW + j; a slot past the end repeats the last one, the empty half repeats the
    // slot's first tap (both computed, never written)
    int tap[SPW];
    const float* pb[SPW];
#pragma unroll
    for (int j = 0; j < SPW; ++j) {
        const int sl = min(wave * SPW + j, kNP - 1);
        const int t = slot_tap(sl, lq);
        tap[j] = wave * SPW + j < kNP ? t : -1;
        const int tt = t < 0 ? slot_tap(sl, 0) : t;
        const int ky = tt / 5, kx = tt % 5;
        pb[j] = fs + lb * FS + ky * RS + ((kx & 1) ? OB + (kx >> 1) : (kx >> 1)) + lk;
    }

    acc_t run[SPW];
#pragma unroll
    for (int j = 0; j < SPW; ++j)
#pragma unroll
        for (int r = 0; r < F::ACC; ++r) run[j][r] = 0.f;

    for (int tile = t0; tile < t1; ++tile) {
        const wshare::Tile t = wshare::decode(a.g, tile);
        const int x0 = t.bx * TX, y0 = t.by * TY, z = t.z;
        __syncthreads();   // every wave is done reading the previous tile
        wshare::stage_rows<MF, TY, TX>(as, AS, a.gy, 0, MF, cvol, cplane, z, y0, x0, a.Hc, a.Wc, tid);
        // the fine halo: columns 2 x0 - 2 .. 2 x0 + 2 TX of rows 2 y0 - 2 .. 2 y0 + 2 TY, read along x and written split by parity:
        // column 2 x0 - 2 + f -> [f / 2] (f even), [OB + f / 2] (f odd)
        constexpr int FW = 2 * TX + 3;
        for (int i = tid; i < CB * IY * FW; i += 256) {
            const int c = i / (IY * FW), r = i % (IY * FW);
            const int py = r / FW, f = r % FW;
            const int gy = 2 * y0 + py - 2, gx = 2 * x0 + f - 2;
            float v = 0.f;
            if (gy >= 0 && gy < a.Hf && gx >= 0 && gx < a.Wf) v = a.x[(size_t)c * fvol + z * fplane + (size_t)gy * a.Wf + gx];
            fs[c * FS + py * RS + ((f & 1) ? OB + (f >> 1) : (f >> 1))] = v;
        }
        __syncthreads();
        tile_chain<MF, SPW, TY, RS>(as + ln * AS + lk, pb, run);
    }
    store_partial<MF, CB, SPW>(a.ws + (size_t)s * kNT * a.Ca * CB, a.Ca, 0, lk, lb, tap, run);
}

// gw[a][b][tap] (+)= sum_{s = 0 .. S-1} ws[s][tap][a][b], s ascending.  One thread per element, in workspace order.
__global__ __launch_bounds__(256) void conv_wgrad_k5s2_reduce_kernel(const float* __restrict__ ws, float* __restrict__ gw, int Ca, int Cb,
                                                                      int S, int accumulate) {
    wshare::reduce(ws, kNT * Ca * Cb, S, accumulate, [=](int e) { return wshare::tap_last(gw, e, Ca, Cb, kNT); });
}

inline bool shape_ok(int Ca) { return Ca == 16 || Ca == 32; }

// the coarse extents and the one-block grid of ty x tx coarse pixels; false: an extent < 1 or too large, or >= 2^22 tiles
inline bool tile_grid(int D, int Hf, int Wf, int ty, int tx, int& Hc, int& Wc, wshare::Grid& g) {
    if (Hf > (1 << 21) || Wf > (1 << 21) || D > (1 << 21)) return false;   // 2 * coarse extent + 2 stays an int
    Hc = (Hf + 1) / 2; Wc = (Wf + 1) / 2;
    return wshare::grid(D, Hc, Wc, ty, tx, 1, g);
}

// the launch geometry of K3k, one source of truth for the launcher, the workspace size and the plan
inline bool geometry(int Ca, int D, int Hf, int Wf, Args& a) {
    a.Ca = Ca; a.D = D; a.Hf = Hf; a.Wf = Wf;
    return tile_grid(D, Hf, Wf, kTY, kTX, a.Hc, a.Wc, a.g);
}

template <int MF>
int launch(const Args& a, float* gw, int accumulate, hipStream_t st) {
    typedef Geom<MF> G;
    constexpr size_t lds = (size_t)G::LDS_F * sizeof(float);
    static_assert(lds <= 160 * 1024, "the two tiles must fit the 160 KB LDS");
    return wshare::launch(conv_wgrad_k5s2_kernel<MF>, a, lds, st, conv_wgrad_k5s2_reduce_kernel, kNT * a.Ca * G::CB, a.ws, gw, a.Ca, G::CB,
                          a.g.S, accumulate);
}

// ------------------------------------------------------------------------------------------------------------------ K3d
constexpr int kDJ = 8, kDI = 32;   // rows x columns of (j, i) of a K3d tile: 16 x 64 fine pixels

template <int CB>
struct DGeom {
    static constexpr int CA = 2 * CB;
    static constexpr int RW = kDI + 2, NR = kDJ + 2;    // the coarse tile with its one-pixel halo
    static constexpr int DS = pad32(NR * RW, 16);       // channel stride: 2 k-lanes x 16 pixels of a half wave on 32 banks
    static constexpr int NWT = CB == 16 ? 25 : 15;      // weight blocks [a][16]: (ky, kx) resp. (ky, tx) with the x parities merged
    static constexpr int WL = NWT * CA * 16;
    static constexpr int LDS_F = WL + CA * DS;
};

struct DArgs {
    const float* gy;   // coarse [Ca][D][Hc][Wc]
    const float* w;    // [Ca][Cb][5][5]
    float* gx;         // fine   [Cb][D][Hf][Wf]
    int D, Hf, Wf, Hc, Wc;
    wshare::Grid g;   // one block
};

template <int CB>
__global__ __launch_bounds__(256, 1) void conv_dgrad_k5s2_kernel(DArgs a) {
    typedef Frag<16> F;
    typedef F::acc_t acc_t;
    typedef DGeom<CB> G;
    constexpr int CA = G::CA, RW = G::RW, NR = G::NR, DS = G::DS, WL = G::WL;
    constexpr int NPX = CB == 16 ? 2 : 1;   // accumulators per y parity: the x parities apart (Cb = 16) or merged in M (Cb = 8)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* wl = smem;
    float* ds = smem + WL;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ln = lane & 15, lk = lane >> 4;
    const int s = wshare::place(a.g, blockIdx.x);
    if (s < 0) return;
    const int t0 = wshare::first_tile(a.g, s), t1 = wshare::first_tile(a.g, s + 1);
    const size_t cplane = (size_t)a.Hc * a.Wc, cvol = cplane * a.D;
    const size_t fplane = (size_t)a.Hf * a.Wf, fvol = fplane * a.D;

    // the weights, once: wl[block][a][m]
    for (int i = tid; i < WL; i += 256) {
        const int blk = i / (CA * 16), ca = (i / 16) % CA, m = i % 16;
        float v;
        if (CB == 16) {
            v = a.w[((size_t)ca * CB + m) * 25 + blk];
        } else {
            const int ky = blk / 3, kx = 2 * (blk % 3) + (m >> 3);
            v = kx < 5 ? a.w[((size_t)ca * CB + (m & 7)) * 25 + ky * 5 + kx] : 0.f;
        }
        wl[i] = v;
    }

    for (int tile = t0; tile < t1; ++tile) {
        const wshare::Tile t = wshare::decode(a.g, tile);
        const int i0 = t.bx * kDI, j0 = t.by * kDJ, z = t.z;
        __syncthreads();   // every wave is done reading the previous tile
        for (int i = tid; i < CA * NR * RW; i += 256) {
            const int c = i / (NR * RW), r = i % (NR * RW), y = j0 + r / RW - 1, x = i0 + r % RW - 1;
            float v = 0.f;
            if (y >= 0 && y < a.Hc && x >= 0 && x < a.Wc) v = a.gy[(size_t)c * cvol + z * cplane + (size_t)y * a.Wc + x];
            ds[c * DS + r] = v;
        }
        __syncthreads();

        // this wave: rows 2 wave, 2 wave + 1 of the tile x column blocks 0, 1; block nb = row * 2 + column block
        acc_t acc[2][NPX][4];
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int q = 0; q < NPX; ++q)
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[p][q][nb][r] = 0.f;
        // dY[a = 4 ks + lk][j + 1 - ty][i + 1 - tx] of pixel (j, i) = (2 wave + row, 16 cb + ln): staged row j + 2 - ty, column i + 2 - tx
        const float* pd = ds + lk * DS + (2 * wave + 2) * RW + ln + 2;
        const float* pw = wl + lk * 16 + ln;
#pragma unroll
        for (int ty = 0; ty < 3; ++ty) {
#pragma unroll
            for (int tx = 0; tx < 3; ++tx) {
#pragma unroll 2
                for (int ks = 0; ks < CA / 4; ++ks) {
                    float bv[4];
#pragma unroll
                    for (int nb = 0; nb < 4; ++nb) bv[nb] = pd[ks * 4 * DS + ((nb >> 1) - ty) * RW + (nb & 1) * 16 - tx];
#pragma unroll
                    for (int p = 0; p < 2; ++p) {
                        if (2 * ty + p > 4) continue;
#pragma unroll
                        for (int q = 0; q < NPX; ++q) {
                            if (CB == 16 && 2 * tx + q > 4) continue;
                            const int blk = CB == 16 ? (2 * ty + p) * 5 + 2 * tx + q : (2 * ty + p) * 3 + tx;
                            const float av = pw[(blk * CA + ks * 4) * 16];
#pragma unroll
                            for (int nb = 0; nb < 4; ++nb) acc[p][q][nb] = F::mfma(av, bv[nb], acc[p][q][nb]);
                        }
                    }
                }
            }
        }

        // D[m = 4 lk + r][n = ln]: m = b (Cb = 16) or px * 8 + b (Cb = 8)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int j = j0 + 2 * wave + (nb >> 1), i = i0 + (nb & 1) * 16 + ln;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int Yf = 2 * j + p;
#pragma unroll
                for (int q = 0; q < NPX; ++q) {
                    const int Xf = 2 * i + (CB == 16 ? q : (lk >> 1));
                    if (Yf < a.Hf && Xf < a.Wf) {
                        float* o = a.gx + z * fplane + (size_t)Yf * a.Wf + Xf;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int b = CB == 16 ? 4 * lk + r : 4 * (lk & 1) + r;
                            o[(size_t)b * fvol] = acc[p][q][nb][r];
                        }
                    }
                }
            }
        }
    }
}

inline bool dgeometry(int D, int Hf, int Wf, DArgs& a) {
    a.D = D; a.Hf = Hf; a.Wf = Wf;
    return tile_grid(D, Hf, Wf, kDJ, kDI, a.Hc, a.Wc, a.g);
}

template <int CB>
int dlaunch(const DArgs& a, hipStream_t st) {
    typedef DGeom<CB> G;
    constexpr size_t lds = (size_t)G::LDS_F * sizeof(float);
    static_assert(lds <= 160 * 1024, "the weights and the tile must fit the 160 KB LDS");
    static_assert(G::DS % 32 == 16, "the two k-lanes of a half wave must fall on other banks");
    auto kernel = conv_dgrad_k5s2_kernel<CB>;
    if (int e = dmvs_ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), lds)) return e;
    kernel<<<dim3(xcd_grid(a.g.nwg)), 256, lds, st>>>(a);
    DMVS_LAUNCH_CHECK();
}

}  // namespace k5s2

extern "C" long dmvs_conv2d_k5s2_wgrad_workspace(int Ca, int D, int Hf, int Wf) {
    k5s2::Args a;
    if (!k5s2::shape_ok(Ca) || !k5s2::geometry(Ca, D, Hf, Wf, a)) return 0;
    return wshare::workspace(1, (long)k5s2::kNT * Ca * (Ca / 2));
}

extern "C" int dmvs_conv2d_k5s2_wgrad_plan(int Ca, int D, int Hf, int Wf) {
    k5s2::Args a;
    if (!k5s2::shape_ok(Ca)) return DMVS_EUNSUPPORTED;
    if (!k5s2::geometry(Ca, D, Hf, Wf, a)) return DMVS_EINVAL;
    return wshare::plan(a.g);
}

extern "C" int dmvs_conv2d_k5s2_wgrad(const float* gy, const float* x, float* gw, float* workspace, int Ca, int D, int Hf, int Wf,
                                      int accumulate, dmvs_stream_t stream) {
    if (!gy || !x || !gw || !workspace || D < 1 || Hf < 1 || Wf < 1) return DMVS_EINVAL;
    if (!k5s2::shape_ok(Ca)) return DMVS_EUNSUPPORTED;
    k5s2::Args a;
    if (!k5s2::geometry(Ca, D, Hf, Wf, a)) return DMVS_EINVAL;
    a.gy = gy; a.x = x; a.ws = workspace;
    hipStream_t st = (hipStream_t)stream;
    const int acc = accumulate ? 1 : 0;
    return Ca == 16 ? k5s2::launch<16>(a, gw, acc, st) : k5s2::launch<32>(a, gw, acc, st);
}

extern "C" int dmvs_conv2d_k5s2_dgrad(const float* gy, const float* w, float* gx, int Ca, int D, int Hf, int Wf, dmvs_stream_t stream) {
    if (!gy || !w || !gx || D < 1 || Hf < 1 || Wf < 1) return DMVS_EINVAL;
    if (!k5s2::shape_ok(Ca)) return DMVS_EUNSUPPORTED;
    k5s2::DArgs a;
    if (!k5s2::dgeometry(D, Hf, Wf, a)) return DMVS_EINVAL;
    a.gy = gy; a.w = w; a.gx = gx;
    hipStream_t st = (hipStream_t)stream;
    return Ca == 16 ? k5s2::dlaunch<8>(a, st) : k5s2::dlaunch<16>(a, st);
}
