// K3f: weight and bias gradient of FeatureNet's rectangular stride-1 2D convolutions on the fp32 matrix cores -- device code, launcher
// and its three C entries, included at the end of conv3d_direct.hip after K3k / K3d.  docs/kernels/K3f_conv_wgrad_fpn.md.
//
// Replaces what autograd runs behind the reference's FeatureNet (networks/module.py:274-340) for the weight (and bias) of
//   conv0.0  3 -> 8   3x3  (:284)      out1    32 -> 64  1x1         (:301)
//   conv0.1  8 -> 8   3x3  (:285)      inner1  16 -> 32  1x1 + bias  (:305)
//   out3     32 -> 16 3x3  (:309)      inner2   8 -> 32  1x1 + bias  (:306)
// on tensors [C][D][H][W] of D independent planes (K3's kdepth-1 layout), k = 3 with padding 1 or k = 1:
//
//   dW[co][ci][ky][kx] = sum_{d,y,x} dY[co][d][y][x] * X[ci][d][y + ky - k/2][x + kx - k/2]     (zero outside the plane)
//   db[co]             = sum_{d,y,x} dY[co][d][y][x]
//
// GEMM view: M = Cout rows (padded to the MFMA's 16 or 32; the padding rows are staged as zeros), N = the columns n = ci * k * k + tap
// -- the order of gw[co] as it lies -- plus, for the two layers with a bias, ONE more column whose X value is the constant 1 inside the
// plane: db is that column of the same product.  Reduction over the D * H * W pixels.
//   MFMA     v_mfma_f32_16x16x4_f32 (Cout <= 16) / v_mfma_f32_32x32x2_f32 (Cout >= 32), exact fp32.  A = dY[co = lane % M][pixel],
//            B = X[column n = lane % M][pixel]: every lane of a B fragment carries its OWN LDS offset (ci(n), tap(n)), computed once per
//            column block (K3g's tap is wave-uniform; here a block of 16 columns spans several taps and channels).
//   columns  3 -> 8: 27 = 2 blocks of 16;  8 -> 8: 72 = 5;  32 -> 16: 288 = 18;  32 -> 64: 32 = 1 block of 32 for each of the 2 row
//            blocks;  16 -> 32: 17 = 1;  8 -> 32: 9 = 1.  Columns past the end repeat the last one: computed, never written.
//   tile     one plane x TY = 4 rows x TX = 32 columns.  LDS holds dY[rows][TY][TX] and X[Cin (+ the ones plane)][TY + 2h][TX + 2h],
//            h = k / 2, the halo staged as zeros outside the plane: the zero padding.  Loads are checked against H, W; no global address
//            is formed outside the two tensors.  Staging walks x fastest: a wave reads 2 x 128 contiguous bytes.
//   waves    3x3: the 4 waves split the column BLOCKS (1 / 2 / 5 per wave), each walks all 128 pixels of the tile.
//            1x1: one block, so the waves split the tile's PIXELS (wave w = row w); their four accumulators are added in wave order
//            through LDS when the share is done.
//   grid, sums   wgrad_share.h, one block: a tile is one MFMA chain from zero per wave, the partials are [S][co][column] and go onto
//            gw / gbias.
#pragma once
#include "conv3d_wgrad.h"
#include "wgrad_share.h"

namespace wgrad_fpn {

using wgrad::Frag;
using wgrad::pad_to;

constexpr int kTY = 4, kTX = 32;   // pixel tile of one plane; dmvs_conv2d_wgrad_fpn_plan counts these

template <int CIN, int COUT, int KS, bool BIAS>
struct Geom {
    static_assert(KS == 3 || (KS == 1 && COUT % 32 == 0), "3x3 on the 16-row MFMA or 1x1 on the 32-row one");
    static_assert(!BIAS || KS == 1, "the ones column is a tap-0 column");
    static constexpr int M = KS == 1 ? 32 : 16;
    static constexpr int MB = (COUT + M - 1) / M;        // row blocks (out1: 2)
    static constexpr int ROWS = MB * M;                  // dY channels staged, zeros past COUT
    static constexpr int KK = Frag<M>::KK, ACC = Frag<M>::ACC;
    static constexpr int NT = KS * KS;
    static constexpr int NW = NT * CIN;                  // columns of gw[co]
    static constexpr int NC = NW + (BIAS ? 1 : 0);       // GEMM columns
    static constexpr int NB = (NC + M - 1) / M;          // column blocks
    static constexpr bool PIX = KS == 1;                 // the waves split the pixels, not the blocks
    static constexpr int BPW = PIX ? NB : (NB + 3) / 4;  // blocks per wave
    static_assert(!PIX || NB == 1, "a 1x1 layer is one column block");
    static constexpr int H2 = KS / 2, IY = kTY + 2 * H2, IXP = kTX + 2 * H2;
    static constexpr int XCH = CIN + (BIAS ? 1 : 0);     // X channels staged: the last one is the ones plane
    static constexpr int BANK = M == 16 ? 4 : 2;
    static constexpr int XS = pad_to(IY * IXP, BANK);    // channel stride of the X tile
    static constexpr int DYS = pad_to(kTY * kTX, BANK);  // ... of the dY tile
    static constexpr int TILE_F = XCH * XS + ROWS * DYS;
    static constexpr int RED_F = PIX ? 4 * MB * ACC * 64 : 0;   // the four waves' accumulators
    static constexpr int LDS_F = TILE_F > RED_F ? TILE_F : RED_F;
};

struct Args {
    const float* x;
    const float* gy;
    float* ws;
    int D, H, W;
    wshare::Grid g;   // one block
};

template <int CIN, int COUT, int KS, bool BIAS>
__global__ __launch_bounds__(256) void conv_wgrad_fpn_kernel(Args a) {
    typedef Geom<CIN, COUT, KS, BIAS> G;
    typedef Frag<G::M> F;
    typedef typename F::acc_t acc_t;
    constexpr int M = G::M, MB = G::MB, KK = G::KK, NT = G::NT, NC = G::NC, NB = G::NB, BPW = G::BPW, IY = G::IY, IXP = G::IXP, XS = G::XS,
                  DYS = G::DYS, H2 = G::H2;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* xs = smem;
    float* dys = smem + G::XCH * XS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ln = lane % M, lk = lane / M;
    const int s = wshare::place(a.g, blockIdx.x);
    if (s < 0) return;
    const int t0 = wshare::first_tile(a.g, s), t1 = wshare::first_tile(a.g, s + 1);
    const size_t plane = (size_t)a.H * a.W, vol = plane * a.D;

    // the lane's column of each of the wave's blocks: LDS offset of (ci(n), tap(n)); a column or block past the end repeats the last one
    int boff[BPW];
#pragma unroll
    for (int j = 0; j < BPW; ++j) {
        const int blk = G::PIX ? j : min(wave * BPW + j, NB - 1);
        const int n = min(blk * M + ln, NC - 1), ci = n / NT, t = n % NT;   // (the ones column: ci = CIN, tap 0)
        boff[j] = ci * XS + (t / KS) * IXP + t % KS;
    }
    const bool live = G::PIX || wave * BPW < NB;
    const int ya = G::PIX ? wave : 0, yb = G::PIX ? wave + 1 : kTY;   // the wave's rows of the tile

    acc_t run[MB][BPW];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int j = 0; j < BPW; ++j)
#pragma unroll
            for (int r = 0; r < F::ACC; ++r) run[mb][j][r] = 0.f;

    for (int tile = t0; tile < t1; ++tile) {
        const wshare::Tile t = wshare::decode(a.g, tile);
        const int x0 = t.bx * kTX, y0 = t.by * kTY, z = t.z;
        __syncthreads();   // every wave is done reading the previous tile
        wshare::stage_rows<G::ROWS, kTY, kTX>(dys, DYS, a.gy, 0, COUT, vol, plane, z, y0, x0, a.H, a.W, tid);
        for (int i = tid; i < G::XCH * IY * IXP; i += 256) {
            const int c = i / (IY * IXP), r = i % (IY * IXP), y = y0 + r / IXP - H2, x = x0 + r % IXP - H2;
            float v = 0.f;
            if (y >= 0 && y < a.H && x >= 0 && x < a.W) v = c < CIN ? a.x[(size_t)c * vol + z * plane + (size_t)y * a.W + x] : 1.f;
            xs[c * XS + r] = v;
        }
        __syncthreads();
        if (live) {
            acc_t acc[MB][BPW];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int j = 0; j < BPW; ++j)
#pragma unroll
                    for (int r = 0; r < F::ACC; ++r) acc[mb][j][r] = 0.f;
            const float* pa = dys + ln * DYS + lk;
            const float* pb = xs + lk;
#pragma unroll 1
            for (int y = ya; y < yb; ++y) {
#pragma unroll
                for (int g = 0; g < kTX / KK; ++g) {
                    float bv[BPW];
#pragma unroll
                    for (int j = 0; j < BPW; ++j) bv[j] = pb[boff[j] + y * IXP + g * KK];
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) {
                        const float av = pa[mb * M * DYS + y * kTX + g * KK];
#pragma unroll
                        for (int j = 0; j < BPW; ++j) acc[mb][j] = F::mfma(av, bv[j], acc[mb][j]);
                    }
                }
            }
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int j = 0; j < BPW; ++j) run[mb][j] += acc[mb][j];
        }
    }

    // partial of this share: ws[s][co][column]
    float* w = a.ws + (size_t)s * COUT * NC;
    if constexpr (!G::PIX) {
        if (live) {
#pragma unroll
            for (int j = 0; j < BPW; ++j) {
                const int blk = wave * BPW + j, n = blk * M + ln;
                if (blk < NB && n < NC) {
#pragma unroll
                    for (int r = 0; r < F::ACC; ++r) {
                        const int co = F::row(r, lk);
                        if (co < COUT) w[co * NC + n] = run[0][j][r];
                    }
                }
            }
        }
    } else {
        // the four waves' sums, added in wave order
        constexpr int PER = MB * F::ACC * 64;
        __syncthreads();   // the tiles are read
        float* red = smem;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int r = 0; r < F::ACC; ++r) red[wave * PER + (mb * F::ACC + r) * 64 + lane] = run[mb][0][r];
        __syncthreads();
        for (int i = tid; i < PER; i += 256) {
            float sum = red[i];
#pragma unroll
            for (int wv = 1; wv < 4; ++wv) sum += red[wv * PER + i];
            const int mb = i / (F::ACC * 64), r = (i / 64) % F::ACC, l = i % 64;
            const int co = mb * M + F::row(r, l / M), n = l % M;
            if (co < COUT && n < NC) w[co * NC + n] = sum;
        }
    }
}

// gw[co][column] (+)= sum_{s = 0 .. S-1} ws[s][co][column], s ascending; the column past gw's NW is the bias gradient (skipped when
// gbias is null).  One thread per element, in workspace order.
__global__ __launch_bounds__(256) void conv_wgrad_fpn_reduce_kernel(const float* __restrict__ ws, float* __restrict__ gw,
                                                                     float* __restrict__ gbias, int Cout, int NW, int NC, int S, int accumulate) {
    wshare::reduce(ws, Cout * NC, S, accumulate, [=](int e) {
        const int co = e / NC, col = e % NC;
        return col < NW ? gw + (size_t)co * NW + col : (gbias ? gbias + co : nullptr);
    });
}

// the six layers: index into the shape table, -1 for any other shape
struct Shape { int cin, cout, ks, bias; };
constexpr Shape kShapes[] = {{3, 8, 3, 0}, {8, 8, 3, 0}, {32, 16, 3, 0}, {32, 64, 1, 0}, {16, 32, 1, 1}, {8, 32, 1, 1}};
inline const Shape* find_shape(int Cin, int Cout, int ksize) {
    for (const Shape& s : kShapes)
        if (s.cin == Cin && s.cout == Cout && s.ks == ksize) return &s;
    return nullptr;
}
inline int columns_of(const Shape& s) { return s.ks * s.ks * s.cin + s.bias; }

// the launch geometry, one source of truth for the launcher, the workspace size and the plan
inline bool geometry(int D, int H, int W, Args& a) {
    a.D = D; a.H = H; a.W = W;
    return wshare::grid(D, H, W, kTY, kTX, 1, a.g);
}

template <int CIN, int COUT, int KS, bool BIAS>
int launch(const Args& a, float* gw, float* gbias, int accumulate, hipStream_t st) {
    typedef Geom<CIN, COUT, KS, BIAS> G;
    constexpr size_t lds = (size_t)G::LDS_F * sizeof(float);
    static_assert(lds <= 160 * 1024, "the two tiles must fit the 160 KB LDS");
    return wshare::launch(conv_wgrad_fpn_kernel<CIN, COUT, KS, BIAS>, a, lds, st, conv_wgrad_fpn_reduce_kernel, COUT * G::NC, a.ws, gw, gbias,
                          COUT, G::NW, G::NC, a.g.S, accumulate);
}

}  // namespace wgrad_fpn

extern "C" long dmvs_conv2d_wgrad_fpn_workspace(int Cin, int Cout, int ksize, int D, int H, int W) {
    wgrad_fpn::Args a;
    const wgrad_fpn::Shape* s = wgrad_fpn::find_shape(Cin, Cout, ksize);
    if (!s || !wgrad_fpn::geometry(D, H, W, a)) return 0;
    return wshare::workspace(1, (long)Cout * wgrad_fpn::columns_of(*s));
}

extern "C" int dmvs_conv2d_wgrad_fpn_plan(int Cin, int Cout, int ksize, int D, int H, int W) {
    wgrad_fpn::Args a;
    if (!wgrad_fpn::find_shape(Cin, Cout, ksize)) return DMVS_EUNSUPPORTED;
    if (!wgrad_fpn::geometry(D, H, W, a)) return DMVS_EINVAL;
    return wshare::plan(a.g);
}

extern "C" int dmvs_conv2d_wgrad_fpn(const float* x, const float* gy, float* gw, float* gbias, float* workspace, int Cin, int Cout, int D,
                                     int H, int W, int ksize, int accumulate, dmvs_stream_t stream) {
    if (!x || !gy || !gw || !workspace || D < 1 || H < 1 || W < 1) return DMVS_EINVAL;
    const wgrad_fpn::Shape* s = wgrad_fpn::find_shape(Cin, Cout, ksize);
    if (!s) return DMVS_EUNSUPPORTED;
    if (gbias && !s->bias) return DMVS_EINVAL;   // the layer has no bias
    wgrad_fpn::Args a;
    if (!wgrad_fpn::geometry(D, H, W, a)) return DMVS_EINVAL;
    a.x = x; a.gy = gy; a.ws = workspace;
    hipStream_t st = (hipStream_t)stream;
    const int acc = accumulate ? 1 : 0;
    if (ksize == 3) {
        if (Cin == 3) return wgrad_fpn::launch<3, 8, 3, false>(a, gw, gbias, acc, st);
        if (Cin == 8) return wgrad_fpn::launch<8, 8, 3, false>(a, gw, gbias, acc, st);
        return wgrad_fpn::launch<32, 16, 3, false>(a, gw, gbias, acc, st);
    }
    if (Cin == 32) return wgrad_fpn::launch<32, 64, 1, false>(a, gw, gbias, acc, st);
    if (Cin == 16) return wgrad_fpn::launch<16, 32, 1, true>(a, gw, gbias, acc, st);
    return wgrad_fpn::launch<8, 32, 1, true>(a, gw, gbias, acc, st);
}
