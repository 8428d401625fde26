// K2g: weight gradient of the 2-channel ends of the regularisation U-Nets -- conv0 (2 -> 8) and `prob` (8 -> 2), 3x3x3, stride 1,
// pad 1 -- device code and launcher, included at the end of conv3d_direct.hip.
//
// Replaces what autograd runs behind the reference's conv0 block and `prob` (networks/module.py:361, 379, 403, 421) for their weight.
// Both layers are ONE formula on a pair of equally sized volumes, P with 8 channels and Q with 2:
//
//   G[p][q][tz][ty][tx] = sum_v P[p][v] * Q[q][v + (tz - 1, ty - 1, tx - 1)]                              (Q is zero outside the volume)
//
//   conv0 (Cin 2, Cout 8): P = dY, Q = X,  dW[co = p][ci = q][t] = G[p][q][t]
//   prob  (Cin 8, Cout 2): P = X,  Q = dY, dW[co = q][ci = p][t] = G[p][q][26 - t]   (u = v + t: the taps come out flipped)
//
// The role and the flip are an index map on the 432 outputs, applied by the second kernel.
//
// Form: VALU, lane = voxel.  The MFMA form pads M 8 -> 16 and N 54 -> 64 (1024 issued MACs per voxel for 432 useful ones; 3 of 4 with
// the shifted-copy trick, at the price of a second staged operand layout); here every issued fmaf is a useful one, the LDS reads are
// 64 consecutive floats of one row (conflict-free without padding) and there is no operand layout to get wrong.
//   tile     one z plane x TY = 4 rows x TX = 64 columns of voxels.  LDS holds P[8][TY][TX] and Q[2][3][TY + 2][TX + 2] (one-voxel halo,
//            staged as zeros outside the volume: the zero padding; no global address is formed outside the two tensors) -- 17.3 KB.
//            The NEXT tile's values are loaded into registers (8 + 10 per lane) before the current tile is computed and stored to
//            LDS after it: the loads are in flight during the arithmetic (unconditional loads at clamped coordinates, then a select).
//   waves    the 4 waves of a workgroup split the 27 TAPS (7 + 7 + 7 + 6), as K3g does: every wave walks all voxels of the tile, a row
//            of 64 per step, and a lane owns 7 x 8 x 2 = 112 accumulators.  Per row: 8 LDS reads of P, then per tap 2 reads of Q (a tap
//            is a wave-uniform LDS offset) feeding 16 fmaf.
//   grid, sums   wgrad_share.h, one block.  Within a share a lane adds its voxel of every row of every tile to its running sums in walk
//            order (one fmaf chain per accumulator); at the end of the share the 64 lanes are folded ONCE by a butterfly over
//            lane ^ 32, 16, .. 1 (both partners form the same a + b).  The partials are [S][tap][p][q].
#pragma once
#include "wgrad_share.h"

namespace wgrad_c2 {

constexpr int kTY = 4, kTX = 64;   // voxel tile (one z plane); dmvs_conv3d_wgrad_c2_plan counts these
constexpr int kP = 8, kQ = 2, kNT = 27, kTPW = 7;   // channels of P and Q, taps, taps per wave
constexpr int kG = kNT * kP * kQ;                   // 432 outputs
constexpr int kIY = kTY + 2, kIXP = kTX + 2;
constexpr int kQS = 3 * kIY * kIXP;                 // channel stride of the Q tile (1188)
constexpr int kPS = kTY * kTX;                      // ... of the P tile (256: one element per thread and channel)
constexpr int kQN = kQ * kQS;                       // 2376 staged Q values
constexpr int kQR = (kQN + 255) / 256;              // ... per thread (10, the last one partial)

struct Args {
    const float* p;   // [8][D][H][W]
    const float* q;   // [2][D][H][W]
    float* ws;
    int D, H, W;
    wshare::Grid g;   // one block
};

struct Staged {
    float p[kP], q[kQR];
    unsigned in;   // bit 0: the P voxel is inside the volume; bit 1 + k: q[k] is
};

// the values thread `tid` stages for `tile`.  Every load is unconditional at coordinates clamped into the volume (so no address is
// formed outside the two tensors); which of them are inside goes into a bit mask, and the zero is selected only when the value is
// stored to LDS (store_tile): nothing between the 18 loads of a thread and the arithmetic waits for them
__device__ __forceinline__ void load_tile(const Args& a, int tile, int tid, Staged& r) {
    const wshare::Tile t = wshare::decode(a.g, tile);
    const int x0 = t.bx * kTX, y0 = t.by * kTY, z = t.z;
    const size_t plane = (size_t)a.H * a.W, vol = plane * a.D;
    {
        const int y = y0 + tid / kTX, x = x0 + tid % kTX;
        r.in = y < a.H && x < a.W ? 1u : 0u;
        const float* p = a.p + (size_t)z * plane + (size_t)min(y, a.H - 1) * a.W + min(x, a.W - 1);
#pragma unroll
        for (int c = 0; c < kP; ++c) r.p[c] = p[(size_t)c * vol];
    }
#pragma unroll
    for (int k = 0; k < kQR; ++k) {
        const int i = min(tid + k * 256, kQN - 1);   // (the last round is partial: its spare threads re-load the last value, unused)
        const int c = i / kQS, e = i % kQS;
        const int pz = e / (kIY * kIXP), py = (e / kIXP) % kIY, px = e % kIXP;
        const int gz = z + pz - 1, y = y0 + py - 1, x = x0 + px - 1;
        if (gz >= 0 && gz < a.D && y >= 0 && y < a.H && x >= 0 && x < a.W) r.in |= 2u << k;
        r.q[k] = a.q[(size_t)c * vol + (size_t)min(max(gz, 0), a.D - 1) * plane + (size_t)min(max(y, 0), a.H - 1) * a.W +
                            min(max(x, 0), a.W - 1)];
    }
}

// ... and their way into LDS: zeros outside the volume (the zero padding)
__device__ __forceinline__ void store_tile(const Staged& r, int tid, float* ps, float* qs) {
#pragma unroll
    for (int c = 0; c < kP; ++c) ps[c * kPS + tid] = (r.in & 1u) ? r.p[c] : 0.f;
#pragma unroll
    for (int k = 0; k < kQR; ++k)
        if (tid + k * 256 < kQN) qs[tid + k * 256] = (r.in & (2u << k)) ? r.q[k] : 0.f;
}

__global__ __launch_bounds__(256, 1) void conv_wgrad_c2_kernel(Args a) {
    __shared__ float ps[kP * kPS];
    __shared__ float qs[kQN];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s = wshare::place(a.g, blockIdx.x);
    if (s < 0) return;
    const int t0 = wshare::first_tile(a.g, s), t1 = wshare::first_tile(a.g, s + 1);

    // the wave's taps wave * 7 + j; the 28th repeats the 27th (computed, never written)
    int toff[kTPW];
#pragma unroll
    for (int j = 0; j < kTPW; ++j) {
        const int t = min(wave * kTPW + j, kNT - 1);
        toff[j] = ((t / 9) * kIY + (t / 3) % 3) * kIXP + t % 3;
    }

    float acc[kTPW][kP][kQ];
#pragma unroll
    for (int j = 0; j < kTPW; ++j)
#pragma unroll
        for (int c = 0; c < kP; ++c) acc[j][c][0] = acc[j][c][1] = 0.f;

    Staged r;
    load_tile(a, t0, tid, r);   // (S <= tiles: every share has at least one tile)
    for (int tile = t0; tile < t1; ++tile) {
        __syncthreads();   // every wave is done reading the previous tile
        store_tile(r, tid, ps, qs);
        __syncthreads();
        if (tile + 1 < t1) load_tile(a, tile + 1, tid, r);   // in flight while this tile is computed
#pragma unroll 2
        for (int y = 0; y < kTY; ++y) {
            float pv[kP];
#pragma unroll
            for (int c = 0; c < kP; ++c) pv[c] = ps[c * kPS + y * kTX + lane];
            const float* qb = qs + y * kIXP + lane;
#pragma unroll
            for (int j = 0; j < kTPW; ++j) {
                const float q0 = qb[toff[j]], q1 = qb[kQS + toff[j]];
#pragma unroll
                for (int c = 0; c < kP; ++c) {
                    acc[j][c][0] = fmaf(pv[c], q0, acc[j][c][0]);
                    acc[j][c][1] = fmaf(pv[c], q1, acc[j][c][1]);
                }
            }
        }
    }

    // one fold of the 64 lanes per share, then lane 0 writes the wave's taps of ws[s][tap][p][q]
    float* w = a.ws + (size_t)s * kG;
#pragma unroll
    for (int j = 0; j < kTPW; ++j) {
        const int t = wave * kTPW + j;
#pragma unroll
        for (int c = 0; c < kP; ++c)
#pragma unroll
            for (int q = 0; q < kQ; ++q) {
                float v = acc[j][c][q];
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
                if (lane == 0 && t < kNT) w[(t * kP + c) * kQ + q] = v;
            }
    }
}

// gw (+)= sum_{s = 0 .. S-1} ws[s][tap][p][q], s ascending, through the role map: conv0 (prob == 0) gw[p][q][t], prob gw[q][p][26 - t].
__global__ __launch_bounds__(256) void conv_wgrad_c2_reduce_kernel(const float* __restrict__ ws, float* __restrict__ gw, int S, int prob,
                                                                    int accumulate) {
    wshare::reduce(ws, kG, S, accumulate, [=](int e) {
        const int t = e / (kP * kQ), p = (e / kQ) % kP, q = e % kQ;
        return gw + (prob ? (q * kP + p) * kNT + (kNT - 1 - t) : (p * kQ + q) * kNT + t);
    });
}

inline bool shape_ok(int Cin, int Cout) { return (Cin == 2 && Cout == 8) || (Cin == 8 && Cout == 2); }

// the launch geometry, one source of truth for the launcher, the workspace size and the plan
inline bool geometry(int D, int H, int W, Args& a) {
    a.D = D; a.H = H; a.W = W;
    return wshare::grid(D, H, W, kTY, kTX, 1, a.g);
}

}  // namespace wgrad_c2

extern "C" long dmvs_conv3d_wgrad_c2_workspace(int Cin, int Cout, int D, int H, int W) {
    wgrad_c2::Args a;
    if (!wgrad_c2::shape_ok(Cin, Cout) || !wgrad_c2::geometry(D, H, W, a)) return 0;
    return wshare::workspace(1, wgrad_c2::kG);
}

extern "C" int dmvs_conv3d_wgrad_c2_plan(int Cin, int Cout, int D, int H, int W) {
    wgrad_c2::Args a;
    if (!wgrad_c2::shape_ok(Cin, Cout)) return DMVS_EUNSUPPORTED;
    if (!wgrad_c2::geometry(D, H, W, a)) return DMVS_EINVAL;
    return wshare::plan(a.g);
}

extern "C" int dmvs_conv3d_wgrad_c2(const float* x, const float* gy, float* gw, float* workspace, int Cin, int Cout, int D, int H, int W,
                                    int accumulate, dmvs_stream_t stream) {
    if (!x || !gy || !gw || !workspace || D < 1 || H < 1 || W < 1) return DMVS_EINVAL;
    if (!wgrad_c2::shape_ok(Cin, Cout)) return DMVS_EUNSUPPORTED;
    wgrad_c2::Args a;
    if (!wgrad_c2::geometry(D, H, W, a)) return DMVS_EINVAL;
    const int prob = Cin == 8;   // P is the 8-channel tensor, Q the 2-channel one
    a.p = prob ? x : gy; a.q = prob ? gy : x; a.ws = workspace;
    hipStream_t st = (hipStream_t)stream;
    return wshare::launch(wgrad_c2::conv_wgrad_c2_kernel, a, 0, st, wgrad_c2::conv_wgrad_c2_reduce_kernel, wgrad_c2::kG, workspace, gw,
                          a.g.S, prob, accumulate ? 1 : 0);   // (static LDS)
}
