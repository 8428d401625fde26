// K5: BatchNorm + ReLU of the reference's Conv3d / Deconv3d / Conv2d / Deconv2d blocks (networks/module.py: `self.bn(...)` then
// `F.relu(x, inplace=True)`), train and eval mode, forward and backward -- device code, launchers and the five C entries, included at
// the end of conv3d_direct.hip.  docs/kernels/K5_batchnorm_relu.md has the figures.
//
//   tensors    x, y, gy, gx fp32 [B][C][V], V = D * H * W (2D layers: H * W), C in {8, 16, 32, 64}.  The batch is inside the kernels.
//   partition  ONE function for all four streaming kernels (share_range below, also exported to the host).  A channel's N = B * V
//              elements are the flattened index i = b * V + v; they are cut into chunks of kChunk = 256 lanes x 4 floats and
//              S = min(chunks, kMaxWg / C) shares; share s owns the chunks [s * chunks / S, (s + 1) * chunks / S), a contiguous index
//              range that may cross sample boundaries (it is walked sample segment by sample segment, all bounds wave-uniform).
//              Grid: C * S workgroups of 256 (at most 2048), workgroup = (channel, share): the channel constants are wave-uniform.
//              A lane loads 16 bytes when V % 4 == 0 and every base pointer is 16-byte aligned (VEC = 4), else 4 bytes (VEC = 1, the
//              same walk in steps of 256 elements); kUnroll loads are in flight before the first use.
//   forward    bn_stats_kernel: partial (sum (x - p), sum (x - p)^2) of every share around the channel's pivot p: the mean of its
//              first min(V, 256) elements, cut to 12 significant bits, which every workgroup of the channel computes by the same
//              tree (same bits).  mean = p + sum (x - p) / N, var = sum (x - p)^2 / N - (sum (x - p) / N)^2 -- never a raw
//              E[x^2] - E[x]^2: the error does not grow with mean^2 / var.  Why 12 bits: a pivot with a full mantissa has bits
//              below the ulp of the larger |x|, which shift every fp32 difference x - p of one binade by the SAME fraction of an
//              ulp -- a bias of up to 3e-8 per element that does not average out (measured: 1.5e-8 on a mean of 1e-3 over 2 M
//              elements, 7 times the bound).  With 12 bits x - p is exact or rounds on x's own last bit for every |x| <= 4096 |p|.
//              bn_apply_kernel: prologue = the fold of the channel's S partials in the order s = 0 .. S-1 in fp64 (every workgroup of
//              the channel repeats it and gets the same bits; no finalize launch), then y = relu(pre(x)) with pre() below.  The
//              workgroup of share 0 alone stores mean / invstd and blends running_mean / running_var (unbiased variance there).
//   backward   bn_bwd_reduce_kernel: partial (sum g, sum g * xhat), g = gy * [pre(x) > 0]: pre() is the forward's own function on the
//              forward's own constants, so the mask is the forward's, and y is neither saved nor read.
//              bn_bwd_apply_kernel: the same fp64 fold in its prologue, gx = gamma * invstd * ((g - sum_g / N) - xhat * sum_gxhat / N)
//              (eval: the two coupling terms are zero); share 0 stores g_gamma = sum_gxhat and g_beta = sum_g.
//              bn_bwd_fold_kernel (C workgroups) stores the two instead when no gx is wanted and the apply launch is skipped.
//   sums       thread: 4 independent fp32 chains (one per vector slot), each as long as the share's chunks (at most
//              ceil(chunks / S)) ; then ((a0 + a1) + (a2 + a3)); wave: a 6-level butterfly; workgroup: (w0 + w1) + (w2 + w3); partials:
//              fp64, sequential.  Nothing is exchanged between workgroups inside a launch; nothing is atomic: same input, same bits.
//   sync       statistics over R ranks (torch.nn.SyncBatchNorm's semantics), one more fold level in the same style; the collectives
//              themselves are the host's (kernel and entries: batchnorm_sync.h).  bn_stats_kernel as above, then bn_moments_kernel
//              (C workgroups) folds the S partials and
//              writes the rank's (n_r, mean_r = p + f0 / n_r, M2_r = f1 - f0^2 / n_r) in fp64: ranks have different pivots, so
//              MOMENTS travel, never raw sums.  bn_apply_kernel<VEC, true>: the prologue combines the gathered [R][C][3] triples in
//              the order r = 0 .. R-1 in fp64 (combine() below: N = sum n_r, mean = sum n_r mean_r / N,
//              M2 = sum (M2_r + n_r (mean_r - mean)^2), var = M2 / N), the same chain in every thread of every workgroup of the channel
//              on every rank: mean / invstd and the running buffers are the same bits on all ranks.  Backward: bn_bwd_reduce_kernel
//              on the global mean / invstd, bn_bwd_fold_kernel<true> stores g_beta / g_gamma (the LOCAL sums) and the fp64 pair,
//              bn_bwd_apply_kernel<VEC, true> adds the gathered [R][C][2] pairs in rank order and divides by the global N.
#pragma once
#include "common.h"

namespace bn {

constexpr int kLanes = 256, kChunk = 4 * kLanes;   // a chunk: 256 lanes x 16 bytes
constexpr int kMaxWg = 2048;                       // C * Smax workgroups: 8 per CU
constexpr int kUnroll = 4;                         // loads in flight per lane
constexpr int kPivot = 256;                        // elements behind the pivot
constexpr int kMaxRanks = 16;                      // ranks whose statistics the sync kernels combine

inline bool channels_ok(int C) { return C == 8 || C == 16 || C == 32 || C == 64; }

// shares of a channel of n elements
__host__ __device__ inline int shares_of(int C, long n) {
    const long chunks = (n + kChunk - 1) / kChunk, smax = kMaxWg / C;
    return (int)(chunks < smax ? chunks : smax);
}

// [lo, hi) of share s of S: whole chunks, the last one cut at n
__host__ __device__ inline void share_range(long n, int S, int s, long& lo, long& hi) {
    const long chunks = (n + kChunk - 1) / kChunk;
    const long c0 = (long)s * chunks / S, c1 = (long)(s + 1) * chunks / S;
    lo = c0 * kChunk;
    hi = c1 * kChunk < n ? c1 * kChunk : n;
}

struct Args {
    const float* x;
    const float* gy;       // backward
    const float* gamma;
    const float* beta;
    const float* mean_in;  // eval forward: running_mean; backward: the saved mean
    const float* var_in;   // eval forward: running_var;  backward: the saved invstd
    float* out;            // y / gx
    float* mean;           // forward: [C] out
    float* invstd;         // forward: [C] out
    float* run_mean;       // train forward: blended in place
    float* run_var;
    float* g_gamma;
    float* g_beta;
    float* ws;             // [C][S][2] partials, then [C] pivots
    int B, C, V, S;
    long n;                // B * V
    float momentum, eps;
    int relu, train;
    // sync kernels only
    const double* gathered;  // forward: [R][C][3] (n_r, mean_r, M2_r); backward: [R][C][2] (sum g, sum g * xhat)
    double* dout;            // this rank's [C][3] moments / [C][2] sums
    double N;                // backward: the global count
    int R;
};

// ---- the one statement of the pre-activation: forward apply and backward mask both call it on the same fp32 constants
__device__ __forceinline__ float pre_act(float x, float mean, float scale, float beta) { return fmaf(x - mean, scale, beta); }
__device__ __forceinline__ float scale_of(float invstd, float gamma) { return invstd * gamma; }

// VEC floats of one lane: one 16-byte access (VEC = 4) or one 4-byte access (VEC = 1)
template <int VEC> __device__ __forceinline__ void load(const float* p, float (&d)[VEC]) {
    if constexpr (VEC == 4) {
        const float4_t v = *reinterpret_cast<const float4_t*>(p);
        d[0] = v[0]; d[1] = v[1]; d[2] = v[2]; d[3] = v[3];
    } else {
        d[0] = *p;
    }
}
template <int VEC> __device__ __forceinline__ void store(float* p, const float (&d)[VEC]) {
    if constexpr (VEC == 4) *reinterpret_cast<float4_t*>(p) = float4_t{d[0], d[1], d[2], d[3]};
    else *p = d[0];
}
template <int VEC> __device__ __forceinline__ void zero(float (&d)[VEC]) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) d[j] = 0.f;
}
// ((a0 + a1) + (a2 + a3)) of a lane's VEC chains
template <int VEC> __device__ __forceinline__ float lane_sum(const float (&d)[VEC]) {
    if constexpr (VEC == 4) return (d[0] + d[1]) + (d[2] + d[3]);
    else return d[0];
}

// sum over the workgroup in a fixed shape: butterfly over the 64 lanes, then (w0 + w1) + (w2 + w3).  Every thread returns the sum.
__device__ __forceinline__ float block_sum(float v, float* red /* [4] */) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    __syncthreads();   // the previous use of red is over
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// Walk the index range [lo, hi) of channel c, sample segment by sample segment (bounds wave-uniform).  body(base, v, v1): this lane
// owns the VEC elements at tensor offset base + v + u * kLanes * VEC for u in [0, kUnroll), those with v + u * kLanes * VEC < v1.
template <int VEC, class Body>
__device__ __forceinline__ void walk(const Args& a, int c, long lo, long hi, Body body) {
    const int tid = threadIdx.x;
    const int b0 = (int)(lo / a.V), b1 = (int)((hi - 1) / a.V);
    for (int b = b0; b <= b1; ++b) {   // sample segments of the share
        const long sb = (long)b * a.V;
        const int v0 = (int)((lo > sb ? lo : sb) - sb), v1 = (int)((hi < sb + a.V ? hi : sb + a.V) - sb);
        const size_t base = ((size_t)b * a.C + c) * (size_t)a.V;
        for (int v = v0 + tid * VEC; v < v1; v += kUnroll * kLanes * VEC) body(base, v, v1);
    }
}

// pivot of channel c: the mean of its first min(V, kPivot) elements (sample 0) cut to 12 significant bits, the same tree in every
// workgroup
__device__ __forceinline__ float pivot_of(const Args& a, int c, float* red) {
    const int m = a.V < kPivot ? a.V : kPivot;
    const float v = (int)threadIdx.x < m ? a.x[(size_t)c * a.V + threadIdx.x] : 0.f;
    return __uint_as_float(__float_as_uint(block_sum(v, red) / (float)m) & 0xfffff000u);
}

template <int VEC>
__global__ __launch_bounds__(kLanes) void bn_stats_kernel(Args a) {
    __shared__ float red[4];
    const int c = blockIdx.x / a.S, s = blockIdx.x % a.S;
    long lo, hi;
    share_range(a.n, a.S, s, lo, hi);
    const float p = pivot_of(a, c, red);
    float s1[VEC], s2[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) s1[j] = s2[j] = 0.f;
    walk<VEC>(a, c, lo, hi, [&](size_t base, int v, int v1) {
        float r[kUnroll][VEC];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int vu = v + u * kLanes * VEC;
            if (vu < v1) load<VEC>(a.x + base + vu, r[u]); else zero<VEC>(r[u]);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (v + u * kLanes * VEC < v1) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float d = r[u][j] - p;
                    s1[j] += d;
                    s2[j] = fmaf(d, d, s2[j]);
                }
            }
        }
    });
    const float t1 = block_sum(lane_sum<VEC>(s1), red), t2 = block_sum(lane_sum<VEC>(s2), red);
    if (threadIdx.x == 0) {
        float* w = a.ws + ((size_t)c * a.S + s) * 2;
        w[0] = t1; w[1] = t2;
        if (s == 0) a.ws[(size_t)a.C * a.S * 2 + c] = p;
    }
}

// the two sums of the S partials of channel c, added in the order s = 0 .. S-1 in fp64: staged in LDS by one parallel read, then the
// same two chains of at most kMaxWg / 8 = 256 adds in every thread of every workgroup of the channel (same bits everywhere)
constexpr int kMaxShares = kMaxWg / 8;
__device__ __forceinline__ void fold(const Args& a, int c, double* part /* [2 * kMaxShares] */, double& f0, double& f1) {
    const float* w = a.ws + (size_t)c * a.S * 2;
    for (int i = threadIdx.x; i < 2 * a.S; i += blockDim.x) part[i] = (double)w[i];
    __syncthreads();
    f0 = 0.0; f1 = 0.0;
#pragma unroll 8
    for (int s = 0; s < a.S; ++s) { f0 += part[2 * s]; f1 += part[2 * s + 1]; }
}

// K values of every rank for channel c of the gathered [R][C][K] buffer, staged in LDS by one parallel read: part[r * K + k]
template <int K> __device__ __forceinline__ void stage_ranks(const Args& a, int c, double* part /* [K * kMaxRanks] */) {
    for (int i = threadIdx.x; i < K * a.R; i += blockDim.x) part[i] = a.gathered[((size_t)(i / K) * a.C + c) * K + i % K];
    __syncthreads();
}

// the global count, mean and sum of squared deviations of channel c from the R triples, in the order r = 0 .. R-1 in fp64; the same
// chain in every thread of every workgroup of the channel (R is wave-uniform, at most kMaxRanks)
__device__ __forceinline__ void combine(const Args& a, int c, double* part, double& N, double& mean, double& M2) {
    stage_ranks<3>(a, c, part);
    double sm = 0.0;
    N = 0.0;
    for (int r = 0; r < a.R; ++r) { N += part[3 * r]; sm += part[3 * r] * part[3 * r + 1]; }
    mean = sm / N;
    M2 = 0.0;
    for (int r = 0; r < a.R; ++r) {
        const double d = part[3 * r + 1] - mean;
        M2 += part[3 * r + 2] + part[3 * r] * (d * d);
    }
}

template <int VEC, bool SYNC = false>
__global__ __launch_bounds__(kLanes) void bn_apply_kernel(Args a) {
    const int c = blockIdx.x / a.S, s = blockIdx.x % a.S;
    long lo, hi;
    share_range(a.n, a.S, s, lo, hi);
    __shared__ double part[2 * kMaxShares];
    float mean, invstd;
    if constexpr (SYNC) {
        double N, m, M2;
        combine(a, c, part, N, m, M2);
        const double var = M2 / N;                               // biased; M2 is a sum of non-negative terms
        mean = (float)m;
        invstd = (float)(1.0 / sqrt(var + (double)a.eps));
        if (s == 0 && threadIdx.x == 0) {
            a.mean[c] = mean; a.invstd[c] = invstd;
            const double mo = (double)a.momentum;
            a.run_mean[c] = (float)((1.0 - mo) * (double)a.run_mean[c] + mo * (double)mean);
            a.run_var[c] = (float)((1.0 - mo) * (double)a.run_var[c] + mo * (M2 / (N - 1.0)));
        }
    } else if (a.train) {
        double f0, f1;
        fold(a, c, part, f0, f1);
        const double n = (double)a.n, d = f0 / n;               // mean - pivot
        double var = f1 / n - d * d;                             // biased
        var = var > 0.0 ? var : 0.0;
        mean = (float)((double)a.ws[(size_t)a.C * a.S * 2 + c] + d);
        invstd = (float)(1.0 / sqrt(var + (double)a.eps));
        if (s == 0 && threadIdx.x == 0) {
            a.mean[c] = mean; a.invstd[c] = invstd;
            const double m = (double)a.momentum;
            a.run_mean[c] = (float)((1.0 - m) * (double)a.run_mean[c] + m * (double)mean);
            a.run_var[c] = (float)((1.0 - m) * (double)a.run_var[c] + m * (var * (n / (n - 1.0))));
        }
    } else {
        mean = a.mean_in[c];
        invstd = (float)(1.0 / sqrt((double)a.var_in[c] + (double)a.eps));
        if (s == 0 && threadIdx.x == 0) { a.mean[c] = mean; a.invstd[c] = invstd; }
    }
    const float scale = scale_of(invstd, a.gamma[c]), beta = a.beta[c];
    const bool relu = a.relu != 0;
    walk<VEC>(a, c, lo, hi, [&](size_t base, int v, int v1) {
        float r[kUnroll][VEC];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int vu = v + u * kLanes * VEC;
            if (vu < v1) load<VEC>(a.x + base + vu, r[u]); else zero<VEC>(r[u]);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int vu = v + u * kLanes * VEC;
            if (vu < v1) {
                float o[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float pre = pre_act(r[u][j], mean, scale, beta);
                    o[j] = relu && pre < 0.f ? 0.f : pre;   // (a NaN stays a NaN, as ATen's relu)
                }
                store<VEC>(a.out + base + vu, o);
            }
        }
    });
}

template <int VEC>
__global__ __launch_bounds__(kLanes) void bn_bwd_reduce_kernel(Args a) {
    __shared__ float red[4];
    const int c = blockIdx.x / a.S, s = blockIdx.x % a.S;
    long lo, hi;
    share_range(a.n, a.S, s, lo, hi);
    const float mean = a.mean_in[c], invstd = a.var_in[c];
    const float scale = scale_of(invstd, a.gamma[c]), beta = a.beta[c];
    const bool relu = a.relu != 0;
    float s1[VEC], s2[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) s1[j] = s2[j] = 0.f;
    walk<VEC>(a, c, lo, hi, [&](size_t base, int v, int v1) {
        float r[kUnroll][VEC], q[kUnroll][VEC];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int vu = v + u * kLanes * VEC;
            if (vu < v1) { load<VEC>(a.x + base + vu, r[u]); load<VEC>(a.gy + base + vu, q[u]); } else { zero<VEC>(r[u]); zero<VEC>(q[u]); }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (v + u * kLanes * VEC < v1) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float xv = r[u][j];
                    const float g = relu && !(pre_act(xv, mean, scale, beta) > 0.f) ? 0.f : q[u][j];
                    s1[j] += g;
                    s2[j] = fmaf(g, (xv - mean) * invstd, s2[j]);
                }
            }
        }
    });
    const float t1 = block_sum(lane_sum<VEC>(s1), red), t2 = block_sum(lane_sum<VEC>(s2), red);
    if (threadIdx.x == 0) {
        float* w = a.ws + ((size_t)c * a.S + s) * 2;
        w[0] = t1; w[1] = t2;
    }
}

template <int VEC, bool SYNC = false>
__global__ __launch_bounds__(kLanes) void bn_bwd_apply_kernel(Args a) {
    const int c = blockIdx.x / a.S, s = blockIdx.x % a.S;
    long lo, hi;
    share_range(a.n, a.S, s, lo, hi);
    __shared__ double part[2 * kMaxShares];
    double f0, f1;
    float k1, k2;
    if constexpr (SYNC) {   // the sums of all ranks, added in rank order; g_gamma / g_beta are the fold launch's
        stage_ranks<2>(a, c, part);
        f0 = 0.0; f1 = 0.0;
        for (int r = 0; r < a.R; ++r) { f0 += part[2 * r]; f1 += part[2 * r + 1]; }
        k1 = (float)(f0 / a.N); k2 = (float)(f1 / a.N);
    } else {
        fold(a, c, part, f0, f1);
        if (s == 0 && threadIdx.x == 0) { a.g_beta[c] = (float)f0; a.g_gamma[c] = (float)f1; }
        k1 = a.train ? (float)(f0 / (double)a.n) : 0.f; k2 = a.train ? (float)(f1 / (double)a.n) : 0.f;
    }
    const float mean = a.mean_in[c], invstd = a.var_in[c];
    const float scale = scale_of(invstd, a.gamma[c]), beta = a.beta[c];
    const bool relu = a.relu != 0;
    walk<VEC>(a, c, lo, hi, [&](size_t base, int v, int v1) {
        float r[kUnroll][VEC], q[kUnroll][VEC];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int vu = v + u * kLanes * VEC;
            if (vu < v1) { load<VEC>(a.x + base + vu, r[u]); load<VEC>(a.gy + base + vu, q[u]); } else { zero<VEC>(r[u]); zero<VEC>(q[u]); }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int vu = v + u * kLanes * VEC;
            if (vu < v1) {
                float o[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    const float xv = r[u][j];
                    const float g = relu && !(pre_act(xv, mean, scale, beta) > 0.f) ? 0.f : q[u][j];
                    o[j] = scale * ((g - k1) - ((xv - mean) * invstd) * k2);
                }
                store<VEC>(a.out + base + vu, o);
            }
        }
    });
}

// g_gamma / g_beta alone (no gx wanted): the same fold, one workgroup per channel.  SYNC: also the fp64 pair that travels
template <bool SYNC = false>
__global__ __launch_bounds__(64) void bn_bwd_fold_kernel(Args a) {
    __shared__ double part[2 * kMaxShares];
    double f0, f1;
    fold(a, blockIdx.x, part, f0, f1);
    if (threadIdx.x == 0) {
        a.g_beta[blockIdx.x] = (float)f0; a.g_gamma[blockIdx.x] = (float)f1;
        if constexpr (SYNC) { a.dout[2 * blockIdx.x] = f0; a.dout[2 * blockIdx.x + 1] = f1; }
    }
}

inline bool geometry(int B, int C, int V, Args& a) {
    if (B < 1 || V < 1) return false;
    const long n = (long)B * V;
    if (n > 0x7fffffffL - kUnroll * kChunk) return false;   // per-channel indices are 32-bit in the walk; tensor offsets are 64-bit
    a.B = B; a.C = C; a.V = V; a.n = n;
    a.S = shares_of(C, n);
    return true;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace bn

extern "C" long dmvs_bn_workspace(int C, int B, int V) {
    bn::Args a;
    if (!bn::channels_ok(C) || !bn::geometry(B, C, V, a)) return 0;
    return 2L * bn::kMaxWg + C;   // [C][Smax][2] partials and [C] pivots, whatever the volume
}

extern "C" int dmvs_bn_plan(int C, int B, int V) {
    bn::Args a;
    if (!bn::channels_ok(C) || !bn::geometry(B, C, V, a)) return DMVS_EINVAL;
    return a.S;
}

extern "C" int dmvs_bn_share_range(int C, int B, int V, int s, long* lo, long* hi) {
    bn::Args a;
    if (!lo || !hi || !bn::channels_ok(C)) return DMVS_EINVAL;
    if (!bn::geometry(B, C, V, a) || s < 0 || s >= a.S) return DMVS_EINVAL;
    bn::share_range(a.n, a.S, s, *lo, *hi);
    return 0;
}

extern "C" int dmvs_bn_relu_forward(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                    float* y, float* mean, float* invstd, float* workspace, int B, int C, int V, float momentum,
                                    float eps, int flags, dmvs_stream_t stream) {
    if (!x || !gamma || !beta || !running_mean || !running_var || !y || !mean || !invstd || !workspace) return DMVS_EINVAL;
    if (flags & ~(DMVS_RELU | DMVS_BN_TRAIN)) return DMVS_EINVAL;
    if (!bn::channels_ok(C)) return DMVS_EINVAL;
    bn::Args a = {};
    if (!bn::geometry(B, C, V, a)) return DMVS_EINVAL;
    a.train = (flags & DMVS_BN_TRAIN) ? 1 : 0;
    if (a.train && a.n < 2) return DMVS_EINVAL;
    if (!(eps >= 0.f) || !(momentum >= 0.f && momentum <= 1.f)) return DMVS_EINVAL;
    a.relu = (flags & DMVS_RELU) ? 1 : 0;
    a.x = x; a.gamma = gamma; a.beta = beta; a.out = y; a.mean = mean; a.invstd = invstd; a.ws = workspace;
    a.run_mean = running_mean; a.run_var = running_var; a.mean_in = running_mean; a.var_in = running_var;
    a.momentum = momentum; a.eps = eps;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = V % 4 == 0 && bn::aligned16(x) && bn::aligned16(y);
    const dim3 grid((unsigned)(C * a.S));
    if (a.train) {
        if (vec) bn::bn_stats_kernel<4><<<grid, bn::kLanes, 0, st>>>(a);
        else bn::bn_stats_kernel<1><<<grid, bn::kLanes, 0, st>>>(a);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    }
    if (vec) bn::bn_apply_kernel<4><<<grid, bn::kLanes, 0, st>>>(a);
    else bn::bn_apply_kernel<1><<<grid, bn::kLanes, 0, st>>>(a);
    DMVS_LAUNCH_CHECK();
}

extern "C" int dmvs_bn_relu_backward(const float* x, const float* gy, const float* gamma, const float* beta, const float* mean,
                                     const float* invstd, float* gx, float* g_gamma, float* g_beta, float* workspace, int B, int C,
                                     int V, int flags, dmvs_stream_t stream) {
    if (!x || !gy || !gamma || !beta || !mean || !invstd || !g_gamma || !g_beta || !workspace) return DMVS_EINVAL;   // gx may be NULL
    if (flags & ~(DMVS_RELU | DMVS_BN_TRAIN)) return DMVS_EINVAL;
    if (!bn::channels_ok(C)) return DMVS_EINVAL;
    bn::Args a = {};
    if (!bn::geometry(B, C, V, a)) return DMVS_EINVAL;
    a.train = (flags & DMVS_BN_TRAIN) ? 1 : 0;
    if (a.train && a.n < 2) return DMVS_EINVAL;
    a.relu = (flags & DMVS_RELU) ? 1 : 0;
    a.x = x; a.gy = gy; a.gamma = gamma; a.beta = beta; a.mean_in = mean; a.var_in = invstd; a.out = gx;
    a.g_gamma = g_gamma; a.g_beta = g_beta; a.ws = workspace;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = V % 4 == 0 && bn::aligned16(x) && bn::aligned16(gy) && (!gx || bn::aligned16(gx));
    const dim3 grid((unsigned)(C * a.S));
    if (vec) bn::bn_bwd_reduce_kernel<4><<<grid, bn::kLanes, 0, st>>>(a);
    else bn::bn_bwd_reduce_kernel<1><<<grid, bn::kLanes, 0, st>>>(a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    if (!gx) bn::bn_bwd_fold_kernel<false><<<dim3((unsigned)C), 64, 0, st>>>(a);
    else if (vec) bn::bn_bwd_apply_kernel<4><<<grid, bn::kLanes, 0, st>>>(a);
    else bn::bn_bwd_apply_kernel<1><<<grid, bn::kLanes, 0, st>>>(a);
    DMVS_LAUNCH_CHECK();
}

#include "batchnorm_sync.h"
