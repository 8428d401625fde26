// K5, synchronised statistics: the fold kernel of a rank's moments and the four C entries around the host's two all-gathers -- included
// at the end of batchnorm.h, whose header comment has the launch sequence.  The sync forms of the apply and fold kernels are template
// arguments of K5's own kernels there.
#pragma once

namespace bn {

// this rank's moments of every channel from the partials of bn_stats_kernel: (n_r, mean_r, M2_r about mean_r), one workgroup per channel
__global__ __launch_bounds__(64) void bn_moments_kernel(Args a) {
    __shared__ double part[2 * kMaxShares];
    double f0, f1;
    fold(a, blockIdx.x, part, f0, f1);
    if (threadIdx.x == 0) {
        const double n = (double)a.n, m2 = f1 - f0 * f0 / n;
        double* o = a.dout + 3 * (size_t)blockIdx.x;
        o[0] = n;
        o[1] = (double)a.ws[(size_t)a.C * a.S * 2 + blockIdx.x] + f0 / n;
        o[2] = m2 > 0.0 ? m2 : 0.0;
    }
}

// The gathered counts, read back and checked on the host (the one stream synchronisation of a sync forward): every n_r a positive
// integer, the same for every channel of a rank.  -> the global count in *N.
inline int gathered_count(const double* gathered, int R, int C, hipStream_t st, long* N) {
    double h[kMaxRanks * 64 * 3];
    if (hipError_t e = hipMemcpyAsync(h, gathered, sizeof(double) * 3 * R * C, hipMemcpyDeviceToHost, st); e != hipSuccess) return (int)e;
    if (hipError_t e = hipStreamSynchronize(st); e != hipSuccess) return (int)e;
    long total = 0;
    for (int r = 0; r < R; ++r) {
        const double n = h[(size_t)r * C * 3];
        if (!(n >= 1.0 && n <= 2147483647.0) || n != (double)(long)n) return DMVS_EINVAL;
        for (int c = 1; c < C; ++c)
            if (h[((size_t)r * C + c) * 3] != n) return DMVS_EINVAL;
        total += (long)n;
    }
    *N = total;
    return 0;
}

}  // namespace bn

extern "C" int dmvs_bn_sync_moments(const float* x, double* moments, float* workspace, int B, int C, int V, dmvs_stream_t stream) {
    if (!x || !moments || !workspace) return DMVS_EINVAL;
    if (!bn::channels_ok(C)) return DMVS_EINVAL;
    bn::Args a = {};
    if (!bn::geometry(B, C, V, a)) return DMVS_EINVAL;
    a.x = x; a.ws = workspace; a.dout = moments;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(C * a.S));
    if (V % 4 == 0 && bn::aligned16(x)) bn::bn_stats_kernel<4><<<grid, bn::kLanes, 0, st>>>(a);
    else bn::bn_stats_kernel<1><<<grid, bn::kLanes, 0, st>>>(a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    bn::bn_moments_kernel<<<dim3((unsigned)C), 64, 0, st>>>(a);
    DMVS_LAUNCH_CHECK();
}

extern "C" int dmvs_bn_sync_forward(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                                    const double* gathered, float* y, float* mean, float* invstd, long* n_total, int B, int C, int V,
                                    int R, float momentum, float eps, int flags, dmvs_stream_t stream) {
    if (!x || !gamma || !beta || !running_mean || !running_var || !gathered || !y || !mean || !invstd || !n_total) return DMVS_EINVAL;
    if (flags & ~DMVS_RELU) return DMVS_EINVAL;   // train mode is the only one: eval takes no statistics from anybody
    if (!bn::channels_ok(C) || R < 1 || R > bn::kMaxRanks) return DMVS_EINVAL;
    bn::Args a = {};
    if (!bn::geometry(B, C, V, a)) return DMVS_EINVAL;
    if (!(eps >= 0.f) || !(momentum >= 0.f && momentum <= 1.f)) return DMVS_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    long N = 0;
    if (int e = bn::gathered_count(gathered, R, C, st, &N); e) return e;
    if (N < 2) return DMVS_EINVAL;
    *n_total = N;
    a.train = 1; a.relu = (flags & DMVS_RELU) ? 1 : 0;
    a.x = x; a.gamma = gamma; a.beta = beta; a.out = y; a.mean = mean; a.invstd = invstd;
    a.run_mean = running_mean; a.run_var = running_var; a.momentum = momentum; a.eps = eps;
    a.gathered = gathered; a.R = R;
    const dim3 grid((unsigned)(C * a.S));
    if (V % 4 == 0 && bn::aligned16(x) && bn::aligned16(y)) bn::bn_apply_kernel<4, true><<<grid, bn::kLanes, 0, st>>>(a);
    else bn::bn_apply_kernel<1, true><<<grid, bn::kLanes, 0, st>>>(a);
    DMVS_LAUNCH_CHECK();
}

extern "C" int dmvs_bn_sync_backward_sums(const float* x, const float* gy, const float* gamma, const float* beta, const float* mean,
                                          const float* invstd, double* sums, float* g_gamma, float* g_beta, float* workspace, int B,
                                          int C, int V, int flags, dmvs_stream_t stream) {
    if (!x || !gy || !gamma || !beta || !mean || !invstd || !sums || !g_gamma || !g_beta || !workspace) return DMVS_EINVAL;
    if (flags & ~DMVS_RELU) return DMVS_EINVAL;
    if (!bn::channels_ok(C)) return DMVS_EINVAL;
    bn::Args a = {};
    if (!bn::geometry(B, C, V, a)) return DMVS_EINVAL;
    a.train = 1; a.relu = (flags & DMVS_RELU) ? 1 : 0;
    a.x = x; a.gy = gy; a.gamma = gamma; a.beta = beta; a.mean_in = mean; a.var_in = invstd;
    a.g_gamma = g_gamma; a.g_beta = g_beta; a.ws = workspace; a.dout = sums;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(C * a.S));
    if (V % 4 == 0 && bn::aligned16(x) && bn::aligned16(gy)) bn::bn_bwd_reduce_kernel<4><<<grid, bn::kLanes, 0, st>>>(a);
    else bn::bn_bwd_reduce_kernel<1><<<grid, bn::kLanes, 0, st>>>(a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    bn::bn_bwd_fold_kernel<true><<<dim3((unsigned)C), 64, 0, st>>>(a);
    DMVS_LAUNCH_CHECK();
}

extern "C" int dmvs_bn_sync_backward_apply(const float* x, const float* gy, const float* gamma, const float* beta, const float* mean,
                                           const float* invstd, const double* gathered, float* gx, int B, int C, int V, int R, long N,
                                           int flags, dmvs_stream_t stream) {
    if (!x || !gy || !gamma || !beta || !mean || !invstd || !gathered || !gx) return DMVS_EINVAL;
    if (flags & ~DMVS_RELU) return DMVS_EINVAL;
    if (!bn::channels_ok(C) || R < 1 || R > bn::kMaxRanks) return DMVS_EINVAL;
    bn::Args a = {};
    if (!bn::geometry(B, C, V, a)) return DMVS_EINVAL;
    if (N < 2 || N < a.n) return DMVS_EINVAL;   // the global count holds this rank's own
    a.train = 1; a.relu = (flags & DMVS_RELU) ? 1 : 0;
    a.x = x; a.gy = gy; a.gamma = gamma; a.beta = beta; a.mean_in = mean; a.var_in = invstd; a.out = gx;
    a.gathered = gathered; a.R = R; a.N = (double)N;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(C * a.S));
    if (V % 4 == 0 && bn::aligned16(x) && bn::aligned16(gy) && bn::aligned16(gx)) bn::bn_bwd_apply_kernel<4, true><<<grid, bn::kLanes, 0, st>>>(a);
    else bn::bn_bwd_apply_kernel<1, true><<<grid, bn::kLanes, 0, st>>>(a);
    DMVS_LAUNCH_CHECK();
}
