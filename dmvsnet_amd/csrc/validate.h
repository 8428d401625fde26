// N6: validation mode -- the dual-depth regression loss and the depth metrics on ground truth, one fused pass per stage.
// Device code, included at the end of fusion.hip (like cloud_eval.h: what becomes of the depth maps).
//
// Replaces the arithmetic of the reference's loss.py:5-80 (mvs_loss, mode "regression"), loss.py:106-159
// (Monte_Carlo_sampling_loss mode "center", regression_loss) and tools.py:159-201 (AbsDepthError_metrics, Thres_metrics).
//
// Arithmetic: every per-element term is fp32 in the reference's operation order (the library is built with -ffp-contract=off);
// sl1(d) = |d| < 1 ? 0.5 d d : |d| - 0.5; term = sl1 * weight.  Invalid pixels and cells are SELECTED out (v_cndmask, never a
// multiply by zero): a NaN under the mask reaches no sum.  Sums are fp64 per lane -> wave (xor tree) -> LDS -> one row of VAL_NP
// doubles per workgroup in the caller's workspace; the finishing kernel (one workgroup) adds the rows in a fixed order, divides in
// fp64, rounds each mean to fp32 and does the reference's fp32 adds.  No float atomics, one writer per output: two runs give the
// same bits.
//
// Shape: lane = column, a wave marches down VAL_ROWS rows (+ the row below for the 2x2 cells) and keeps the previous row's
// horizontal pair sums in registers; column x + 1 comes from lane + 1 (__shfl_down), so a column tile is 64 lanes for 63 owned
// columns (lane 63 is the overlap column: it only feeds lane 62).  Every plane is read once, except the overlap row / column.
//
// Cell centre: grid_sample at the centre of a 2x2 cell is a bilinear sample with four weights of 1/4; here the weights are exact:
// S = (((a00 + a01) + a10) + a11) * 0.25f, corners in grid_sample's order (nw, ne, sw, se).
#pragma once
#include "common.h"

constexpr int VAL_WG = 256;                 // 4 waves
constexpr int VAL_ROWS = 8;                 // rows a wave owns
constexpr int VAL_TILE = 63;                // columns a wave owns (64 lanes, one overlap column)
constexpr int VAL_NP = 24;                  // doubles per workgroup row of the workspace
// workspace row: [0..7] main sums, [8..15] refine sums (depth small, depth huge, var small, var huge, centre 1..4),
// [16] n, [17] n_cells, [18] abs_err_sum, [19] n_valid, [20..22] n above the three thresholds, [23] unused
constexpr int VAL_N = 16, VAL_NCELLS = 17, VAL_ABS = 18, VAL_NVALID = 19, VAL_GT = 20;

struct ValArgs {
    const float* dsp[2];  // main, refine [B][4][h][w]
    const float* gt;      // [B][h][w]
    const float* mask;    // [B][h][w], valid <=> > 0.5
    const float* depth;   // [B][h][w] or NULL
    int h, w;
    float weight, thres[3];
    double* ws;
};

__device__ __forceinline__ float val_sl1(float d) {
    const float a = fabsf(d);
    return a < 1.f ? 0.5f * a * a : a - 0.5f;
}
// torch.min / torch.max over the channel pair: a NaN in either operand comes out
__device__ __forceinline__ float val_min(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float val_max(float a, float b) { return (a > b || a != a) ? a : b; }

__device__ __forceinline__ double val_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <bool LOSS, bool METRICS>
__global__ __launch_bounds__(VAL_WG) void dual_depth_loss_kernel(const ValArgs a) {
    __shared__ double part[VAL_WG / 64][VAL_NP];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = blockIdx.x * VAL_TILE + lane;
    const int y0 = (blockIdx.y * (VAL_WG / 64) + wv) * VAL_ROWS;
    const int b = blockIdx.z;
    const bool in_x = x < a.w, own_x = lane < VAL_TILE && in_x;
    const size_t HW = (size_t)a.h * a.w;
    const float* gt_b = a.gt + b * HW;
    const float* mask_b = a.mask + b * HW;

    double sum[LOSS ? 16 : 1];
#pragma unroll
    for (int k = 0; k < (LOSS ? 16 : 1); ++k) sum[k] = 0.0;
    double abs_sum = 0.0;
    int n = 0, n_cells = 0, n_valid = 0, n_gt[3] = {0, 0, 0};

    // previous row: horizontal pair sums (own + right neighbour) of the eight surfaces and of gt, and the pair's validity
    float ph[LOSS ? 8 : 1], pg = 0.f;
    bool pv = false;
#pragma unroll
    for (int k = 0; k < (LOSS ? 8 : 1); ++k) ph[k] = 0.f;

    // One row's loads.  The address is clamped to the last row / column, so every load is in bounds and none sits behind a
    // branch: the next row's loads are issued before this row's arithmetic (the march is latency-bound, not bandwidth-bound).
    struct Row {
        float g, m, e, v[LOSS ? 8 : 1];
    };
    const int xc = in_x ? x : a.w - 1;
    auto load_row = [&](int y) {
        Row r;
        const size_t p = (size_t)(y < a.h ? y : a.h - 1) * a.w + xc;
        r.g = gt_b[p];
        r.m = mask_b[p];
        r.e = METRICS ? a.depth[b * HW + p] : 0.f;
        if (LOSS) {
#pragma unroll
            for (int k = 0; k < 8; ++k) r.v[LOSS ? k : 0] = a.dsp[k >> 2][((size_t)b * 4 + (k & 3)) * HW + p];
        }
        return r;
    };

    constexpr int NROWS = LOSS ? VAL_ROWS + 1 : VAL_ROWS;   // the loss needs the row below for the 2x2 cells
    Row next = load_row(y0);
#pragma unroll
    for (int r = 0; r < NROWS; ++r) {
        const int y = y0 + r;
        const Row cur = next;
        if (r + 1 < NROWS) next = load_row(y + 1);
        const bool in_y = y < a.h;                  // wave-uniform
        const float g = cur.g;
        const bool valid = in_x && in_y && cur.m > 0.5f;
        const bool own = valid && own_x && r < VAL_ROWS;   // this lane accounts for the pixel
        if (METRICS) {
            const float e = fabsf(cur.e - g);
            abs_sum += own ? (double)e : 0.0;
            n_valid += __popcll(__ballot(own));
#pragma unroll
            for (int t = 0; t < 3; ++t) n_gt[t] += __popcll(__ballot(own && e > a.thres[t]));
        }
        if (LOSS) {
            n += __popcll(__ballot(own));
            const bool cm = ((x ^ y) & 1) == 0;  // row % 2 == col % 2
            float ch[8];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
#pragma unroll
                for (int q = 0; q < 2; ++q) {    // q = 0: channels 0, 1 ("small"); q = 1: channels 2, 3 ("huge")
                    const float d0 = cur.v[LOSS ? 4 * s + 2 * q : 0], d1 = cur.v[LOSS ? 4 * s + 2 * q + 1 : 0];
                    const float t0 = val_sl1(d0 - g) * a.weight, t1 = val_sl1(d1 - g) * a.weight;
                    sum[8 * s + q] += own ? (double)t0 + (double)t1 : 0.0;
                    const float a0 = fabsf(d0 - g), a1 = fabsf(d1 - g);
                    const float var_gt = a0 < a1 ? a1 : a0;
                    const float tv = val_sl1(fabsf(d0 - d1) - var_gt) * a.weight;
                    sum[8 * s + 2 + q] += own ? (double)tv : 0.0;
                    const float mn = val_min(d0, d1), mx = val_max(d0, d1);
                    ch[4 * s + 2 * q] = cm ? mn : mx;       // where(cm, min, max)
                    ch[4 * s + 2 * q + 1] = cm ? mx : mn;   // where(~cm, min, max)
                }
            }
            // horizontal pair sums of this row; lane 63 gets its own value back and owns no cell
            const bool vr = __shfl_down((int)valid, 1) != 0;
            const bool cv = valid && vr && lane < VAL_TILE;
            const float gr = __shfl_down(g, 1);
            const float cg = g + gr;
            const bool cell = pv && cv && r > 0;
            n_cells += __popcll(__ballot(cell));
            const float gbar = ((pg + g) + gr) * 0.25f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float right = __shfl_down(ch[k], 1);
                const float sbar = ((ph[k] + ch[k]) + right) * 0.25f;
                const float t = val_sl1(sbar - gbar) * a.weight;
                sum[8 * (k >> 2) + 4 + (k & 3)] += cell ? (double)t : 0.0;
                ph[k] = ch[k] + right;
            }
            pg = cg;
            pv = cv;
        }
    }

    // wave -> LDS -> one row per workgroup
#pragma unroll
    for (int k = 0; k < (LOSS ? 16 : 1); ++k) sum[k] = val_wave_sum(sum[k]);
    abs_sum = val_wave_sum(abs_sum);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 16; ++k) part[wv][k] = LOSS ? sum[LOSS ? k : 0] : 0.0;
        part[wv][VAL_N] = (double)n;
        part[wv][VAL_NCELLS] = (double)n_cells;
        part[wv][VAL_ABS] = abs_sum;
        part[wv][VAL_NVALID] = (double)n_valid;
#pragma unroll
        for (int t = 0; t < 3; ++t) part[wv][VAL_GT + t] = (double)n_gt[t];
        part[wv][VAL_NP - 1] = 0.0;
    }
    __syncthreads();
    if (threadIdx.x < VAL_NP) {
        double s = part[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < VAL_WG / 64; ++k) s += part[k][threadIdx.x];
        const size_t row = ((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        a.ws[row * VAL_NP + threadIdx.x] = s;
    }
}

struct ValFinishArgs {
    const double* ws;
    int rows_per_image, B, loss, metrics;
    float* total_loss;       // [1], += the stage's contribution (NULL: not wanted)
    float* terms16;          // [16] or NULL
    long long* counts2;      // [2] or NULL: n, n_cells
    double* image_sums;      // [B][5] or NULL: abs_err_sum, n_valid, n above each threshold
    float* metrics4;         // [4] or NULL: batch means of abs error and the three rates
};

// Sums of columns [col0, col0 + N) over rows [row0, row0 + nrows), in every thread: thread t adds rows t, t + 256, .. in order (all
// columns in one sweep, so the loads of a sweep are independent), then the xor tree per column, then the four waves in order.
template <int N>
__device__ __forceinline__ void val_column_sums(const double* __restrict__ ws, int row0, int nrows, int col0, double (*red)[VAL_NP],
                                                double* out) {
    double s[N];
#pragma unroll
    for (int c = 0; c < N; ++c) s[c] = 0.0;
    for (int i = threadIdx.x; i < nrows; i += VAL_WG) {
        const double* row = ws + (size_t)(row0 + i) * VAL_NP + col0;
#pragma unroll
        for (int c = 0; c < N; ++c) s[c] += row[c];
    }
    __syncthreads();                             // red is free again
#pragma unroll
    for (int c = 0; c < N; ++c) {
        const double v = val_wave_sum(s[c]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][c] = v;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < N; ++c) out[c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
}

__global__ __launch_bounds__(VAL_WG) void dual_depth_finish_kernel(const ValFinishArgs a) {
    __shared__ double red[VAL_WG / 64][VAL_NP];
    if (a.loss) {
        const int rows = a.rows_per_image * a.B;  // the loss pools the batch's pixels (loss.py:157: index by the whole mask)
        double v[18];
        val_column_sums<18>(a.ws, 0, rows, 0, red, v);
        const double n = v[VAL_N], nc = v[VAL_NCELLS];
        float contrib[2];
        for (int s = 0; s < 2; ++s) {
            float m[8];
            for (int k = 0; k < 8; ++k) {
                const double den = k < 2 ? 2.0 * n : (k < 4 ? n : nc);   // 0 / 0 = NaN on an empty mask, as torch's mean of nothing
                m[k] = (float)(v[8 * s + k] / den);
                if (a.terms16 && threadIdx.x == 0) a.terms16[8 * s + k] = m[k];
            }
            const float loss_depth = 2.f * m[0] + 2.f * m[1];            // loss.py:25-26
            const float loss_m = ((m[4] + m[5]) + m[6]) + m[7];          // loss.py:44-47
            contrib[s] = ((loss_depth + m[2]) + m[3]) + loss_m;          // loss.py:49
        }
        if (threadIdx.x == 0) {
            if (a.total_loss) {
                float t = a.total_loss[0];
                t += contrib[0];   // main first, then refine (loss.py:49, 80)
                t += contrib[1];
                a.total_loss[0] = t;
            }
            if (a.counts2) {
                a.counts2[0] = (long long)n;
                a.counts2[1] = (long long)nc;
            }
        }
    }
    if (a.metrics) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int b = 0; b < a.B; ++b) {
            double v[5];
            val_column_sums<5>(a.ws, b * a.rows_per_image, a.rows_per_image, VAL_ABS, red, v);
            if (a.image_sums && threadIdx.x == 0)
                for (int k = 0; k < 5; ++k) a.image_sums[5 * b + k] = v[k];
            // per image, an empty image counts 0 (tools.py:160-171), then the mean over the batch in fp32
            acc[0] += v[1] > 0.0 ? (float)(v[0] / v[1]) : 0.f;
            for (int t = 0; t < 3; ++t) acc[1 + t] += v[1] > 0.0 ? (float)v[2 + t] / (float)v[1] : 0.f;
        }
        if (a.metrics4 && threadIdx.x == 0)
            for (int k = 0; k < 4; ++k) a.metrics4[k] = acc[k] / (float)a.B;
    }
}

static inline bool val_dims_ok(int B, int h, int w) {
    // plane offsets are size_t; the grid's z is the batch, and a [B][4][h][w] tensor must stay addressable
    return B >= 1 && B <= 65535 && h >= 2 && w >= 2 && (long)h * w <= 0x7fffffffL / 4;
}

extern "C" long dmvs_dual_depth_loss_workspace(int B, int h, int w) {
    if (!val_dims_ok(B, h, w)) return DMVS_EINVAL;
    return (long)B * ceil_div(h, VAL_ROWS * (VAL_WG / 64)) * ceil_div(w, VAL_TILE) * VAL_NP;
}

extern "C" int dmvs_dual_depth_loss(const float* dsp_main, const float* dsp_refine, const float* gt, const float* mask,
                                    const float* depth, int B, int h, int w, float weight, const float* thres3,
                                    double* workspace, float* total_loss, float* terms16, long long* counts2,
                                    double* image_sums, float* metrics4, dmvs_stream_t stream) {
    if (!gt || !mask || !workspace || !val_dims_ok(B, h, w)) return DMVS_EINVAL;
    const bool loss = dsp_main || dsp_refine, metrics = depth != nullptr;
    if (!loss && !metrics) return DMVS_EINVAL;
    if (loss && (!dsp_main || !dsp_refine || !(total_loss || terms16 || counts2))) return DMVS_EINVAL;
    if (!loss && (total_loss || terms16 || counts2)) return DMVS_EINVAL;
    if (metrics && (!thres3 || !(image_sums || metrics4))) return DMVS_EINVAL;
    if (!metrics && (image_sums || metrics4)) return DMVS_EINVAL;
    ValArgs a;
    a.dsp[0] = dsp_main;
    a.dsp[1] = dsp_refine;
    a.gt = gt;
    a.mask = mask;
    a.depth = depth;
    a.h = h;
    a.w = w;
    a.weight = weight;
    for (int t = 0; t < 3; ++t) a.thres[t] = metrics ? thres3[t] : 0.f;
    a.ws = workspace;
    const dim3 grid(ceil_div(w, VAL_TILE), ceil_div(h, VAL_ROWS * (VAL_WG / 64)), B);
    if (loss && metrics)
        dual_depth_loss_kernel<true, true><<<grid, VAL_WG, 0, (hipStream_t)stream>>>(a);
    else if (loss)
        dual_depth_loss_kernel<true, false><<<grid, VAL_WG, 0, (hipStream_t)stream>>>(a);
    else
        dual_depth_loss_kernel<false, true><<<grid, VAL_WG, 0, (hipStream_t)stream>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const ValFinishArgs f{workspace, (int)(grid.x * grid.y), B, loss ? 1 : 0, metrics ? 1 : 0, total_loss, terms16, counts2,
                          image_sums, metrics4};
    dual_depth_finish_kernel<<<1, VAL_WG, 0, (hipStream_t)stream>>>(f);
    DMVS_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------------------------------ N6b
// Backward of the loss part of dual_depth_loss_kernel: d total / d dsp_main, d total / d dsp_refine, written as a GATHER.  A thread
// owns one pixel and collects its own terms (the four smooth-L1 depth terms, the two "variance" terms, in which var_gt depends on
// the estimate too) and a quarter of the derivative of each of the up to four 2x2 cells the pixel is a corner of, each term divided
// by the count the forward divided its sum by (n, n_cells: the forward's counts2).  The cell centres are recomputed in the forward's
// order, (((nw + ne) + sw) + se) * 0.25; min / max go to the channel val_min / val_max returned.  One writer per element, a fixed
// order of the four cells, no atomics: two runs give the same bits.  Masked pixels and cells are SELECTED out as in the forward: a
// masked pixel gets exactly 0, a NaN under the mask reaches nothing, and a count of zero (empty mask: the forward's loss is NaN)
// selects no term, so the gradient is all zeros, as autograd's is for the mean of nothing.
struct ValBwdArgs {
    const float* dsp[2];
    const float* gt;
    const float* mask;
    const long long* counts2;   // n, n_cells of the forward
    const float* g_total;       // [1] upstream gradient on the total
    float* g_dsp[2];
    int h, w;
    float weight;
};

// d sl1(u) / du
__device__ __forceinline__ float val_dsl1(float u) { return fabsf(u) < 1.f ? u : (u > 0.f ? 1.f : -1.f); }
__device__ __forceinline__ float val_sgn(float u) { return u > 0.f ? 1.f : (u < 0.f ? -1.f : 0.f); }

__global__ __launch_bounds__(256) void dual_depth_loss_bwd_kernel(const ValBwdArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= a.w) return;
    const size_t HW = (size_t)a.h * a.w, pix = (size_t)y * a.w + x;
    const float* gt_b = a.gt + b * HW;
    const float* mask_b = a.mask + b * HW;
    const double n = (double)a.counts2[0], nc = (double)a.counts2[1], gw = (double)a.g_total[0] * (double)a.weight;
    // total = sum over the two outputs of 2 m0 + 2 m1 + m2 + m3 + m4..m7; m0, m1 are means over 2n, m2, m3 over n, m4..m7 over n_cells
    const float kd = (float)(gw / n), kv = (float)(gw / n), kc = (float)(gw * 0.25 / nc);

    // 3x3 neighbourhood: validity, ground truth, addresses (clamped: every load is in bounds)
    bool nv[3][3];
    float ng[3][3];
    size_t np[3][3];
    bool ncm[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int yy = y + i - 1, xx = x + j - 1;
            const bool in = yy >= 0 && yy < a.h && xx >= 0 && xx < a.w;
            const int yc = yy < 0 ? 0 : (yy < a.h ? yy : a.h - 1), xc = xx < 0 ? 0 : (xx < a.w ? xx : a.w - 1);
            np[i][j] = (size_t)yc * a.w + xc;
            nv[i][j] = in && mask_b[np[i][j]] > 0.5f;
            ng[i][j] = gt_b[np[i][j]];
            ncm[i][j] = ((xx ^ yy) & 1) == 0;   // row % 2 == col % 2
        }
    const bool valid = nv[1][1];
    // the four cells the pixel is a corner of: cell (i, j) has the corners (i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1)
    bool cv[2][2];
    float gbar[2][2];
    bool anyc = false;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            cv[i][j] = nv[i][j] && nv[i][j + 1] && nv[i + 1][j] && nv[i + 1][j + 1];
            gbar[i][j] = (((ng[i][j] + ng[i][j + 1]) + ng[i + 1][j]) + ng[i + 1][j + 1]) * 0.25f;
            anyc = anyc || cv[i][j];
        }
    const float g = ng[1][1];

#pragma unroll
    for (int s = 0; s < 2; ++s) {
        if (!a.g_dsp[s]) continue;
        const float* dsp_b = a.dsp[s] + (size_t)b * 4 * HW;
        float* out_b = a.g_dsp[s] + (size_t)b * 4 * HW;
#pragma unroll
        for (int q = 0; q < 2; ++q) {   // q = 0: channels 0, 1 ("small"); q = 1: channels 2, 3 ("huge")
            const float* p0 = dsp_b + (size_t)(2 * q) * HW;
            const float* p1 = p0 + HW;
            const float d0 = p0[pix], d1 = p1[pix];
            // depth terms: 2 * mean over 2n of sl1(d - g) * weight
            float o0 = kd * val_dsl1(d0 - g), o1 = kd * val_dsl1(d1 - g);
            // variance term: sl1(|d0 - d1| - var_gt), var_gt the larger of |d0 - g|, |d1 - g| (the forward's where)
            const float a0 = fabsf(d0 - g), a1 = fabsf(d1 - g);
            const bool far1 = a0 < a1;
            const float du = kv * val_dsl1(fabsf(d0 - d1) - (far1 ? a1 : a0));
            const float sd = val_sgn(d0 - d1);
            o0 += du * (sd - (far1 ? 0.f : val_sgn(d0 - g)));
            o1 += du * (-sd - (far1 ? val_sgn(d1 - g) : 0.f));
            // cell centres: surfaces A = where(cm, min, max), B = where(~cm, min, max) of the pair
            float A[3][3], Bs[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const float e0 = p0[np[i][j]], e1 = p1[np[i][j]];
                    const float mn = val_min(e0, e1), mx = val_max(e0, e1);
                    A[i][j] = ncm[i][j] ? mn : mx;
                    Bs[i][j] = ncm[i][j] ? mx : mn;
                }
            float DA = 0.f, DB = 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float sa = (((A[i][j] + A[i][j + 1]) + A[i + 1][j]) + A[i + 1][j + 1]) * 0.25f;
                    const float sb = (((Bs[i][j] + Bs[i][j + 1]) + Bs[i + 1][j]) + Bs[i + 1][j + 1]) * 0.25f;
                    DA += cv[i][j] ? val_dsl1(sa - gbar[i][j]) : 0.f;
                    DB += cv[i][j] ? val_dsl1(sb - gbar[i][j]) : 0.f;
                }
            const bool min0 = d0 < d1 || d0 != d0, max0 = d0 > d1 || d0 != d0;   // val_min / val_max returned channel 0
            const float gmin = ncm[1][1] ? DA : DB, gmax = ncm[1][1] ? DB : DA;
            const float c0 = kc * ((min0 ? gmin : 0.f) + (max0 ? gmax : 0.f));
            const float c1 = kc * ((min0 ? 0.f : gmin) + (max0 ? 0.f : gmax));
            o0 += anyc ? c0 : 0.f;
            o1 += anyc ? c1 : 0.f;
            out_b[(size_t)(2 * q) * HW + pix] = valid ? o0 : 0.f;
            out_b[(size_t)(2 * q + 1) * HW + pix] = valid ? o1 : 0.f;
        }
    }
}

extern "C" int dmvs_dual_depth_loss_backward(const float* dsp_main, const float* dsp_refine, const float* gt, const float* mask,
                                             int B, int h, int w, float weight, const long long* counts2, const float* g_total,
                                             float* g_dsp_main, float* g_dsp_refine, dmvs_stream_t stream) {
    if (!dsp_main || !dsp_refine || !gt || !mask || !counts2 || !g_total || !val_dims_ok(B, h, w)) return DMVS_EINVAL;
    if (!g_dsp_main && !g_dsp_refine) return DMVS_EINVAL;
    ValBwdArgs a;
    a.dsp[0] = dsp_main;
    a.dsp[1] = dsp_refine;
    a.gt = gt;
    a.mask = mask;
    a.counts2 = counts2;
    a.g_total = g_total;
    a.g_dsp[0] = g_dsp_main;
    a.g_dsp[1] = g_dsp_refine;
    a.h = h;
    a.w = w;
    a.weight = weight;
    dual_depth_loss_bwd_kernel<<<dim3(ceil_div(w, 256), h, B), 256, 0, (hipStream_t)stream>>>(a);
    DMVS_LAUNCH_CHECK();
}
