// N4: geometric-consistency check of one (reference, source) depth-map pair, fused into one kernel.
//
// Replaces reproject_with_depth_pytorch + check_geometric_consistency(_pytorch)
// (/root/reference/filter/pcd.py:151-242): project every reference pixel with its depth into the source view,
// bilinearly sample the source depth map there (grid_sample bilinear / zeros / align_corners=True, i.e. at the
// projected pixel coordinate), lift the sample back into the reference view, and keep the pixel when the
// reprojection lands within `dist_thresh` px and the depths agree to `rel_thresh` (1 px / 1 % in the reference).
// The reference materialises ~15 [H*W]-sized temporaries per pair; here: one pass, HBM-bound
// (reads 2 depth maps, writes mask + reprojected depth, accumulates the per-pixel vote and depth sums that
// filter_depth (pcd.py:283-300) builds with numpy).
//
// The chained 3x3 / 4x4 products of the reference are folded on the host (fp64, rounded once) into
//   P[0..11]  A1 (3x3), b1 (3):  K_src * xyz_src            = A1 * (x, y, 1) * d_ref + b1
//   P[12..23] A2 (3x3), t2 (3):  xyz_reprojected (ref cam)  = A2 * (xs, ys, 1) * d_sampled + t2
//   P[24..32] K_ref (3x3)
#include "common.h"

// LADDER: the dynamic-threshold variant of the Tanks&Temples filter (filter/dypcd_tanks.py:164-184): nine gates
// (dist < i * dist_base and rel < i * rel_base, i = 2..10) are evaluated on the same reprojection; level_votes[i-2]
// accumulates gate i per pixel, the last gate (i = 10) plays the role of the single gate for mask / depth / sums.
// That variant does not patch zero reference depths (rel = |d_reproj - d| / d is inf / NaN there: all gates false).
// One (reference pixel, source view) pair: the projection, the four taps of the bilinear sample, the lift back and the
// gates, shared by the per-pair kernels below and the per-view fused pass (fuse_view_kernel).  Returns the verdict of the
// single gate (static) or of the last gate i = 10 (LADDER) and sets `rz` to the reprojected depth; `gate(i, ok)` sees every
// gate i = 2..10 of the ladder in order (unused by the static variant).
template <bool LADDER, typename Gate>
__device__ __forceinline__ bool geo_pair(float fx, float fy, float d, const float* depth_src,
                                         const float* P, int H, int W, float dist_thresh, float rel_thresh,
                                         float& rz, Gate&& gate) {
    // reference pixel -> source image
    const float hx = (P[0] * fx + P[1] * fy + P[2]) * d + P[9];
    const float hy = (P[3] * fx + P[4] * fy + P[5]) * d + P[10];
    const float hz = (P[6] * fx + P[7] * fy + P[8]) * d + P[11];
    const float xs = hx / hz, ys = hy / hz;
    // bilinear sample of the source depth at (xs, ys); taps outside the image contribute zero
    const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
    const float x0f = floorf(xs), y0f = floorf(ys);
    const float tx = xs - x0f, ty = ys - y0f;
    const bool x0in = (x0f >= 0.f) && (x0f <= wm1), x1in = (x0f >= -1.f) && (x0f <= wm1 - 1.f);
    const bool y0in = (y0f >= 0.f) && (y0f <= hm1), y1in = (y0f >= -1.f) && (y0f <= hm1 - 1.f);
    const int x0 = (int)fminf(fmaxf(x0f, 0.f), wm1), x1 = (int)fminf(fmaxf(x0f + 1.f, 0.f), wm1);
    const int y0 = (int)fminf(fmaxf(y0f, 0.f), hm1), y1 = (int)fminf(fmaxf(y0f + 1.f, 0.f), hm1);
    const float s00 = depth_src[(size_t)y0 * W + x0], s01 = depth_src[(size_t)y0 * W + x1];
    const float s10 = depth_src[(size_t)y1 * W + x0], s11 = depth_src[(size_t)y1 * W + x1];
    const float sd = ((x0in && y0in) ? (1.f - tx) * (1.f - ty) * s00 : 0.f) + ((x1in && y0in) ? tx * (1.f - ty) * s01 : 0.f) +
                     ((x0in && y1in) ? (1.f - tx) * ty * s10 : 0.f) + ((x1in && y1in) ? tx * ty * s11 : 0.f);
    // sampled source point -> reference camera
    const float rx = (P[12] * xs + P[13] * ys + P[14]) * sd + P[21];
    const float ry = (P[15] * xs + P[16] * ys + P[17]) * sd + P[22];
    rz = (P[18] * xs + P[19] * ys + P[20]) * sd + P[23];
    const float kx = P[24] * rx + P[25] * ry + P[26] * rz;
    const float ky = P[27] * rx + P[28] * ry + P[29] * rz;
    float kz = P[30] * rx + P[31] * ry + P[32] * rz;
    if (kz == 0.f) kz += 0.00001f;  // pcd.py:194
    const float xr = kx / kz, yr = ky / kz;
    const float dist = sqrtf((xr - fx) * (xr - fx) + (yr - fy) * (yr - fy));
    const float dref = (!LADDER && d == 0.f) ? 1e-4f : d;  // pcd.py:219 (the ladder variant divides by the raw depth)
    const float rel = fabsf(rz - dref) / dref;
    bool ok;
    if constexpr (LADDER) {
        // dist_thresh / rel_thresh carry the BASES; gate i compares with i * base (dypcd_tanks.py:179-181)
        ok = false;
#pragma unroll
        for (int i = 2; i <= 10; ++i) {
            ok = dist < (float)i * dist_thresh && rel < (float)i * rel_thresh;
            gate(i, ok);
        }
    } else
        ok = dist < dist_thresh && rel < rel_thresh;  // NaN compares false, as in the reference
    return ok;
}

template <bool LADDER>
__global__ __launch_bounds__(256) void geo_consistency_kernel(const float* __restrict__ depth_ref,
                                                              const float* __restrict__ depth_src,
                                                              const float* __restrict__ P, int H, int W,
                                                              float dist_thresh, float rel_thresh,
                                                              unsigned char* __restrict__ mask,
                                                              float* __restrict__ depth_reproj,
                                                              int* __restrict__ vote_sum, float* __restrict__ depth_sum,
                                                              int* __restrict__ level_votes) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const size_t pix = (size_t)y * W + x;
    float rz;
    const bool ok = geo_pair<LADDER>((float)x, (float)y, depth_ref[pix], depth_src, P, H, W, dist_thresh, rel_thresh, rz,
                                     [&](int i, bool g) {
                                         if (level_votes) level_votes[(size_t)(i - 2) * H * W + pix] += g ? 1 : 0;
                                     });
    if (mask) mask[pix] = ok ? 1 : 0;
    if (depth_reproj) depth_reproj[pix] = ok ? rz : 0.f;
    if (vote_sum) vote_sum[pix] += ok ? 1 : 0;
    if (depth_sum) depth_sum[pix] += ok ? rz : 0.f;
}

extern "C" int dmvs_geo_consistency(const float* depth_ref, const float* depth_src, const float* proj33, int H, int W,
                                    float dist_thresh, float rel_thresh, unsigned char* mask, float* depth_reproj,
                                    int* vote_sum, float* depth_sum, dmvs_stream_t stream) {
    if (!depth_ref || !depth_src || !proj33 || H < 1 || W < 1) return DMVS_EINVAL;
    dim3 grid(ceil_div(W, 256), H);
    geo_consistency_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(depth_ref, depth_src, proj33, H, W, dist_thresh,
                                                                         rel_thresh, mask, depth_reproj, vote_sum, depth_sum, nullptr);
    DMVS_LAUNCH_CHECK();
}

extern "C" int dmvs_geo_consistency_ladder(const float* depth_ref, const float* depth_src, const float* proj33, int H,
                                           int W, float dist_base, float rel_base, int* level_votes,
                                           unsigned char* mask, float* depth_reproj, int* vote_sum, float* depth_sum,
                                           dmvs_stream_t stream) {
    if (!depth_ref || !depth_src || !proj33 || H < 1 || W < 1) return DMVS_EINVAL;
    dim3 grid(ceil_div(W, 256), H);
    geo_consistency_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(depth_ref, depth_src, proj33, H, W, dist_base,
                                                                        rel_base, mask, depth_reproj, vote_sum, depth_sum, level_votes);
    DMVS_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------------------------------
// The per-view fused pass (scan-level fusion, fusion.ScanFusion): ONE launch takes a reference view against all of its
// sources.  A thread owns a pixel and keeps the vote count, the nine ladder counts and the fp32 depth sum in registers
// while it walks the sources in pair order (the per-pair kernels' read-modify-writes of vote_sum / depth_sum /
// level_votes in HBM, same arithmetic: geo_pair), then finishes the pixel the way fusion.ViewFilter.finish does:
// photometric mask, geometric mask, final mask, averaged depth.  Pixels are numbered row-major and a workgroup owns
// FUSE_WG consecutive ones, so the per-workgroup counts of final pixels, scanned, place every point at its
// torch.nonzero position (emit kernel).  No atomics: order and bits do not depend on timing.
constexpr int FUSE_WG = 256;

struct FuseViewArgs {
    const float* depth_ref;
    const float *conf3, *conf2, *conf1;
    int H, W, nsrc, thres_view;
    float t1, t2, t3, dist, rel;
    unsigned char* masks;  // [3][H][W] photo, geo, final as 0 / 255
    float* depth_avg;      // [H][W] fp32
    double* depth_avg64;   // [H][W] fp64, written at final pixels only
    int* counts;           // [workgroups] final pixels per workgroup
    const float* src[DMVS_FUSE_MAX_SRC];
    float proj[DMVS_FUSE_MAX_SRC][33];
};

template <bool LADDER>
__global__ __launch_bounds__(FUSE_WG) void fuse_view_kernel(const FuseViewArgs a) {
    __shared__ int wave_n[FUSE_WG / 64];
    const int HW = a.H * a.W;
    const int p = blockIdx.x * FUSE_WG + threadIdx.x;
    bool fin = false;
    if (p < HW) {
        const int x = p % a.W, y = p / a.W;
        const float d = a.depth_ref[p];
        int votes = 0, lv[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        float sum = 0.f;
        for (int s = 0; s < a.nsrc; ++s) {
            float rz;
            const bool ok = geo_pair<LADDER>((float)x, (float)y, d, a.src[s], a.proj[s], a.H, a.W, a.dist, a.rel, rz,
                                             [&](int i, bool g) { lv[i - 2] += g ? 1 : 0; });
            votes += ok ? 1 : 0;
            sum += ok ? rz : 0.f;  // fp32, in source order from 0, as depth_sum accumulates
        }
        const bool photo = a.conf3[p] > a.t3 && a.conf2[p] > a.t2 && a.conf1[p] > a.t1;
        bool geo;
        if constexpr (LADDER) {
            // at least i views under gate i, for any i in [2, nsrc]; or votes >= nsrc + 1 (never true, kept as in finish)
            geo = votes >= a.nsrc + 1;
#pragma unroll
            for (int i = 2; i <= 10; ++i) geo = geo || (i <= a.nsrc && lv[i - 2] >= i);
        } else
            geo = votes >= a.thres_view;
        fin = photo && geo;
        // the static filter averages with the zero-patched reference depth (pcd.py:235); fp32 sum, fp64 division
        const float d_base = (!LADDER && d == 0.f) ? 1e-4f : d;
        const double avg = (double)(sum + d_base) / (double)(votes + 1);
        a.masks[p] = photo ? 255 : 0;
        a.masks[(size_t)HW + p] = geo ? 255 : 0;
        a.masks[2 * (size_t)HW + p] = fin ? 255 : 0;
        a.depth_avg[p] = (float)avg;
        if (fin) a.depth_avg64[p] = avg;
    }
    const unsigned long long m = __ballot(fin);
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
#pragma unroll
        for (int w = 0; w < FUSE_WG / 64; ++w) n += wave_n[w];
        a.counts[blockIdx.x] = n;
    }
}

// Exclusive scan of the per-workgroup counts by one workgroup: offsets[b] = sum of counts[0..b), offsets[nblk] = total.
__global__ __launch_bounds__(FUSE_WG) void fuse_scan_kernel(const int* __restrict__ counts, int nblk,
                                                            int* __restrict__ offsets) {
    __shared__ int buf[FUSE_WG];
    int carry = 0;
    for (int base = 0; base < nblk; base += FUSE_WG) {
        const int i = base + threadIdx.x;
        const int v = i < nblk ? counts[i] : 0;
        buf[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < FUSE_WG; off <<= 1) {  // Hillis-Steele inclusive scan
            const int t = threadIdx.x >= off ? buf[threadIdx.x - off] : 0;
            __syncthreads();
            buf[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < nblk) offsets[i] = carry + buf[threadIdx.x] - v;
        carry += buf[FUSE_WG - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) offsets[nblk] = carry;
}

struct FuseEmitArgs {
    const unsigned char* final_mask;  // [H][W], nonzero = final
    const double* depth_avg64;
    const int* offsets;
    int H, W;
    double kinv[9], einv[16];
    float* xyz;  // [total][3]
};

// World point of every final pixel at its row-major rank: Einv . [Kinv . (x d, y d, d); 1] in fp64 (ViewFilter.finish),
// rounded to fp32 last.  The rank is the workgroup's offset + the earlier waves' counts + the lanes below (v_mbcnt).
__global__ __launch_bounds__(FUSE_WG) void fuse_emit_kernel(const FuseEmitArgs a) {
    __shared__ int wave_n[FUSE_WG / 64];
    const int HW = a.H * a.W;
    const int p = blockIdx.x * FUSE_WG + threadIdx.x;
    const bool fin = p < HW && a.final_mask[2 * (size_t)HW + p] != 0;
    const unsigned long long m = __ballot(fin);
    const int lane_rank = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wave_n[wave] = __popcll(m);
    __syncthreads();
    if (!fin) return;
    int rank = a.offsets[blockIdx.x] + lane_rank;
    for (int w = 0; w < wave; ++w) rank += wave_n[w];
    const double d = a.depth_avg64[p];
    const double v0 = (double)(p % a.W) * d, v1 = (double)(p / a.W) * d, v2 = d;
    double c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = fma(a.kinv[3 * i + 2], v2, fma(a.kinv[3 * i + 1], v1, a.kinv[3 * i] * v0));
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double w = fma(a.einv[4 * i + 3], 1.0, fma(a.einv[4 * i + 2], c[2], fma(a.einv[4 * i + 1], c[1], a.einv[4 * i] * c[0])));
        a.xyz[3 * (size_t)rank + i] = (float)w;
    }
}

extern "C" long dmvs_fuse_workgroups(int H, int W) {
    if (H < 1 || W < 1) return DMVS_EINVAL;
    return ((long)H * W + FUSE_WG - 1) / FUSE_WG;
}

extern "C" int dmvs_fuse_view(const float* depth_ref, const float* conf3, const float* conf2, const float* conf1, int H,
                              int W, int nsrc, const float* const* depth_src, const float* proj33, float t1, float t2,
                              float t3, int dynamic, int thres_view, float dist, float rel, unsigned char* masks,
                              float* depth_avg, double* depth_avg64, int* counts, dmvs_stream_t stream) {
    if (!depth_ref || !conf3 || !conf2 || !conf1 || !depth_src || !proj33 || !masks || !depth_avg || !depth_avg64 ||
        !counts || H < 1 || W < 1 || (long)H * W > 0x7fffffffL - FUSE_WG)
        return DMVS_EINVAL;
    // nine gates: the dynamic geo mask reads level i - 2 for i <= nsrc
    if (nsrc < 1 || nsrc > (dynamic ? 10 : DMVS_FUSE_MAX_SRC)) return DMVS_EINVAL;
    FuseViewArgs a;
    a.depth_ref = depth_ref;
    a.conf3 = conf3;
    a.conf2 = conf2;
    a.conf1 = conf1;
    a.H = H;
    a.W = W;
    a.nsrc = nsrc;
    a.thres_view = thres_view;
    a.t1 = t1;
    a.t2 = t2;
    a.t3 = t3;
    a.dist = dist;
    a.rel = rel;
    a.masks = masks;
    a.depth_avg = depth_avg;
    a.depth_avg64 = depth_avg64;
    a.counts = counts;
    for (int s = 0; s < DMVS_FUSE_MAX_SRC; ++s) {
        a.src[s] = s < nsrc ? depth_src[s] : nullptr;
        if (s < nsrc && !a.src[s]) return DMVS_EINVAL;
        for (int k = 0; k < 33; ++k) a.proj[s][k] = s < nsrc ? proj33[33 * s + k] : 0.f;
    }
    const int nblk = (int)dmvs_fuse_workgroups(H, W);
    if (dynamic)
        fuse_view_kernel<true><<<nblk, FUSE_WG, 0, (hipStream_t)stream>>>(a);
    else
        fuse_view_kernel<false><<<nblk, FUSE_WG, 0, (hipStream_t)stream>>>(a);
    DMVS_LAUNCH_CHECK();
}

extern "C" int dmvs_fuse_emit(const unsigned char* masks, const double* depth_avg64, const int* counts, int H, int W,
                              const double* kinv9, const double* einv16, int* offsets, float* xyz, dmvs_stream_t stream) {
    if (!masks || !depth_avg64 || !counts || !kinv9 || !einv16 || !offsets || !xyz || H < 1 || W < 1 ||
        (long)H * W > 0x7fffffffL - FUSE_WG)
        return DMVS_EINVAL;
    const int nblk = (int)dmvs_fuse_workgroups(H, W);
    fuse_scan_kernel<<<1, FUSE_WG, 0, (hipStream_t)stream>>>(counts, nblk, offsets);
    FuseEmitArgs a;
    a.final_mask = masks;
    a.depth_avg64 = depth_avg64;
    a.offsets = offsets;
    a.H = H;
    a.W = W;
    for (int k = 0; k < 9; ++k) a.kinv[k] = kinv9[k];
    for (int k = 0; k < 16; ++k) a.einv[k] = einv16[k];
    a.xyz = xyz;
    fuse_emit_kernel<<<nblk, FUSE_WG, 0, (hipStream_t)stream>>>(a);
    DMVS_LAUNCH_CHECK();
}

// N5: the point-cloud evaluation kernels (an extension of N4: what becomes of the fused cloud) live in a header of their own
#include "cloud_eval.h"

// N6: validation mode (what the depth maps are worth against ground truth): the dual-depth loss and the depth metrics
#include "validate.h"
