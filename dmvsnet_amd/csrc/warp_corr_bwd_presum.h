// K1b, pre-summed scatter: the dSrc scatter of warp_corr_bwd.h with the adds of one workgroup summed in an LDS window first
// (included by warp_corr_bwd.h after both sinks, before the launcher; docs/kernels/K1b_warp_corr_backward.md, "Pre-summed
// scatter").  The plain scatter issues four global atomics per sample and channel and is bound by their NUMBER; the 256 samples of
// a 64 x 4 tile on the 8 planes of a chunk hit a few hundred texels between them.  So a workgroup
//   1. takes the bounding box of every in-image tap of its samples over the planes of its chunk (the ACTUAL taps, from
//      ref_order_taps: integer min / max per lane, a wave reduction, four rows in LDS) -- the window holds every in-image tap by
//      construction, whatever the camera and however the hypotheses differ per pixel;
//   2. box <= cap texels: clears a window of QPT * 4 channels x box in LDS, adds every addend there with a no-return LDS atomic
//      (fp32 for AtomicSink, the 64-bit integer q = rint(t * 2^k) for FixedSink -- the numbers the plain scatter adds, from the
//      same code, warp_bwd_sample_adds), then walks the window, consecutive lanes along a destination row, and issues ONE global
//      add through the sink per element that is not zero;
//   3. box > cap: does what the plain scatter does, global adds per tap (a workgroup-uniform decision);
//   4. no in-image tap: adds nothing.
// FixedSink: integer sums do not depend on grouping, so the result equals dmvs_warp_corr_backward_det's bit for bit.  AtomicSink:
// the same addends in another order of fp32 sums.
//
// Barriers: no lane leaves before the last one.  A lane outside the map has no samples and takes part in every barrier; the
// sink's idle exit is taken before the first barrier by the whole workgroup or by nobody (the scale comes from two words every
// lane reads).  LDS offsets come from clamped tap coordinates minus the box origin, and a tap is added only if it is in the image
// AND its offset is inside the box, so no coordinate (NaN, behind the camera, 1e9 away) can address outside the window.
#pragma once
#include <climits>

constexpr int kPresumTestCap = 256;   // variant bit 1: maps of a few tiles reach the windowed path, the direct path and their boundary

// Window capacity in texels.  A texel costs QPT * 4 accumulators: 32 B (fp32) / 64 B (int64) at QPT = 2.  1536 texels = 48 KB: three
// workgroups in a CU's 160 KB; 960 texels = 60 KB: two.  Both stay below the 64 KB a workgroup's static LDS may take.
template <class Sink> struct PresumCap;
template <> struct PresumCap<AtomicSink> { static constexpr int full = 1536; };
template <> struct PresumCap<FixedSink> { static constexpr int full = 960; };

// The adds of ONE sample, written once for both paths of the kernel below: the fp32 addend t = w_tap * gw with gw = g * r (two fp32
// products, no FMA), the four taps in ATen's order and the skip rule (a tap outside the image adds nothing) -- the text of
// warp_corr_bwd_src_kernel's loop body, which stays its own copy: routed through this function its instantiations keep their
// length but swap the operands of commutative v_mul_f32 (46 in the AtomicSink form), and they are to stay instruction for
// instruction what they were.  `base` is channel 0 of the destination -- a planar gradient (pitch W, channel stride H W) or an LDS
// window (pitch and stride of the box) -- and t's coordinates and range tests are relative to it; add(p, t) joins one addend.
template <int QPT, class T, class Add>
__device__ __forceinline__ void warp_bwd_sample_adds(T* base, int pitch, size_t cstride, const RefTaps& t, float g0, float g1,
                                                     const float4_t (&r)[QPT], Add add) {
    const bool in00 = t.x0in && t.y0in, in01 = t.x1in && t.y0in, in10 = t.x0in && t.y1in, in11 = t.x1in && t.y1in;
    T* const p00 = base + t.y0 * pitch + t.x0;
    T* const p01 = base + t.y0 * pitch + t.x1;
    T* const p10 = base + t.y1 * pitch + t.x0;
    T* const p11 = base + t.y1 * pitch + t.x1;
#pragma unroll
    for (int q = 0; q < QPT; ++q) {
        const float gw[4] = {g0 * r[q].x, g1 * r[q].y, g0 * r[q].z, g1 * r[q].w};   // dL/dwarped of the quad
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t c = (size_t)(q * 4 + j) * cstride;
            if (in00) add(p00 + c, t.w00 * gw[j]);
            if (in01) add(p01 + c, t.w01 * gw[j]);
            if (in10) add(p10 + c, t.w10 * gw[j]);
            if (in11) add(p11 + c, t.w11 * gw[j]);
        }
    }
}

template <class T>
__device__ __forceinline__ void presum_lds_add(T* p, T v) {   // return value unused: ds_add_f32 / ds_add_u64
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ int presum_wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int presum_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// path_counts: NULL, or three words the caller zeroed: workgroups windowed, direct, empty (lane 0 adds one).
template <int NQ, int QPT, int DCH, bool REV, class Sink>
__global__ __launch_bounds__(kBwdTX * kBwdTY) void warp_corr_bwd_src_presum_kernel(WarpBwdArgs a, int nqg, int nch, Sink sink, int cap,
                                                                                    unsigned* path_counts) {
    using Acc = typename Sink::Acc;
    constexpr int NCH = QPT * 4;
    __shared__ Acc win[PresumCap<Sink>::full * NCH];   // [NCH][box rows][box columns]
    __shared__ int part[kBwdTY][4];
    const int x = blockIdx.x * kBwdTX + threadIdx.x, y = blockIdx.y * kBwdTY + threadIdx.y;
    const int tid = threadIdx.y * kBwdTX + threadIdx.x;
    const int z = REV ? (int)(gridDim.z - 1 - blockIdx.z) : (int)blockIdx.z;
    const int chunk = z % nch, qg = (z / nch) % nqg, i = z / (nch * nqg);
    const int W = a.W, H = a.H;
    const typename Sink::Scale sc = sink.scale();
    if (Sink::idle(sc)) return;   // uniform, before any barrier
    const bool live = x < W && y < H;
    const int v = a.view[i], q0 = qg * QPT;
    const size_t plane = (size_t)H * W, pix = live ? (size_t)y * W + x : 0;
    const float fx = (float)x, fy = (float)y;
    const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
    const float half_w = wm1 / 2.0f, half_h = hm1 / 2.0f;
    const float inv = 2.0f / (float)(NQ * 4);
    const float* P = a.proj + v * 12;
    const int dbeg = chunk * DCH, dend = live ? min((chunk + 1) * DCH, a.D) : dbeg;   // a lane outside the map: no samples

    // 1. the box of every in-image tap.  The in-image taps of a sample are {in-image x} x {in-image y}.
    int xlo = INT_MAX, xhi = -1, ylo = INT_MAX, yhi = -1;
    for (int d = dbeg; d < dend; ++d) {
        const RefTaps t = ref_order_taps(P, fx, fy, a.depth[(size_t)d * plane + pix], wm1, hm1, half_w, half_h);
        if ((t.x0in || t.x1in) && (t.y0in || t.y1in)) {
            xlo = min(xlo, t.x0in ? t.x0 : t.x1);
            xhi = max(xhi, t.x1in ? t.x1 : t.x0);
            ylo = min(ylo, t.y0in ? t.y0 : t.y1);
            yhi = max(yhi, t.y1in ? t.y1 : t.y0);
        }
    }
    xlo = presum_wave_min(xlo); xhi = presum_wave_max(xhi);
    ylo = presum_wave_min(ylo); yhi = presum_wave_max(yhi);
    if (threadIdx.x == 0) {
        part[threadIdx.y][0] = xlo; part[threadIdx.y][1] = xhi;
        part[threadIdx.y][2] = ylo; part[threadIdx.y][3] = yhi;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kBwdTY; ++w) {
        xlo = min(xlo, part[w][0]); xhi = max(xhi, part[w][1]);
        ylo = min(ylo, part[w][2]); yhi = max(yhi, part[w][3]);
    }
    const int bx0 = __builtin_amdgcn_readfirstlane(xlo), bx1 = __builtin_amdgcn_readfirstlane(xhi);
    const int by0 = __builtin_amdgcn_readfirstlane(ylo), by1 = __builtin_amdgcn_readfirstlane(yhi);
    if (bx1 < bx0) {   // 4. no in-image tap: uniform; no barrier follows for this workgroup
        if (path_counts && tid == 0) atomicAdd(path_counts + 2, 1u);
        return;
    }
    const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1, n = bw * bh;   // bw <= W, bh <= H
    const bool windowed = n <= cap;
    if (path_counts && tid == 0) atomicAdd(path_counts + (windowed ? 0 : 1), 1u);

    float4_t r[QPT];
#pragma unroll
    for (int q = 0; q < QPT; ++q)
        r[q] = live ? reinterpret_cast<const float4_t*>(a.ref)[(size_t)(q0 + q) * plane + pix] : float4_t{0.f, 0.f, 0.f, 0.f};
    auto* const Gs = sink.dest(a, i, (size_t)(NQ * 4) * plane) + (size_t)q0 * 4 * plane;

    if (!windowed) {   // 3. the plain scatter
        for (int s = dbeg; s < dend; ++s) {
            const int d = REV ? dbeg + dend - 1 - s : s;
            const float depth = a.depth[(size_t)d * plane + pix];
            const float g0 = a.gsim[(size_t)d * plane + pix] * inv, g1 = a.gsim[(size_t)(a.D + d) * plane + pix] * inv;
            const RefTaps t = ref_order_taps(P, fx, fy, depth, wm1, hm1, half_w, half_h);
            warp_bwd_sample_adds<QPT>(Gs, W, plane, t, g0, g1, r, [&](auto* p, float tv) { Sink::add(p, tv, sc); });
        }
        return;
    }

    // 2. the window
    for (int e = tid; e < n * NCH; e += kBwdTX * kBwdTY) win[e] = Acc(0);
    __syncthreads();
    for (int s = dbeg; s < dend; ++s) {
        const int d = REV ? dbeg + dend - 1 - s : s;
        const float depth = a.depth[(size_t)d * plane + pix];
        const float g0 = a.gsim[(size_t)d * plane + pix] * inv, g1 = a.gsim[(size_t)(a.D + d) * plane + pix] * inv;
        RefTaps t = ref_order_taps(P, fx, fy, depth, wm1, hm1, half_w, half_h);
        // window coordinates; the box holds every in-image tap, the range tests keep any other offset out of the window
        t.x0 -= bx0; t.x1 -= bx0; t.y0 -= by0; t.y1 -= by0;
        t.x0in = t.x0in && (unsigned)t.x0 < (unsigned)bw; t.x1in = t.x1in && (unsigned)t.x1 < (unsigned)bw;
        t.y0in = t.y0in && (unsigned)t.y0 < (unsigned)bh; t.y1in = t.y1in && (unsigned)t.y1 < (unsigned)bh;
        warp_bwd_sample_adds<QPT>(win, bw, (size_t)n, t, g0, g1, r, [&](Acc* p, float tv) { presum_lds_add(p, Sink::quant(tv, sc)); });
    }
    __syncthreads();
    // the flush: consecutive lanes walk a window row, i.e. a contiguous run of a destination row
    for (int e = tid; e < n; e += kBwdTX * kBwdTY) {
        const int ry = e / bw, rx = e - ry * bw;
        auto* const dst = Gs + (by0 + ry) * W + (bx0 + rx);
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const Acc sum = win[c * n + e];
            if (sum != Acc(0)) Sink::flush(dst + (size_t)c * plane, sum, sc);
        }
    }
}

// what the entry hands down when the pre-summed scatter is asked for (NULL: the plain one)
struct WarpBwdPresum {
    unsigned* path_counts;   // NULL or three zeroed device words
};

static int presum_cap(bool det, int variant) {
    return (variant & 2) ? kPresumTestCap : det ? PresumCap<FixedSink>::full : PresumCap<AtomicSink>::full;
}

// variant bit 0: 4-plane chunks, reversed walk, reversed blockIdx.z; bit 1: the test capacity
template <int NQ, int QPT, class Sink>
static void launch_presum_scatter(const WarpBwdArgs& a, dim3 grid, dim3 block, int nqg, int nch, const Sink& sink, int variant,
                                  const WarpBwdPresum& ps, hipStream_t st) {
    const int cap = presum_cap(std::is_same<Sink, FixedSink>::value, variant);
    if (variant & 1) warp_corr_bwd_src_presum_kernel<NQ, QPT, 4, true><<<grid, block, 0, st>>>(a, nqg, nch, sink, cap, ps.path_counts);
    else warp_corr_bwd_src_presum_kernel<NQ, QPT, 8, false><<<grid, block, 0, st>>>(a, nqg, nch, sink, cap, ps.path_counts);
}

extern "C" long dmvs_warp_corr_backward_presum_cap(int C, int det, int variant) {
    if ((C != 8 && C != 16 && C != 32) || variant < 0 || variant > 3) return 0;
    return presum_cap(det != 0, variant);
}
