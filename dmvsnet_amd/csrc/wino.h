// Winograd F(2x2, 3x3) building blocks shared by K3w (conv3d_wino.hip), K3r (conv3d_coarse.hip) and K3z (conv3d_zmarch.hip):
// the transforms, the BatchNorm + ReLU store epilogue, the persistent tile walk and the loaders' range test, each written once.
// Force-inlined functions on registers only: no state, no LDS layout, no schedule -- those stay with the kernels.
// GRANULARITY.  These kernels sit at their register limits and hipcc's instruction order follows the order of the inlined IR: a
// helper that takes a kernel's arrays (a whole patch, a piece of four outputs with its store) measurably reorders the code around
// it, while one that takes and returns scalars does not.  So the arithmetic lives here as scalar functions (wino_bt4, wino_at0 /
// wino_at1, wino_bn_relu, wino_store16) plus the array forms that left every kernel's code object as it was (wino_read_patch,
// wino_in_row, wino_out_half, wino_out_xform); the loops over a tile's pieces stay in the kernels.  Compare the disassembly
// (profiles/wino_refactor_static.txt) before moving more in here.
//
//   Y = A^T [ sum_{ci,kz} (G g G^T) .* (B^T d B) ] A          per 2x2 output patch ("tile"), d = its 4x4 input patch
//   B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]   G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]   A^T = [1 1 1 0; 0 1 -1 -1]
//
// (G g G^T is the host's part: wino_filter in common.h.)  The build runs with -ffp-contract=off: every function below keeps
// ONE operation order, which is what makes the kernels' results reproducible bit for bit.
#pragma once
#include "common.h"

typedef float acc4_t __attribute__((ext_vector_type(4)));
typedef unsigned v4u_t __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------- input transform
// The 4 patch columns 3 + 2n .. 6 + 2n of tile n in a tile row that starts 4 floats left of the first output column, read as the
// three aligned pairs from p = row + 2 + 2n (ds_read_b64); the patch values are q[0].y, q[1].x, q[1].y, q[2].x.
__device__ __forceinline__ void wino_read_pairs(const float* p, float2_t* q) {
#pragma unroll
    for (int h = 0; h < 3; ++h) q[h] = *reinterpret_cast<const float2_t*>(p + 2 * h);
}
// B^T applied to a 4-vector: the column step (rows of the patch) and the row step (columns) of B^T d B alike
__device__ __forceinline__ void wino_bt4(float d0, float d1, float d2, float d3, float& t0, float& t1, float& t2, float& t3) {
    t0 = d0 - d2; t1 = d1 + d2; t2 = d2 - d1; t3 = d1 - d3;
}
// full form (K3w): read the lane's 4x4 patch d, rows `ixp` floats apart; then, in the kernel,
//     for x: wino_bt4(d[0][x], d[1][x], d[2][x], d[3][x], d[0][x], d[1][x], d[2][x], d[3][x]);          B^T d
//     for y: wino_bt4(d[y][0], d[y][1], d[y][2], d[y][3], v[4 y], v[4 y + 1], v[4 y + 2], v[4 y + 3]);   (.) B
__device__ __forceinline__ void wino_patch_row(const float2_t* q, float* d) { d[0] = q[0].y; d[1] = q[1].x; d[2] = q[1].y; d[3] = q[2].x; }
__device__ __forceinline__ void wino_read_patch(const float* p, int ixp, float (&d)[4][4]) {
#pragma unroll
    for (int y = 0; y < 4; ++y) {
        float2_t q[3];
        wino_read_pairs(p + y * ixp, q);
        wino_patch_row(q, d[y]);
    }
}
// per-row form (K3r, K3z: a wave owns transform row i): row i of B^T d is d[ra] + sg * d[rb], two of the four patch rows;
// q[0..2] = the pairs of patch row ra, q[3..5] = those of row rb (wino_read_pairs)
__device__ __forceinline__ void wino_in_row(float sg, const float2_t (&q)[6], float (&v)[4]) {
    const float t0 = fmaf(sg, q[3].y, q[0].y), t1 = fmaf(sg, q[4].x, q[1].x), t2 = fmaf(sg, q[4].y, q[1].y), t3 = fmaf(sg, q[5].x, q[2].x);
    wino_bt4(t0, t1, t2, t3, v[0], v[1], v[2], v[3]);
}

// --------------------------------------------------------------------------------------------------------- output transform
// the two rows of A^T applied to four values: used along both axes, on whole accumulators and on the waves' partial sums (the
// finishing row sum of K3r / K3z: output row 0 = wino_at0 over the transform rows 0..2, row 1 = wino_at1 over rows 1..3)
__device__ __forceinline__ float wino_at0(float m0, float m1, float m2) { return (m0 + m1) + m2; }
__device__ __forceinline__ float wino_at1(float m1, float m2, float m3) { return (m1 - m2) - m3; }
// wave-split half (K3r, K3z): the wave's transform row M[i][0..3] A -> the two output columns
__device__ __forceinline__ float2_t wino_out_half(float m0, float m1, float m2, float m3) {
    float2_t s;
    s.x = wino_at0(m0, m1, m2);
    s.y = wino_at1(m1, m2, m3);
    return s;
}
// full form (K3w): component r of the 16 accumulators m[4 i + j] -> A^T M A, the tile's 2x2 outputs: y0 = its first row, y1 = its second
__device__ __forceinline__ void wino_out_xform(const acc4_t (&m)[16], int r, float* y0, float* y1) {
    float s0[4], s1[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const float m0 = m[b][r], m1 = m[4 + b][r], m2 = m[8 + b][r], m3 = m[12 + b][r];
        s0[b] = wino_at0(m0, m1, m2);
        s1[b] = wino_at1(m1, m2, m3);
    }
    y0[0] = wino_at0(s0[0], s0[1], s0[2]);
    y0[1] = wino_at1(s0[1], s0[2], s0[3]);
    y1[0] = wino_at0(s1[0], s1[1], s1[2]);
    y1[1] = wino_at1(s1[1], s1[2], s1[3]);
}

// ----------------------------------------------------------------------------------------------------------------- epilogue
// BatchNorm scale / shift and ReLU (lo = 0 or -inf) of one value, as the bits the buffer stores take
__device__ __forceinline__ unsigned wino_bn_relu(float y, float sc, float sh, float lo) {
    return __builtin_bit_cast(unsigned, fmaxf(y * sc + sh, lo));
}
// A piece outside the tensor is stored at offset 2^31, which the buffer descriptor drops: off = in range ? byte offset : kWinoInvalid.
// KO: the kernel's development knock-out of its output stores (DMVS_WKO & 4, DMVS_ZKO & 2; the value test keeps the arithmetic alive).
constexpr unsigned kWinoInvalid = 0x80000000u;
template <bool KO>
__device__ __forceinline__ void wino_store16(__amdgpu_buffer_rsrc_t rs_out, v4u_t qv, unsigned off) {
    __builtin_amdgcn_raw_buffer_store_b128(qv, rs_out, (KO && qv.x != 0x12345678u) ? kWinoInvalid : off, 0, 0);
}

// ---------------------------------------------------------------------------------------------------------------- tile walk
// Persistent workgroups on the XCD-aware tile order of common.h (see xcd_grid there): the workgroup walks the virtual block ids
// vb = blockIdx.x, + gridDim.x, ...; gridDim.x is a multiple of 8, so vb % 8 stays its XCD, whose contiguous eighth of the tile
// list it works through.  How a list position splits into (x, y, z) is the kernel's business.
struct XcdTileWalk {
    int ntiles, per_xcd;
    __device__ __forceinline__ explicit XcdTileWalk(int ntiles_) : ntiles(ntiles_), per_xcd((ntiles_ + 7) >> 3) {}
    // position of virtual block vb in the tile list; false past the end of the XCD's eighth or of the list
    __device__ __forceinline__ bool id_of(int vb, int& id) const {
        const int q = vb >> 3;
        id = (vb & 7) * per_xcd + q;
        if (q >= per_xcd || id >= ntiles) return false;
        return true;
    }
};

// --------------------------------------------------------------------------------------- range test of the LDS-direct tile loads
// A lane's tile coordinates (NB of them, each < 64) packed one per byte are tested against [lo, hi] per axis in one go: with the
// guard bit 7 of every byte set, a byte-wise subtraction keeps the guard iff it did not borrow.
template <int NB>
struct ByteRange {
    static_assert(NB == 2 || NB == 3, "two or three coordinates");
    static constexpr unsigned kGuard = NB == 3 ? 0x808080u : 0x8080u;
    static constexpr unsigned kNever = NB == 3 ? 0x3f3f3fu : 0x3f3fu;     // a coordinate triple that fails every test (pad pieces)
    static constexpr unsigned kNothing = NB == 3 ? 0x7f7f7fu : 0x7f7fu;   // a lower bound no coordinate reaches
    static __device__ __forceinline__ unsigned pack(unsigned c0, unsigned c1, unsigned c2 = 0) { return c0 | (c1 << 8) | (c2 << 16); }
    static __device__ __forceinline__ unsigned pack_hi(unsigned c0, unsigned c1, unsigned c2 = 0) { return pack(c0, c1, c2) | kGuard; }
    static __device__ __forceinline__ bool in_range(unsigned v, unsigned lo, unsigned hi_guarded) {
        const unsigned ge = (v | kGuard) - lo, le = hi_guarded - v;
        return (ge & le & kGuard) == kGuard;
    }
};
