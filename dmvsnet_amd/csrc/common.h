// Shared helpers for libdmvs_hip.so (gfx950 only; no CUDA / multi-backend paths).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dmvs.h"

#define DMVS_LAUNCH_CHECK()                         \
    do {                                            \
        hipError_t e__ = hipGetLastError();         \
        return e__ == hipSuccess ? 0 : (int)e__;    \
    } while (0)

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// > 64 KB of dynamic LDS needs hipFuncAttributeMaxDynamicSharedMemorySize once per (device, kernel) -- and again when
// a later launch of the same kernel asks for more.  One process-wide, mutex-guarded table (conv3d_mfma.hip).
int dmvs_ensure_dynamic_lds(const void* kernel, size_t lds_bytes);

typedef float float4_t __attribute__((ext_vector_type(4)));
typedef float float2_t __attribute__((ext_vector_type(2)));

// XCD-aware tile order.  The dispatcher deals workgroups round-robin to the 8 XCDs (workgroup id % 8), each with
// its own 4 MB L2; with the natural blockIdx order the 6-26 neighbours whose halo a tile shares all sit on OTHER
// XCDs and every L2 pulls the halo over the fabric again (measured: the tile loads of a 3x3x3 layer run 2-2.6x
// faster with this remap).  Launch a 1-D grid of xcd_grid(n) workgroups; XCD k then walks the k-th contiguous
// eighth of the tile list.  Tile list order: x fastest, then z, then y when `z_fast` (3D kernels: the depth halo
// is the largest one and a (x, z) slab of tiles fits the L2), else x, y, z (per-slice 2D kernels).
static inline unsigned xcd_grid(int ntiles) { return 8u * (unsigned)((ntiles + 7) / 8); }

// Host side of every Winograd F(2x2, 3x3) filter packer (K3w, K3r, K3z): (G g G^T)[i][p] of one 3x3 filter g[ky * 3 + kx],
// formed in double in a fixed order (ky outer) and rounded once by the caller.
static inline double wino_filter(const double g[9], int i, int p) {
    static const double Gm[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    double u = 0.0;
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) u += Gm[i][ky] * Gm[p][kx] * g[ky * 3 + kx];
    return u;
}

// Zero-padding depth taps (dmvs_tune("zpad_skip")).  A 3x3x3 layer on a shallow volume multiplies whole planes of zero
// padding: on depth D, 2 of the 3 * D (output plane, depth tap) pairs of a stride-1 layer, 1 of 3 * D/2 of a stride-2 layer
// and 1 of 3 * D of a transposed one.  These products are exact zeros, so a kernel may leave them out (the live products keep
// their order: the result is value-equal for finite inputs).  zpad_live_mask is the ONE statement of which pairs are live;
// every skipping kernel derives its skip from it: per tile (K3w) or per unit (K3r) in scalar registers, or once on the host where
// the whole launch has the same dead taps (K3 on volumes of one output / input plane).  Skipping pays only where every wave that
// meets at a barrier skips the same work: a form in which only some waves of a workgroup skip was measured and dropped (K3's
// two-plane tiles, the `prob` head: docs/kernels/K3_conv_mfma.md, K2_prob_and_direct.md).
//   bit 3 * p + kz: plane p of the tile (p in [0, TZ), plane oz0 + p of the volume) takes a non-padding plane through tap kz
//   DMVS_ZFORM_S1: stride 1, pad 1; planes are OUTPUT planes of a depth-D volume, tap kz reads input plane z + kz - 1
//   DMVS_ZFORM_S2: stride 2, pad 1; planes are OUTPUT planes z < (D + 1) / 2, tap kz reads input plane 2 z + kz - 1 of D
//   DMVS_ZFORM_T2: transposed, stride 2, pad 1, output_padding 1 in the kernels' GATHER form on the input grid: planes are
//                  INPUT planes z < D; taps 1 and 2 (output planes 2 z and 2 z + 1) read plane z, tap 0 (output plane
//                  2 z + 1) reads plane z + 1 -- the scatter view's dead pair (input plane 0, tap 0 -> output plane -1) never
//                  appears in this form, the dead one is (plane D - 1, tap 0), which reads the padding plane D.
// A plane of the tile past the end of the volume has no live tap.  TZ <= 10.
enum { DMVS_ZFORM_S1 = 0, DMVS_ZFORM_S2 = 1, DMVS_ZFORM_T2 = 2 };
#ifdef __HIPCC__
__host__ __device__
#endif
constexpr unsigned zpad_live_mask(int form, int D, int oz0, int TZ) {
    unsigned m = 0;
    for (int p = 0; p < TZ; ++p) {
        const int z = oz0 + p;
        const int nplanes = form == DMVS_ZFORM_S2 ? (D + 1) / 2 : D;
        if (z < 0 || z >= nplanes) continue;
        for (int kz = 0; kz < 3; ++kz) {
            const int iz = form == DMVS_ZFORM_S1 ? z + kz - 1 : form == DMVS_ZFORM_S2 ? 2 * z + kz - 1 : (kz == 0 ? z + 1 : z);
            if (iz >= 0 && iz < D) m |= 1u << (3 * p + kz);
        }
    }
    return m;
}

// launches on input volumes up to this depth take the skipping instantiations.  From the layer table (config 2, one layer alone):
// depth 2 -14 .. -16 % (K3r conv4, K3w conv2), depth 4 -5 % (K3w) and -2 % (K3r), depth 8 +1 % (K3r conv4: 8 % dead pairs do
// not pay for the per-unit choice of a code copy) -- and deeper volumes must keep exactly the code they had.
constexpr int kZpadMaxDepth = 4;
extern long g_zpad_skip;   // layout.hip, dmvs_tune("zpad_skip")
static inline bool zpad_skip_wanted(int D) { return g_zpad_skip && D <= kZpadMaxDepth; }

#ifdef __HIPCC__
__device__ __forceinline__ bool xcd_tile(int nx, int ny, int nz, bool z_fast, int& bx, int& by, int& bz) {
    const int n = nx * ny * nz, per = (n + 7) >> 3;
    const int id = blockIdx.x, t = (id & 7) * per + (id >> 3);
    if (t >= n) return false;
    bx = t % nx;
    const int r = t / nx;
    if (z_fast) { bz = r % nz; by = r / nz; } else { by = r % ny; bz = r / ny; }
    return true;
}
#endif
