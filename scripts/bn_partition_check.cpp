// Stand-alone host check of K5's partition (dmvsnet_amd/csrc/batchnorm.h: shares_of / share_range behind dmvs_bn_plan and
// dmvs_bn_share_range), meant to be built with the host sanitizers and run on the CPU -- no GPU is touched:
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I dmvsnet_amd/csrc scripts/bn_partition_check.cpp -o /tmp/bn_partition_check && /tmp/bn_partition_check
//
// It walks the shapes of tests/test_bn_grad_gpu.py (and the limits of the index range) and verifies that the shares tile
// [0, B * V) exactly once, in order, on chunk boundaries.  Exit status 0 and the line "bn partition: ok" mean no finding.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "batchnorm.h"

long g_zpad_skip = 0;                                                  // common.h declares it; layout.hip is not linked here
int dmvs_ensure_dynamic_lds(const void*, size_t) { return 0; }

static int fail(const char* what, int C, int B, int V, int s) {
    std::fprintf(stderr, "bn partition: %s at C %d B %d V %d share %d\n", what, C, B, V, s);
    return 1;
}

static int walk(int C, int B, int V) {
    const long n = (long)B * V;
    const int S = dmvs_bn_plan(C, B, V);
    if (S < 1 || S > bn::kMaxWg / C) return fail("bad share count", C, B, V, S);
    std::vector<long> bounds;   // heap: out-of-range writes are the sanitizer's to see
    bounds.reserve(S + 1);
    long end = 0;
    for (int s = 0; s < S; ++s) {
        long lo = -1, hi = -1;
        if (dmvs_bn_share_range(C, B, V, s, &lo, &hi) != 0) return fail("refused", C, B, V, s);
        if (lo != end || hi <= lo) return fail("gap, overlap or empty share", C, B, V, s);
        if (lo % bn::kChunk || (hi % bn::kChunk && hi != n)) return fail("not on a chunk boundary", C, B, V, s);
        if (V % 4 == 0 && (lo % 4 || hi % 4)) return fail("not on a 16-byte boundary", C, B, V, s);
        bounds.push_back(lo);
        end = hi;
    }
    bounds.push_back(end);
    if (end != n || (int)bounds.size() != S + 1) return fail("does not end at B * V", C, B, V, S);
    long lo, hi;
    if (dmvs_bn_share_range(C, B, V, -1, &lo, &hi) != DMVS_EINVAL || dmvs_bn_share_range(C, B, V, S, &lo, &hi) != DMVS_EINVAL ||
        dmvs_bn_share_range(C, B, V, 0, nullptr, &hi) != DMVS_EINVAL)
        return fail("a bad share index or pointer was accepted", C, B, V, S);
    return 0;
}

int main() {
    const int chunk = bn::kChunk;
    int bad = 0, walked = 0;
    for (int C : {8, 16, 32, 64}) {
        const int smax = bn::kMaxWg / C;
        const int grid_v = smax * chunk * 8 / 2 + 148;
        const int shapes[][2] = {{1, 90}, {2, 90}, {1, 540}, {2, 540}, {1, 670}, {1, chunk + 4}, {1, 3 * chunk + 1}, {2, grid_v}, {1, 2},
                                 {1, chunk}, {1, chunk + 1}, {3, chunk}, {1, smax * chunk}, {1, smax * chunk + 1}, {7, 100 * chunk + 3},
                                 {1, 8 * 16 * 32}, {1, 4 * 8 * 16}, {1, 2 * 4 * 8}, {1, 8}, {1, 0x7fffffff - 4 * chunk - 8}, {16, 1 << 26}};
        for (const auto& bv : shapes) { bad += walk(C, bv[0], bv[1]); ++walked; }
        if (dmvs_bn_plan(C, 2, 1 << 30) != DMVS_EINVAL || dmvs_bn_plan(C, 1, 0x7fffffff) != DMVS_EINVAL || dmvs_bn_plan(C, 0, 8) != DMVS_EINVAL)
            bad += fail("an index range past 2^31 or an empty batch was accepted", C, 0, 0, 0);
    }
    if (dmvs_bn_plan(12, 1, 64) != DMVS_EINVAL || dmvs_bn_workspace(12, 1, 64) != 0) bad += fail("C = 12 was accepted", 12, 1, 64, 0);
    if (bad) return 1;
    std::printf("bn partition: ok (%d shapes)\n", walked);
    return 0;
}
