// Stand-alone host check of the weight-gradient kernels' share scheme (dmvsnet_amd/csrc/wgrad_share.h: grid, place, first_tile, decode,
// behind the geometry of K3g, K3h, K2g, K3k / K3d and K3f), meant to be built with the host sanitizers and run on the CPU -- no GPU is
// touched:
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I dmvsnet_amd/csrc scripts/wgrad_share_check.cpp -o /tmp/wgrad_share_check && /tmp/wgrad_share_check
//
// For every family's geometry it walks the volumes of that family's GPU tests and the limits (one tile, tiles = S, tiles = S + 1, just
// under 2^22 tiles) and verifies that every workgroup of the padded launch is idle or has a (block, share) of its own, that all
// blocks x S of them are taken, that the shares' ranges are non-empty and tile [0, tiles) once and in order, and that the tile decode
// is a bijection onto nx x ny x D.  Exit status 0 and the line "wgrad share: ok" mean no finding.
#include <cstdio>
#include <functional>
#include <vector>
#include "conv3d_wgrad_c2.h"
#include "conv2d_k5s2_bwd.h"   // (K3g and K3h come with it)
#include "conv2d_wgrad_fpn.h"

long g_zpad_skip = 0;                                                  // common.h declares it; layout.hip is not linked here
int dmvs_ensure_dynamic_lds(const void*, size_t) { return 0; }

using wshare::Grid;

struct Family {
    const char* name;
    int ty, tx, blocks;   // tile of the family's tile domain (K3h / K3k / K3d: the coarse grid), operand blocks
    int dmax;             // planes at which the family stops, by the tile count or by its own extent guard
    bool fine;            // its entry takes the fine extents, twice the tile domain's
    // the family's own geometry and plan entry for its entry arguments (D, H, W); rows x cols: the tile domain
    std::function<bool(int, int, int, Grid&, int&, int&, int&)> geo;
    std::vector<std::vector<int>> shapes;
};

static int fail(const char* what, const Family& f, int D, int H, int W, long at) {
    std::fprintf(stderr, "wgrad share: %s: %s at D %d H %d W %d (%ld)\n", f.name, what, D, H, W, at);
    return 1;
}

static int walk(const Family& f, int D, int H, int W) {
    Grid g;
    int rows, cols, plan;
    if (!f.geo(D, H, W, g, rows, cols, plan)) return fail("refused", f, D, H, W, 0);
    const long nt = (long)((cols + f.tx - 1) / f.tx) * ((rows + f.ty - 1) / f.ty) * D;
    const int smax = 256 / f.blocks, S = nt < smax ? (int)nt : smax;
    if (g.nx != (cols + f.tx - 1) / f.tx || g.ny != (rows + f.ty - 1) / f.ty || g.ntiles != nt || g.S != S || g.nwg != S * f.blocks)
        return fail("bad grid", f, D, H, W, g.ntiles);
    const int launched = 8 * ((g.nwg + 7) / 8);
    if (plan != g.ntiles * 512 + launched || launched > 256) return fail("bad plan", f, D, H, W, plan);
    // the places: every workgroup idle or on a (block, share) of its own, all of them taken
    std::vector<char> taken(g.nwg, 0);   // heap: out-of-range writes are the sanitizer's to see
    int idle = 0;
    for (int bid = 0; bid < launched; ++bid) {
        const int wg = wshare::place(g, bid);
        if (wg < 0) { ++idle; continue; }
        if (wg >= g.nwg || wg / f.blocks >= g.S || taken[wg]) return fail("a place out of range or taken twice", f, D, H, W, bid);
        taken[wg] = 1;
    }
    if (idle != launched - g.nwg) return fail("a (block, share) without a workgroup", f, D, H, W, idle);
    // the ranges: non-empty, [0, tiles) once and in order
    int end = 0;
    for (int s = 0; s < g.S; ++s) {
        const int lo = wshare::first_tile(g, s), hi = wshare::first_tile(g, s + 1);
        if (lo != end || hi <= lo) return fail("gap, overlap or empty share", f, D, H, W, s);
        end = hi;
    }
    if (end != g.ntiles) return fail("the shares do not end at the last tile", f, D, H, W, end);
    // the decode: x fastest, then y, then z, onto nx x ny x D
    std::vector<char> seen(g.ntiles, 0);
    for (int tile = 0; tile < g.ntiles; ++tile) {
        const wshare::Tile t = wshare::decode(g, tile);
        if (t.bx < 0 || t.bx >= g.nx || t.by < 0 || t.by >= g.ny || t.z < 0 || t.z >= D) return fail("a tile outside the grid", f, D, H, W, tile);
        const long at = ((long)t.z * g.ny + t.by) * g.nx + t.bx;
        if (at != tile || seen[at]) return fail("the decode is no bijection", f, D, H, W, tile);
        seen[at] = 1;
    }
    return 0;
}

int main() {
    using V = std::vector<std::vector<int>>;
    const V vol3 = {{1, 5, 7}, {3, 19, 35}, {2, 20, 36}, {5, 9, 131}, {2, 6, 33}, {2, 9, 13}, {9, 41, 67}, {7, 33, 65}};
    const V vol_s2 = {{1, 3, 4}, {2, 5, 9}, {3, 10, 18}, {2, 5, 67}, {9, 41, 67}, {5, 21, 67}, {2, 48, 176}};
    const V vol_c2 = {{1, 3, 4}, {2, 5, 9}, {3, 10, 18}, {2, 5, 67}, {2, 9, 13}, {9, 41, 131}};
    const V planes = {{1, 1, 1}, {1, 2, 3}, {1, 5, 8}, {1, 17, 67}, {2, 18, 70}, {2, 33, 130}, {1, 9, 70}, {3, 40, 300}, {1, 9, 40}};
    V k5 = planes, fpn = planes;
    k5.push_back({3, 163, 259});
    fpn.push_back({3, 81, 131});
    std::vector<Family> fams;
    for (int C : {16, 32, 64})
        fams.push_back({"K3g", wgrad::kTY, wgrad::kTX, wgrad::blocks_of(C), 1 << 22, false, [C](int D, int H, int W, Grid& g, int& r, int& c, int& p) {
            wgrad::Args a{}; r = H; c = W; p = dmvs_conv3d_wgrad_plan(C, D, H, W, 3);
            const bool ok = wgrad::geometry(C, D, H, W, a); g = a.g; return ok; }, vol3});
    for (int i = 0; i < 4; ++i) {
        const int Ca = i == 0 ? 16 : i == 1 ? 32 : 64, kd = i == 3 ? 1 : 3;
        fams.push_back({"K3h", wgrad_s2::tile_rows(Ca, kd), wgrad_s2::kTX, wgrad_s2::blocks_of(Ca), 1 << 20, false,
                        [Ca, kd](int D, int H, int W, Grid& g, int& r, int& c, int& p) {
            wgrad_s2::Args a{}; r = H; c = W; p = dmvs_conv3d_wgrad_s2_plan(Ca, D, H, W, kd);
            const bool ok = wgrad_s2::geometry(Ca, D, H, W, kd, a); g = a.g; return ok; }, vol_s2});
    }
    fams.push_back({"K2g", wgrad_c2::kTY, wgrad_c2::kTX, 1, 1 << 22, false, [](int D, int H, int W, Grid& g, int& r, int& c, int& p) {
        wgrad_c2::Args a{}; r = H; c = W; p = dmvs_conv3d_wgrad_c2_plan(2, 8, D, H, W);
        const bool ok = wgrad_c2::geometry(D, H, W, a); g = a.g; return ok; }, vol_c2});
    fams.push_back({"K3k", k5s2::kTY, k5s2::kTX, 1, 1 << 21, true, [](int D, int H, int W, Grid& g, int& r, int& c, int& p) {
        k5s2::Args a{}; r = (H + 1) / 2; c = (W + 1) / 2; p = dmvs_conv2d_k5s2_wgrad_plan(16, D, H, W);
        const bool ok = k5s2::geometry(16, D, H, W, a); g = a.g; return ok && a.Hc == r && a.Wc == c; }, k5});
    fams.push_back({"K3d", k5s2::kDJ, k5s2::kDI, 1, 1 << 21, true, [](int D, int H, int W, Grid& g, int& r, int& c, int& p) {
        k5s2::DArgs a{}; r = (H + 1) / 2; c = (W + 1) / 2;
        const bool ok = k5s2::dgeometry(D, H, W, a); g = a.g; p = ok ? wshare::plan(g) : DMVS_EINVAL; return ok && a.Hc == r && a.Wc == c; }, k5});
    fams.push_back({"K3f", wgrad_fpn::kTY, wgrad_fpn::kTX, 1, 1 << 22, false, [](int D, int H, int W, Grid& g, int& r, int& c, int& p) {
        wgrad_fpn::Args a{}; r = H; c = W; p = dmvs_conv2d_wgrad_fpn_plan(8, 8, 3, D, H, W);
        const bool ok = wgrad_fpn::geometry(D, H, W, a); g = a.g; return ok; }, fpn});

    int bad = 0, walked = 0;
    for (const Family& f : fams) {
        for (const auto& v : f.shapes) { bad += walk(f, v[0], v[1], v[2]); ++walked; }
        // the limits, on one tile per plane (K3k / K3d take fine extents: 2 is one coarse pixel): one tile, tiles = S, S + 1, the cap
        const int S = 256 / f.blocks;
        for (int D : {1, S, S + 1, 3 * S - 1}) { bad += walk(f, D, 2, 2); ++walked; }
        // just under 2^22 tiles, on k = 2^22 / dmax tiles of one pixel row per plane, then exactly 2^22, which the plan cannot hold
        const int k = (1 << 22) / f.dmax, cols = (k - 1) * f.tx + 1, W = f.fine ? 2 * cols : cols;
        bad += walk(f, f.dmax - 1, 1, W); ++walked;
        Grid g; int r, c, p;
        if (f.geo(f.dmax, 1, W, g, r, c, p) || p != DMVS_EINVAL) bad += fail("2^22 tiles were accepted", f, f.dmax, 1, W, p);
        if (f.geo(0, 4, 4, g, r, c, p) || f.geo(1, 0, 4, g, r, c, p) || f.geo(1, 4, 0, g, r, c, p)) bad += fail("an empty extent was accepted", f, 0, 0, 0, 0);
    }
    if (bad) return 1;
    std::printf("wgrad share: ok (%d walks)\n", walked);
    return 0;
}
