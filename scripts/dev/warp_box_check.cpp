// Stand-alone check of the box / arena / plane rules of the LDS-staged warp kernels (wild_deep_mvs_amd/csrc/warp_box.h), meant for the
// host sanitizers:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/dev/warp_box_check.cpp -o warp_box_check && ./warp_box_check
// Compares wl_box_of (three policies), wl_split_size, wl_arena_alloc and plan_planes against transcriptions of the rules the three
// kernels and the three host launchers carried in line before the header existed (kept below, verbatim but for the variable
// names), over boxes astride and beyond every image border, at and one texel over the size limits, arenas exactly full and one
// texel over at each view position, 1-4 source views, 1-64 planes, and chunk plans either side of the 1024- / 4096-block thresholds.
// Prints the number of comparisons and of mismatches; any mismatch is a failure.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../wild_deep_mvs_amd/csrc/warp_box.h"

using namespace pscv;
using std::max;
using std::min;

static long comparisons = 0, mismatches = 0;
static void expect(bool same, const char* what, int line) {
    ++comparisons;
    if (!same && ++mismatches <= 20) std::printf("MISMATCH line %d: %s\n", line, what);
}
#define SAME(cond) expect((cond), #cond, __LINE__)

// ---- the rules as the kernels had them -------------------------------------------------------------------------------------------
// warp_cost_tiled.hip (k < n_src): clip to the image, pitch rounded up to 4, whatever is not staged reset to the empty 16-bit record
static WlBox old_box_tiled(int X0, int Y0, int X1, int Y1, bool ok, int hs, int ws) {
    int cX0 = 0, cY0 = 0, cX1 = -1, cY1 = -1, pitch = 4, mode = WL_DIRECT;
    if (ok) {
        const bool outside = X1 < 0 || Y1 < 0 || X0 > ws - 1 || Y0 > hs - 1;
        const bool inside = X0 >= 0 && Y0 >= 0 && X1 <= ws - 1 && Y1 <= hs - 1;
        cX0 = max(X0, 0); cX1 = min(X1, ws - 1); cY0 = max(Y0, 0); cY1 = min(Y1, hs - 1);
        const int bw = cX1 - cX0 + 1, bh = cY1 - cY0 + 1;
        pitch = (bw + 3) & ~3;
        if (outside) { mode = WL_ZERO; cX0 = 0; cY0 = 0; cX1 = -1; cY1 = -1; pitch = 4; }
        else if (bw <= 16 && bh <= WL_BOX_H) mode = inside ? WL_FAST : WL_GEN;
        else { cX0 = 0; cY0 = 0; cX1 = -1; cY1 = -1; pitch = 4; }
    } else { cX0 = 0; cY0 = 0; cX1 = -1; cY1 = -1; pitch = 4; }
    return WlBox{cX0, cY0, cX1, cY1, pitch, mode};
}
// warp_cost_lv.hip and warp_gc_lv.hip (k < n_src): clip to the image +- 2, pitch = width, extents kept whatever the mode
static WlBox old_box_lv(int X0, int Y0, int X1, int Y1, bool ok, int hs, int ws) {
    int cX0 = 0, cY0 = 0, cX1 = 1, cY1 = 1, pitch = 2, mode = WL_DIRECT;
    if (ok) {
        const bool outside = X1 < 0 || Y1 < 0 || X0 > ws - 1 || Y0 > hs - 1;
        const bool inside = X0 >= 0 && Y0 >= 0 && X1 <= ws - 1 && Y1 <= hs - 1;
        cX0 = max(X0, -2); cX1 = min(X1, ws + 1); cY0 = max(Y0, -2); cY1 = min(Y1, hs + 1);
        const int bw = cX1 - cX0 + 1, bh = cY1 - cY0 + 1;
        pitch = bw;
        if (outside) mode = WL_ZERO;
        else if (bw <= LV_BOX_W && bh <= LV_BOX_H) mode = inside ? WL_FAST : WL_GEN;
    }
    return WlBox{cX0, cY0, cX1, cY1, pitch, mode};
}
static int old_split(int m) { return m >= 4 ? ((m / 2 + 1) & ~1) : m; }
// arena: `kind` 0 = warp_cost_tiled.hip (modes as published), 1 = warp_cost_lv.hip (views >= n_src count as ZERO), 2 = warp_gc_lv.hip
// with "warp_tile" = 7 (as 1, and nothing is staged)
static bool old_arena(int kind, const int* mode_in, const int* need, int n_src, int arena, int* mode_out, int* base) {
    int used = 0;
    bool direct = false;
    for (int k = 0; k < WL_MAX_SRC; ++k) {
        int mode = kind == 0 || k < n_src ? mode_in[k] : WL_ZERO;
        if ((mode == WL_FAST || mode == WL_GEN) && used + need[k] > arena) mode = WL_DIRECT;
        if (kind == 2 && (mode == WL_FAST || mode == WL_GEN)) mode = WL_DIRECT;
        base[k] = used;
        if (mode == WL_FAST || mode == WL_GEN) used += need[k];
        mode_out[k] = mode;
        direct = direct || ((kind != 0 || k < n_src) && mode == WL_DIRECT);
    }
    return direct;
}
// planes per block: launch_geom (warp_cost.hip), warp_cost_q2_try (warp_cost_quad.hip), wl_plan (warp_lds.h)
static int old_planes_generic(long units, int D, int ovr) {
    int ppd = ovr > 0 ? ovr : 8;
    while (ppd > 1 && units * ((D + ppd - 1) / ppd) < 4096) ppd >>= 1;
    return ppd;
}
static int old_planes_q2(long units, int D, int ovr) {
    int ppd = ovr > 0 ? ((ovr + 1) & ~1) : 8;
    while (ppd > 2 && units * ((D + ppd - 1) / ppd) < 4096) ppd >>= 1;
    return ppd;
}
static int old_planes_lds(long tiles, int D, int ovr, int ppd_default, int ppd_max) {
    int ppd = ovr > 0 ? min((ovr + 1) & ~1, ppd_max) : ppd_default;
    while (ppd > 4 && tiles * ((D + ppd - 1) / ppd) < 1024) ppd >>= 1;
    return ppd;
}

static bool same_box(const WlBox& a, const WlBox& b) {
    return a.X0 == b.X0 && a.Y0 == b.Y0 && a.X1 == b.X1 && a.Y1 == b.Y1 && a.pitch == b.pitch && a.mode == b.mode;
}

int main() {
    // ---- boxes: first texel either side of and far beyond each border, widths / heights round the limits of both layouts ----
    const int maps[][2] = {{30, 40}, {21, 21}, {128, 160}, {16384, 16384}};      // hs, ws
    const int widths[] = {1, 2, 3, 4, 5, 15, 16, 17, 18, 31, 32, 33, 34, 35, 36, 37, 50}, heights[] = {1, 2, 7, 8, 9, 10, 11, 12, 13, 15, 16, 17, 18, 19, 20, 21, 40};
    for (const auto& m : maps) {
        const int hs = m[0], ws = m[1];
        std::vector<int> xs, ys;
        for (int d : {-100000, -60, -40, -36, -33, -32, -20, -18, -17, -16, -15, -5, -4, -3, -2, -1, 0, 1, 2, 3}) { xs.push_back(d); ys.push_back(d); }
        for (int d = -40; d <= 5; ++d) { xs.push_back(ws + d); ys.push_back(hs + d); }
        xs.push_back(ws + 100000); ys.push_back(hs + 100000);
        for (int X0 : xs) for (int bw : widths) for (int Y0 : ys) for (int bh : heights) for (int ok = 0; ok < 2; ++ok) {
            const int X1 = X0 + bw - 1, Y1 = Y0 + bh - 1;
            SAME(same_box(wl_box_of(X0, Y0, X1, Y1, ok != 0, hs, ws, WL_BOX_QUAD), old_box_tiled(X0, Y0, X1, Y1, ok != 0, hs, ws)));
            SAME(same_box(wl_box_of(X0, Y0, X1, Y1, ok != 0, hs, ws, WL_BOX_LANE), old_box_lv(X0, Y0, X1, Y1, ok != 0, hs, ws)));
            SAME(same_box(wl_box_of(X0, Y0, X1, Y1, ok != 0, hs, ws, WL_BOX_GC), old_box_lv(X0, Y0, X1, Y1, ok != 0, hs, ws)));
        }
    }
    // the limits themselves, inside the image: 16 x WL_BOX_H and LV_BOX_W x LV_BOX_H are staged, one texel more is not
    SAME(wl_box_of(4, 4, 4 + 15, 4 + WL_BOX_H - 1, true, 128, 160, WL_BOX_QUAD).mode == WL_FAST);
    SAME(wl_box_of(4, 4, 4 + 16, 4 + WL_BOX_H - 1, true, 128, 160, WL_BOX_QUAD).mode == WL_DIRECT);
    SAME(wl_box_of(4, 4, 4 + 15, 4 + WL_BOX_H, true, 128, 160, WL_BOX_QUAD).mode == WL_DIRECT);
    SAME(wl_box_of(4, 4, 4 + LV_BOX_W - 1, 4 + LV_BOX_H - 1, true, 128, 160, WL_BOX_LANE).mode == WL_FAST);
    SAME(wl_box_of(4, 4, 4 + LV_BOX_W, 4 + LV_BOX_H - 1, true, 128, 160, WL_BOX_LANE).mode == WL_DIRECT);
    SAME(wl_box_of(4, 4, 4 + LV_BOX_W - 1, 4 + LV_BOX_H, true, 128, 160, WL_BOX_GC).mode == WL_DIRECT);
    // the records of a view that does not exist
    SAME(same_box(wl_box_none(WL_BOX_QUAD, WL_ZERO), WlBox{0, 0, -1, -1, 4, WL_ZERO}));
    SAME(same_box(wl_box_none(WL_BOX_LANE, WL_ZERO), WlBox{0, 0, 1, 1, 2, WL_ZERO}));
    SAME(same_box(wl_box_none(WL_BOX_GC, WL_ZERO), WlBox{0, 0, 1, 1, 2, WL_ZERO}));

    // ---- split sizes: 1-64 planes (and a few beyond), halves and quarters ----
    for (int m = 0; m <= 130; ++m) {
        SAME(wl_split_size(m) == old_split(m));
        const int h = wl_split_size(m);
        SAME(wl_split_size(h) == old_split(old_split(m)) && wl_split_size(m - h) == old_split(m - old_split(m)));
    }

    // ---- arena: exactly full and one texel over at each view position; every mode pattern; 1-4 views; both arenas ----
    for (int arena : {WL_ARENA, LV_ARENA}) {
        std::vector<std::vector<int>> needs;
        for (int pos = 0; pos < WL_MAX_SRC; ++pos)
            for (int over = 0; over <= 1; ++over) {
                std::vector<int> n(WL_MAX_SRC, 16);                // views before `pos` take 16 texels each, view `pos` the rest (+ 1)
                n[pos] = arena - 16 * pos + over;
                needs.push_back(n);
                n[pos] = arena - 16 * pos + over - 40;             // ... or leaves 40 - over texels, which the next view fills / overfills
                if (pos + 1 < WL_MAX_SRC) { n[pos + 1] = 40; needs.push_back(n); n[pos + 1] = 39; needs.push_back(n); n[pos + 1] = 41; needs.push_back(n); }
            }
        needs.push_back({arena / 4, arena / 4, arena / 4, arena / 4});
        needs.push_back({arena / 4, arena / 4, arena / 4, arena - 3 * (arena / 4) + 1});
        needs.push_back({0, 0, 0, 0});
        needs.push_back({arena + 1, 1, arena, 1});
        needs.push_back({8, 512, 8, 512});
        for (const auto& need : needs)
            for (int pat = 0; pat < 256; ++pat)                    // mode of view k = two bits of pat
                for (int n_src = 1; n_src <= WL_MAX_SRC; ++n_src)
                    for (int kind = 0; kind < 3; ++kind) {
                        int in[WL_MAX_SRC], want_mode[WL_MAX_SRC], want_base[WL_MAX_SRC], got_mode[WL_MAX_SRC], got_base[WL_MAX_SRC], nd[WL_MAX_SRC];
                        for (int k = 0; k < WL_MAX_SRC; ++k) { in[k] = (pat >> (2 * k)) & 3; nd[k] = need[k]; }
                        const bool want = old_arena(kind, in, nd, n_src, arena, want_mode, want_base);
                        // (the lane-owner kernels read a record of a view >= n_src as ZERO before they allocate)
                        for (int k = 0; k < WL_MAX_SRC; ++k) got_mode[k] = kind == 0 || k < n_src ? in[k] : WL_ZERO;
                        const bool got = wl_arena_alloc(got_mode, nd, got_base, n_src, arena, kind == 2);
                        bool same = want == got;
                        for (int k = 0; k < WL_MAX_SRC; ++k) same = same && want_mode[k] == got_mode[k] && want_base[k] == got_base[k];
                        SAME(same);
                    }
    }

    // ---- planes per block: the three launch rules ----
    const long units[] = {1, 2, 5, 10, 11, 21, 22, 31, 32, 33, 42, 43, 63, 64, 65, 85, 86, 127, 128, 129, 170, 171, 255, 256, 257, 341, 342,
                          511, 512, 513, 585, 586, 682, 683, 1023, 1024, 1025, 1365, 1366, 2047, 2048, 2049, 4095, 4096, 4097, 100000, 4194303};
    const int overrides[] = {0, -1, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 31, 32, 33, 47, 48, 49, 63, 64, 65, 66, 100, 1001};
    for (int D : {1, 7, 8, 95, 96, 192})
        for (long u : units)
            for (int ovr : overrides) {
                SAME(plan_planes(u, D, ovr, 8, 1, 4096, false, 0) == old_planes_generic(u, D, ovr));
                SAME(plan_planes(u, D, ovr, 8, 2, 4096, true, 0) == old_planes_q2(u, D, ovr));
                SAME(plan_planes(u, D, ovr, D >= 96 ? 48 : 32, 4, 1024, true, 64) == old_planes_lds(u, D, ovr, D >= 96 ? 48 : 32, 64));      // quad-owner
                SAME(plan_planes(u, D, ovr, 32, 4, 1024, true, 64) == old_planes_lds(u, D, ovr, 32, 64));                                  // lane-owner, gc per-batch planes
                SAME(plan_planes(u, D, ovr, 32, 4, 1024, true, 32) == old_planes_lds(u, D, ovr, 32, 32));                                  // gc per-pixel planes
            }
    // the known oddity stays: 48 planes halve to 3 on a small map
    SAME(plan_planes(12, 192, 0, 48, 4, 1024, true, 64) == 3);

    std::printf("warp_box: %ld comparisons, %ld mismatches\n", comparisons, mismatches);
    return mismatches ? 1 : 0;
}
