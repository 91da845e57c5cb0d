// The integer rules of the LDS-staged plane-sweep kernels (warp_cost_tiled.hip, warp_cost_lv.hip, warp_gc_lv.hip), once: which texel
// box of a source view a (tile, plane range) stages and in which mode, how the boxes of up to four views share the arena, where a
// plane range is split, and how many planes a workgroup takes.  Plain C++ (no HIP): the kernels, the host launchers and the host
// check scripts/dev/warp_box_check.cpp include the same text.
#pragma once

#if defined(__HIPCC__)
#define WL_HD __host__ __device__ __forceinline__
#else
#define WL_HD inline
#endif

namespace pscv {

constexpr int WL_MAX_SRC = 4;                // source views of the LDS-staged kernels (more: quad kernel)

// per-(block, view) staging mode, wave-uniform
constexpr int WL_DIRECT = 0;   // not staged (a corner at / behind the source camera, or the box does not fit): global taps
constexpr int WL_GEN = 1;      // box clipped at the image border: LDS taps, general (zero-padding) weights
constexpr int WL_FAST = 2;     // box strictly inside the image: LDS taps, no masks / clamps
constexpr int WL_ZERO = 3;     // box entirely outside the image: every tap is zero padding, the view contributes f = 0

WL_HD bool wl_staged(int mode) { return mode == WL_FAST || mode == WL_GEN; }
WL_HD int wl_imin(int a, int b) { return a < b ? a : b; }
WL_HD int wl_imax(int a, int b) { return a > b ? a : b; }

// What differs between the kernels' box rules.  pad: texels of zero padding staged beyond a clipped image border (the lane-owner
// kernels clamp the top-left tap onto it instead of masking weights).  pitch_round: the box pitch is the width rounded up to this power
// of two (4: the quads of a ds_read_b128 lane group stay conflict-free across rows).  max_w x max_h: the largest box the staging phase
// covers.  rec_bytes: the record the box is published in -- 16: packed 16-bit pairs, so a box that is not staged is reset to the empty
// record; 32: plain ints, and a box that is not staged keeps its clipped extents (nobody reads them).
struct WlBoxPolicy { int pad; int pitch_round; int max_w, max_h; int rec_bytes; };

// geometry of the three kernels that the rules below depend on
#ifndef WL_TILE_H
#define WL_TILE_H 4
#endif
constexpr int WL_TH = WL_TILE_H;             // quad-owner tile height: 8 (512 threads, two workgroups per CU) or 4 (256 threads, four per CU)
constexpr int WL_ARENA = WL_TH == 8 ? 636 : 316;   // staged texels per block (all views): 80 / 40 KiB of fp32
constexpr int WL_STAGE_ROWS = 8;             // box rows one wave stages (one load batch)
constexpr int WL_BOX_W = 16;                 // widest box: a wave loads 64 16-byte pieces of a row
constexpr int WL_BOX_H = WL_STAGE_ROWS * (WL_TH / WL_MAX_SRC);   // tallest box the staging phase covers (waves per view x rows per wave): 8 / 16
#ifndef LV_OCC
#define LV_OCC 3                             // lane-owner blocks per CU (= waves per SIMD): 3 -> 52 KiB arena, 168 registers; 4 -> 39.5 KiB, 128
#endif
constexpr int LV_ARENA = LV_OCC == 3 ? 416 : 316;   // staged texels per block (all views), fp32
constexpr int LV_BOX_W = 32, LV_BOX_H = 16;  // largest box the staging phase covers (one wave per view, batches of 8 rows x 16 texels)

constexpr WlBoxPolicy WL_BOX_QUAD = {0, 4, WL_BOX_W, WL_BOX_H, 16};      // warp_cost_tiled.hip
constexpr WlBoxPolicy WL_BOX_LANE = {2, 1, LV_BOX_W, LV_BOX_H, 32};      // warp_cost_lv.hip
constexpr WlBoxPolicy WL_BOX_GC = WL_BOX_LANE;                            // warp_gc_lv.hip: the lane-owner layout

struct WlBox { int X0, Y0, X1, Y1, pitch, mode; };      // inclusive texel extents; pitch in texels
WL_HD int wl_box_texels(const WlBox& b) { return b.pitch * (b.Y1 - b.Y0 + 1); }

// The record of a view without a box (no such view, a corner behind the camera): pad x pad texels at the origin (empty without padding).
WL_HD WlBox wl_box_none(const WlBoxPolicy p, int mode) { return WlBox{0, 0, p.pad - 1, p.pad - 1, wl_imax(p.pad, p.pitch_round), mode}; }

// (X0, Y0) .. (X1, Y1): floor'ed extents of the samples (with their slack, X1 / Y1 including the right / lower tap); ok: every corner
// lies in front of the source camera at a finite position.  FAST / GEN here mean "staged if the arena has room" (wl_arena_alloc).
WL_HD WlBox wl_box_of(int X0, int Y0, int X1, int Y1, bool ok, int hs, int ws, const WlBoxPolicy p) {
    WlBox r = wl_box_none(p, WL_DIRECT);
    if (ok) {
        const bool outside = X1 < 0 || Y1 < 0 || X0 > ws - 1 || Y0 > hs - 1;
        const bool inside = X0 >= 0 && Y0 >= 0 && X1 <= ws - 1 && Y1 <= hs - 1;
        const int cX0 = wl_imax(X0, -p.pad), cX1 = wl_imin(X1, ws - 1 + p.pad), cY0 = wl_imax(Y0, -p.pad), cY1 = wl_imin(Y1, hs - 1 + p.pad);
        const int bw = cX1 - cX0 + 1, bh = cY1 - cY0 + 1;
        if (outside) r.mode = WL_ZERO;
        else if (bw <= p.max_w && bh <= p.max_h) r.mode = inside ? WL_FAST : WL_GEN;
        if (wl_staged(r.mode) || p.rec_bytes != 16) {
            r.X0 = cX0; r.Y0 = cY0; r.X1 = cX1; r.Y1 = cY1;
            r.pitch = (bw + p.pitch_round - 1) & ~(p.pitch_round - 1);
        }
    }
    return r;
}

// Planes of the first part (even) when a range of m planes is split in two; no split below 4 planes.
WL_HD int wl_split_size(int m) { return m >= 4 ? ((m / 2 + 1) & ~1) : m; }

// Arena allocation, greedy in view order: a view whose box (need texels) does not fit behind the earlier ones becomes DIRECT.
// One view: mode in, what the box phase published; returns the final mode; used: arena texels taken so far = the view's first texel.
// stage_none ("warp_tile" = 7 in the group-correlation kernel, a test aid): every box takes global taps.
WL_HD int wl_arena_take(int mode, int need, int& used, int arena, bool stage_none = false) {
    if (wl_staged(mode) && (used + need > arena || stage_none)) mode = WL_DIRECT;
    if (wl_staged(mode)) used += need;
    return mode;
}
// All views of a block.  mode[]: in / out; base[k]: first arena texel of view k.  Returns whether some view k < n_src is DIRECT.
// (The kernels run the same loop themselves, one wl_arena_take per record as they read it: with all records read first the quad-owner
//  kernel spills more scalar registers.)
WL_HD bool wl_arena_alloc(int (&mode)[WL_MAX_SRC], const int (&need)[WL_MAX_SRC], int (&base)[WL_MAX_SRC], int n_src, int arena, bool stage_none = false) {
    int used = 0;
    bool direct = false;
    for (int k = 0; k < WL_MAX_SRC; ++k) {
        base[k] = used;
        mode[k] = wl_arena_take(mode[k], need[k], used, arena, stage_none);
        direct = direct || (k < n_src && mode[k] == WL_DIRECT);
    }
    return direct;
}

// Depth planes per workgroup: `start`, or the "warp_ppd" override (rounded up to even where the kernel sweeps plane pairs, capped at
// `max` where max > 0); halved while more than `floor` planes would leave fewer than `min_blocks` workgroups (the per-block phases
// amortise over the planes, but the chip wants filling first).  units: workgroups per depth chunk.
WL_HD int plan_planes(long units, int D, int ppd_override, int start, int floor, long min_blocks, bool even, int max) {
    int ppd = start;
    if (ppd_override > 0) {
        ppd = even ? (ppd_override + 1) & ~1 : ppd_override;
        if (max > 0) ppd = wl_imin(ppd, max);
    }
    while (ppd > floor && units * ((D + ppd - 1) / ppd) < min_blocks) ppd >>= 1;
    return ppd;
}

}  // namespace pscv
