// Pieces shared by the LDS-staged plane-sweep kernels (warp_cost_tiled.hip: a quad of lanes owns a voxel; warp_cost_lv.hip, warp_gc_lv.hip:
// a lane owns a voxel): DPP broadcasts / reductions, the saturating 16-bit pack, the tile decode and block prologue, the box phase
// (corner projections -> box record; the integer rule itself is warp_box.h), the records and the launch plan.
#pragma once
#include "warp_box.h"
#include "warp_common.h"

namespace pscv {

typedef const __attribute__((address_space(4))) float* wl_cf;   // camera blocks through the scalar cache
typedef float wl_f4 __attribute__((ext_vector_type(4)));

// quad broadcast: every lane of a quad reads quad lane CTRL & 3.  (bound_ctrl with full row / bank masks: no lane keeps its
// old value, so the compiler needs no copy of the source in front of the move.)
template <int CTRL> __device__ __forceinline__ int wl_dpp_i(int x) { return __builtin_amdgcn_mov_dpp(x, CTRL, 0xf, 0xf, true); }
template <int CTRL> __device__ __forceinline__ float wl_dpp_f(float x) {
    return __builtin_bit_cast(float, wl_dpp_i<CTRL>(__builtin_bit_cast(int, x)));
}


// min / max over groups of 8 lanes (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror) and over the whole wave (+ row_mirror,
// row_bcast15, row_bcast31; the result is read from lane 63): vector-ALU DPP modifiers instead of LDS-crossbar shuffles
template <bool MAX> __device__ __forceinline__ float wl_mm(float a, float b) { return MAX ? fmaxf(a, b) : fminf(a, b); }
template <bool MAX, int CTRL, int ROWMASK = 0xf> __device__ __forceinline__ float wl_red_step(float x) {
    const int xi = __builtin_bit_cast(int, x);
    const float y = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(xi, xi, CTRL, ROWMASK, 0xf, false));
    return wl_mm<MAX>(x, y);
}
template <bool MAX> __device__ __forceinline__ float wl_reduce8(float x) {
    x = wl_red_step<MAX, 0xB1>(x);     // quad_perm [1,0,3,2]
    x = wl_red_step<MAX, 0x4E>(x);     // quad_perm [2,3,0,1]
    return wl_red_step<MAX, 0x141>(x); // row_half_mirror
}
template <bool MAX> __device__ __forceinline__ float wl_wave_reduce(float x) {
    x = wl_reduce8<MAX>(x);
    x = wl_red_step<MAX, 0x140>(x);          // row_mirror: all 16 lanes of a row
    x = wl_red_step<MAX, 0x142, 0xa>(x);     // row_bcast15 into rows 1 and 3
    x = wl_red_step<MAX, 0x143, 0xc>(x);     // row_bcast31 into rows 2 and 3
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}

// fp16 stores saturate at +-65504 like every other kernel of the engine (pscv_common.h), but through the MODE.FP16_OVFL bit the
// kernel sets at its start ("an overflowed FP16 result is clamped to +-MAX_FP16 ... preserving true INF"): the per-element
// saturation of pack_f16x2 (then a v_med3_f32 per element) cost 8 vector-ALU instructions per voxel here, 5 % of the sweep
template <typename TOut> __device__ __forceinline__ uint32_t wl_pack2(float lo, float hi) {
    if constexpr (Half16<TOut>::dtype == PSCV_F16) {
        h2_t v;
        v[0] = (_Float16)lo;
        v[1] = (_Float16)hi;
        return __builtin_bit_cast(uint32_t, v);
    } else {
        return Half16<TOut>::pack(lo, hi);
    }
}

// ---- work decode of the LDS-staged kernels: grid = (8 x tiles-per-XCD, depth chunks), tiles of T x TH reference pixels.  Hardware
//      places consecutive workgroups on consecutive XCDs, so blockIdx.x & 7 is the XCD: XCD k gets a contiguous run of tiles (its source
//      footprint stays inside that XCD's 4 MiB L2; the depth chunks of a tile re-read nearly the same texels).  Float reciprocals
//      replace integer division.  False for the workgroups that pad the grid to a multiple of 8. ----
template <int T, int TH> __device__ __forceinline__ bool wl_tile_decode(const WarpArgs& a, int& b, int& tyi, int& txi) {
    const int tpx = gridDim.x >> 3;
    const int ntx = (a.w + T - 1) / T, nty = (a.h + TH - 1) / TH;
    const int tile = ((int)blockIdx.x & 7) * tpx + ((int)blockIdx.x >> 3);
    if (tile >= a.B * nty * ntx) return false;
    const int trow = (int)(((float)tile + 0.5f) * (1.0f / (float)ntx));     // exact: tile < 2^22
    txi = tile - trow * ntx;
    b = (int)(((float)trow + 0.5f) * (1.0f / (float)nty));
    tyi = trow - b * nty;
    return true;
}

// What every workgroup of the three kernels sets up first.  The box / staging phase of a new workgroup runs at raised priority: the
// (older) waves of the CU's other workgroups are in their vector-ALU-bound sweep and would otherwise win every issue slot (arbitration
// is priority, then age), stretching this short phase -- and with it the time the CU runs on the other workgroups' waves only -- to
// ~25 000 cycles.  MODE.FP16_OVFL: see wl_pack2.
struct WlBlock {
    int x0t, y0t;               // first reference pixel of the tile
    int d0, d1;                 // depth planes [d0, d1) of the chunk
    const float* depth_b;       // planes of this batch item
};
// (tid / wave / lane stay in the kernels: derived in here, the quad-owner kernel's lane -> pixel map compiles to one instruction more)
template <int T, int TH> __device__ __forceinline__ WlBlock wl_block_prologue(const WarpArgs& a, int b, int tyi, int txi) {
    __builtin_amdgcn_s_setprio(3);
    __builtin_amdgcn_s_setreg((1 - 1) << 11 | 23 << 6 | 1, 1);     // hwreg(HW_REG_MODE, 23, 1) = FP16_OVFL: saturating f32 -> f16 stores
    WlBlock k;
    k.x0t = txi * T; k.y0t = tyi * TH;
    k.d0 = (int)blockIdx.y * a.ppd; k.d1 = min(a.D, k.d0 + a.ppd);
    k.depth_b = a.depth + (long)b * a.depth_bstride;
    return k;
}

// ---- box phase: lanes = the 8 corners (tile corners x depth extremes) of a plane range, one range per group of 8 lanes ----
// Corner `corner & 3` of the tile in reference pixel coordinates (HOMOG: half-pixel centres, homography.py:78-79).
template <int T, int TH, int GEOM> __device__ __forceinline__ void wl_tile_corner(const WarpArgs& a, const WlBlock& k, int corner, float& cx, float& cy) {
    cx = (corner & 1) ? (float)min(k.x0t + T - 1, a.w - 1) : (float)k.x0t;
    cy = (float)(((corner & 2) ? min(k.y0t + TH - 1, a.h - 1) : k.y0t) + a.ref_y0);
    if (GEOM == PSCV_GEOM_HOMOG) { cx += 0.5f; cy += 0.5f; }
}
// Sample position (u, v) of reference point (cx, cy) on plane d in the source view of `cam`, without the behind-camera test and the
// grid clamp of sweep_index; okf = 1 if the point lies in front of the camera at a finite position (also rejects NaN), else 0.
template <int GEOM> __device__ __forceinline__ void wl_corner_uv(wl_cf cam, float cx, float cy, float d, const WarpArgs& a, float& u, float& v, float& okf) {
    const float ax = fmaf(cam[1], cy, cam[0] * cx) + cam[2];
    const float ay = fmaf(cam[4], cy, cam[3] * cx) + cam[5];
    const float az = fmaf(cam[7], cy, cam[6] * cx) + cam[8];
    if (GEOM == PSCV_GEOM_PROJ) {
        const float hx = fmaf(ax, d, cam[9]), hy = fmaf(ay, d, cam[10]), hz = fmaf(az, d, cam[11]);
        const float inv_z = __builtin_amdgcn_rcpf(hz);
        u = hx * inv_z; v = hy * inv_z;
        okf = (hz > 1e-6f && fabsf(u) < 1e6f && fabsf(v) < 1e6f) ? 1.0f : 0.0f;
    } else {
        const float bx = fmaf(cam[10], cy, cam[9] * cx) + cam[11];
        const float by = fmaf(cam[13], cy, cam[12] * cx) + cam[14];
        const float bz = fmaf(cam[16], cy, cam[15] * cx) + cam[17];
        const float inv_d = __builtin_amdgcn_rcpf(d + 1e-9f);
        const float hx = fmaf(-bx, inv_d, ax), hy = fmaf(-by, inv_d, ay), hz = fmaf(-bz, inv_d, az);
        const float inv_z = __builtin_amdgcn_rcpf(hz);
        u = hx * inv_z * a.sx; v = hy * inv_z * a.sy;
        okf = (d > 1e-6f && hz > 1e-6f && fabsf(u) < 1e6f && fabsf(v) < 1e6f) ? 1.0f : 0.0f;
    }
}
// The box of one (plane range, view) from its 8 corner samples: min / max per 8-lane group (every lane of a group holds the group's
// result), slack, floor, wl_box_of.  Slack of 1/32 texel: the per-pixel fp32 evaluation (different rounding, 1-ulp rcp on both sides)
// differs from the corners' by < 2e-6 relative, i.e. < 1/32 for maps up to 16384 texels wide (larger ones are refused).
// UNIFORM: every group of the wave holds the same range, so the extents go through scalar registers.
template <bool UNIFORM> __device__ __forceinline__ WlBox wl_corner_box(float u, float v, float okf, const WarpArgs& a, const WlBoxPolicy p) {
    const float umin = wl_reduce8<false>(u), umax = wl_reduce8<true>(u);
    const float vmin = wl_reduce8<false>(v), vmax = wl_reduce8<true>(v);
    const float okmin = wl_reduce8<false>(okf);
    const float sl = 1.0f / 32.0f;
    if (UNIFORM) {
        const bool ok = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, okmin)) != 0;
        const int X0 = __builtin_amdgcn_readfirstlane((int)floorf(umin - sl)), X1 = __builtin_amdgcn_readfirstlane((int)floorf(umax + sl)) + 1;
        const int Y0 = __builtin_amdgcn_readfirstlane((int)floorf(vmin - sl)), Y1 = __builtin_amdgcn_readfirstlane((int)floorf(vmax + sl)) + 1;
        return wl_box_of(X0, Y0, X1, Y1, ok, a.hs, a.ws, p);
    } else {
        const bool ok = okmin != 0.0f;
        const int X0 = (int)floorf(umin - sl), X1 = (int)floorf(umax + sl) + 1;
        const int Y0 = (int)floorf(vmin - sl), Y1 = (int)floorf(vmax + sl) + 1;
        return wl_box_of(X0, Y0, X1, Y1, ok, a.hs, a.ws, p);
    }
}

// ---- box records in LDS, [plane range][view], written by one lane of the box phase and read by every wave into scalar registers.
//      16 bytes: X0 | Y0, X1 | Y1, pitch | mode as 16-bit pairs (the quad-owner kernel: 7 ranges x 4 views next to a 40 KiB arena leave
//      no room for more); 32 bytes: (X0, Y0, X1, Y1), (0, pitch, mode, 0) as ints (the lane-owner kernels, whose padded boxes of a
//      view that is not staged need not fit 16 bits).  idx = range * WL_MAX_SRC + view. ----
template <int REC_BYTES> __device__ __forceinline__ void wl_record_write(int* table, int idx, const WlBox& r) {
    if constexpr (REC_BYTES == 16) {
        *reinterpret_cast<uint4*>(table + idx * 4) =
            make_uint4(((unsigned)r.X0 & 0xffffu) | ((unsigned)r.Y0 << 16), ((unsigned)r.X1 & 0xffffu) | ((unsigned)r.Y1 << 16),
                       (unsigned)r.pitch | ((unsigned)r.mode << 16), 0u);
    } else {
        int4* row = reinterpret_cast<int4*>(table + idx * 8);
        row[0] = make_int4(r.X0, r.Y0, r.X1, r.Y1);
        row[1] = make_int4(0, r.pitch, r.mode, 0);
    }
}
template <int REC_BYTES> __device__ __forceinline__ WlBox wl_record_read(const int* table, int idx) {
    WlBox r;
    if constexpr (REC_BYTES == 16) {
        const uint4 rec = *reinterpret_cast<const uint4*>(table + idx * 4);
        const int rx = __builtin_amdgcn_readfirstlane((int)rec.x), ry = __builtin_amdgcn_readfirstlane((int)rec.y);
        const int rz = __builtin_amdgcn_readfirstlane((int)rec.z);
        r.X0 = (short)(rx & 0xffff); r.Y0 = rx >> 16;
        r.X1 = (short)(ry & 0xffff); r.Y1 = ry >> 16;
        r.pitch = rz & 0xffff; r.mode = rz >> 16;
    } else {
        const int4 r0 = *reinterpret_cast<const int4*>(table + idx * 8), r1 = *reinterpret_cast<const int4*>(table + idx * 8 + 4);
        r.X0 = __builtin_amdgcn_readfirstlane(r0.x); r.Y0 = __builtin_amdgcn_readfirstlane(r0.y);
        r.X1 = __builtin_amdgcn_readfirstlane(r0.z); r.Y1 = __builtin_amdgcn_readfirstlane(r0.w);
        r.pitch = __builtin_amdgcn_readfirstlane(r1.y); r.mode = __builtin_amdgcn_readfirstlane(r1.z);
    }
    return r;
}

// (The "wave k takes view k's record and source pointer" select chains stay spelled out in the three kernels: as a function over
//  the per-view arrays, by reference or through a callback, each form tried changed a kernel's register or scratch count.)

// Host side of the same: what the three kernels cover in common (C = 32, 16-bit features, source maps of <= 16384 texels a side,
// fewer than 2^22 tiles: the decode above is exact below that), the planes per workgroup (plan_planes: `ppd_default`, floor 4, 1024
// workgroups) and the grid.  Fills a.ppd / a.n_dchunks.  0 = covered, 1 = not, -1 = bad grid.
inline int wl_plan(const char* what, WarpArgs& a, const WarpCall& c, int T, int TH, int ppd_default, int ppd_max, dim3& grid) {
    if (c.C != 32 || (c.in_dtype != PSCV_F16 && c.in_dtype != PSCV_BF16)) return 1;
    if (a.ws > 16384 || a.hs > 16384) return 1;
    const long tiles = (long)a.B * ((a.h + TH - 1) / TH) * ((a.w + T - 1) / T);
    if (tiles >= (1L << 22)) return 1;
    long nblk;
    if (!plan_grid(a, tiles, plan_planes(tiles, a.D, c.ppd_override, ppd_default, 4, 1024, true, ppd_max), nblk)) { set_error("%s: bad grid %ld", what, nblk); return -1; }
    grid = dim3(8 * (unsigned)((tiles + 7) / 8), a.n_dchunks);
    return 0;
}

}  // namespace pscv
