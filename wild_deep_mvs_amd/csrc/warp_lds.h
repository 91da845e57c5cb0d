// Pieces shared by the LDS-staged plane-sweep kernels (warp_cost_tiled.hip: a quad of lanes owns a voxel; warp_cost_lv.hip, warp_gc_lv.hip:
// a lane owns a voxel): DPP broadcasts / reductions, the saturating 16-bit pack, the per-(block, view) staging modes, the tile decode
// and the launch plan.
#pragma once
#include "warp_common.h"

namespace pscv {

constexpr int WL_MAX_SRC = 4;                // source views of the LDS-staged kernels (more: quad kernel)
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
// v_med3_f32 clamp of pack_f16x2 costs 8 vector-ALU instructions per voxel here, 5 % of the sweep
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
// per-(block, view) staging mode, wave-uniform
constexpr int WL_DIRECT = 0;   // not staged (a corner at / behind the source camera, or the box does not fit): global taps
constexpr int WL_GEN = 1;      // box clipped at the image border: LDS taps, general (zero-padding) weights
constexpr int WL_FAST = 2;     // box strictly inside the image: LDS taps, no masks / clamps
constexpr int WL_ZERO = 3;     // box entirely outside the image: every tap is zero padding, the view contributes f = 0


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

// Host side of the same: what the three kernels cover in common (C = 32, 16-bit features, source maps of <= 16384 texels a side,
// fewer than 2^22 tiles: the decode above is exact below that), the planes per workgroup (`ppd_default`, or the "warp_ppd" override
// rounded to even and capped at `ppd_max`; halved while fewer than 1024 workgroups would result: the box + staging phases amortise
// over the planes, but the chip wants filling first) and the grid.  Fills a.ppd / a.n_dchunks.  0 = covered, 1 = not, -1 = bad grid.
inline int wl_plan(const char* what, WarpArgs& a, int C, int in_dtype, int T, int TH, int ppd_override, int ppd_default, int ppd_max, dim3& grid) {
    if (C != 32 || (in_dtype != PSCV_F16 && in_dtype != PSCV_BF16)) return 1;
    if (a.ws > 16384 || a.hs > 16384) return 1;
    const long tiles = (long)a.B * ((a.h + TH - 1) / TH) * ((a.w + T - 1) / T);
    if (tiles >= (1L << 22)) return 1;
    int ppd = ppd_override > 0 ? min((ppd_override + 1) & ~1, ppd_max) : ppd_default;
    while (ppd > 4 && tiles * ((a.D + ppd - 1) / ppd) < 1024) ppd >>= 1;
    a.ppd = ppd;
    a.n_dchunks = (a.D + ppd - 1) / ppd;
    const long nblk = tiles * a.n_dchunks;
    if (nblk <= 0 || nblk > 0x7fffffffL) { set_error("%s: bad grid %ld", what, nblk); return -1; }
    grid = dim3(8 * (unsigned)((tiles + 7) / 8), a.n_dchunks);
    return 0;
}

}  // namespace pscv
