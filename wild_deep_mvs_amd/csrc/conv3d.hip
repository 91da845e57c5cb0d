// 3x3x3 convolution over a channels-last bf16 volume as an MFMA implicit GEMM (gfx950, wave64).
//
// GEMM view (per output voxel n, output channel m):  D[m][n] = sum_k W[m][k] * X[k][n],
//   k = (tap, c_in) flattened, K = 27 * C_in (zero padded to a multiple of 32);
//   A operand = packed weights (16 output channels x 32 k per v_mfma_f32_16x16x32_bf16),
//   B operand = 16 x-adjacent output voxels x 32 k, read with ds_read_b128 from an LDS brick that holds
//   the input halo region of the workgroup's output tile (every input voxel is fetched once per tile);
//   D: lane (n = lane&15, g = lane>>4) owns 4 consecutive output channels of voxel n, so the epilogue
//   (folded BatchNorm affine, ReLU, skip add) ends in one 8-byte bf16 store per lane.
// Both MFMA operands use the same (lane, j) -> k mapping, so the contraction is independent of the
// instruction's internal k ordering; only "row/col = lane & 15" and the D layout are relied on.
//
// Kinds: S1 (stride 1), S2 (stride 2), T2 (transposed, stride 2, output_padding 1: decomposed into its 8
// output-parity classes, each a dense 1/2/4/8-tap convolution over the input grid -- no zero insertion).
//
// Replaces (fdarmon/wild_deep_mvs): models/MVSNet/module.py:41-58 ConvBnReLU3D/ConvBn3D, the
// Sequential(ConvTranspose3d, BatchNorm3d, ReLU) blocks and `prob` of models/MVSNet/model.py:43-84,
// models/CVP_MVSNet/models/net.py:50-85 and the 3-D members of models/VisMVSNet/nn_utils.py:194-278.
#include "conv_common.h"
#include "conv_dev.h"
#include <type_traits>

namespace pscv {

PSCV_PROF_BUFFER(conv)

struct ConvArgs : ConvIO {
    int Di, Hi, Wi, Do, Ho, Wo;
    int cout, epi;
    int ntd, nth, ntw;   // tile counts along d, h, w
    unsigned mg_td, mg_th, mg_tw;   // fast_div_magic of the tile counts
    int nt_total;        // 16-channel output tiles of the layer (blockIdx.y picks this block's first tile)
};

// ---- compile-time geometry ----------------------------------------------------------------------
template <int KIND, int TD, int TH> struct Brick;
template <int TD, int TH> struct Brick<PSCV_CONV_S1, TD, TH> { static constexpr int BD = TD + 2, BH = TH + 2, BW = 18; };
template <int TD, int TH> struct Brick<PSCV_CONV_S2, TD, TH> { static constexpr int BD = 2 * TD + 1, BH = 2 * TH + 1, BW = 33; };
template <int TD, int TH> struct Brick<PSCV_CONV_T2, TD, TH> { static constexpr int BD = TD + 1, BH = TH + 1, BW = 17; };

__host__ __device__ constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }
// number of taps / k-steps of T2 parity class pc = pd*4 + ph*2 + pw
__host__ __device__ constexpr int t2_ntaps(int pc) { return (1 + ((pc >> 2) & 1)) * (1 + ((pc >> 1) & 1)) * (1 + (pc & 1)); }
__host__ __device__ constexpr int t2_nsteps(int pc, int cin) { return ceil_div(t2_ntaps(pc) * cin, 32); }
__host__ __device__ constexpr int t2_stepbase(int pc, int cin) {
    int s = 0;
    for (int i = 0; i < pc; ++i) s += t2_nsteps(i, cin);
    return s;
}
__host__ __device__ constexpr int conv_total_steps(int kind, int cin) {
    return kind == PSCV_CONV_T2 ? t2_stepbase(8, cin) : ceil_div(27 * cin, 32);
}

// LDS bytes per voxel: channels + padding, chosen so that the four 16-lane groups a `ds_read_b128` is served in ({0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31} and the same + 32: MI355X_MICROARCH.md, LDS table) each touch 16 different 16-byte bank granules in every k-step
// of the layer (scripts/dev/lds_conflicts.py brute-forces the model; SQ_LDS_BANK_CONFLICT agrees: 45 % of the LDS cycles of the
// 16 -> 16 layer with the former 48-byte stride, 37 % of the 64 -> 64 layer with 144).  A lane reads voxel (anchor + SXY n) chunk
// (g or g & 1): with voxels one stride apart (stride 1, transposed) the stride must be 2 mod 4 granules, with two strides apart (stride 2)
// it must be odd.
__host__ __device__ constexpr int conv_vs(int kind, int cin, int th = 4) {
    if (kind == PSCV_CONV_S1 && cin == 64 && th == 8) return 144;          // (the 4 x 8 x 16 tile: 160 would not fit the LDS)
    if (kind == PSCV_CONV_S2) return cin == 32 ? 80 : cin * 2 + 16;        // 8: 32 (2-way; 48 would be free -- the 8-channel layers run on the sweep kernels), 16: 48, 32: 80, 64: 144
    return cin == 16 ? 32 : cin == 8 ? 48 : cin * 2 + 32;                   // 8: 48, 16: 32, 32: 96, 64: 160
}
__host__ __device__ constexpr int conv_epi_bytes(int nt) { return 3 * nt * 16 * 4; }

// first LDS region: the input brick; workgroups with one M-tile per wave of a dense kind reuse it for the k-split
// reduction (4 waves x 4 M-tiles x NT N-tiles x 64 lanes x 16 B), so it is at least that large
__host__ __device__ constexpr int conv_region0(int kind, int cin, int nt, int td, int th) {
    const int bd = kind == PSCV_CONV_S1 ? td + 2 : kind == PSCV_CONV_S2 ? 2 * td + 1 : td + 1;
    const int bh = kind == PSCV_CONV_S1 ? th + 2 : kind == PSCV_CONV_S2 ? 2 * th + 1 : th + 1;
    const int bw = kind == PSCV_CONV_S1 ? 18 : kind == PSCV_CONV_S2 ? 33 : 17;
    const int brick = (bd * bh * bw * conv_vs(kind, cin, th) + 15) & ~15;
    const int red = (td * th == 4 && kind != PSCV_CONV_T2) ? 16 * 1024 * nt : 0;
    return brick > red ? brick : red;
}

// LDS byte offset (relative to the lane's output-voxel anchor) of tap `tap` for the dense kinds
template <int KIND, int BH, int BW, int VS> __device__ __forceinline__ int tap_off_dense(int tap) {
    tap = tap > 26 ? 26 : tap;   // k padding: any finite in-brick voxel (its weights are zero)
    const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
    return ((kd * BH + kh) * BW + kw) * VS;
}
// same for a T2 parity class: per dim, parity 0 -> one tap (k=1, offset 0); parity 1 -> two taps
// (sub 0: k=0 at input offset +1, sub 1: k=2 at offset 0)
template <int BH, int BW, int VS> __device__ __forceinline__ int tap_off_t2(int pc, int t) {
    const int pd = (pc >> 2) & 1, ph = (pc >> 1) & 1, pw = pc & 1;
    const int nt = (1 + pd) * (1 + ph) * (1 + pw);
    t = t >= nt ? nt - 1 : t;
    const int tw = t % (1 + pw), th = (t / (1 + pw)) % (1 + ph), td = t / ((1 + pw) * (1 + ph));
    const int od = (pd && td == 0) ? 1 : 0, oh = (ph && th == 0) ? 1 : 0, ow = (pw && tw == 0) ? 1 : 0;
    return ((od * BH + oh) * BW + ow) * VS;
}

// channel group that is cut by c_out (c_out not a multiple of 4): element-wise skip add and stores, out of line
template <typename H>
__device__ __noinline__ void epi_ragged(float y0, float y1, float y2, float y3, const uint16_t* sp, void* op, int cnt, int out_f32,
                                        float lo_post) {
    float y[4] = {y0, y1, y2, y3};
    for (int k = 0; k < cnt; ++k) {
        float v = y[k];
        if (sp) v += Half16<H>::one(sp[k]);
        v = relu_floor(v, lo_post);
        if (out_f32) reinterpret_cast<float*>(op)[k] = v;
        else reinterpret_cast<uint16_t*>(op)[k] = Half16<H>::bits(v);
    }
}

// HOT: the store side of the layers the U-Nets run -- 16-bit output, c_out a multiple of 16, output and skip slice of a batch item
// below 2 GiB and 8-byte aligned (chosen on the host, launch_conv).  Output and skip tensor are addressed through one buffer
// descriptor each, made once per workgroup from the batch item's base: a lane's 32-bit byte offset inside a row is made once (lanes
// beyond the volume carry an out-of-range offset: the hardware drops their stores and zero-fills their loads), the wave-uniform row
// offset is the instruction's scalar offset, and the epilogue has no flag, bounds or channel-count branch.  Every other call runs the
// general instance: flat 64-bit addresses, run-time flags, epi_ragged.  The arithmetic of the two is the same, operation by operation.
template <typename H, int CIN, int NT, int KIND, int TD, int TH, bool HOT>
__global__ __launch_bounds__(256) void conv3d_kernel(const ConvArgs a) {
    using BR = Brick<KIND, TD, TH>;
    constexpr int BD = BR::BD, BH = BR::BH, BW = BR::BW;
    constexpr int VS = conv_vs(KIND, CIN, TH);   // LDS bytes per voxel (padded against bank conflicts)
    constexpr int CCH = CIN / 8;                 // 16-byte chunks per voxel
    constexpr int NVOX = BD * BH * BW;
    constexpr int NMT = TD * TH;                 // M-tiles (rows of 16 x-adjacent voxels) per workgroup
    constexpr int MB = NMT / 4;                  // M-tiles per wave
    static_assert(NMT % 4 == 0, "tile rows must split evenly over the 4 waves");
    constexpr int SXY = (KIND == PSCV_CONV_S2) ? 2 : 1;   // input step per output voxel

    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    PSCV_PROF_BEGIN

    // The argument block in ONE burst of scalar loads.  Left to itself the compiler fetches each field where it is first used, behind
    // the branches of the tile decode and the fetch lambdas: some fifteen dependent s_load / s_waitcnt round trips, 2.7 K of a
    // workgroup's 10-14 K cycles before its first weight load went out (scripts/dev/phase_prof.py, slot "prologue").  Naming the
    // fields as scalar inputs of an empty asm makes them live here, all at once.
    asm volatile("" ::"s"(a.in), "s"(a.wpk), "s"(a.scale), "s"(a.bias), "s"(a.floor), "s"(a.skip), "s"(a.out), "s"(a.epi), "s"(a.in_cs),
                 "s"(a.in_co), "s"(a.skip_cs), "s"(a.skip_co), "s"(a.out_cs), "s"(a.out_co), "s"(a.Di), "s"(a.Hi), "s"(a.Wi), "s"(a.Do),
                 "s"(a.Ho), "s"(a.Wo), "s"(a.cout), "s"(a.ntd), "s"(a.nth), "s"(a.ntw), "s"(a.mg_td), "s"(a.mg_th), "s"(a.mg_tw),
                 "s"(a.nt_total));

    // ---- which tile (XCD-aware bijective remap: each XCD gets a contiguous run of tiles) ----
    int wg = xcd_remap(blockIdx.x, gridDim.x);
    const int tw_i = fast_divmod(wg, a.ntw, a.mg_tw);
    const int th_i = fast_divmod(wg, a.nth, a.mg_th);
    const int td_i = fast_divmod(wg, a.ntd, a.mg_td);
    const int b = wg;

    // tile anchor in "row space": output coords for S1/S2, input coords for T2
    const int t0d = td_i * TD, t0h = th_i * TH, t0w = tw_i * 16;
    // brick origin in input coords
    const int o_d = (KIND == PSCV_CONV_S1) ? t0d - 1 : (KIND == PSCV_CONV_S2) ? 2 * t0d - 1 : t0d;
    const int o_h = (KIND == PSCV_CONV_S1) ? t0h - 1 : (KIND == PSCV_CONV_S2) ? 2 * t0h - 1 : t0h;
    const int o_w = (KIND == PSCV_CONV_S1) ? t0w - 1 : (KIND == PSCV_CONV_S2) ? 2 * t0w - 1 : t0w;

    // ---- weight fragments ----
    // Workgroups with one M-tile per wave (the 1x4x16 small-volume tiles and the 2x2x16 stride-2 tiles) would have all four
    // waves fetch the SAME A fragments: four times the layer's weights through the CU's 64 B/clk vector-memory path per 64
    // output voxels -- 4x more bytes than the input brick, and what these workgroups waited on (scripts/dev/phase_prof.py).
    // There the waves split the REDUCTION instead of the rows:
    //   dense kinds (KSPLIT): wave w runs k-steps w, w+4, ... over all four M-tiles; the four partial accumulators are summed
    //     through LDS in a fixed order (0+1+2+3) before the epilogue of the wave's own M-tile;
    //   transposed kind (CSPLIT): wave w owns the output-parity classes w and 7-w (9/6/6/6 of the 27 taps) of all four
    //     M-tiles -- no reduction at all.
    // Either way a wave fetches a quarter of the weights, all of them up front (<= 24 fragments in flight), together with
    // the skip values of its outputs, so the only memory latency of the workgroup is the one it shares with the brick.
    // Larger tiles (MB > 1) keep the row split with a prefetch ring of the next 24/NT k-steps.
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, g = lane >> 4;
    const int nt0 = blockIdx.y * NT;
    const uint4* wpk = reinterpret_cast<const uint4*>(a.wpk);
    constexpr int NSTEPS_ALL = conv_total_steps(KIND, CIN);
    constexpr bool KSPLIT = MB == 1 && KIND != PSCV_CONV_T2;
    constexpr bool CSPLIT = MB == 1 && KIND == PSCV_CONV_T2;
    constexpr int SPW = (NSTEPS_ALL + 3) / 4;    // k-steps per wave under the k-split
    constexpr int PF_WANT = 24 / NT;
    constexpr int PF_SRC = KSPLIT ? SPW : NSTEPS_ALL;
    constexpr int PF = (KIND == PSCV_CONV_T2) ? 1 : (PF_SRC < PF_WANT ? PF_SRC : PF_WANT);
    uint4 wring[PF][NT];
    if (KIND != PSCV_CONV_T2) {
#pragma unroll
        for (int s = 0; s < PF; ++s) {
            int st = KSPLIT ? wave + 4 * s : s;
            st = st < NSTEPS_ALL ? st : NSTEPS_ALL - 1;   // (a wave with one step less re-reads its last one; never used)
#pragma unroll
            for (int m = 0; m < NT; ++m) wring[s][m] = wpk[(st * a.nt_total + nt0 + m) * 64 + lane];
        }
    }
    // class split: all fragments of classes `wave` and `7 - wave`, and the skip values of their outputs
    constexpr int CS_MAXW = CSPLIT ? t2_nsteps(0, CIN) + t2_nsteps(7, CIN) : 1;
    uint4 wcls[CS_MAXW][NT];
    uint2 skc[CSPLIT ? 8 : 1][NT];
    // Output / skip addressing shared by the prefetches and the epilogue.  A row of 16 x-adjacent output voxels has
    // wave-uniform (od, oh): its base is scalar 64-bit arithmetic from per-workgroup constants, and a lane adds one 32-bit
    // element offset computed ONCE here (x position of the lane's voxel * channel stride + its 4-channel group; the
    // transposed kind adds pw * channel stride).  (Per-call 64-bit voxel arithmetic made the prologue and the epilogue of
    // the small-tile kernels instruction-issue bound: ~70 instructions per 8-byte skip load.)
    constexpr int XS = KIND == PSCV_CONV_T2 ? 2 : 1;
    const int ox0 = XS * (t0w + n);                                 // lane's output x (pw = 0)
    const int cg = nt0 * 16 + g * 4;                                // lane's first channel in N-tile 0
    // Row offsets (RowT): elements from the tensor's start in the general instance, bytes from the descriptor's base (the batch
    // item's first voxel, channel offset included) in the HOT one, where they fit 32 bits.
    using RowT = std::conditional_t<HOT, unsigned, long>;
    constexpr int EB = HOT ? 2 : 1;
    constexpr unsigned OOR = 0x80000000u;   // beyond any HOT descriptor's range (< 0x7fff0000 bytes), and OOR + row + tile offset does not wrap 32 bits
    const bool lane_ok = t0w + n < (KIND == PSCV_CONV_T2 ? a.Wi : a.Wo);
    const unsigned lane_out = HOT && !lane_ok ? OOR : (unsigned)(ox0 * a.out_cs + cg) * EB;
    const unsigned lane_skip = HOT && !lane_ok ? OOR : (unsigned)(ox0 * a.skip_cs + cg) * EB;
    const RowT plane_out = (RowT)((long)a.Ho * a.Wo * a.out_cs * EB), plane_skip = (RowT)((long)a.Ho * a.Wo * a.skip_cs * EB);
    using StrideT = std::conditional_t<HOT, unsigned, int>;
    const StrideT row_out = (StrideT)(a.Wo * a.out_cs * EB), row_skip = (StrideT)(a.Wo * a.skip_cs * EB);
    const int bDo = b * a.Do;
    const bool cout4 = HOT || (a.cout & 3) == 0;
    __amdgpu_buffer_rsrc_t ors, srs;
    if constexpr (HOT) {
        const long item_out = (long)a.Do * a.Ho * a.Wo * a.out_cs, item_skip = (long)a.Do * a.Ho * a.Wo * a.skip_cs;   // elements
        // (conv_dev.h; a missing skip tensor gets an empty descriptor: its loads return the +0 that the epilogue adds)
        ors = buf_rsrc(reinterpret_cast<const uint16_t*>(a.out) + (long)b * item_out + a.out_co, (int)((item_out - a.out_co) * 2));
        srs = buf_rsrc(a.skip + (a.skip ? (long)b * item_skip + a.skip_co : 0), a.skip ? (int)((item_skip - a.skip_co) * 2) : 0);
    }
    auto out_row = [&](int od, int oh) -> RowT {
        if constexpr (HOT) return (unsigned)od * plane_out + (unsigned)oh * row_out;
        else return (long)(bDo + od) * plane_out + (long)oh * row_out + a.out_co;
    };
    auto skip_row = [&](int od, int oh) -> RowT {
        if constexpr (HOT) return (unsigned)od * plane_skip + (unsigned)oh * row_skip;
        else return (long)(bDo + od) * plane_skip + (long)oh * row_skip + a.skip_co;
    };
    auto skip_fetch = [&](RowT srow, int pw, int m) -> uint2 {           // srow: wave-uniform row inside the volume
        uint2 sv = make_uint2(0u, 0u);
        if constexpr (HOT) {
            if (a.skip)
                sv = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(srs, (int)(lane_skip + (unsigned)(m * 32)),
                                                                                    (int)(srow + (unsigned)(pw * a.skip_cs * 2)), 0));
        } else if (a.skip && cout4) {
            if (lane_ok && cg + m * 16 < a.cout)
                sv = *reinterpret_cast<const uint2*>(a.skip + srow + (lane_skip + (unsigned)(pw * a.skip_cs + m * 16)));
        }
        return sv;
    };
    // class split: rows of the wave's outputs relative to the tile origin (od = 2 t0d + pd, oh = 2 (t0h + i) + ph)
    const RowT cs_orow0 = CSPLIT ? out_row(2 * t0d, 2 * t0h) : 0, cs_srow0 = CSPLIT ? skip_row(2 * t0d, 2 * t0h) : 0;
    auto cls_fetch = [&](auto pcc, auto woffc, auto soffc) {
        constexpr int pc = decltype(pcc)::value, WOFF = decltype(woffc)::value, SOFF = decltype(soffc)::value;
        constexpr int nsteps = t2_nsteps(pc, CIN), sbase = t2_stepbase(pc, CIN);
#pragma unroll
        for (int s = 0; s < nsteps; ++s)
#pragma unroll
            for (int m = 0; m < NT; ++m) wcls[WOFF + s][m] = wpk[((sbase + s) * a.nt_total + nt0 + m) * 64 + lane];
        constexpr int pd = (pc >> 2) & 1, ph = (pc >> 1) & 1, pw = pc & 1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int id = t0d + i / TH, ih = t0h + i % TH;
            const bool in_ok = id < a.Di && ih < a.Hi;     // wave-uniform
#pragma unroll
            for (int m = 0; m < NT; ++m)
                skc[SOFF + i][m] = in_ok ? skip_fetch(cs_srow0 + (pd ? plane_skip : (RowT)0) + (2 * i + ph) * row_skip, pw, m) : make_uint2(0u, 0u);
        }
    };
    if constexpr (CSPLIT) {
        using std::integral_constant;
#define PSCV_CLS_PAIR(W) case W: cls_fetch(integral_constant<int, W>{}, integral_constant<int, 0>{}, integral_constant<int, 0>{}); \
                             cls_fetch(integral_constant<int, 7 - W>{}, integral_constant<int, t2_nsteps(W, CIN)>{}, integral_constant<int, 4>{}); break;
        switch (wave) { PSCV_CLS_PAIR(0) PSCV_CLS_PAIR(1) PSCV_CLS_PAIR(2) default: PSCV_CLS_PAIR(3) }
#undef PSCV_CLS_PAIR
    }
    // k-split: skip values of the wave's own M-tile
    uint2 skk[NT];
    if constexpr (KSPLIT) {
#pragma unroll
        for (int m = 0; m < NT; ++m) {
            const int od = t0d + wave / TH, oh = t0h + wave % TH;
            skk[m] = (od < a.Do && oh < a.Ho) ? skip_fetch(skip_row(od, oh), 0, m) : make_uint2(0u, 0u);
        }
    }
    // per-channel epilogue constants of this block's NT output tiles: requested here, ahead of the brick, and written to LDS with it
    // (requested behind the brick, their round trip stood between the last brick write and the barrier)
    float e_sc = 1.0f, e_bi = 0.0f, e_fl = (a.epi & PSCV_EPI_RELU_PRE) ? 0.0f : -__builtin_inff();
    if (tid < NT * 16) {
        const int c = nt0 * 16 + tid;
        const bool cv = c < a.cout;
        if (a.scale && cv) e_sc = a.scale[c];
        if (a.bias && cv) e_bi = a.bias[c];
        if ((a.epi & PSCV_EPI_RELU_PRE) && a.floor && cv) e_fl = a.floor[c];
    }
    PSCV_STAMP(6)   // (profile builds: slot 6 = tile decode, weight / skip fetches issued; slot 5 is the final drain alone)

    // ---- stage the input brick into LDS (zero fill outside the volume = the conv's padding) ----
    // A thread owns the same in-plane positions (row, column, 16-byte channel chunk) in EVERY plane of the brick: their
    // decomposition, bounds test, 32-bit global offset and LDS offset are computed once per slot, and the plane advances through
    // a wave-uniform base pointer and an immediate LDS offset.  (A flat chunk id decomposed per load cost ~45 vector-ALU
    // instructions per 16-byte chunk: the stride-2 8 -> 16 layer at full resolution and every small-volume layer spent more
    // cycles on that arithmetic than on anything else -- scripts/dev/phase_prof.py.)  Loads are issued in groups of planes that
    // keep <= 16 chunks per thread in flight before any of them is written to LDS, so a group shares one memory latency.
    {
        constexpr int PC = BH * BW * CCH;                 // chunks per brick plane
        constexpr int NS = (PC + 255) / 256;              // in-plane slots per thread
        constexpr int PG = (16 / NS) < 1 ? 1 : ((16 / NS) > BD ? BD : (16 / NS));   // planes per group
        const unsigned long plane_bytes = (unsigned long)a.Hi * a.Wi * a.in_cs * 2;
        const char* inb = reinterpret_cast<const char*>(a.in + (long)b * a.Di * a.Hi * a.Wi * a.in_cs + a.in_co);
        unsigned goff[NS];
        int lds_off[NS];
        bool ok[NS];
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) {
            const int c = sl * 256 + tid;
            const int v = c / CCH, cc = c - v * CCH;
            const int bh = v / BW, bw = v - bh * BW;
            const int gh = o_h + bh, gw = o_w + bw;
            ok[sl] = c < PC && (unsigned)gh < (unsigned)a.Hi && (unsigned)gw < (unsigned)a.Wi;
            goff[sl] = ok[sl] ? (unsigned)(gh * a.Wi + gw) * (unsigned)(a.in_cs * 2) + (unsigned)(cc * 16) : 0u;
            lds_off[sl] = c < PC ? v * VS + cc * 16 : -1;
        }
#pragma unroll
        for (int p0 = 0; p0 < BD; p0 += PG) {
            uint4 val[PG][NS];
#pragma unroll
            for (int pp = 0; pp < PG; ++pp) {
                const int gd = o_d + p0 + pp;                                   // wave-uniform
                const bool pv = p0 + pp < BD && (unsigned)gd < (unsigned)a.Di;
                const char* pb = inb + (unsigned long)(pv ? gd : 0) * plane_bytes;
#pragma unroll
                for (int sl = 0; sl < NS; ++sl) {
                    val[pp][sl] = make_uint4(0u, 0u, 0u, 0u);
                    if (pv && ok[sl]) val[pp][sl] = *reinterpret_cast<const uint4*>(pb + goff[sl]);
                }
            }
            PSCV_STAMP(0)
            PSCV_STAMP_WAIT(1)
#pragma unroll
            for (int pp = 0; pp < PG; ++pp)
#pragma unroll
                for (int sl = 0; sl < NS; ++sl)
                    if (p0 + pp < BD && lds_off[sl] >= 0)
                        *reinterpret_cast<uint4*>(smem + (p0 + pp) * (BH * BW * VS) + lds_off[sl]) = val[pp][sl];
        }
    }
    // per-channel epilogue constants -> LDS (one global read per block)
    constexpr int REGION0 = conv_region0(KIND, CIN, NT, TD, TH);   // brick, later reused by the k-split reduction
    float* epi_sc = reinterpret_cast<float*>(smem + REGION0);
    float* epi_bi = epi_sc + NT * 16;
    float* epi_fl = epi_bi + NT * 16;
    if (tid < NT * 16) {
        epi_sc[tid] = e_sc;
        epi_bi[tid] = e_bi;
        epi_fl[tid] = e_fl;
    }
    __syncthreads();
    PSCV_STAMP(2)

    // per-M-tile LDS anchors of this lane's voxel column (row split: the wave's MB tiles; k / class split: all four)
    constexpr int NA = MB == 1 ? 4 : MB;
    int anchor[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int mt = MB == 1 ? i : wave * MB + i;
        const int td = mt / TH, th = mt % TH;
        anchor[i] = ((td * SXY * BH + th * SXY) * BW + n * SXY) * VS;
    }

    // ---- epilogue (shared by all kinds) ----
    // od, oh are wave-uniform (a row of 16 x-adjacent voxels per M-tile): the row base is scalar arithmetic and a lane adds a
    // 32-bit offset.  The ReLU switches are folded into clamp constants (epi_fl holds -inf without RELU_PRE, lo_post is -inf
    // without RELU_POST) and a missing skip tensor adds +0, so the common case -- a channel count that is a multiple of 4 --
    // is straight-line code: the epilogue is inlined up to 32 times per kernel and its branches used to dominate the code size.
    // The HOT instance reads the lane's 12 constants per N-tile into registers once per contraction (epi_consts, called behind the
    // MFMA loop so that they are not live across it) and not once per row -- up to two N-tiles: the 48 registers of four cost the
    // large tiles a workgroup per CU, and the class split keeps its reads per row too (its first class's epilogue runs with the second
    // class's weights and skip values live: 132 instead of 120 VGPRs at 32 -> 16, a workgroup per CU).  Every caller hands it the
    // skip values.
    const float lo_post = epi_lo_post(a.epi);
    constexpr bool CREG = HOT && NT < 4 && !CSPLIT;
    float4 hsc[CREG ? NT : 1], hbi[CREG ? NT : 1], hfl[CREG ? NT : 1];
    auto epi_consts = [&]() {
        if constexpr (CREG) {
#pragma unroll
            for (int m = 0; m < NT; ++m) {
                hsc[m] = *reinterpret_cast<const float4*>(epi_sc + m * 16 + g * 4);
                hbi[m] = *reinterpret_cast<const float4*>(epi_bi + m * 16 + g * 4);
                hfl[m] = *reinterpret_cast<const float4*>(epi_fl + m * 16 + g * 4);
            }
        }
    };
    auto epilogue_row = [&](const f32x4 (&acc)[NT], RowT orow, RowT srow, int pw, const uint2* pre) {
#pragma unroll
        for (int m = 0; m < NT; ++m) {
            float4 sc, bi, fl;
            if constexpr (CREG) { sc = hsc[m]; bi = hbi[m]; fl = hfl[m]; }
            else {
                sc = *reinterpret_cast<const float4*>(epi_sc + m * 16 + g * 4);
                bi = *reinterpret_cast<const float4*>(epi_bi + m * 16 + g * 4);
                fl = *reinterpret_cast<const float4*>(epi_fl + m * 16 + g * 4);
            }
            float y[4] = {relu_floor(fmaf(acc[m][0], sc.x, bi.x), fl.x), relu_floor(fmaf(acc[m][1], sc.y, bi.y), fl.y),
                          relu_floor(fmaf(acc[m][2], sc.z, bi.z), fl.z), relu_floor(fmaf(acc[m][3], sc.w, bi.w), fl.w)};
            if constexpr (HOT) {
                add_skip4_clamp<H>(y, pre[m], lo_post);
                __builtin_amdgcn_raw_buffer_store_b64(buf_u32x2{Half16<H>::pack(y[0], y[1]), Half16<H>::pack(y[2], y[3])}, ors,
                                                      (int)(lane_out + (unsigned)(m * 32)), (int)(orow + (unsigned)(pw * a.out_cs * 2)), 0);
                continue;
            }
            const unsigned lo = lane_out + (unsigned)(pw * a.out_cs + m * 16), ls = lane_skip + (unsigned)(pw * a.skip_cs + m * 16);
            if (lane_ok && cg + m * 16 < a.cout) {
                if (cout4) {
                    uint2 sv = make_uint2(0u, 0u);
                    if (pre) sv = pre[m];
                    else if (a.skip) sv = *reinterpret_cast<const uint2*>(a.skip + srow + ls);
                    y[0] = relu_floor(y[0] + Half16<H>::lo(sv.x), lo_post); y[1] = relu_floor(y[1] + Half16<H>::hi(sv.x), lo_post);
                    y[2] = relu_floor(y[2] + Half16<H>::lo(sv.y), lo_post); y[3] = relu_floor(y[3] + Half16<H>::hi(sv.y), lo_post);
                    if (a.out_f32) *reinterpret_cast<float4*>(reinterpret_cast<float*>(a.out) + orow + lo) = make_float4(y[0], y[1], y[2], y[3]);
                    else *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(a.out) + orow + lo) =
                             make_uint2(Half16<H>::pack(y[0], y[1]), Half16<H>::pack(y[2], y[3]));
                } else {
                    void* op = a.out_f32 ? static_cast<void*>(reinterpret_cast<float*>(a.out) + orow + lo)
                                         : static_cast<void*>(reinterpret_cast<uint16_t*>(a.out) + orow + lo);
                    epi_ragged<H>(y[0], y[1], y[2], y[3], a.skip ? a.skip + srow + ls : nullptr, op, min(4, a.cout - (cg + m * 16)),
                                  a.out_f32, lo_post);
                }
            }
        }
    };
    auto epilogue = [&](const f32x4 (&acc)[NT], int od, int oh, int pw, const uint2* pre = nullptr) {
        if (od >= a.Do || oh >= a.Ho) return;                      // wave-uniform
        epilogue_row(acc, out_row(od, oh), skip_row(od, oh), pw, pre);
    };

    if constexpr (KSPLIT) {
        // ---- dense kinds, k-split: wave w contracts k-steps w, w+4, ... for all four M-tiles ----
        constexpr int NSTEPS = NSTEPS_ALL;
        f32x4 acc[4][NT];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int m = 0; m < NT; ++m) acc[i][m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < SPW; ++j) {
            const int s = wave + 4 * j;              // wave-uniform
            if (s < NSTEPS) {
                const int kk0 = s * 32 + g * 8;
                const int koff = tap_off_dense<KIND, BH, BW, VS>(kk0 / CIN) + (kk0 % CIN) * 2;
                uint4 wf[NT];
#pragma unroll
                for (int m = 0; m < NT; ++m) wf[m] = wring[j % PF][m];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint4 xf = *reinterpret_cast<const uint4*>(smem + anchor[i] + koff);
#pragma unroll
                    for (int m = 0; m < NT; ++m) acc[i][m] = Mfma<H>::run(wf[m], xf, acc[i][m]);
                }
                if (j + PF < SPW) {
                    int st = s + 4 * PF;
                    st = st < NSTEPS ? st : NSTEPS - 1;
#pragma unroll
                    for (int m = 0; m < NT; ++m) wring[j % PF][m] = wpk[(st * a.nt_total + nt0 + m) * 64 + lane];
                }
            }
        }
        PSCV_STAMP(3)
        epi_consts();
        // partial sums -> LDS (over the brick, which every wave has finished reading), summed in wave order 0..3
        __syncthreads();
        f32x4* red = reinterpret_cast<f32x4*>(smem);       // [source wave][M-tile][N-tile][lane]
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int m = 0; m < NT; ++m) red[((wave * 4 + i) * NT + m) * 64 + lane] = acc[i][m];
        __syncthreads();
        f32x4 fin[NT];
#pragma unroll
        for (int m = 0; m < NT; ++m) {
            f32x4 f = red[((0 * 4 + wave) * NT + m) * 64 + lane];
            f += red[((1 * 4 + wave) * NT + m) * 64 + lane];
            f += red[((2 * 4 + wave) * NT + m) * 64 + lane];
            f += red[((3 * 4 + wave) * NT + m) * 64 + lane];
            fin[m] = f;
        }
        epilogue(fin, t0d + wave / TH, t0h + wave % TH, 0, skk);
        PSCV_STAMP(4)
    } else if constexpr (CSPLIT) {
        // ---- transposed kind, class split: wave w computes parity classes w and 7-w of all four M-tiles ----
        auto cls_run = [&](auto pcc, auto woffc, auto soffc) {
            constexpr int pc = decltype(pcc)::value, WOFF = decltype(woffc)::value, SOFF = decltype(soffc)::value;
            constexpr int nsteps = t2_nsteps(pc, CIN);
            constexpr int pd = (pc >> 2) & 1, ph = (pc >> 1) & 1, pw = pc & 1;
            f32x4 acc[4][NT];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int m = 0; m < NT; ++m) acc[i][m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < nsteps; ++s) {
                const int kk0 = s * 32 + g * 8;
                const int koff = tap_off_t2<BH, BW, VS>(pc, kk0 / CIN) + (kk0 % CIN) * 2;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint4 xf = *reinterpret_cast<const uint4*>(smem + anchor[i] + koff);
#pragma unroll
                    for (int m = 0; m < NT; ++m) acc[i][m] = Mfma<H>::run(wcls[WOFF + s][m], xf, acc[i][m]);
                }
            }
            PSCV_STAMP(3)
            epi_consts();
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int id = t0d + i / TH, ih = t0h + i % TH;
                if (id < a.Di && ih < a.Hi)
                    epilogue_row(acc[i], cs_orow0 + (pd ? plane_out : (RowT)0) + (2 * i + ph) * row_out,
                                 cs_srow0 + (pd ? plane_skip : (RowT)0) + (2 * i + ph) * row_skip, pw, skc[SOFF + i]);
            }
            PSCV_STAMP(4)
        };
        using std::integral_constant;
#define PSCV_CLS_PAIR(W) case W: cls_run(integral_constant<int, W>{}, integral_constant<int, 0>{}, integral_constant<int, 0>{}); \
                             cls_run(integral_constant<int, 7 - W>{}, integral_constant<int, t2_nsteps(W, CIN)>{}, integral_constant<int, 4>{}); break;
        switch (wave) { PSCV_CLS_PAIR(0) PSCV_CLS_PAIR(1) PSCV_CLS_PAIR(2) default: PSCV_CLS_PAIR(3) }
#undef PSCV_CLS_PAIR
    } else if constexpr (KIND != PSCV_CONV_T2) {
        constexpr int NSTEPS = NSTEPS_ALL;
        f32x4 acc[MB][NT];
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int m = 0; m < NT; ++m) acc[i][m] = f32x4{0.f, 0.f, 0.f, 0.f};
        // skip values of the wave's rows, requested before the contraction (inside the epilogue every row waited for its own 8 bytes)
        uint2 skp[MB][NT];
#pragma unroll
        for (int i = 0; i < MB; ++i) {
            const int mt = wave * MB + i;
            const int od = t0d + mt / TH, oh = t0h + mt % TH;
            const bool row_ok = od < a.Do && oh < a.Ho;         // wave-uniform
#pragma unroll
            for (int m = 0; m < NT; ++m) skp[i][m] = row_ok ? skip_fetch(skip_row(od, oh), 0, m) : make_uint2(0u, 0u);
        }

#pragma unroll
        for (int s = 0; s < NSTEPS; ++s) {
            const int kk0 = s * 32 + g * 8;
            const int koff = tap_off_dense<KIND, BH, BW, VS>(kk0 / CIN) + (kk0 % CIN) * 2;
            uint4 wf[NT];
#pragma unroll
            for (int m = 0; m < NT; ++m) wf[m] = wring[s % PF][m];
#pragma unroll
            for (int i = 0; i < MB; ++i) {
                const uint4 xf = *reinterpret_cast<const uint4*>(smem + anchor[i] + koff);
#pragma unroll
                for (int m = 0; m < NT; ++m) acc[i][m] = Mfma<H>::run(wf[m], xf, acc[i][m]);
            }
            if (s + PF < NSTEPS) {
#pragma unroll
                for (int m = 0; m < NT; ++m)
                    wring[s % PF][m] = wpk[((s + PF) * a.nt_total + nt0 + m) * 64 + lane];
            }
        }
        PSCV_STAMP(3)
        epi_consts();
#pragma unroll
        for (int i = 0; i < MB; ++i) {
            const int mt = wave * MB + i;
            epilogue(acc[i], t0d + mt / TH, t0h + mt % TH, 0, skp[i]);
        }
        PSCV_STAMP(4)
    } else {
#pragma unroll
        for (int pc = 0; pc < 8; ++pc) {
            const int nsteps = t2_nsteps(pc, CIN);
            const int sbase = t2_stepbase(pc, CIN);
            f32x4 acc[MB][NT];
#pragma unroll
            for (int i = 0; i < MB; ++i)
#pragma unroll
                for (int m = 0; m < NT; ++m) acc[i][m] = f32x4{0.f, 0.f, 0.f, 0.f};
            // the class's skip values are requested before its contraction (loaded inside the epilogue, every row waited for its own
            // 8 bytes: 8 classes x MB dependent round trips per wave)
            const int pd = (pc >> 2) & 1, ph = (pc >> 1) & 1, pw = pc & 1;
            uint2 skp[MB][NT];
#pragma unroll
            for (int i = 0; i < MB; ++i) {
                const int mt = wave * MB + i;
                const int id = t0d + mt / TH, ih = t0h + mt % TH;
                const bool in_ok = id < a.Di && ih < a.Hi;      // wave-uniform
#pragma unroll
                for (int m = 0; m < NT; ++m) skp[i][m] = in_ok ? skip_fetch(skip_row(2 * id + pd, 2 * ih + ph), pw, m) : make_uint2(0u, 0u);
            }
#pragma unroll
            for (int s = 0; s < 16; ++s) {   // 16 = max k-steps of a class (8 taps x C_in 64)
                if (s < nsteps) {
                    const int kk0 = s * 32 + g * 8;
                    const int koff = tap_off_t2<BH, BW, VS>(pc, kk0 / CIN) + (kk0 % CIN) * 2;
                    const int fs = sbase + s;   // flat step index over all classes (compile-time after unrolling)
                    uint4 wf[NT];
#pragma unroll
                    for (int m = 0; m < NT; ++m) wf[m] = wpk[(fs * a.nt_total + nt0 + m) * 64 + lane];
#pragma unroll
                    for (int i = 0; i < MB; ++i) {
                        const uint4 xf = *reinterpret_cast<const uint4*>(smem + anchor[i] + koff);
#pragma unroll
                        for (int m = 0; m < NT; ++m) acc[i][m] = Mfma<H>::run(wf[m], xf, acc[i][m]);
                    }
                }
            }
            PSCV_STAMP(3)
            epi_consts();
#pragma unroll
            for (int i = 0; i < MB; ++i) {
                const int mt = wave * MB + i;
                const int id = t0d + mt / TH, ih = t0h + mt % TH;
                if (id < a.Di && ih < a.Hi) epilogue(acc[i], 2 * id + pd, 2 * ih + ph, pw, skp[i]);
            }
            PSCV_STAMP(4)
        }
    }
    PSCV_STAMP_WAIT(5)
    PSCV_PROF_END(conv, blockIdx.x + gridDim.x * blockIdx.y)
}

// ---- host side ---------------------------------------------------------------------------------
template <typename H, int CIN, int NT, int KIND, int TD, int TH>
static int launch_conv(ConvArgs& a, int n_split, hipStream_t st) {
    constexpr int LDS = conv_region0(KIND, CIN, NT, TD, TH) + conv_epi_bytes(NT);
    static_assert(LDS <= 160 * 1024, "brick does not fit the 160 KiB LDS");
    const int rd = KIND == PSCV_CONV_T2 ? a.Di : a.Do, rh = KIND == PSCV_CONV_T2 ? a.Hi : a.Ho,
              rw = KIND == PSCV_CONV_T2 ? a.Wi : a.Wo;
    a.ntd = ceil_div(rd, TD); a.nth = ceil_div(rh, TH); a.ntw = ceil_div(rw, 16);
    const long nblk = finish_grid("pscv_conv3d", a.B, a.ntd, a.nth, a.ntw, a.mg_td, a.mg_th, a.mg_tw);
    if (nblk < 0) return -1;
    // the descriptor instance: 32-bit byte offsets inside a batch item's output / skip slice, 8-byte loads and stores
    // (not for the 4 x 4 x 16 tile of 32 -> 64: 264 instead of 248 registers would cost it the second workgroup per CU)
    constexpr bool HOT_FITS = !(KIND == PSCV_CONV_S1 && CIN == 32 && NT == 4 && TD == 4 && TH == 4);
    const long vox = (long)a.Do * a.Ho * a.Wo;
    const bool hot = HOT_FITS && !a.out_f32 && a.cout % 16 == 0 && vox * a.out_cs * 2 < 0x7fff0000L && (reinterpret_cast<uintptr_t>(a.out) & 7) == 0 &&
                     (!a.skip || (vox * a.skip_cs * 2 < 0x7fff0000L && (reinterpret_cast<uintptr_t>(a.skip) & 7) == 0));
    if constexpr (HOT_FITS)
        if (hot) return launch("pscv_conv3d", conv3d_kernel<H, CIN, NT, KIND, TD, TH, true>, dim3((unsigned)nblk, (unsigned)n_split), dim3(256), LDS, st, a);
    return launch("pscv_conv3d", conv3d_kernel<H, CIN, NT, KIND, TD, TH, false>, dim3((unsigned)nblk, (unsigned)n_split), dim3(256), LDS, st, a);
}

// Tile choice.  Large volumes: 4x4x16 (S1), 2x2x16 (S2), 2x4x16 input voxels (T2) with all NT output tiles in one
// workgroup.  Small volumes (the 1/4 and 1/8 resolution levels: 61 k and 7.7 k voxels at the headline size) would
// leave most of the 256 CUs idle, so they use 1x4x16 tiles and one 16-channel output tile per workgroup
// (blockIdx.y splits the output channels): up to 16x more workgroups, each re-reading the L2-resident brick.
template <typename H, int CIN, int NT>
static int launch_kind(ConvArgs& a, int kind, hipStream_t st) {
    a.nt_total = NT;
    const int rd = kind == PSCV_CONV_T2 ? a.Di : a.Do, rh = kind == PSCV_CONV_T2 ? a.Hi : a.Ho,
              rw = kind == PSCV_CONV_T2 ? a.Wi : a.Wo;
    const int TDb = kind == PSCV_CONV_S1 ? 4 : 2, THb = kind == PSCV_CONV_S2 ? 2 : 4;
    const long big = (long)a.B * ceil_div(rd, TDb) * ceil_div(rh, THb) * ceil_div(rw, 16);
    // (stride-2 layers keep the large variant: both have 4 row-tiles per workgroup and the N-split would only
    //  re-read the 5x5x33 input brick once per output tile)
    const bool small = big < 1024 && g_conv_small_tiles && kind != PSCV_CONV_S2;
    // Output-channel tiles per workgroup (NTS) of the small-volume variants and of the stride-2 layers: the grid is
    // tiles x (NT / NTS); fewer, heavier workgroups re-read the brick less often, more, lighter ones fill the CUs of a small
    // volume.  Default: one tile per workgroup (small S1 / T2), all tiles (S2); "conv_small_nt" overrides where it divides NT.
    const int want = (int)g_conv_small_nt;
    auto nts_of = [&](int dflt) { return (want == 1 || want == 2 || want == 4) && want <= NT && NT % want == 0 ? want : dflt; };
#define PSCV_NTS_SWITCH(NTSV, KINDV, TDV, THV)                                                                     \
    switch (NTSV) {                                                                                                  \
        case 1: return launch_conv<H, CIN, 1, KINDV, TDV, THV>(a, NT, st);                                           \
        case 2: if constexpr (NT >= 2) return launch_conv<H, CIN, 2, KINDV, TDV, THV>(a, NT / 2, st); break;         \
        default: if constexpr (NT >= 4) return launch_conv<H, CIN, 4, KINDV, TDV, THV>(a, NT / 4, st); break;        \
    }
    switch (kind) {
        case PSCV_CONV_S1:
            // (measured at the headline size, scripts/dev/small_layers.py: 32 output channels as ONE workgroup per tile -- 1152 workgroups,
            //  one generation -- 11.3 against 12.5 us for two per tile; 64 output channels stay at one tile per workgroup)
            if (small) { PSCV_NTS_SWITCH(nts_of(NT == 2 ? 2 : 1), PSCV_CONV_S1, 1, 4) }
            if constexpr (CIN == 64) {
                // 64 input channels (CVP's 64 -> 64 / 64 -> 32 layers): a wave fetches NT KB of A fragments per k-step for MB x NT
                // MFMAs, and at MB = 4 (4x4x16 tiles) that is 64 B/clk per CU -- the whole vector-memory path, 25 % of the MFMA
                // peak measured.  4x8x16 tiles (MB = 8, 155 KB brick: one workgroup per CU) halve the fetch per MFMA.
                if (g_conv_tall64 == 2 || (g_conv_tall64 && (long)a.B * ceil_div(rd, 4) * ceil_div(rh, 8) * ceil_div(rw, 16) >= 256))
                    return launch_conv<H, CIN, NT, PSCV_CONV_S1, 4, 8>(a, 1, st);
            }
            return launch_conv<H, CIN, NT, PSCV_CONV_S1, 4, 4>(a, 1, st);
        case PSCV_CONV_S2: { PSCV_NTS_SWITCH(nts_of(NT), PSCV_CONV_S2, 2, 2) } break;
        case PSCV_CONV_T2:
            if (small) { PSCV_NTS_SWITCH(nts_of(1), PSCV_CONV_T2, 1, 4) }
            return launch_conv<H, CIN, NT, PSCV_CONV_T2, 2, 4>(a, 1, st);
    }
#undef PSCV_NTS_SWITCH
    set_error("pscv_conv3d: unknown kind %d", kind);
    return -1;
}

template <typename H>
static int launch_channels(ConvArgs& a, int c_in, int c_out, int kind, hipStream_t st) {
    const int nt = (c_out + 15) / 16;
#define PSCV_CONV_CASE(CI, NTV) if (c_in == CI && nt == NTV) return launch_kind<H, CI, NTV>(a, kind, st);
    PSCV_CONV_CASE(8, 1) PSCV_CONV_CASE(8, 2)
    PSCV_CONV_CASE(16, 1) PSCV_CONV_CASE(16, 2)
    PSCV_CONV_CASE(32, 1) PSCV_CONV_CASE(32, 2) PSCV_CONV_CASE(32, 4)
    PSCV_CONV_CASE(64, 2) PSCV_CONV_CASE(64, 4)
#undef PSCV_CONV_CASE
    set_error("pscv_conv3d: unsupported channel combination c_in=%d c_out=%d", c_in, c_out);
    return -1;
}

}  // namespace pscv

PSCV_PROF_EXPORT(conv)

extern "C" int pscv_conv3d_cat2(const void* in_a, int a_cstride, int a_coff, const void* in_b, int b_cstride, int b_coff, int dtype,
                                const uint16_t* packed, const float* scale, const float* bias, const float* floor, const void* skip,
                                int skip_cstride, int skip_coff, void* out, int out_cstride, int out_coff, int out_dtype, int B, int D,
                                int H, int W, int c_out, int epi_flags, void* stream) {
    using namespace pscv;
    PSCV_CHECK_ARG(in_a && in_b && packed && out, "pscv_conv3d_cat2: null pointer argument");
    PSCV_CHECK_ARG(B > 0 && D > 0 && H > 0 && W > 0, "pscv_conv3d_cat2: bad sizes");
    PSCV_CHECK_ARG(c_out == 8 || c_out == 16, "pscv_conv3d_cat2: c_out=%d must be 8 or 16", c_out);
    PSCV_CHECK_ARG(a_cstride % 8 == 0 && a_coff % 8 == 0 && a_coff + 8 <= a_cstride && b_cstride % 8 == 0 && b_coff % 8 == 0 && b_coff + 8 <= b_cstride,
                   "pscv_conv3d_cat2: both inputs contribute an 8-aligned slice of 8 channels");
    PSCV_CHECK_ARG(out_coff + c_out <= out_cstride && out_cstride % 4 == 0 && out_coff % 4 == 0, "pscv_conv3d_cat2: bad output channel slice");
    PSCV_CHECK_ARG(!skip || (skip_cstride % 4 == 0 && skip_coff % 4 == 0), "pscv_conv3d_cat2: skip slice must be 4-aligned");
    PSCV_CHECK_ARG(dtype == PSCV_BF16 || dtype == PSCV_F16, "pscv_conv3d_cat2: storage dtype %d must be bf16 or fp16", dtype);
    PSCV_CHECK_ARG(out_dtype == dtype || out_dtype == PSCV_F32, "pscv_conv3d_cat2: out dtype %d must be the storage dtype or fp32", out_dtype);
    ConvCall c{};
    c.io = {reinterpret_cast<const uint16_t*>(in_a), packed, scale, bias, floor, reinterpret_cast<const uint16_t*>(skip), out,
            a_cstride, a_coff, skip_cstride, skip_coff, out_cstride, out_coff, out_dtype == PSCV_F32, B};
    c.dtype = dtype; c.D = D; c.H = H; c.W = W; c.c_in = 16; c.c_out = c_out; c.epi = epi_flags;
    c.st = reinterpret_cast<hipStream_t>(stream);
    c.in2 = reinterpret_cast<const uint16_t*>(in_b); c.in2_cs = b_cstride; c.in2_co = b_coff;
    return conv3d_sweepc_launch(c);
}

extern "C" int pscv_conv3d(const void* in, int dtype, int in_cstride, int in_coff, const uint16_t* packed, const float* scale,
                           const float* bias, const float* floor, const void* skip, int skip_cstride, int skip_coff,
                           void* out, int out_cstride, int out_coff, int out_dtype, int B, int Di, int Hi, int Wi,
                           int c_in, int c_out, int kind, int epi_flags, void* stream) {
    using namespace pscv;
    PSCV_CHECK_ARG(in && packed && out, "pscv_conv3d: null pointer argument");
    PSCV_CHECK_ARG(B > 0 && Di > 0 && Hi > 0 && Wi > 0, "pscv_conv3d: bad sizes");
    PSCV_CHECK_ARG(in_cstride % 8 == 0 && in_coff % 8 == 0 && in_coff + c_in <= in_cstride,
                   "pscv_conv3d: input channel slice [%d,%d) of stride %d must be 8-aligned", in_coff, in_coff + c_in, in_cstride);
    PSCV_CHECK_ARG(out_coff + c_out <= out_cstride, "pscv_conv3d: output channel slice exceeds stride");
    PSCV_CHECK_ARG(c_out < 4 || (out_cstride % 4 == 0 && out_coff % 4 == 0), "pscv_conv3d: output slice must be 4-aligned");
    PSCV_CHECK_ARG(!skip || c_out < 4 || (skip_cstride % 4 == 0 && skip_coff % 4 == 0), "pscv_conv3d: skip slice must be 4-aligned");
    PSCV_CHECK_ARG(dtype == PSCV_BF16 || dtype == PSCV_F16, "pscv_conv3d: storage dtype %d must be bf16 or fp16", dtype);
    PSCV_CHECK_ARG(out_dtype == dtype || out_dtype == PSCV_F32, "pscv_conv3d: out dtype %d must be the storage dtype or fp32", out_dtype);
    ConvCall c{};
    c.io = {reinterpret_cast<const uint16_t*>(in), packed, scale, bias, floor, reinterpret_cast<const uint16_t*>(skip), out,
            in_cstride, in_coff, skip_cstride, skip_coff, out_cstride, out_coff, out_dtype == PSCV_F32, B};
    c.dtype = dtype; c.D = Di; c.H = Hi; c.W = Wi; c.c_in = c_in; c.c_out = c_out; c.epi = epi_flags;
    c.st = reinterpret_cast<hipStream_t>(stream);
    if (kind == PSCV_CONV_S1P8) {
        PSCV_CHECK_ARG(((c_in == 8 || c_in == 16 || c_in == 32) && c_out == 8) || (c_in == 16 && c_out == 16),
                       "pscv_conv3d: the sweep kernels (S1P8) are for 8|16|32 -> 8 and 16 -> 16 (got %d -> %d)", c_in, c_out);
        return c_in == 32 ? conv3d_sweep8_launch(c) : conv3d_sweepc_launch(c);
    }
    if (kind == PSCV_CONV_T2P8) {
        PSCV_CHECK_ARG(c_in == 16 && c_out == 8, "pscv_conv3d: the parity-pair kernel (T2P8) is for c_in=16, c_out=8 (got %d -> %d)", c_in, c_out);
        return conv3d_t2p8_launch(c);
    }
    if (kind == PSCV_CONV_S1C1) {
        PSCV_CHECK_ARG(c_out == 1 && (c_in == 8 || c_in == 16), "pscv_conv3d: the 1-channel kernel (S1C1) is for c_in 8/16 -> 1 (got %d -> %d)", c_in, c_out);
        return conv3d_c1_launch(c);
    }
    // the two kernels that take a layer only at some sizes: 1 = not theirs, the brick kernel below runs it
    if (kind == PSCV_CONV_S2) {      // 8-channel inputs on large volumes: the stride-2 depth sweep (conv3d_sweep_s2.hip), same packing
        const int rc = conv3d_sweep_s2_launch(c);
        if (rc != 1) return rc;
    }
    if (kind == PSCV_CONV_S1) {      // wide layers (32 | 64 -> 32 | 64) on large volumes: 8-wave workgroups, weights through LDS (conv3d_wide.hip)
        const int rc = conv3d_wide_launch(c);
        if (rc != 1) return rc;
    }
    ConvArgs a;
    static_cast<ConvIO&>(a) = c.io;
    a.Di = Di; a.Hi = Hi; a.Wi = Wi;
    if (kind == PSCV_CONV_S1) { a.Do = Di; a.Ho = Hi; a.Wo = Wi; }
    else if (kind == PSCV_CONV_S2) { a.Do = (Di + 1) / 2; a.Ho = (Hi + 1) / 2; a.Wo = (Wi + 1) / 2; }
    else { a.Do = 2 * Di; a.Ho = 2 * Hi; a.Wo = 2 * Wi; }
    a.cout = c_out; a.epi = epi_flags;
    return with_half("pscv_conv3d", dtype, [&](auto t) { return launch_channels<typename decltype(t)::type>(a, c_in, c_out, kind, c.st); });
}
