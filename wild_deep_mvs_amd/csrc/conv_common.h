// Host half shared by the 3-D convolution kernels (conv3d*.hip): the head of their argument blocks, the call descriptor that the
// extern "C" entry points hand to the launchers, the launchers' declarations, the depth-chunk plan and the grid finish.
// A new conv kernel is a kernel, a `struct XArgs : ConvIO`, a launcher declared here and one branch in pscv_conv3d.
// The device half -- buffer descriptors and the zero-padding rule, the plane fetch, the epilogue pieces -- is conv_dev.h.
#pragma once
#include "pscv_common.h"

namespace pscv {

// What every conv kernel is told about its tensors: channels-last 16-bit volumes addressed as (voxel * channel stride + channel offset).
// The kernels' argument blocks derive from it (C1Args excepted: see there) and add their own dimension, tile and reciprocal fields,
// which are named and counted differently per kernel -- so the base stops at B, at 88 bytes without tail padding, and what follows
// it starts at the same byte in every kernel.
struct ConvIO {
    const uint16_t* in;
    const uint16_t* wpk;     // packed weights (pscv_pack_conv3d_weights; the layout is the kernel's, stated at its XArgs)
    const float* scale;      // per output channel, device; each may be null
    const float* bias;
    const float* floor;
    const uint16_t* skip;    // null = no skip add
    void* out;
    int in_cs, in_co, skip_cs, skip_co, out_cs, out_co;
    int out_f32;             // out holds fp32, else the storage type
    int B;
};
static_assert(sizeof(ConvIO) == 88, "7 pointers + 8 ints: the kernels' own fields follow at byte 88");

// One call of a conv entry point, built once by the extern "C" function after its argument checks.
struct ConvCall {
    ConvIO io;
    int dtype;               // storage type of in / skip (and of out unless io.out_f32)
    int D, H, W;             // the INPUT volume
    int c_in, c_out, epi;
    hipStream_t st;
    const uint16_t* in2;     // pscv_conv3d_cat2: input channels 8..15 come from this tensor (null: from io.in)
    int in2_cs, in2_co;
};

// Fused-head outputs of the 1-channel kernel (pscv_prob_softargmin, pscv_head_index_entropy); all null for a plain convolution.
struct HeadOut {
    const float* depth;      // [B][D] depth planes, row stride depth_bstride
    long depth_bstride;
    float* part;             // workspace of part_floats floats: per-chunk softmax partials
    long part_floats;
    float *o_depth, *o_conf;
    float *o_index, *o_entropy;
};

// The launchers behind pscv_conv3d / pscv_conv3d_cat2, one per kernel file.  All return 0 when they launched, 1 when the layer or size
// is not this kernel's (nothing was launched and no error is set: the caller falls through to the next kernel), and a negative
// code with set_error otherwise.  A launcher that returned 0 has checked its launch (pscv::launch).
int conv3d_sweep8_launch(const ConvCall& c);      // conv3d_sweep.hip: S1P8, 32 -> 8
int conv3d_sweepc_launch(const ConvCall& c);      // conv3d_sweep.hip: S1P8, 8 | 16 -> 8 and 16 -> 16; c.in2 for cat2
int conv3d_sweep_s2_launch(const ConvCall& c);    // conv3d_sweep_s2.hip: S2, 8 -> <= 32 on large volumes
int conv3d_wide_launch(const ConvCall& c);        // conv3d_wide.hip: S1, 32 | 64 -> 32 | 64 on large volumes
int conv3d_c1_launch(const ConvCall& c);          // conv3d_c1.hip: S1C1
int conv3d_t2p8_launch(const ConvCall& c);        // conv3d_t2p8.hip: T2P8
// conv3d_c1.hip: merges the per-chunk softmax partials h.part of `ndc` depth chunks into h.o_depth / h.o_conf (null: no confidence).  Of `c`
// it reads io.out (the fp32 logits), io.B, D, H, W (of the logits) and st.  Launches only: the caller checks.
void softargmin_merge_launch(const ConvCall& c, const HeadOut& h, int ndc);

// Depth-chunk plan of the sweep kernels: `tiles` in-plane tiles share `slots` workgroups that are resident at once, so the depth axis
// is cut into slots / tiles chunks -- one round of workgroups, and as few chunk seams as that allows.  Returns the planes per chunk:
// at least min_dc, rounded up to even where the kernel walks plane pairs (`even`), replaced by a positive `forced` (a knob; made
// even by rounding down), never more than the depth (rounded up to even).  The caller derives its chunk count, ceil(D / dc).
inline int plan_depth_chunk(int D, long tiles, long slots, int min_dc, bool even, int forced) {
    const long ndc_want = tiles >= slots ? 1 : slots / tiles;
    int dc = (int)((D + ndc_want - 1) / ndc_want);
    if (even) dc = (dc + 1) & ~1;
    dc = dc < min_dc ? min_dc : dc;
    if (forced > 0) dc = even ? forced & ~1 : forced;
    return dc > D ? (even ? (D + 1) & ~1 : D) : dc;
}

// Grid finish: the reciprocals of the three tile counts that a workgroup decodes its id with (fast_divmod), and the 1-D grid
// B * n0 * n1 * n2.  Returns the grid, or -1 with "<what>: bad grid" set where it is empty or beyond 2^31 - 1.
inline long finish_grid(const char* what, int B, int n0, int n1, int n2, unsigned& mg0, unsigned& mg1, unsigned& mg2) {
    mg0 = fast_div_magic(n0); mg1 = fast_div_magic(n1); mg2 = fast_div_magic(n2);
    const long nblk = (long)B * n0 * n1 * n2;
    if (nblk <= 0 || nblk > 0x7fffffffL) { set_error("%s: bad grid %ld", what, nblk); return -1; }
    return nblk;
}

}  // namespace pscv
