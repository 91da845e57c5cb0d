// Image preparation: PIL's Lanczos resize of 8-bit images, bit for bit, and the nearest-neighbour resize + crop of a ground-truth
// depth map (the reference's preprocess.py:157-164, data/MVSDataset.py:read_img, data/md_yao.py:99-102,123; INTEGRATION.md
// section 2k).  gfx950.
//
// ---- pscv_resample_u8_pass --------------------------------------------------------------------------------------------
// PIL resamples separably (libImaging/Resample.c): the horizontal pass, its result rounded to 8 bits, then the vertical pass.  Per
// output sample o of a pass the host tables (ops.lanczos_tables) hold first(o), n(o) and n 22-bit fixed-point weights, and
//     acc = 2^21 + sum_k coeff[o][k] * src[first + k]     (int32)
//     out = clamp(acc >> 22, 0, 255)                      (arithmetic shift)
// for every channel.  Integers only, so the result does not depend on the order of the sum and equals PIL's byte for byte.
// Mapping: one lane per output pixel, all of its channels.
//   horizontal  block 64 x 4: 64 neighbouring output columns of 4 rows.  The table is stored TRANSPOSED, [ksize][out_len], so the
//               64 lanes read 64 neighbouring weights per tap; their source bytes lie within 64 * scale * C bytes of one row.
//   vertical    block 256 x 1: 256 neighbouring columns of ONE output row, so first, n and the weights are uniform over the
//               workgroup (scalar loads from the [out_len][ksize] table) and every tap reads 256 * C consecutive bytes of a row.
//   A table entry is never trusted with an address: first and n are clipped to the source before the loop.
// The launches move a few MB each and are bound by latency; nothing is staged in LDS.
// The optional fp32 output is planar ([C][rows][cols]) and holds lut[v], the caller's 256-entry table of float(v) / 255.0f
// (numpy's division on the host: a multiply by the reciprocal does not give the same bits).
// coeff == NULL on the vertical axis is the identity pass (output row o = source row out_first + o): the crop, and the fp32
// conversion, of an image that needs no resampling.
//
// ---- pscv_depth_nearest_crop ------------------------------------------------------------------------------------------
// F.interpolate(mode="nearest") on CPU torch, per axis: src = min((int)floorf(dst * scale), in - 1), scale = (float)in / (float)out
// in fp32; then the window, and mask = (d >= min_d) & (d < max_d) (a NaN depth fails both).  One lane per output pixel.
#include "pscv_common.h"

namespace pscv {

constexpr int RS_PRECISION_BITS = 32 - 8 - 2;
constexpr int RS_HX = 64, RS_HY = 4;           // horizontal pass: columns x rows of a workgroup
constexpr int RS_VX = 256;                     // vertical pass: columns of a workgroup
constexpr int RS_MAX_GRID_Y = 65535;

__device__ __forceinline__ unsigned char rs_clip8(int acc) {
    const int v = acc >> RS_PRECISION_BITS;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// src: `lines` rows of in_len pixels, row pitch src_pitch bytes.  dst [lines][out_count][C]; dst_f32 [C][lines][out_count].
template <int C>
__global__ __launch_bounds__(RS_HX* RS_HY) void resample_h_kernel(const unsigned char* __restrict__ src, long src_pitch, int lines,
                                                                   int in_len, const int* __restrict__ coeff_t,
                                                                   const int* __restrict__ bounds, int ksize, int out_len,
                                                                   int out_first, int out_count, unsigned char* __restrict__ dst,
                                                                   float* __restrict__ dst_f32, const float* __restrict__ lut) {
    const int x = blockIdx.x * RS_HX + threadIdx.x;
    const int row = blockIdx.y * RS_HY + threadIdx.y;
    if (x >= out_count || row >= lines) return;
    const int o = out_first + x;
    int first = bounds[2 * o], n = bounds[2 * o + 1];
    first = first < 0 ? 0 : (first > in_len ? in_len : first);
    n = n < 0 ? 0 : (n > ksize ? ksize : n);
    n = n > in_len - first ? in_len - first : n;
    const unsigned char* s = src + (long)row * src_pitch + (long)first * C;
    const int* ck = coeff_t + o;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (RS_PRECISION_BITS - 1);
    for (int k = 0; k < n; ++k) {
        const int w = ck[(long)k * out_len];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += w * (int)s[k * C + c];
    }
    const long pix = (long)row * out_count + x;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const unsigned char v = rs_clip8(acc[c]);
        dst[pix * C + c] = v;
        if (dst_f32) dst_f32[(long)c * lines * out_count + pix] = lut[v];
    }
}

// src: in_len rows of `lines` pixels, row pitch src_pitch bytes.  dst [out_count][lines][C]; dst_f32 [C][out_count][lines].
// coeff == nullptr: the identity pass.
template <int C>
__global__ __launch_bounds__(RS_VX) void resample_v_kernel(const unsigned char* __restrict__ src, long src_pitch, int lines, int in_len,
                                                           const int* __restrict__ coeff, const int* __restrict__ bounds, int ksize,
                                                           int out_first, int out_count, unsigned char* __restrict__ dst,
                                                           float* __restrict__ dst_f32, const float* __restrict__ lut) {
    const int x = blockIdx.x * RS_VX + threadIdx.x;
    const int y = blockIdx.y;                                  // uniform: the row's table entries come through scalar loads
    if (x >= lines) return;
    const int o = out_first + y;
    int acc[C];
    if (coeff) {
        int first = bounds[2 * o], n = bounds[2 * o + 1];
        first = first < 0 ? 0 : (first > in_len ? in_len : first);
        n = n < 0 ? 0 : (n > ksize ? ksize : n);
        n = n > in_len - first ? in_len - first : n;
        const unsigned char* s = src + (long)first * src_pitch + (long)x * C;
        const int* ck = coeff + (long)o * ksize;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 1 << (RS_PRECISION_BITS - 1);
        for (int k = 0; k < n; ++k) {
            const int w = ck[k];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += w * (int)s[(long)k * src_pitch + c];
        }
    } else {
        const unsigned char* s = src + (long)o * src_pitch + (long)x * C;      // (the host checks o < in_len)
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = (int)s[c] << RS_PRECISION_BITS;
    }
    const long pix = (long)y * lines + x;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const unsigned char v = rs_clip8(acc[c]);
        dst[pix * C + c] = v;
        if (dst_f32) dst_f32[(long)c * out_count * lines + pix] = lut[v];
    }
}

__global__ __launch_bounds__(256) void depth_nearest_crop_kernel(const float* __restrict__ depth, int th, int tw, float scale_h,
                                                                 float scale_w, int y0, int x0, int ch, int cw, float min_d,
                                                                 float max_d, float* __restrict__ out_depth,
                                                                 unsigned char* __restrict__ out_mask) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= cw || y >= ch) return;
    int sy = (int)floorf((float)(y0 + y) * scale_h);
    int sx = (int)floorf((float)(x0 + x) * scale_w);
    sy = sy > th - 1 ? th - 1 : (sy < 0 ? 0 : sy);
    sx = sx > tw - 1 ? tw - 1 : (sx < 0 ? 0 : sx);
    const float d = depth[(long)sy * tw + sx];
    const long k = (long)y * cw + x;
    out_depth[k] = d;
    out_mask[k] = (d >= min_d && d < max_d) ? 1 : 0;
}

}  // namespace pscv

extern "C" int pscv_resample_u8_pass(const unsigned char* src, long src_pitch, int lines, int in_len, int C, int axis, const int* coeff,
                                     const int* bounds, int ksize, int out_len, int out_first, int out_count, unsigned char* dst,
                                     float* dst_f32, const float* lut, void* stream) {
    using namespace pscv;
    const char* what = "pscv_resample_u8_pass";
    PSCV_CHECK_ARG(src && dst, "%s: null pointer argument", what);
    PSCV_CHECK_ARG(C == 1 || C == 3, "%s: C=%d must be 1 or 3", what, C);
    PSCV_CHECK_ARG(axis == 0 || axis == 1, "%s: axis=%d must be 0 (horizontal) or 1 (vertical)", what, axis);
    PSCV_CHECK_ARG(lines >= 1 && in_len >= 1 && out_len >= 1, "%s: lines=%d, in_len=%d, out_len=%d must be >= 1", what, lines, in_len,
                   out_len);
    PSCV_CHECK_ARG(out_first >= 0 && out_count >= 1 && out_count <= out_len - out_first,
                   "%s: outputs [%d, %d + %d) outside [0, %d)", what, out_first, out_first, out_count, out_len);
    PSCV_CHECK_ARG(!dst_f32 || lut, "%s: the fp32 output needs the 256-entry table", what);
    const long row_bytes = (long)(axis == 0 ? in_len : lines) * C;
    PSCV_CHECK_ARG(src_pitch >= row_bytes, "%s: src_pitch=%ld below a row's %ld bytes", what, src_pitch, row_bytes);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (axis == 0) {
        PSCV_CHECK_ARG(coeff && bounds && ksize >= 1, "%s: the horizontal pass needs its tables (ksize=%d)", what, ksize);
        const dim3 grid((unsigned)((out_count + RS_HX - 1) / RS_HX), (unsigned)((lines + RS_HY - 1) / RS_HY));
        PSCV_CHECK_ARG(grid.y <= (unsigned)RS_MAX_GRID_Y, "%s: lines=%d: more than %d rows", what, lines, RS_MAX_GRID_Y * RS_HY);
        const dim3 block(RS_HX, RS_HY);
        return C == 3 ? launch(what, resample_h_kernel<3>, grid, block, 0, st, src, src_pitch, lines, in_len, coeff, bounds, ksize, out_len,
                               out_first, out_count, dst, dst_f32, lut)
                      : launch(what, resample_h_kernel<1>, grid, block, 0, st, src, src_pitch, lines, in_len, coeff, bounds, ksize, out_len,
                               out_first, out_count, dst, dst_f32, lut);
    }
    if (coeff)
        PSCV_CHECK_ARG(bounds && ksize >= 1, "%s: the vertical pass needs both tables (ksize=%d)", what, ksize);
    else
        PSCV_CHECK_ARG(out_len == in_len, "%s: the identity pass needs out_len == in_len (%d, %d)", what, out_len, in_len);
    PSCV_CHECK_ARG(out_count <= RS_MAX_GRID_Y, "%s: out_count=%d: more than %d rows", what, out_count, RS_MAX_GRID_Y);
    const dim3 grid((unsigned)((lines + RS_VX - 1) / RS_VX), (unsigned)out_count);
    return C == 3 ? launch(what, resample_v_kernel<3>, grid, dim3(RS_VX), 0, st, src, src_pitch, lines, in_len, coeff, bounds, ksize,
                           out_first, out_count, dst, dst_f32, lut)
                  : launch(what, resample_v_kernel<1>, grid, dim3(RS_VX), 0, st, src, src_pitch, lines, in_len, coeff, bounds, ksize,
                           out_first, out_count, dst, dst_f32, lut);
}

extern "C" int pscv_depth_nearest_crop(const float* depth, int th, int tw, int oh, int ow, int y0, int x0, int ch, int cw, float min_d,
                                       float max_d, float* out_depth, unsigned char* out_mask, void* stream) {
    using namespace pscv;
    const char* what = "pscv_depth_nearest_crop";
    PSCV_CHECK_ARG(depth && out_depth && out_mask, "%s: null pointer argument", what);
    PSCV_CHECK_ARG(th >= 1 && tw >= 1 && oh >= 1 && ow >= 1, "%s: sizes %d x %d -> %d x %d must be >= 1", what, th, tw, oh, ow);
    PSCV_CHECK_ARG(y0 >= 0 && x0 >= 0 && ch >= 1 && cw >= 1 && ch <= oh - y0 && cw <= ow - x0,
                   "%s: window (%d, %d, %d, %d) outside the %d x %d map", what, y0, x0, ch, cw, oh, ow);
    PSCV_CHECK_ARG(ch <= RS_MAX_GRID_Y, "%s: ch=%d: more than %d rows", what, ch, RS_MAX_GRID_Y);
    const float scale_h = (float)th / (float)oh, scale_w = (float)tw / (float)ow;
    return launch(what, depth_nearest_crop_kernel, dim3((unsigned)((cw + 255) / 256), (unsigned)ch), dim3(256), 0,
                  reinterpret_cast<hipStream_t>(stream), depth, th, tw, scale_h, scale_w, y0, x0, ch, cw, min_d, max_d, out_depth, out_mask);
}
