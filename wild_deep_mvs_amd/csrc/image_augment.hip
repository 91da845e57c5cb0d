// Training-view augmentation: the reference's MVSDataset.data_augmentation (data/MVSDataset.py:124-150; BlendedMVS in train mode)
// on V views of one size, interleaved uint8 [V][H][W][3] in, planar fp32 [V][3][ch][cw] out.  gfx950.
//
// ---- the rule ---------------------------------------------------------------------------------------------------------
// Colour jitter is torchvision's ColorJitter on a PIL image: ImageEnhance.Brightness and ImageEnhance.Contrast, each of which is
// Image.blend(degenerate, image, factor) (libImaging/Blend.c).  Per byte v, with a the fp32 factor and deg the degenerate byte,
//     t = (float)deg + a * (float)((int)v - (int)deg)        the product rounded to fp32, THEN the sum rounded to fp32
//     0 <= a <= 1: the byte is t truncated;  otherwise 0 where t <= 0, 255 where t >= 255, else t truncated.
// Brightness: deg = 0.  Contrast: deg = m in every channel, m = int(mean(L) + 0.5) over the WHOLE image as it stands when the
// contrast step runs (after brightness where that comes first), L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16; in integers
// m = (2 S + n) / (2 n) with S the 64-bit sum of L and n = H W.
// The blur is a 3 x 3 correlation of lut[byte] (the caller's float32(v) / 255) with nine fp32 weights under BORDER_REFLECT_101 at
// the borders of the whole image: taps of weight zero are neither read nor added; the others are accumulated in row-major order,
// every product and every sum rounded to fp32.  A kernel whose only weight is the centre's 1 returns lut[byte] bit for bit.
// Both are TWO-ROUNDING rules: a fused multiply-add gives other bits.  The Makefile compiles this file with -ffp-contract=off and
// the pragma below says the same to whoever compiles it otherwise.
//
// ---- the launches -----------------------------------------------------------------------------------------------------
// augment_sum_kernel    grid (blocks of AUG_SUM_PIXELS pixels, V): per view that has a contrast step, the sum of L, one integer
//                       atomic per workgroup onto the view's 64-bit word (zeroed on the stream in front of the launch).  Integer
//                       addition: the order does not matter, equal inputs give equal sums.  A view that starts on a 4-byte
//                       boundary is read 4 pixels (3 words) per lane; any other, byte by byte.
// augment_apply_kernel  grid (window tiles of 64 x 16, V).  A view's colour steps depend on the byte alone, so a workgroup first makes
//                       the 256-entry table byte -> lut[jittered byte] in LDS (one blend chain per lane, m derived from the sum
//                       on the device), then stages its tile plus a one-pixel halo through the table ONCE: no tap recomputes a
//                       blend.  Lane j stages byte j of every row (neighbouring bytes of an image row, but for the reflected
//                       ends; all of a lane's loads are in flight together).  Every lane then sums the live taps of 4 pixels of
//                       one column; a wave writes 64 neighbouring floats of a plane's row.
// The per-view records (two operations, two factors, nine weights) travel in the kernel arguments.
#include "pscv_common.h"

#pragma clang fp contract(off)

namespace pscv {

constexpr int AUG_MAX_VIEWS = PSCV_AUG_MAX_VIEWS;
constexpr int AUG_SUM_BLOCK = 256;
constexpr int AUG_SUM_PIXELS = AUG_SUM_BLOCK * 16;      // of one workgroup: 4096 * 255 fits a 32-bit partial sum.  Measured at 5 x 576 x 768:
                                                        // 1024 pixels (four times the atomics on a view's word) took 28.6 us, 4096 take 10.8 us
constexpr int AUG_TW = 64, AUG_TH = 16;                 // the apply launch's tile of the window
constexpr int AUG_LANE_ROWS = 4;                        // block 64 x (AUG_TH / AUG_LANE_ROWS)
constexpr int AUG_BLOCK = AUG_TW * AUG_TH / AUG_LANE_ROWS;
constexpr int AUG_ROW_BYTES = (AUG_TW + 2) * 3;         // of a staged row: the tile's columns and one more on either side
constexpr int AUG_PITCH = AUG_ROW_BYTES + 1;            // floats of a staged row (odd: rows start on different banks)
constexpr int AUG_MAX_GRID_Y = 65535;

struct AugTable {
    int op[AUG_MAX_VIEWS][2];
    float factor[AUG_MAX_VIEWS][2];
    int inside[AUG_MAX_VIEWS][2];                       // 0 <= factor <= 1: Blend.c's branch without the clip
    float weight[AUG_MAX_VIEWS][9];
};

__device__ __forceinline__ int aug_blend(int deg, int v, float a, int inside) {
    const float t = (float)deg + a * (float)(v - deg);
    if (inside) return (int)t;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

__device__ __forceinline__ int aug_reflect101(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);         // (n = 1 reads 0; never an address outside the row)
}

// m of the contrast step of view v
__device__ __forceinline__ int aug_mean(const unsigned long long* __restrict__ sums, int v, long n) {
    const unsigned long long s = sums[v];
    const unsigned long long m = (2ull * s + (unsigned long long)n) / (2ull * (unsigned long long)n);
    return m > 255ull ? 255 : (int)m;
}

// L of one pixel, after the brightness step where that runs in front of contrast
__device__ __forceinline__ unsigned int aug_luma(int r, int g, int b, bool bright, float a, int inside) {
    if (bright) {
        r = aug_blend(0, r, a, inside);
        g = aug_blend(0, g, a, inside);
        b = aug_blend(0, b, a, inside);
    }
    return (unsigned int)(19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16;
}
__device__ __forceinline__ int aug_byte(const unsigned int (&w)[3], int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 0xffu); }

__global__ __launch_bounds__(AUG_SUM_BLOCK) void augment_sum_kernel(const unsigned char* __restrict__ imgs, long n, AugTable tab,
                                                                    unsigned long long* __restrict__ sums) {
    const int v = blockIdx.y;
    const int step = tab.op[v][0] == PSCV_AUG_CONTRAST ? 0 : (tab.op[v][1] == PSCV_AUG_CONTRAST ? 1 : -1);
    if (step < 0) return;
    const bool bright = step == 1 && tab.op[v][0] == PSCV_AUG_BRIGHTNESS;
    const float a = tab.factor[v][0];
    const int inside = tab.inside[v][0];
    const unsigned char* img = imgs + (long)v * n * 3;
    unsigned int acc = 0;
    if (((uintptr_t)img & 3) == 0) {
        // the view starts on a word: 4 pixels = 3 words per lane and load, a wave reads 768 neighbouring bytes
        const long groups = n >> 2;
        const unsigned int* words = reinterpret_cast<const unsigned int*>(img);
        for (int k = 0; k < AUG_SUM_PIXELS / 4 / AUG_SUM_BLOCK; ++k) {
            const long g = (long)blockIdx.x * (AUG_SUM_PIXELS / 4) + (long)k * AUG_SUM_BLOCK + threadIdx.x;
            if (g < groups) {
                const unsigned int w[3] = {words[3 * g], words[3 * g + 1], words[3 * g + 2]};
#pragma unroll
                for (int p = 0; p < 4; ++p) acc += aug_luma(aug_byte(w, 3 * p), aug_byte(w, 3 * p + 1), aug_byte(w, 3 * p + 2), bright, a, inside);
            }
        }
        const long p = 4 * groups + threadIdx.x;                          // the last n % 4 pixels, once
        if (blockIdx.x == 0 && p < n) acc += aug_luma(img[3 * p], img[3 * p + 1], img[3 * p + 2], bright, a, inside);
    } else {
        const long first = (long)blockIdx.x * AUG_SUM_PIXELS;
        for (int k = 0; k < AUG_SUM_PIXELS / AUG_SUM_BLOCK; ++k) {
            const long p = first + (long)k * AUG_SUM_BLOCK + threadIdx.x;
            if (p < n) acc += aug_luma(img[3 * p], img[3 * p + 1], img[3 * p + 2], bright, a, inside);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    __shared__ unsigned int wave_sum[AUG_SUM_BLOCK / 64];
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
#pragma unroll
        for (int w = 0; w < AUG_SUM_BLOCK / 64; ++w) total += wave_sum[w];
        atomicAdd(&sums[v], total);
    }
}

__global__ __launch_bounds__(AUG_BLOCK) void augment_apply_kernel(const unsigned char* __restrict__ imgs, int H, int W, AugTable tab,
                                                                  const unsigned long long* __restrict__ sums, int x0, int y0, int cw,
                                                                  int ch, const float* __restrict__ lut, float* __restrict__ out) {
    __shared__ float tile[(AUG_TH + 2) * AUG_PITCH];
    __shared__ float unit[256];
    const int v = blockIdx.z;
    const long n = (long)H * W;
    const unsigned char* img = imgs + (long)v * n * 3;
    const int tx0 = blockIdx.x * AUG_TW, ty0 = blockIdx.y * AUG_TH;
    const int tw = min(AUG_TW, cw - tx0), th = min(AUG_TH, ch - ty0);     // the tile's part of the window, >= 1 each
    const int tid = threadIdx.y * AUG_TW + threadIdx.x;

    // the view's colour steps are a function of the byte alone: lane b makes entry b of the table byte -> lut[jittered byte]
    static_assert(AUG_BLOCK == 256, "one lane per byte value");
    {
        int b = tid;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int op = tab.op[v][s];
            if (op != PSCV_AUG_NONE) b = aug_blend(op == PSCV_AUG_CONTRAST ? aug_mean(sums, v, n) : 0, b, tab.factor[v][s], tab.inside[v][s]);
        }
        unit[tid] = lut[b];
    }

    // stage rows ty0 - 1 .. ty0 + th and columns tx0 - 1 .. tx0 + tw of the window, reflected at the image's borders: lane j takes
    // byte j of every staged row (neighbouring lanes, neighbouring bytes of an image row, but for the reflected ends; the row is
    // uniform, so its reflection is scalar work); every load is issued before the first is used
    static_assert(AUG_ROW_BYTES <= AUG_BLOCK, "one lane per byte of a staged row");
    const int px = tid / 3;
    const bool stages = px < tw + 2;
    const long col = (long)aug_reflect101(x0 + tx0 - 1 + px, W) * 3 + (tid - 3 * px);
    int bytes[AUG_TH + 2];
#pragma unroll
    for (int r = 0; r < AUG_TH + 2; ++r) {
        bytes[r] = 0;
        if (stages && r < th + 2) bytes[r] = img[(long)aug_reflect101(y0 + ty0 - 1 + r, H) * W * 3 + col];
    }
    __syncthreads();                                                      // (the table)
    if (stages) {
#pragma unroll
        for (int r = 0; r < AUG_TH + 2; ++r) tile[r * AUG_PITCH + tid] = unit[bytes[r]];
    }
    __syncthreads();

    // every lane: AUG_LANE_ROWS pixels of one column, three channels; the taps outermost, so that a dead tap costs one scalar branch
    const int x = min((int)threadIdx.x, tw - 1);                          // (lanes and rows past the tile's part compute, but do not store)
    float acc[AUG_LANE_ROWS][3];
    bool any = false;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const float w = tab.weight[v][t];                                 // uniform over the workgroup
        if (w != 0.0f) {
#pragma unroll
            for (int k = 0; k < AUG_LANE_ROWS; ++k) {
                const int y = min((int)threadIdx.y + k * (AUG_TH / AUG_LANE_ROWS), th - 1);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float p = w * tile[(y + t / 3) * AUG_PITCH + (x + t % 3) * 3 + c];
                    acc[k][c] = any ? acc[k][c] + p : p;
                }
            }
            any = true;
        }
    }
    if ((int)threadIdx.x >= tw) return;
    const long plane = (long)ch * cw;
    float* o = out + (long)v * 3 * plane + (long)ty0 * cw + tx0 + threadIdx.x;
#pragma unroll
    for (int k = 0; k < AUG_LANE_ROWS; ++k) {
        const int y = threadIdx.y + k * (AUG_TH / AUG_LANE_ROWS);         // a wave's 64 lanes share y: one output row per store
        if (y < th) {
#pragma unroll
            for (int c = 0; c < 3; ++c) o[(long)c * plane + (long)y * cw] = any ? acc[k][c] : 0.0f;
        }
    }
}

// The parallel host arrays -> the table of the kernel arguments; -1 with the error set.  weights may be null (the sum launch).
static int aug_table(const char* what, int V, const int* ops, const float* factors, const float* weights, AugTable& tab, bool& contrast) {
    PSCV_CHECK_ARG(V >= 1 && V <= AUG_MAX_VIEWS, "%s: V=%d views, 1 to %d in one call", what, V, AUG_MAX_VIEWS);
    PSCV_CHECK_ARG(ops && factors, "%s: null pointer argument (ops / factors)", what);
    contrast = false;
    for (int v = 0; v < AUG_MAX_VIEWS; ++v) {
        for (int s = 0; s < 2; ++s) {
            const bool live = v < V;
            const int op = live ? ops[2 * v + s] : PSCV_AUG_NONE;
            PSCV_CHECK_ARG(op == PSCV_AUG_NONE || op == PSCV_AUG_BRIGHTNESS || op == PSCV_AUG_CONTRAST,
                           "%s: ops[%d][%d]=%d is no operation", what, v, s, op);
            const float a = op != PSCV_AUG_NONE ? factors[2 * v + s] : 1.0f;
            PSCV_CHECK_ARG(a - a == 0.0f, "%s: factors[%d][%d] is not finite", what, v, s);
            tab.op[v][s] = op;
            tab.factor[v][s] = a;
            tab.inside[v][s] = (a >= 0.0f && a <= 1.0f) ? 1 : 0;
            contrast = contrast || op == PSCV_AUG_CONTRAST;
        }
        PSCV_CHECK_ARG(tab.op[v][0] == PSCV_AUG_NONE || tab.op[v][0] != tab.op[v][1], "%s: ops[%d] lists operation %d twice", what, v,
                       tab.op[v][0]);
        for (int t = 0; t < 9; ++t) {
            const float w = (weights && v < V) ? weights[9 * v + t] : 0.0f;
            PSCV_CHECK_ARG(w - w == 0.0f, "%s: weights[%d][%d] is not finite", what, v, t);
            tab.weight[v][t] = w;
        }
    }
    return 0;
}

static int aug_image(const char* what, const void* imgs, int H, int W) {
    PSCV_CHECK_ARG(imgs, "%s: null pointer argument (imgs)", what);
    PSCV_CHECK_ARG(H >= 1 && W >= 1 && (long)H * W < (1L << 33), "%s: image %d x %d: sizes >= 1, under 2^33 pixels", what, H, W);
    return 0;
}

}  // namespace pscv

extern "C" long pscv_augment_workspace(int V) {
    PSCV_CHECK_ARG(V >= 1 && V <= pscv::AUG_MAX_VIEWS, "pscv_augment_workspace: V=%d views, 1 to %d in one call", V, pscv::AUG_MAX_VIEWS);
    return (long)V * (long)sizeof(unsigned long long);
}

extern "C" int pscv_augment_grey_sums(const unsigned char* imgs, int V, int H, int W, const int* ops, const float* factors,
                                      void* workspace, void* stream) {
    using namespace pscv;
    const char* what = "pscv_augment_grey_sums";
    AugTable tab;
    bool contrast;
    if (aug_table(what, V, ops, factors, nullptr, tab, contrast) || aug_image(what, imgs, H, W)) return -1;
    if (!contrast) return 0;                                               // no view needs a mean: no launch
    PSCV_CHECK_ARG(workspace && ((uintptr_t)workspace & 7) == 0, "%s: workspace must be non-null and 8-byte aligned", what);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const hipError_t e = hipMemsetAsync(workspace, 0, (size_t)V * sizeof(unsigned long long), st);
    if (e != hipSuccess) {
        set_error("%s: clearing the workspace failed: %s", what, hipGetErrorString(e));
        return -2;
    }
    const long n = (long)H * W;
    return launch(what, augment_sum_kernel, dim3((unsigned)((n + AUG_SUM_PIXELS - 1) / AUG_SUM_PIXELS), (unsigned)V), dim3(AUG_SUM_BLOCK), 0,
                  st, imgs, n, tab, static_cast<unsigned long long*>(workspace));
}

extern "C" int pscv_augment_apply(const unsigned char* imgs, int V, int H, int W, const int* ops, const float* factors, const float* weights,
                                  const void* workspace, int x0, int y0, int cw, int ch, const float* lut, float* out, void* stream) {
    using namespace pscv;
    const char* what = "pscv_augment_apply";
    AugTable tab;
    bool contrast;
    PSCV_CHECK_ARG(weights, "%s: null pointer argument (weights)", what);
    if (aug_table(what, V, ops, factors, weights, tab, contrast) || aug_image(what, imgs, H, W)) return -1;
    PSCV_CHECK_ARG(lut && out, "%s: null pointer argument (lut / out)", what);
    PSCV_CHECK_ARG(!contrast || (workspace && ((uintptr_t)workspace & 7) == 0),
                   "%s: a contrast step needs the workspace pscv_augment_grey_sums filled (non-null, 8-byte aligned)", what);
    PSCV_CHECK_ARG(x0 >= 0 && y0 >= 0 && cw >= 1 && ch >= 1 && cw <= W - x0 && ch <= H - y0,
                   "%s: window (%d, %d, %d, %d) outside the %d x %d image", what, x0, y0, cw, ch, W, H);
    const dim3 grid((unsigned)((cw + AUG_TW - 1) / AUG_TW), (unsigned)((ch + AUG_TH - 1) / AUG_TH), (unsigned)V);
    PSCV_CHECK_ARG(grid.y <= (unsigned)AUG_MAX_GRID_Y, "%s: ch=%d: more than %d rows", what, ch, AUG_MAX_GRID_Y * AUG_TH);
    return launch(what, augment_apply_kernel, grid, dim3(AUG_TW, AUG_TH / AUG_LANE_ROWS), 0, reinterpret_cast<hipStream_t>(stream), imgs, H, W,
                  tab, static_cast<const unsigned long long*>(workspace), x0, y0, cw, ch, lut, out);
}
