// Depth maps against something: the loss reductions at the end of a training step (models/trainer.py:114-198 of the reference)
// and the depth-map scores of Trainer.test / depthmap_eval.py (models/utils.py:138-171), gfx950.
//   - pscv_loss_terms:     ONE reduce launch over a table of up to 32 masked-mean terms (blocks are dealt to the terms by a host-made
//                          prefix, csrc/loss_plan.h) + one finishing launch; pscv_loss_terms_bwd: one launch for every gradient.
//   - pscv_depth_metrics:  bilinear upsampling of the estimate, division by the depth step and all sums / counts of the five metric
//                          functions in one pass per image + one finishing launch.
// HBM-bound single passes: four consecutive pixels per lane (one 16-byte load where the tensor allows it), wave64 shuffles, then LDS
// across the four waves.  Two-phase like train_elem.hip: per-block partials in the caller's workspace, combined in a fixed order in
// fp64 -- no float atomics, equal inputs give equal bits.  The term table travels in the kernel arguments; nothing here waits.
#include "pscv_common.h"
#include "loss_plan.h"

namespace pscv {

static_assert(LOSS_MAX_TERMS == PSCV_LOSS_MAX_TERMS, "loss_plan.h and pscv.h disagree");
constexpr int T_MAX = LOSS_MAX_TERMS;
enum : int { F_KIND = 3, F_MASK_U8 = 4, F_VEC = 8, F_GVEC = 16 };

// the kernel argument of all three loss launches (about 3 KiB of the 4 KiB a launch may carry): struct of arrays, indexed by the
// block's term -- a uniform index, so every field is a scalar load
struct LossTable {
    const float* a[T_MAX];          // d (ground-truth kinds) or l
    const float* u[T_MAX];
    const float* gt[T_MAX];
    const void* mask[T_MAX];
    const float* interval[T_MAX];
    float* ga[T_MAX];               // backward only
    float* gu[T_MAX];
    int npix[T_MAX], h[T_MAX], w[T_MAX], H[T_MAX], W[T_MAX], rh[T_MAX], rw[T_MAX];
    int flags[T_MAX];               // kind | F_MASK_U8 | F_VEC (a, u, mask of the L kinds: 16-byte loads) | F_GVEC (16-byte gradient stores)
    float factor[T_MAX];
    int blk_start[T_MAX + 1];
    int n_terms;
};
static_assert(sizeof(LossTable) <= 3600, "the table must fit the kernel-argument segment with the other arguments");

struct Term {       // one term's fields in registers
    const float *a, *u, *gt, *interval;
    const void* mask;
    int npix, h, w, H, W, rh, rw, kind;
    bool mask_u8, vec;
};
__device__ __forceinline__ Term load_term(const LossTable& tab, int t) {
    Term tm;
    tm.a = tab.a[t]; tm.u = tab.u[t]; tm.gt = tab.gt[t]; tm.interval = tab.interval[t]; tm.mask = tab.mask[t];
    tm.npix = tab.npix[t]; tm.h = tab.h[t]; tm.w = tab.w[t]; tm.H = tab.H[t]; tm.W = tab.W[t]; tm.rh = tab.rh[t]; tm.rw = tab.rw[t];
    const int f = tab.flags[t];
    tm.kind = f & F_KIND; tm.mask_u8 = (f & F_MASK_U8) != 0; tm.vec = (f & F_VEC) != 0;
    return tm;
}
__device__ __forceinline__ int term_of_block(const LossTable& tab, int blk) {
    int t = 0;
    while (t + 1 < tab.n_terms && blk >= tab.blk_start[t + 1]) ++t;
    return t;
}

// ground-truth tap validity: a byte mask counts where non-zero, an fp32 mask (0 or 1) where it is 1 (`interpolate(mask) == 1`)
__device__ __forceinline__ bool gt_tap_valid(const Term& tm, long i) {
    return tm.mask_u8 ? reinterpret_cast<const unsigned char*>(tm.mask)[i] != 0 : reinterpret_cast<const float*>(tm.mask)[i] == 1.0f;
}

// bilinear, align_corners=False, integer ratio: the taps of weight 0.5 (even ratio) or the single tap (odd ratio) per axis
__device__ __forceinline__ void gt_down(const Term& tm, int bi, int y, int x, float& g, bool& m) {
    const int ny = (tm.rh & 1) ? 1 : 2, nx = (tm.rw & 1) ? 1 : 2;
    const int y0 = tm.rh * y + ((tm.rh & 1) ? (tm.rh - 1) / 2 : tm.rh / 2 - 1);
    const int x0 = tm.rw * x + ((tm.rw & 1) ? (tm.rw - 1) / 2 : tm.rw / 2 - 1);
    const long i0 = ((long)bi * tm.H + y0) * tm.W + x0;
    m = gt_tap_valid(tm, i0);
    float r0 = tm.gt[i0];
    if (nx == 2) { r0 = 0.5f * r0 + 0.5f * tm.gt[i0 + 1]; m = m && gt_tap_valid(tm, i0 + 1); }
    g = r0;
    if (ny == 2) {
        const long i1 = i0 + tm.W;
        float r1 = tm.gt[i1];
        m = m && gt_tap_valid(tm, i1);
        if (nx == 2) { r1 = 0.5f * r1 + 0.5f * tm.gt[i1 + 1]; m = m && gt_tap_valid(tm, i1 + 1); }
        g = 0.5f * r0 + 0.5f * r1;
    }
}

// four consecutive elements from p0 (a multiple of 4): one 16-byte load where the term allows it, bounds-checked scalars otherwise
__device__ __forceinline__ void load4(const float* p, int p0, int n, bool vec, float (&v)[4]) {
    if (vec) {
        const float4 q = *reinterpret_cast<const float4*>(p + p0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p0 + j < n ? p[p0 + j] : 0.0f;
    }
}
__device__ __forceinline__ void store4(float* p, int p0, int n, bool vec, const float (&v)[4]) {
    if (vec) {
        *reinterpret_cast<float4*>(p + p0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < n) p[p0 + j] = v[j];
    }
}
// the given mask of the L kinds: valid where non-zero
__device__ __forceinline__ void load_mask4(const Term& tm, int p0, bool (&m)[4]) {
    if (tm.mask_u8) {
        const unsigned char* mp = reinterpret_cast<const unsigned char*>(tm.mask);
        if (tm.vec) {
            const uint32_t q = *reinterpret_cast<const uint32_t*>(mp + p0);
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = ((q >> (8 * j)) & 0xffu) != 0;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = p0 + j < tm.npix && mp[p0 + j] != 0;
        }
    } else {
        float v[4];
        load4(reinterpret_cast<const float*>(tm.mask), p0, tm.npix, tm.vec, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = p0 + j < tm.npix && v[j] != 0.0f;
    }
}

// l, m (and, for the backward of the ground-truth kinds, d - gt_down and interval_b) of the four pixels from p0
struct Quad {
    float l[4], diff[4], interval[4];
    bool m[4];
};
__device__ __forceinline__ void eval_quad(const Term& tm, int p0, Quad& q) {
    float a[4];
    load4(tm.a, p0, tm.npix, tm.vec, a);
    if (tm.kind >= PSCV_LOSS_L_PLAIN) {
        load_mask4(tm, p0, q.m);
#pragma unroll
        for (int j = 0; j < 4; ++j) { q.l[j] = a[j]; q.diff[j] = 0.0f; q.interval[j] = 1.0f; }
        return;
    }
    unsigned row = (unsigned)p0 / (unsigned)tm.w;
    unsigned x = (unsigned)p0 - row * (unsigned)tm.w;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        q.m[j] = false; q.l[j] = 0.0f; q.diff[j] = 0.0f; q.interval[j] = 1.0f;
        if (p0 + j < tm.npix) {
            const int bi = (int)(row / (unsigned)tm.h), y = (int)(row - (unsigned)bi * (unsigned)tm.h);
            float g;
            gt_down(tm, bi, y, (int)x, g, q.m[j]);
            q.interval[j] = tm.interval[bi];
            q.diff[j] = a[j] - g;
            q.l[j] = fabsf(q.diff[j]) / q.interval[j];
        }
        if (++x == (unsigned)tm.w) { x = 0; ++row; }
    }
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;                                          // lane 0 holds the sum, always combined in the same order
}

// ---- forward, phase 1: per-block (S_l, S_u, C) of the block's term ------------------------------------------------------------
__global__ __launch_bounds__(LOSS_BLOCK) void loss_reduce_kernel(const LossTable tab, double* __restrict__ partials) {
    __shared__ double red[LOSS_BLOCK / 64][3];
    const int t = term_of_block(tab, blockIdx.x);
    const int first = tab.blk_start[t], nb = tab.blk_start[t + 1] - first;
    const Term tm = load_term(tab, t);
    const bool bayes = tm.kind == PSCV_LOSS_GT_BAYES || tm.kind == PSCV_LOSS_L_BAYES;
    double sl = 0.0, su = 0.0;
    unsigned cnt = 0;
    const long stride = (long)nb * LOSS_CHUNK;
    for (long p = ((long)(blockIdx.x - first) * LOSS_BLOCK + threadIdx.x) * LOSS_PER_THREAD; p < tm.npix; p += stride) {
        const int p0 = (int)p;
        Quad q;
        eval_quad(tm, p0, q);
        float u[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (bayes) load4(tm.u, p0, tm.npix, tm.vec, u);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (q.m[j]) {
                ++cnt;
                sl += (double)q.l[j];
                if (bayes) su += (double)(q.l[j] * expf(-u[j]) + u[j]);
            }
        }
    }
    const double r0 = wave_sum(sl), r1 = wave_sum(su), r2 = wave_sum((double)cnt);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wv][0] = r0; red[wv][1] = r1; red[wv][2] = r2; }
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < LOSS_BLOCK / 64; ++k) s += red[k][threadIdx.x];
        partials[(long)blockIdx.x * 3 + threadIdx.x] = s;
    }
}

// ---- forward, phase 2: one block; wave v finishes terms v, v + 4, ...: a lane adds its (<= 4) partials in block order, the wave
// combines the lanes in shuffle order, lane 0 writes the term; thread 0 then adds factor x term over the terms in table order ----
__global__ __launch_bounds__(LOSS_BLOCK) void loss_finish_kernel(const LossTable tab, const double* __restrict__ partials,
                                                                  float* __restrict__ loss, float* __restrict__ term,
                                                                  double* __restrict__ sums, float* __restrict__ norm) {
    __shared__ double weighted[T_MAX];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int t = wv; t < tab.n_terms; t += LOSS_BLOCK / 64) {
        const int first = tab.blk_start[t], nb = tab.blk_start[t + 1] - first;
        double s[3] = {0.0, 0.0, 0.0};
        for (int b = lane; b < nb; b += 64) {
#pragma unroll
            for (int k = 0; k < 3; ++k) s[k] += partials[(long)(first + b) * 3 + k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] = wave_sum(s[k]);
        if (lane == 0) {
            const int kind = tab.flags[t] & F_KIND;
            const double Sl = s[0], Su = s[1], Cn = s[2];
            double v, n;
            if (kind == PSCV_LOSS_GT_PLAIN) { v = Sl / Cn; n = 1.0 / Cn; }           // unguarded: NaN / inf when the mask is empty
            else {
                const double tot = (kind == PSCV_LOSS_L_PLAIN) ? Sl : Su + Sl;
                n = Cn != 0.0 ? 1.0 / Cn : 1.0;
                v = Cn != 0.0 ? tot / Cn : tot;
            }
            term[t] = (float)v;
            norm[t] = (float)n;
            sums[t * 3 + 0] = Sl; sums[t * 3 + 1] = Su; sums[t * 3 + 2] = Cn;
            weighted[t] = (double)tab.factor[t] * v;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int t = 0; t < tab.n_terms; ++t) s += weighted[t];
        *loss = (float)s;
    }
}

// ---- backward: recompute per pixel, write the gradients asked for ---------------------------------------------------------------
__global__ __launch_bounds__(LOSS_BLOCK) void loss_bwd_kernel(const LossTable tab, const float* __restrict__ norm,
                                                               const float* __restrict__ grad_out) {
    const int t = term_of_block(tab, blockIdx.x);
    const int first = tab.blk_start[t], nb = tab.blk_start[t + 1] - first;
    float* ga = tab.ga[t];
    float* gu = tab.gu[t];
    if (!ga && !gu) return;
    const Term tm = load_term(tab, t);
    const bool gvec = (tab.flags[t] & F_GVEC) != 0;
    const bool bayes = tm.kind == PSCV_LOSS_GT_BAYES || tm.kind == PSCV_LOSS_L_BAYES;
    const bool has_gt = tm.kind <= PSCV_LOSS_GT_BAYES;
    const float coef = grad_out[0] * tab.factor[t] * norm[t];       // +-inf for a GT_PLAIN term with an empty mask: coef * 0 = NaN, as torch
    const long stride = (long)nb * LOSS_CHUNK;
    for (long p = ((long)(blockIdx.x - first) * LOSS_BLOCK + threadIdx.x) * LOSS_PER_THREAD; p < tm.npix; p += stride) {
        const int p0 = (int)p;
        Quad q;
        eval_quad(tm, p0, q);
        float u[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (bayes) load4(tm.u, p0, tm.npix, tm.vec, u);
        float da[4], du[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float e = bayes ? expf(-u[j]) : 0.0f;
            float wa = bayes ? e + 1.0f : 1.0f;
            if (has_gt) {
                const float sg = q.diff[j] > 0.0f ? 1.0f : q.diff[j] < 0.0f ? -1.0f : 0.0f;
                wa *= sg / q.interval[j];
            }
            da[j] = coef * (q.m[j] ? wa : 0.0f);
            du[j] = coef * (q.m[j] ? 1.0f - q.l[j] * e : 0.0f);
        }
        if (ga) store4(ga, p0, tm.npix, gvec, da);
        if (gu) store4(gu, p0, tm.npix, gvec, du);
    }
}

// ---- scores -----------------------------------------------------------------------------------------------------------------------
constexpr int MT = PSCV_METRIC_MAX_THRESH, NS = PSCV_METRIC_SUMS;
static_assert(NS == 4 + 2 * MT, "C, three sums and two count groups");
struct MetricArgs {
    const float *est, *gt, *step;
    const void* mask;
    int h, w, H, W, mask_u8, vec, n_abs, n_rel;
    float scale_h, scale_w;                    // (float)in / out, torch's area_pixel_compute_scale
    float thr_abs[MT], thr_rel[MT];
};

// torch's upsample_bilinear2d index rule (align_corners=False) in fp32
__device__ __forceinline__ void src_index(float scale, int dst, int in, int& i0, int& i1, float& l0, float& l1) {
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.0f ? 0.0f : s;
    i0 = min((int)s, in - 1);
    i1 = i0 + (i0 < in - 1 ? 1 : 0);
    l1 = s - (float)i0;
    l0 = 1.0f - l1;
}
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || b != b) ? a + b : fmaxf(a, b); }   // torch.max propagates NaN

__global__ __launch_bounds__(LOSS_BLOCK) void metrics_reduce_kernel(const MetricArgs ar, double* __restrict__ partials) {
    __shared__ double red[LOSS_BLOCK / 64][NS];
    const int bi = blockIdx.y, hw = ar.H * ar.W;
    const float* gt = ar.gt + (long)bi * hw;
    const float* est = ar.est + (long)bi * ar.h * ar.w;
    const float st = ar.step ? ar.step[bi] : 1.0f;
    double s_abs = 0.0, s_rel = 0.0, s_sq = 0.0;
    unsigned cnt = 0, c_abs[MT] = {0, 0, 0, 0}, c_rel[MT] = {0, 0, 0, 0};
    const long stride = (long)gridDim.x * LOSS_CHUNK;
    for (long p = ((long)blockIdx.x * LOSS_BLOCK + threadIdx.x) * LOSS_PER_THREAD; p < hw; p += stride) {
        const int p0 = (int)p;
        float g4[4];
        bool m4[4];
        load4(gt, p0, hw, ar.vec != 0, g4);
        if (ar.mask_u8) {
            const unsigned char* mp = reinterpret_cast<const unsigned char*>(ar.mask) + (long)bi * hw;
#pragma unroll
            for (int j = 0; j < 4; ++j) m4[j] = p0 + j < hw && mp[p0 + j] != 0;
        } else {
            float mv[4];
            load4(reinterpret_cast<const float*>(ar.mask) + (long)bi * hw, p0, hw, ar.vec != 0, mv);
#pragma unroll
            for (int j = 0; j < 4; ++j) m4[j] = p0 + j < hw && mv[j] > 0.5f;
        }
        int Y = p0 / ar.W, X = p0 - Y * ar.W;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (m4[j]) {
                int y0, y1, x0, x1;
                float ly0, ly1, lx0, lx1;
                src_index(ar.scale_h, Y, ar.h, y0, y1, ly0, ly1);
                src_index(ar.scale_w, X, ar.w, x0, x1, lx0, lx1);
                const float* r0 = est + (long)y0 * ar.w;
                const float* r1 = est + (long)y1 * ar.w;
                const float up = ly0 * (lx0 * r0[x0] + lx1 * r0[x1]) + ly1 * (lx0 * r1[x0] + lx1 * r1[x1]);
                const float e = up / st, g = g4[j] / st;
                const float ad = fabsf(e - g);
                ++cnt;
                s_abs += (double)ad;
                s_rel += (double)(ad / g);
                s_sq += (double)((e - g) * (e - g) / g);
                const float ratio = nan_max(e / g, g / e);
#pragma unroll
                for (int k = 0; k < MT; ++k) {
                    if (k < ar.n_abs && ad > ar.thr_abs[k]) ++c_abs[k];
                    if (k < ar.n_rel && ratio > ar.thr_rel[k]) ++c_rel[k];
                }
            }
            if (++X == ar.W) { X = 0; ++Y; }
        }
    }
    double v[NS];
    v[0] = (double)cnt; v[1] = s_abs; v[2 + MT] = s_rel; v[3 + MT] = s_sq;
#pragma unroll
    for (int k = 0; k < MT; ++k) { v[2 + k] = (double)c_abs[k]; v[4 + MT + k] = (double)c_rel[k]; }
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const double r = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0) red[wv][k] = r;
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < LOSS_BLOCK / 64; ++k) s += red[k][threadIdx.x];
        partials[((long)bi * gridDim.x + blockIdx.x) * NS + threadIdx.x] = s;
    }
}

// one block: wave v finishes images v, v + 4, ...; then threads 0 .. NS - 2 average the per-image means over the batch in image order
__global__ __launch_bounds__(LOSS_BLOCK) void metrics_finish_kernel(const double* __restrict__ partials, int nb, int b, int n_abs, int n_rel,
                                                                     double* __restrict__ sums, float* __restrict__ means) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int bi = wv; bi < b; bi += LOSS_BLOCK / 64) {
        double s[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] = 0.0;
        for (int blk = lane; blk < nb; blk += 64) {
#pragma unroll
            for (int k = 0; k < NS; ++k) s[k] += partials[((long)bi * nb + blk) * NS + k];
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] = wave_sum(s[k]);
        if (lane == 0) {
            float* mo = means + (long)bi * (NS - 1);
            const double Cn = s[0];                    // 0 / 0 = NaN for an empty mask, as the mean of nothing
#pragma unroll
            for (int k = 0; k < NS; ++k) sums[(long)bi * NS + k] = s[k];
            mo[0] = (float)(s[1] / Cn);
#pragma unroll
            for (int k = 0; k < MT; ++k) {
                mo[1 + k] = k < n_abs ? (float)(s[2 + k] / Cn) : 0.0f;
                mo[3 + MT + k] = k < n_rel ? (float)(1.0 - s[4 + MT + k] / Cn) : 0.0f;
            }
            mo[1 + MT] = (float)(s[2 + MT] / Cn);
            mo[2 + MT] = (float)(s[3 + MT] / Cn);
        }
    }
    __syncthreads();
    if (threadIdx.x < NS - 1) {
        double s = 0.0;
        for (int bi = 0; bi < b; ++bi) s += (double)means[(long)bi * (NS - 1) + threadIdx.x];
        means[(long)b * (NS - 1) + threadIdx.x] = (float)(s / (double)b);
    }
}

static bool aligned(const void* p, size_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

// checks + table for the three loss launches; 0, or -1 with the error set
static int build_table(const char* fn, int n_terms, const int* kinds, const void* const* a, const void* const* u, const void* const* gt,
                       const void* const* mask, const void* const* interval, const int* mask_u8, const long* dims, const float* factors,
                       const void* const* grad_a, const void* const* grad_u, LossTable& tab) {
    PSCV_CHECK_ARG(n_terms <= LOSS_MAX_TERMS, "%s: %d terms, at most %d in one call", fn, n_terms, LOSS_MAX_TERMS);
    PSCV_CHECK_ARG(kinds && a && u && gt && mask && interval && mask_u8 && dims && factors, "%s: null pointer argument (a table array)", fn);
    LossPlan plan;
    if (!loss_plan(n_terms, kinds, dims, plan)) {
        set_error("%s: term %d: %s", fn, plan.error_term, plan.error);
        return -1;
    }
    tab = LossTable{};
    tab.n_terms = n_terms;
    for (int t = 0; t < n_terms; ++t) {
        const int kind = kinds[t];
        const bool has_gt = loss_kind_has_gt(kind), has_u = loss_kind_has_u(kind), u8 = mask_u8[t] != 0;
        PSCV_CHECK_ARG(a[t] && mask[t], "%s: term %d: null pointer argument (a / mask)", fn, t);
        PSCV_CHECK_ARG(!has_u || u[t], "%s: term %d: null pointer argument (u of a Bayes kind)", fn, t);
        PSCV_CHECK_ARG(!has_gt || (gt[t] && interval[t]), "%s: term %d: null pointer argument (gt / interval of a ground-truth kind)", fn, t);
        const long* d = dims + 5L * t;
        tab.a[t] = (const float*)a[t]; tab.u[t] = has_u ? (const float*)u[t] : nullptr;
        tab.gt[t] = has_gt ? (const float*)gt[t] : nullptr; tab.interval[t] = has_gt ? (const float*)interval[t] : nullptr;
        tab.mask[t] = mask[t];
        tab.ga[t] = grad_a ? (float*)grad_a[t] : nullptr;
        tab.gu[t] = (grad_u && has_u) ? (float*)grad_u[t] : nullptr;
        tab.npix[t] = (int)plan.npix[t];
        tab.h[t] = (int)d[1]; tab.w[t] = (int)d[2];
        tab.H[t] = has_gt ? (int)d[3] : 1; tab.W[t] = has_gt ? (int)d[4] : 1;
        tab.rh[t] = plan.rh[t]; tab.rw[t] = plan.rw[t];
        const bool n4 = plan.npix[t] % 4 == 0;
        bool vec = n4 && aligned(a[t], 16) && (!has_u || aligned(u[t], 16));
        if (!has_gt) vec = vec && aligned(mask[t], u8 ? 4 : 16);
        const bool gvec = n4 && (!tab.ga[t] || aligned(tab.ga[t], 16)) && (!tab.gu[t] || aligned(tab.gu[t], 16));
        tab.flags[t] = kind | (u8 ? F_MASK_U8 : 0) | (vec ? F_VEC : 0) | (gvec ? F_GVEC : 0);
        tab.factor[t] = factors[t];
        tab.blk_start[t + 1] = plan.blk_start[t + 1];
    }
    return 0;
}

static long metric_blocks(long hw) {
    long nb = (hw + LOSS_CHUNK - 1) / LOSS_CHUNK;
    return nb > LOSS_MAX_BLOCKS_PER_TERM ? LOSS_MAX_BLOCKS_PER_TERM : nb;
}

}  // namespace pscv

using namespace pscv;

extern "C" long pscv_loss_terms_workspace(int n_terms, const long* dims) {
    PSCV_CHECK_ARG(dims, "pscv_loss_terms_workspace: null pointer argument (dims)");
    PSCV_CHECK_ARG(n_terms >= 1 && n_terms <= LOSS_MAX_TERMS, "pscv_loss_terms_workspace: %d terms, 1 to %d in one call", n_terms, LOSS_MAX_TERMS);
    int kinds[LOSS_MAX_TERMS];
    for (int t = 0; t < n_terms; ++t) kinds[t] = PSCV_LOSS_L_PLAIN;          // the block count depends on b h w only
    LossPlan plan;
    if (!loss_plan(n_terms, kinds, dims, plan)) {
        set_error("pscv_loss_terms_workspace: term %d: %s", plan.error_term, plan.error);
        return -1;
    }
    return (long)plan.blk_start[n_terms] * 3 * (long)sizeof(double);
}

extern "C" int pscv_loss_terms(int n_terms, const int* kinds, const void* const* a, const void* const* u, const void* const* gt,
                               const void* const* mask, const void* const* interval, const int* mask_u8, const long* dims,
                               const float* factors, void* workspace, float* loss, float* term, double* sums, float* norm, void* stream) {
    PSCV_CHECK_ARG(workspace && loss && term && sums && norm, "pscv_loss_terms: null pointer argument (workspace / loss / term / sums / norm)");
    PSCV_CHECK_ARG(aligned(workspace, 8) && aligned(sums, 8), "pscv_loss_terms: workspace and sums must be 8-byte aligned");
    LossTable tab;
    if (build_table("pscv_loss_terms", n_terms, kinds, a, u, gt, mask, interval, mask_u8, dims, factors, nullptr, nullptr, tab)) return -1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    double* partials = reinterpret_cast<double*>(workspace);
    int rc = launch("pscv_loss_terms(reduce)", loss_reduce_kernel, dim3(tab.blk_start[n_terms]), dim3(LOSS_BLOCK), 0, st, tab, partials);
    if (rc) return rc;
    return launch("pscv_loss_terms(finish)", loss_finish_kernel, dim3(1), dim3(LOSS_BLOCK), 0, st, tab, (const double*)partials, loss, term, sums, norm);
}

extern "C" int pscv_loss_terms_bwd(int n_terms, const int* kinds, const void* const* a, const void* const* u, const void* const* gt,
                                   const void* const* mask, const void* const* interval, const int* mask_u8, const long* dims,
                                   const float* factors, const float* norm, const float* grad_out, const void* const* grad_a,
                                   const void* const* grad_u, void* stream) {
    PSCV_CHECK_ARG(norm && grad_out, "pscv_loss_terms_bwd: null pointer argument (norm / grad_out)");
    PSCV_CHECK_ARG(grad_a || grad_u, "pscv_loss_terms_bwd: null pointer argument (no gradient asked for)");
    LossTable tab;
    if (build_table("pscv_loss_terms_bwd", n_terms, kinds, a, u, gt, mask, interval, mask_u8, dims, factors, grad_a, grad_u, tab)) return -1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return launch("pscv_loss_terms_bwd", loss_bwd_kernel, dim3(tab.blk_start[n_terms]), dim3(LOSS_BLOCK), 0, st, tab, norm, grad_out);
}

static int metric_sizes(const char* fn, int b, int H, int W) {
    PSCV_CHECK_ARG(b > 0 && H > 0 && W > 0, "%s: zero or negative size (b=%d H=%d W=%d)", fn, b, H, W);
    PSCV_CHECK_ARG((long)H * W <= 0x7fffffffL && b <= 65535, "%s: more than 2^31 - 1 pixels per image or more than 65535 images", fn);
    return 0;
}

extern "C" long pscv_depth_metrics_workspace(int b, int H, int W) {
    if (metric_sizes("pscv_depth_metrics_workspace", b, H, W)) return -1;
    return (long)b * metric_blocks((long)H * W) * NS * (long)sizeof(double);
}

extern "C" int pscv_depth_metrics(const float* est, const float* gt, const void* mask, int mask_u8, const float* step, int b, int h, int w,
                                  int H, int W, const float* thr_abs, int n_abs, const float* thr_rel, int n_rel, void* workspace,
                                  double* sums, float* means, void* stream) {
    PSCV_CHECK_ARG(est && gt && mask && workspace && sums && means, "pscv_depth_metrics: null pointer argument");
    if (metric_sizes("pscv_depth_metrics", b, H, W)) return -1;
    PSCV_CHECK_ARG(h > 0 && w > 0 && (long)h * w <= 0x7fffffffL, "pscv_depth_metrics: zero or negative size (h=%d w=%d)", h, w);
    PSCV_CHECK_ARG(n_abs >= 0 && n_abs <= MT && n_rel >= 0 && n_rel <= MT, "pscv_depth_metrics: %d and %d thresholds, at most %d of each", n_abs, n_rel, MT);
    PSCV_CHECK_ARG((n_abs == 0 || thr_abs) && (n_rel == 0 || thr_rel), "pscv_depth_metrics: null pointer argument (thresholds)");
    PSCV_CHECK_ARG(aligned(workspace, 8) && aligned(sums, 8), "pscv_depth_metrics: workspace and sums must be 8-byte aligned");
    MetricArgs ar{};
    ar.est = est; ar.gt = gt; ar.step = step; ar.mask = mask;
    ar.h = h; ar.w = w; ar.H = H; ar.W = W; ar.mask_u8 = mask_u8 ? 1 : 0;
    const long hw = (long)H * W;
    ar.vec = (hw % 4 == 0 && aligned(gt, 16) && (mask_u8 || aligned(mask, 16))) ? 1 : 0;
    ar.n_abs = n_abs; ar.n_rel = n_rel;
    ar.scale_h = (float)h / (float)H; ar.scale_w = (float)w / (float)W;
    for (int k = 0; k < n_abs; ++k) ar.thr_abs[k] = thr_abs[k];
    for (int k = 0; k < n_rel; ++k) ar.thr_rel[k] = thr_rel[k];
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nb = (int)metric_blocks(hw);
    double* partials = reinterpret_cast<double*>(workspace);
    int rc = launch("pscv_depth_metrics(reduce)", metrics_reduce_kernel, dim3(nb, b), dim3(LOSS_BLOCK), 0, st, ar, partials);
    if (rc) return rc;
    return launch("pscv_depth_metrics(finish)", metrics_finish_kernel, dim3(1), dim3(LOSS_BLOCK), 0, st, (const double*)partials, nb, b, n_abs, n_rel, sums, means);
}
