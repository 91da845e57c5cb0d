// PatchMatch multi-view stereo (the COLMAP baseline of the reconstruction pipeline: `colmap patch_match_stereo`).  gfx950.
//
// INTEGRATION.md section 2h states the rule; tests/_patch_match_ref.py restates it in numpy.  Per reference pixel the state is a
// plane hypothesis (depth d, unit normal n in the reference camera frame, facing the camera) stored as float4 (d, nx, ny, nz).
// One kernel template serves four entry points:
//   COST    every pixel: the per-source photometric costs c_s (and forward-backward errors e_s) of the given hypotheses;
//   HALF    one red-black half-step: the pixels of one colour evaluate 11 candidates (current, 8 propagated planes, a perturbation,
//           a random plane) and keep the lowest aggregated cost; they read only pixels of the other colour, so the update is in
//           place and independent of scheduling;
//   FILTER  every pixel: COLMAP's filter on the final hypotheses (>= 2 sources with c_s <= 0.9, angle >= 3 deg, e_s <= 1 px).
// plus a small initialisation kernel (candidate 10 for every pixel).
//
// Mapping: a 256-thread workgroup covers 16 rows; in HALF mode 32 columns of which each thread owns the pixel of the half-step's
// colour, otherwise 16 columns with one pixel per thread.  The reference tile plus a halo of the window radius is staged in LDS
// once (clamped to the image edge), and so are the per-source geometry blocks.  The bilateral weights depend on the pixel and the
// offset only: they are recomputed per tap (one exp) and shared by a group of PM_SG sources, whose homographies, running sums and
// centre samples stay in registers.  The window sums are fp64 (the taps are fp32): windows near the variance threshold cancel.  Source samples are bilinear gathers from the fp32 grey images through the caches.
//
// Randomness is a counter hash (lowbias32 chained over seed, view, pixel, iteration, colour, slot), reproduced bit for bit in numpy.
#include "geo_common.h"

namespace pscv {

constexpr int PM_THREADS = 256;
constexpr int PM_ROWS = 16;
constexpr int PM_SG = 4;                       // sources per register group
constexpr int PM_GEO = 28;                     // floats per source geometry block (27 used)
constexpr int PM_TILE_W = 32 + 2 * PSCV_PM_MAX_RADIUS;
constexpr int PM_TILE_H = PM_ROWS + 2 * PSCV_PM_MAX_RADIUS;
constexpr int PM_NCAND = 11;
enum { PM_COST = 0, PM_HALF = 1, PM_FILTER = 2 };

constexpr float PM_SIGMA_COLOR = 0.2f;
constexpr float PM_MIN_VAR = 1e-5f;
constexpr float PM_COS_MIN_TRI = 0.99984769515639123916f;       // cos 1 deg
constexpr float PM_COS_FILTER_TRI = 0.99862953475457387378f;    // cos 3 deg
constexpr float PM_GEOM_LAMBDA = 0.3f;
constexpr float PM_GEOM_EMAX = 3.0f;
constexpr float PM_FILTER_MAX_COST = 0.9f;
constexpr float PM_FILTER_MAX_ERR = 1.0f;
constexpr int PM_FILTER_MIN_CONSISTENT = 2;
constexpr uint32_t PM_INIT_ITERATION = 0xffffffffu;
enum { SLOT_PHI, SLOT_ALPHA, SLOT_DEPTH, SLOT_RDEPTH, SLOT_RZ, SLOT_RAZ };

struct PmArgs {
    float4* state;                                   // [h][w] (d, nx, ny, nz)
    const float* ref;                                // [h][w] grey
    const float* src[PSCV_PM_MAX_SRC];               // [sh][sw] grey
    const float* sdepth[PSCV_PM_MAX_SRC];            // [sh][sw] photometric depth (geometric mode / filter), else null
    int sh[PSCV_PM_MAX_SRC], sw[PSCV_PM_MAX_SRC];
    const float* cams;                               // [n_src + 1][PSCV_GEO_CAM_FLOATS], row 0 = reference
    int h, w, n_src, radius, step, top_k, colour, geom;
    float dmin, dmax, delta, theta;
    uint32_t seed, view, iteration;
    int* out_choice;                                 // HALF: [h][w] chosen candidate (pixels of the colour), may be null
    float4* out_cand;                                // HALF: [h][w][11] candidates (0 = skipped), may be null
    float* out_cost;                                 // COST: [n_src][h][w] photometric c_s
    float* out_err;                                  // COST: [n_src][h][w] e_s (geometric), may be null
    float* out_agg;                                  // COST: [h][w] aggregated cost, may be null
    float* out_depth;                                // FILTER: [h][w]
    float* out_normal;                               // FILTER: [h][w][3]
    int* out_count;                                  // FILTER: [h][w] passing sources, may be null
};

__device__ __forceinline__ uint32_t pm_mix(uint32_t x) {      // lowbias32
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ float pm_uniform(uint32_t seed, uint32_t view, uint32_t pixel, uint32_t iteration, uint32_t colour,
                                            uint32_t slot) {
    uint32_t h = pm_mix(seed ^ 0x9e3779b9u);
    h = pm_mix(h ^ view);
    h = pm_mix(h ^ pixel);
    h = pm_mix(h ^ iteration);
    h = pm_mix(h ^ colour);
    h = pm_mix(h ^ slot);
    return (float)(h >> 8) * 5.9604644775390625e-8f;          // 2^-24
}

__device__ __forceinline__ void mat3mul(const float* a, const float* b, float* o) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

// per source s: A = K_s R_rel K_r^-1 (0-8), b = K_s t_rel (9-11), C = -R_rel^T t_rel (12-14), G = K_r R_rel^T K_s^-1 (15-23),
// c = K_r C (24-26); R_rel = R_s R_r^T, t_rel = t_s - R_rel t_r
__device__ void pm_source_block(const float* cams, int s, float* o) {
    const float* r = cams;
    const float* c = cams + (s + 1) * PSCV_GEO_CAM_FLOATS;
    const float *rR = r + CAM_R, *rt = r + CAM_T, *cR = c + CAM_R, *ct = c + CAM_T;
    float Rr[9], RrT[9], tmp[9], RrtT[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            Rr[3 * i + j] = cR[3 * i] * rR[3 * j] + cR[3 * i + 1] * rR[3 * j + 1] + cR[3 * i + 2] * rR[3 * j + 2];
    float tr[3], C[3];
    for (int i = 0; i < 3; ++i) tr[i] = ct[i] - (Rr[3 * i] * rt[0] + Rr[3 * i + 1] * rt[1] + Rr[3 * i + 2] * rt[2]);
    for (int i = 0; i < 3; ++i) C[i] = -(Rr[i] * tr[0] + Rr[3 + i] * tr[1] + Rr[6 + i] * tr[2]);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) RrT[3 * i + j] = Rr[3 * j + i];
    const float *rK = r + CAM_K, *cK = c + CAM_K;
    mat3mul(cK, Rr, tmp);                     // K_s R_rel
    mat3mul(tmp, r + CAM_KINV, o + 0);        // .. K_r^-1
    for (int i = 0; i < 3; ++i) o[9 + i] = cK[3 * i] * tr[0] + cK[3 * i + 1] * tr[1] + cK[3 * i + 2] * tr[2];
    for (int i = 0; i < 3; ++i) o[12 + i] = C[i];
    mat3mul(rK, RrT, RrtT);                   // K_r R_rel^T
    mat3mul(RrtT, c + CAM_KINV, o + 15);      // .. K_s^-1
    for (int i = 0; i < 3; ++i) o[24 + i] = rK[3 * i] * C[0] + rK[3 * i + 1] * C[1] + rK[3 * i + 2] * C[2];
    o[27] = 0.0f;
}

__device__ __forceinline__ float pm_bilinear(const float* __restrict__ img, int h, int w, float u, float v) {
    u = fminf(fmaxf(u, 0.0f), (float)(w - 1));
    v = fminf(fmaxf(v, 0.0f), (float)(h - 1));
    const int x0 = (int)u, y0 = (int)v;
    const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    const float fx = u - (float)x0, fy = v - (float)y0;
    const float* r0 = img + (long)y0 * w;
    const float* r1 = img + (long)y1 * w;
    const float top = (1.0f - fx) * r0[x0] + fx * r0[x1];
    const float bot = (1.0f - fx) * r1[x0] + fx * r1[x1];
    return (1.0f - fy) * top + fy * bot;
}

// forward-backward error of X0 = d K_r^-1 p against source s's depth map (capped at e_max)
__device__ __forceinline__ float pm_geom_error(const PmArgs& a, const float* g, int s, float d, float col, float row) {
    const float y0 = d * (g[0] * col + g[1] * row + g[2]) + g[9];
    const float y1 = d * (g[3] * col + g[4] * row + g[5]) + g[10];
    const float y2 = d * (g[6] * col + g[7] * row + g[8]) + g[11];
    if (!(y2 > 0.0f)) return PM_GEOM_EMAX;
    const float u = y0 / y2, v = y1 / y2;
    if (!(fabsf(u) < 1073741824.0f && fabsf(v) < 1073741824.0f)) return PM_GEOM_EMAX;
    const int qx = (int)roundf(u), qy = (int)roundf(v);           // half away from zero
    if (qx < 0 || qx >= a.sw[s] || qy < 0 || qy >= a.sh[s]) return PM_GEOM_EMAX;
    const float ds = a.sdepth[s][(long)qy * a.sw[s] + qx];
    if (!(ds > 0.0f)) return PM_GEOM_EMAX;
    const float fx = (float)qx, fy = (float)qy;
    const float r0 = ds * (g[15] * fx + g[16] * fy + g[17]) + g[24];
    const float r1 = ds * (g[18] * fx + g[19] * fy + g[20]) + g[25];
    const float r2 = ds * (g[21] * fx + g[22] * fy + g[23]) + g[26];
    if (!(r2 > 0.0f)) return PM_GEOM_EMAX;
    const float ex = r0 / r2 - col, ey = r1 / r2 - row;
    return fminf(sqrtf(ex * ex + ey * ey), PM_GEOM_EMAX);
}

struct PmPixel {
    int row, col;
    float m[3];                  // K_r^-1 p
    double mr, vr, inv_w;        // reference window: weighted mean and variance of r' = I(p+o) - I(p), 1 / sum of weights
    float centre;                // I_r(p)
};

// aggregated cost of hypothesis (d, n) at the pixel; MODE COST / FILTER also write per-source values
template <int MODE>
__device__ float pm_eval(const PmArgs& a, const PmPixel& px, const float* __restrict__ tile, const float* __restrict__ geo,
                         const float* __restrict__ kinv, int tr0, int tc0, float d, float nx, float ny, float nz, long pix,
                         int* passed) {
    const float col = (float)px.col, row = (float)px.row;
    const float rho = d * (nx * px.m[0] + ny * px.m[1] + nz * px.m[2]);
    const float ir = 1.0f / rho;
    const float g0 = (kinv[0] * nx + kinv[3] * ny + kinv[6] * nz) * ir;
    const float g1 = (kinv[1] * nx + kinv[4] * ny + kinv[7] * nz) * ir;
    const float g2 = (kinv[2] * nx + kinv[5] * ny + kinv[8] * nz) * ir;
    const float X0 = d * px.m[0], X1 = d * px.m[1], X2 = d * px.m[2];
    const float nX0 = sqrtf(X0 * X0 + X1 * X1 + X2 * X2);
    const int R = a.radius, st = a.step, kr = R / st;
    const float inv2ss = 1.0f / (2.0f * (float)R * (float)R);
    constexpr float inv2sc = 1.0f / (2.0f * PM_SIGMA_COLOR * PM_SIGMA_COLOR);
    float tk[PSCV_PM_MAX_TOPK];
#pragma unroll
    for (int i = 0; i < PSCV_PM_MAX_TOPK; ++i) tk[i] = 3.0e38f;
    int npass = 0;
    for (int s0 = 0; s0 < a.n_src; s0 += PM_SG) {
        float H[PM_SG][9], sc[PM_SG], cosa[PM_SG];
        double S1[PM_SG], S2[PM_SG], S3[PM_SG];       // fp64 sums: low-variance windows cancel in the variances
        bool ok[PM_SG];
        const float* sp[PM_SG];
        int shh[PM_SG], sww[PM_SG];
#pragma unroll
        for (int j = 0; j < PM_SG; ++j) {
            const int s = s0 + j;
            ok[j] = false;
            S1[j] = S2[j] = S3[j] = 0.0;
            sc[j] = 0.0f;
            cosa[j] = 1.0f;
            const int sj = s < a.n_src ? s : 0;
            sp[j] = a.src[sj];
            shh[j] = a.sh[sj];
            sww[j] = a.sw[sj];
            const float* g = geo + sj * PM_GEO;
            const float b0 = g[9], b1 = g[10], b2 = g[11];
            H[j][0] = g[0] + b0 * g0; H[j][1] = g[1] + b0 * g1; H[j][2] = g[2] + b0 * g2;
            H[j][3] = g[3] + b1 * g0; H[j][4] = g[4] + b1 * g1; H[j][5] = g[5] + b1 * g2;
            H[j][6] = g[6] + b2 * g0; H[j][7] = g[7] + b2 * g1; H[j][8] = g[8] + b2 * g2;
            if (s >= a.n_src) continue;
            const float x0 = H[j][0] * col + H[j][1] * row + H[j][2];
            const float x1 = H[j][3] * col + H[j][4] * row + H[j][5];
            const float x2 = H[j][6] * col + H[j][7] * row + H[j][8];
            const float u = x2 > 0.0f ? x0 / x2 : 0.0f, v = x2 > 0.0f ? x1 / x2 : 0.0f;
            const bool centre_ok = x2 > 0.0f && u >= 0.0f && u <= (float)(sww[j] - 1) && v >= 0.0f && v <= (float)(shh[j] - 1);
            const float r0 = X0 - g[12], r1 = X1 - g[13], r2 = X2 - g[14];
            cosa[j] = (X0 * r0 + X1 * r1 + X2 * r2) / (nX0 * sqrtf(r0 * r0 + r1 * r1 + r2 * r2));
            ok[j] = centre_ok && px.vr >= (double)PM_MIN_VAR && cosa[j] <= PM_COS_MIN_TRI;
            if (ok[j]) sc[j] = pm_bilinear(sp[j], shh[j], sww[j], u, v);
        }
        if (ok[0] || ok[1] || ok[2] || ok[3]) {
            for (int ky = -kr; ky <= kr; ++ky) {
                const int oy = ky * st;
                const float* trow = tile + (px.row + oy - tr0) * PM_TILE_W + (px.col - tc0);
                const float qy = row + (float)oy;
                for (int kx = -kr; kx <= kr; ++kx) {
                    const int ox = kx * st;
                    const float rp = trow[ox] - px.centre;
                    const float wgt = __expf(-(float)(oy * oy + ox * ox) * inv2ss - rp * rp * inv2sc);
                    const double wd = (double)wgt, wr = (double)(wgt * rp);
                    const float qx = col + (float)ox;
#pragma unroll
                    for (int j = 0; j < PM_SG; ++j) {
                        if (!ok[j]) continue;
                        const float x0 = H[j][0] * qx + H[j][1] * qy + H[j][2];
                        const float x1 = H[j][3] * qx + H[j][4] * qy + H[j][5];
                        const float x2 = H[j][6] * qx + H[j][7] * qy + H[j][8];
                        float u = 0.0f, v = 0.0f;
                        if (x2 > 0.0f) {
                            const float iz = 1.0f / x2;
                            u = x0 * iz;
                            v = x1 * iz;
                        }
                        const double val = (double)(pm_bilinear(sp[j], shh[j], sww[j], u, v) - sc[j]);
                        const double wv = wd * val;
                        S1[j] += wv;
                        S2[j] += wv * val;
                        S3[j] += wr * val;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < PM_SG; ++j) {
            const int s = s0 + j;
            if (s >= a.n_src) continue;
            float c = 2.0f;
            if (ok[j]) {
                const double ms = S1[j] * px.inv_w;
                const double vs = S2[j] * px.inv_w - ms * ms;
                const double cov = S3[j] * px.inv_w - px.mr * ms;
                if (vs >= (double)PM_MIN_VAR) c = fminf(fmaxf(1.0f - (float)(cov / sqrt(px.vr * vs)), 0.0f), 2.0f);
            }
            float e = 0.0f;
            if (a.geom) e = pm_geom_error(a, geo + s * PM_GEO, s, d, col, row);
            if (MODE == PM_COST) {
                a.out_cost[(long)s * a.h * a.w + pix] = c;
                if (a.geom && a.out_err) a.out_err[(long)s * a.h * a.w + pix] = e;
            }
            if (MODE == PM_FILTER) npass += (c <= PM_FILTER_MAX_COST && cosa[j] <= PM_COS_FILTER_TRI && e <= PM_FILTER_MAX_ERR) ? 1 : 0;
            float cc = a.geom ? c + PM_GEOM_LAMBDA * fminf(e, PM_GEOM_EMAX) : c;
#pragma unroll
            for (int i = 0; i < PSCV_PM_MAX_TOPK; ++i) {
                if (cc < tk[i]) {
                    const float t = tk[i];
                    tk[i] = cc;
                    cc = t;
                }
            }
        }
    }
    if (passed) *passed = npass;
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < PSCV_PM_MAX_TOPK; ++i)
        if (i < a.top_k) sum += tk[i];
    return sum / (float)a.top_k;
}

// candidate 10: inverse depth uniform in the range, normal uniform on the sphere flipped to face the camera
__device__ __forceinline__ float4 pm_random(const PmArgs& a, const float* m, uint32_t pixel, uint32_t iteration, uint32_t colour) {
    const float ud = pm_uniform(a.seed, a.view, pixel, iteration, colour, SLOT_RDEPTH);
    const float uz = pm_uniform(a.seed, a.view, pixel, iteration, colour, SLOT_RZ);
    const float ua = pm_uniform(a.seed, a.view, pixel, iteration, colour, SLOT_RAZ);
    const float lo = 1.0f / a.dmax, hi = 1.0f / a.dmin;
    const float d = 1.0f / (lo + ud * (hi - lo));
    const float z = 1.0f - 2.0f * uz;
    const float r = sqrtf(fmaxf(0.0f, 1.0f - z * z));
    const float al = 6.283185307179586f * ua;
    float nx = r * __cosf(al), ny = r * __sinf(al), nz = z;
    if (nx * m[0] + ny * m[1] + nz * m[2] > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
    return make_float4(d, nx, ny, nz);
}

// candidate 9: rotate n by phi = theta u about a tangent axis at angle 2 pi u', move the inverse depth by (2u'' - 1) delta range
__device__ __forceinline__ float4 pm_perturb(const PmArgs& a, const float* m, float4 cur, uint32_t pixel) {
    const float up = pm_uniform(a.seed, a.view, pixel, a.iteration, (uint32_t)a.colour, SLOT_PHI);
    const float ua = pm_uniform(a.seed, a.view, pixel, a.iteration, (uint32_t)a.colour, SLOT_ALPHA);
    const float ud = pm_uniform(a.seed, a.view, pixel, a.iteration, (uint32_t)a.colour, SLOT_DEPTH);
    const float nx = cur.y, ny = cur.z, nz = cur.w;
    const bool ax = fabsf(nx) < 0.9f;              // a = x axis, else y axis; e1 = n x a
    float e1x = ax ? 0.0f : -nz, e1y = ax ? nz : 0.0f, e1z = ax ? -ny : nx;
    const float il = 1.0f / sqrtf(e1x * e1x + e1y * e1y + e1z * e1z);
    e1x *= il; e1y *= il; e1z *= il;
    const float e2x = ny * e1z - nz * e1y, e2y = nz * e1x - nx * e1z, e2z = nx * e1y - ny * e1x;
    const float phi = a.theta * up, al = 6.283185307179586f * ua;
    const float ca = __cosf(al), sa = __sinf(al), cp = __cosf(phi), sp = __sinf(phi);
    float px = cp * nx + sp * (ca * e1x + sa * e2x);
    float py = cp * ny + sp * (ca * e1y + sa * e2y);
    float pz = cp * nz + sp * (ca * e1z + sa * e2z);
    const float ip = 1.0f / sqrtf(px * px + py * py + pz * pz);
    px *= ip; py *= ip; pz *= ip;
    if (!(px * m[0] + py * m[1] + pz * m[2] < 0.0f)) { px = nx; py = ny; pz = nz; }
    const float lo = 1.0f / a.dmax, hi = 1.0f / a.dmin;
    const float inv = fminf(fmaxf(1.0f / cur.x + (2.0f * ud - 1.0f) * a.delta * (hi - lo), lo), hi);
    return make_float4(1.0f / inv, px, py, pz);
}

template <int MODE>
__global__ __launch_bounds__(PM_THREADS) void patch_match_kernel(const PmArgs a) {
    __shared__ float tile[PM_TILE_H * PM_TILE_W];
    __shared__ float geo[PSCV_PM_MAX_SRC * PM_GEO];
    __shared__ float kinv[9];
    const int tid = threadIdx.x;
    const int tw = MODE == PM_HALF ? 32 : 16;
    const int R = a.radius;
    const int r0 = blockIdx.y * PM_ROWS, c0 = blockIdx.x * tw;
    const int tr0 = r0 - R, tc0 = c0 - R;
    for (int k = tid; k < (PM_ROWS + 2 * R) * (tw + 2 * R); k += PM_THREADS) {
        const int lr = k / (tw + 2 * R), lc = k - lr * (tw + 2 * R);
        const int gr = min(max(tr0 + lr, 0), a.h - 1), gc = min(max(tc0 + lc, 0), a.w - 1);
        tile[lr * PM_TILE_W + lc] = a.ref[(long)gr * a.w + gc];
    }
    if (tid < a.n_src) pm_source_block(a.cams, tid, geo + tid * PM_GEO);
    if (tid < 9) kinv[tid] = a.cams[CAM_KINV + tid];
    __syncthreads();

    PmPixel px;
    const int ty = tid / 16, tx = tid - ty * 16;
    px.row = r0 + ty;
    px.col = MODE == PM_HALF ? c0 + 2 * tx + ((px.row + a.colour) & 1) : c0 + tx;
    if (px.row >= a.h || px.col >= a.w) return;
    const long pix = (long)px.row * a.w + px.col;
    const float col = (float)px.col, row = (float)px.row;
    for (int i = 0; i < 3; ++i) px.m[i] = kinv[3 * i] * col + kinv[3 * i + 1] * row + kinv[3 * i + 2];
    px.centre = tile[(px.row - tr0) * PM_TILE_W + (px.col - tc0)];
    {
        const int kr = R / a.step;
        const float inv2ss = 1.0f / (2.0f * (float)R * (float)R);
        constexpr float inv2sc = 1.0f / (2.0f * PM_SIGMA_COLOR * PM_SIGMA_COLOR);
        double W = 0.0, S1 = 0.0, S2 = 0.0;
        for (int ky = -kr; ky <= kr; ++ky) {
            const int oy = ky * a.step;
            const float* trow = tile + (px.row + oy - tr0) * PM_TILE_W + (px.col - tc0);
            for (int kx = -kr; kx <= kr; ++kx) {
                const int ox = kx * a.step;
                const float rp = trow[ox] - px.centre;
                const float wgt = __expf(-(float)(oy * oy + ox * ox) * inv2ss - rp * rp * inv2sc);
                W += (double)wgt;
                S1 += (double)(wgt * rp);
                S2 += (double)(wgt * rp) * (double)rp;
            }
        }
        px.inv_w = 1.0 / W;
        px.mr = S1 * px.inv_w;
        px.vr = S2 * px.inv_w - px.mr * px.mr;
    }

    const float4 cur = a.state[pix];
    if (MODE == PM_COST) {
        const float c = pm_eval<PM_COST>(a, px, tile, geo, kinv, tr0, tc0, cur.x, cur.y, cur.z, cur.w, pix, nullptr);
        if (a.out_agg) a.out_agg[pix] = c;
        return;
    }
    if (MODE == PM_FILTER) {
        int npass = 0;
        if (cur.x > 0.0f) pm_eval<PM_FILTER>(a, px, tile, geo, kinv, tr0, tc0, cur.x, cur.y, cur.z, cur.w, pix, &npass);
        const bool keep = npass >= PM_FILTER_MIN_CONSISTENT;
        a.out_depth[pix] = keep ? cur.x : 0.0f;
        a.out_normal[3 * pix] = keep ? cur.y : 0.0f;
        a.out_normal[3 * pix + 1] = keep ? cur.z : 0.0f;
        a.out_normal[3 * pix + 2] = keep ? cur.w : 0.0f;
        if (a.out_count) a.out_count[pix] = npass;
        return;
    }
    // HALF: candidates in index order, the lowest aggregated cost wins (ties: the lowest index)
    float4* cand_out = a.out_cand ? a.out_cand + pix * PM_NCAND : nullptr;
    float4 best = cur;
    float best_c = 0.0f;
    int best_k = 0;
#pragma unroll 1
    for (int k = 0; k < PM_NCAND; ++k) {
        float4 hyp = cur;
        bool live = true;
        if (k >= 1 && k <= 8) {
            // (0,-1) (0,1) (-1,0) (1,0) (0,-3) (0,3) (-3,0) (3,0) as (drow, dcol)
            const int dist = k <= 4 ? 1 : 3, which = (k - 1) & 3;
            const int qr = px.row + (which == 2 ? -dist : which == 3 ? dist : 0);
            const int qc = px.col + (which == 0 ? -dist : which == 1 ? dist : 0);
            live = qr >= 0 && qr < a.h && qc >= 0 && qc < a.w;
            hyp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (live) {
                const float4 q = a.state[(long)qr * a.w + qc];
                const float fq = (float)qc, fr = (float)qr;
                const float q0 = q.x * (kinv[0] * fq + kinv[1] * fr + kinv[2]);
                const float q1 = q.x * (kinv[3] * fq + kinv[4] * fr + kinv[5]);
                const float q2 = q.x * (kinv[6] * fq + kinv[7] * fr + kinv[8]);
                const float d = (q.y * q0 + q.z * q1 + q.w * q2) / (q.y * px.m[0] + q.z * px.m[1] + q.w * px.m[2]);
                live = d >= a.dmin && d <= a.dmax;
                if (live) hyp = make_float4(d, q.y, q.z, q.w);
            }
        } else if (k == 9) {
            hyp = pm_perturb(a, px.m, cur, (uint32_t)pix);
        } else if (k == 10) {
            hyp = pm_random(a, px.m, (uint32_t)pix, a.iteration, (uint32_t)a.colour);
        }
        if (cand_out) cand_out[k] = hyp;
        if (!live) continue;
        const float c = pm_eval<PM_HALF>(a, px, tile, geo, kinv, tr0, tc0, hyp.x, hyp.y, hyp.z, hyp.w, pix, nullptr);
        if (k == 0 || c < best_c) {
            best_c = c;
            best = hyp;
            best_k = k;
        }
    }
    a.state[pix] = best;
    if (a.out_choice) a.out_choice[pix] = best_k;
}

__global__ __launch_bounds__(PM_THREADS) void patch_match_init_kernel(const PmArgs a) {
    const long pix = (long)blockIdx.x * PM_THREADS + threadIdx.x;
    if (pix >= (long)a.h * a.w) return;
    const int row = (int)(pix / a.w), col = (int)(pix - (long)row * a.w);
    const float* k = a.cams + CAM_KINV;
    float m[3];
    for (int i = 0; i < 3; ++i) m[i] = k[3 * i] * (float)col + k[3 * i + 1] * (float)row + k[3 * i + 2];
    a.state[pix] = pm_random(a, m, (uint32_t)pix, PM_INIT_ITERATION, 0u);
}

int pm_fill(PmArgs& a, const char* what, const float* ref, int h, int w, const float* const* src, const int* src_hw, int n_src,
            const float* cams, const float* const* src_depth, int radius, int step, int top_k) {
    PSCV_CHECK_ARG(ref && cams && (n_src == 0 || (src && src_hw)), "%s: null pointer argument", what);
    PSCV_CHECK_ARG(h > 0 && w > 0 && (long)h * w < (1L << 31), "%s: bad size %dx%d", what, h, w);
    PSCV_CHECK_ARG(n_src >= 1 && n_src <= PSCV_PM_MAX_SRC, "%s: n_src=%d outside [1,%d]", what, n_src, PSCV_PM_MAX_SRC);
    PSCV_CHECK_ARG(radius >= 1 && radius <= PSCV_PM_MAX_RADIUS, "%s: window radius %d outside [1,%d]", what, radius,
                   PSCV_PM_MAX_RADIUS);
    PSCV_CHECK_ARG(step >= 1 && step <= radius, "%s: window step %d outside [1,radius=%d]", what, step, radius);
    PSCV_CHECK_ARG(top_k >= 1 && top_k <= n_src && top_k <= PSCV_PM_MAX_TOPK, "%s: top_k=%d outside [1,min(n_src=%d,%d)]", what,
                   top_k, n_src, PSCV_PM_MAX_TOPK);
    a.ref = ref;
    a.h = h; a.w = w;
    a.n_src = n_src;
    a.cams = cams;
    a.radius = radius; a.step = step; a.top_k = top_k;
    a.geom = src_depth != nullptr;
    for (int s = 0; s < PSCV_PM_MAX_SRC; ++s) {
        const bool on = s < n_src;
        a.src[s] = on ? src[s] : nullptr;
        a.sdepth[s] = on && src_depth ? src_depth[s] : nullptr;
        a.sh[s] = on ? src_hw[2 * s] : 1;
        a.sw[s] = on ? src_hw[2 * s + 1] : 1;
        if (on) {
            PSCV_CHECK_ARG(src[s] && (!src_depth || src_depth[s]), "%s: source %d has a null pointer", what, s);
            PSCV_CHECK_ARG(a.sh[s] > 0 && a.sw[s] > 0 && (long)a.sh[s] * a.sw[s] < (1L << 31), "%s: source %d has bad size %dx%d",
                           what, s, a.sh[s], a.sw[s]);
        }
    }
    return 0;
}

dim3 pm_grid(int mode, int h, int w) {
    const int tw = mode == PM_HALF ? 32 : 16;
    return dim3((unsigned)((w + tw - 1) / tw), (unsigned)((h + PM_ROWS - 1) / PM_ROWS));
}

}  // namespace pscv

extern "C" int pscv_patch_match_init(float* state, int h, int w, const float* cams, float depth_min, float depth_max, int seed,
                                     int view, void* stream) {
    using namespace pscv;
    PSCV_CHECK_ARG(state && cams, "pscv_patch_match_init: null pointer argument");
    PSCV_CHECK_ARG(h > 0 && w > 0 && (long)h * w < (1L << 31), "pscv_patch_match_init: bad size %dx%d", h, w);
    PSCV_CHECK_ARG(depth_min > 0.0f && depth_max > depth_min, "pscv_patch_match_init: need 0 < depth_min < depth_max, got %g, %g",
                   (double)depth_min, (double)depth_max);
    PmArgs a = {};
    a.state = reinterpret_cast<float4*>(state);
    a.cams = cams;
    a.h = h; a.w = w;
    a.dmin = depth_min; a.dmax = depth_max;
    a.seed = (uint32_t)seed; a.view = (uint32_t)view;
    const long n = (long)h * w;
    return launch("pscv_patch_match_init", patch_match_init_kernel, dim3((unsigned)((n + PM_THREADS - 1) / PM_THREADS)), dim3(PM_THREADS), 0,
                  reinterpret_cast<hipStream_t>(stream), a);
}

extern "C" int pscv_patch_match_cost(const float* state, const float* ref, int h, int w, const float* const* src, const int* src_hw,
                                     int n_src, const float* cams, const float* const* src_depth, int radius, int step, int top_k,
                                     float* out_cost, float* out_err, float* out_agg, void* stream) {
    using namespace pscv;
    PmArgs a = {};
    if (pm_fill(a, "pscv_patch_match_cost", ref, h, w, src, src_hw, n_src, cams, src_depth, radius, step, top_k)) return -1;
    PSCV_CHECK_ARG(state && out_cost, "pscv_patch_match_cost: null state or out_cost");
    a.state = reinterpret_cast<float4*>(const_cast<float*>(state));
    a.out_cost = out_cost; a.out_err = out_err; a.out_agg = out_agg;
    return launch("pscv_patch_match_cost", patch_match_kernel<PM_COST>, pm_grid(PM_COST, h, w), dim3(PM_THREADS), 0,
                  reinterpret_cast<hipStream_t>(stream), a);
}

extern "C" int pscv_patch_match_half_step(float* state, const float* ref, int h, int w, const float* const* src, const int* src_hw,
                                          int n_src, const float* cams, const float* const* src_depth, float depth_min,
                                          float depth_max, int radius, int step, int top_k, int seed, int view, int iteration,
                                          int colour, float delta, float theta, int* out_choice, float* out_cand, void* stream) {
    using namespace pscv;
    PmArgs a = {};
    if (pm_fill(a, "pscv_patch_match_half_step", ref, h, w, src, src_hw, n_src, cams, src_depth, radius, step, top_k)) return -1;
    PSCV_CHECK_ARG(state, "pscv_patch_match_half_step: null state");
    PSCV_CHECK_ARG(depth_min > 0.0f && depth_max > depth_min, "pscv_patch_match_half_step: need 0 < depth_min < depth_max, got %g, %g",
                   (double)depth_min, (double)depth_max);
    PSCV_CHECK_ARG(colour == 0 || colour == 1, "pscv_patch_match_half_step: colour %d is not 0 or 1", colour);
    PSCV_CHECK_ARG(delta >= 0.0f && delta <= 1.0f && theta >= 0.0f && theta <= 3.14159265f,
                   "pscv_patch_match_half_step: perturbation delta=%g theta=%g outside [0,1] x [0,pi]", (double)delta, (double)theta);
    a.state = reinterpret_cast<float4*>(state);
    a.dmin = depth_min; a.dmax = depth_max;
    a.seed = (uint32_t)seed; a.view = (uint32_t)view; a.iteration = (uint32_t)iteration;
    a.colour = colour; a.delta = delta; a.theta = theta;
    a.out_choice = out_choice;
    a.out_cand = reinterpret_cast<float4*>(out_cand);
    return launch("pscv_patch_match_half_step", patch_match_kernel<PM_HALF>, pm_grid(PM_HALF, h, w), dim3(PM_THREADS), 0,
                  reinterpret_cast<hipStream_t>(stream), a);
}

extern "C" int pscv_patch_match_filter(const float* state, const float* ref, int h, int w, const float* const* src, const int* src_hw,
                                       int n_src, const float* cams, const float* const* src_depth, int radius, int step,
                                       float* out_depth, float* out_normal, int* out_count, void* stream) {
    using namespace pscv;
    PmArgs a = {};
    PSCV_CHECK_ARG(src_depth, "pscv_patch_match_filter: the sources' depth maps are required");
    if (pm_fill(a, "pscv_patch_match_filter", ref, h, w, src, src_hw, n_src, cams, src_depth, radius, step, 1)) return -1;
    PSCV_CHECK_ARG(state && out_depth && out_normal, "pscv_patch_match_filter: null state or output");
    a.state = reinterpret_cast<float4*>(const_cast<float*>(state));
    a.out_depth = out_depth; a.out_normal = out_normal; a.out_count = out_count;
    return launch("pscv_patch_match_filter", patch_match_kernel<PM_FILTER>, pm_grid(PM_FILTER, h, w), dim3(PM_THREADS), 0,
                  reinterpret_cast<hipStream_t>(stream), a);
}
