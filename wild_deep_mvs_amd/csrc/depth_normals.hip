// Normal maps from depth maps, and the world normals of fused points: what gives a network reconstruction real normals for the
// COLMAP-style fusion's normal test and for meshing.  gfx950.
//
// The rule.  A plane seen by a pinhole camera has inverse depth affine in the pixel, 1/d(u,v) = n^T K^-1 (u,v,1) / delta, so the
// normal is a linear least-squares fit of the inverse depth over a window: no 3-D points, no eigenvectors.  All arithmetic is fp64
// on values converted from the fp32 inputs; products and sums are separate operations in the order written (the Makefile builds
// this file with -ffp-contract=off, like colmap_fusion.hip), which tests/_depth_normals_ref.py reproduces bit for bit:
//   * a pixel is valid when cf_depth_ok(d); an invalid pixel gets normal (0,0,0) and support 0; rho_q = 1.0 / d_q once per pixel;
//   * for a valid centre p = (x, y) the taps q = (x+i, y+j), j = -r..r outer, i = -r..r inner, count when q is inside the image,
//     valid and |d_q - d_p| <= tau d_p; the centre always counts;
//   * with e = d_p rho_q - 1: S1 += 1, Si += i, Sj += j, Sii += i i, Sij += i j, Sjj += j j, Se += e, Sie += i e, Sje += j e
//     (the six geometric sums are small integers: kept in int32 here, exact in fp64 either way); n = S1;
//   * C00 = Sjj S1 - Sj Sj, C01 = Sj Si - Sij S1, C02 = Sij Sj - Sjj Si, C11 = Sii S1 - Si Si, C12 = Sij Si - Sii Sj,
//     C22 = Sii Sjj - Sij Sij, det = Sii C00 + Sij C01 + Si C02 (an exact integer, 0 exactly when the taps are collinear);
//   * A = C00 Sie + C01 Sje + C02 Se, B = C01 Sie + C11 Sje + C12 Se, Cc = C02 Sie + C12 Sje + C22 Se, g2 = det + Cc;
//   * fit when n >= min_support, det > 0 and g2 > 0: g = (A, B, g2 - A x - B y), v = -(K^T g);
//     fallback otherwise: v = -(K^-1 (x, y, 1)), the ray towards the camera;
//   * normal = v / sqrt(v0 v0 + v1 v1 + v2 v2), each component rounded to fp32 (camera frame, n^T K^-1 p < 0);
//     support = n when the fit was used, -n on fallback.
//
// Mapping: one launch for up to PSCV_FUSE_MAX_VIEWS views of different sizes (pointers and sizes travel as kernel arguments;
// grid.y = view, grid.x = tiles of the largest view, a workgroup past its view's tiles leaves at once).  A workgroup of 256 lanes
// owns a tile of DN_TH x DN_TW = 8 x 32 pixels, one per lane, rows contiguous across lanes.  The tile plus a halo of r is staged
// once in LDS as the depth converted to fp64 (NaN = invalid or outside the image, so the gate's one comparison refuses it) and its
// fp64 reciprocal: at r = 4, 16 x 40 x 16 B = 10240 B.  One barrier; then every lane walks its window from LDS (consecutive lanes
// read consecutive 8-byte words: no bank conflicts).
//
// The window walk is bound by the vector ALU, so it is written for few instructions per tap, none of which changes a bit:
//   * a tap that does not count adds e = +0.0 (and i e, j e = +-0.0) instead of being skipped.  Se, Sie and Sje start at +0.0 and a
//     sum is -0.0 only when both addends are, and e = a - 1.0 is never -0.0, so none of the three is ever -0.0 and adding a zero of
//     either sign leaves every bit; for the same reason the products with i = 0 or j = 0 are not added at all;
//   * the six integer sums are kept per row as (count, sum of i, sum of i i) and folded with j once per row.
#include "geo_common.h"

#include <float.h>

namespace pscv {

constexpr int DN_TW = 32, DN_TH = 8, DN_THREADS = DN_TW * DN_TH;
constexpr int DN_MAX_RADIUS = 4;

struct DnArgs {
    const float* depth[PSCV_FUSE_MAX_VIEWS];            // [h_v, w_v]
    float* normal[PSCV_FUSE_MAX_VIEWS];                 // [h_v, w_v, 3]
    int* support[PSCV_FUSE_MAX_VIEWS];                  // [h_v, w_v] or null
    int h[PSCV_FUSE_MAX_VIEWS], w[PSCV_FUSE_MAX_VIEWS];
    const float* cams;                                  // [n][PSCV_GEO_CAM_FLOATS], row v = view v
    double tau;
    int min_support;
};
static_assert(sizeof(DnArgs) <= 4096, "the kernel-argument segment holds 4 KB");

struct DnF3 { float x, y, z; };

template <int R>
__global__ __launch_bounds__(DN_THREADS) void depth_normals_kernel(const DnArgs a) {
    constexpr int PW = DN_TW + 2 * R, PH = DN_TH + 2 * R;
    __shared__ double sd[PH * PW];
    __shared__ double sr[PH * PW];
    const int tid = threadIdx.x;
    const int v = blockIdx.y;
    const int h = a.h[v], w = a.w[v];
    const int tiles_x = (w + DN_TW - 1) / DN_TW, tiles_y = (h + DN_TH - 1) / DN_TH;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;            // (workgroup-uniform: the grid is sized for the largest view)
    const int by = (int)blockIdx.x / tiles_x, bx = (int)blockIdx.x - by * tiles_x;
    const int x0 = bx * DN_TW, y0 = by * DN_TH;
    const float* depth = a.depth[v];
    for (int k = tid; k < PH * PW; k += DN_THREADS) {
        const int ly = k / PW, lx = k - ly * PW;
        const int gy = y0 + ly - R, gx = x0 + lx - R;
        float d = 0.0f;
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) d = depth[(long)gy * w + gx];
        const bool ok = cf_depth_ok(d);
        sd[k] = ok ? (double)d : __builtin_nan("");
        sr[k] = ok ? 1.0 / (double)d : 0.0;
    }
    __syncthreads();

    const int lx = tid & (DN_TW - 1), ly = tid / DN_TW;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= w || y >= h) return;
    const long o = (long)y * w + x;
    DnF3* out_n = reinterpret_cast<DnF3*>(a.normal[v]) + o;
    int* sup = a.support[v];
    const int c = (ly + R) * PW + lx + R;
    const double dp = sd[c];
    if (!(dp > 0.0)) {
        *out_n = DnF3{0.0f, 0.0f, 0.0f};
        if (sup) sup[o] = 0;
        return;
    }
    const double thr = a.tau * dp;
    int n = 0, si = 0, sj = 0, sii = 0, sij = 0, sjj = 0;
    double Se = 0.0, Sie = 0.0, Sje = 0.0;
#pragma unroll
    for (int j = -R; j <= R; ++j) {
        int cnt = 0, ri = 0, rii = 0;
#pragma unroll
        for (int i = -R; i <= R; ++i) {
            const int q = c + j * PW + i;
            const double e_q = dp * sr[q] - 1.0;                              // (for every tap: a select, no branch)
            const bool on = (i == 0 && j == 0) || fabs(sd[q] - dp) <= thr;    // (false for NaN: invalid, or outside the image)
            const double e = on ? e_q : 0.0;
            const int b = on ? 1 : 0;
            cnt += b;
            ri += i * b;
            rii += i * i * b;
            Se += e;
            if (i != 0) Sie += (double)i * e;
            if (j != 0) Sje += (double)j * e;
        }
        n += cnt;
        si += ri;
        sii += rii;
        sj += j * cnt;
        sij += j * ri;
        sjj += j * j * cnt;
    }
    const double S1 = (double)n, Si = (double)si, Sj = (double)sj, Sii = (double)sii, Sij = (double)sij, Sjj = (double)sjj;
    const double C00 = Sjj * S1 - Sj * Sj;
    const double C01 = Sj * Si - Sij * S1;
    const double C02 = Sij * Sj - Sjj * Si;
    const double C11 = Sii * S1 - Si * Si;
    const double C12 = Sij * Si - Sii * Sj;
    const double C22 = Sii * Sjj - Sij * Sij;
    const double det = Sii * C00 + Sij * C01 + Si * C02;
    const double A = C00 * Sie + C01 * Sje + C02 * Se;
    const double B = C01 * Sie + C11 * Sje + C12 * Se;
    const double Cc = C02 * Sie + C12 * Sje + C22 * Se;
    const double g2 = det + Cc;
    const bool fit = n >= a.min_support && det > 0.0 && g2 > 0.0;
    const float* cam = a.cams + (long)v * PSCV_GEO_CAM_FLOATS;
    const double xd = (double)x, yd = (double)y;
    double v0, v1, v2;
    if (fit) {
        const float* K = cam + CAM_K;
        const double g0 = A, g1 = B, gc = g2 - A * xd - B * yd;
        v0 = -((double)K[0] * g0 + (double)K[3] * g1 + (double)K[6] * gc);
        v1 = -((double)K[1] * g0 + (double)K[4] * g1 + (double)K[7] * gc);
        v2 = -((double)K[2] * g0 + (double)K[5] * g1 + (double)K[8] * gc);
    } else {
        const float* Ki = cam + CAM_KINV;
        v0 = -((double)Ki[0] * xd + (double)Ki[1] * yd + (double)Ki[2] * 1.0);
        v1 = -((double)Ki[3] * xd + (double)Ki[4] * yd + (double)Ki[5] * 1.0);
        v2 = -((double)Ki[6] * xd + (double)Ki[7] * yd + (double)Ki[8] * 1.0);
    }
    const double norm = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
    *out_n = DnF3{(float)(v0 / norm), (float)(v1 / norm), (float)(v2 / norm)};
    if (sup) sup[o] = fit ? n : -n;
}

// ---- world normals of fused points: w = R_v^T n_v[pixel] (cf_world_normal, the rule of the fusion's normal test) -----------------
struct PwnArgs {
    const float* normal[PSCV_FUSE_MAX_VIEWS];           // [h_v, w_v, 3]
    int pixels[PSCV_FUSE_MAX_VIEWS];                    // h_v w_v
};
static_assert(sizeof(PwnArgs) <= 4096, "the kernel-argument segment holds 4 KB");

__global__ __launch_bounds__(DN_THREADS) void point_world_normals_kernel(const PwnArgs a, const int* __restrict__ view,
                                                                         const int* __restrict__ pixel,
                                                                         const float* __restrict__ cams, float* __restrict__ out,
                                                                         long n_points, int n_views) {
    __shared__ const float* nrm[PSCV_FUSE_MAX_VIEWS];
    __shared__ int npix[PSCV_FUSE_MAX_VIEWS];
    if (threadIdx.x < PSCV_FUSE_MAX_VIEWS) {
        nrm[threadIdx.x] = a.normal[threadIdx.x];
        npix[threadIdx.x] = a.pixels[threadIdx.x];
    }
    __syncthreads();
    for (long k = (long)blockIdx.x * DN_THREADS + threadIdx.x; k < n_points; k += (long)gridDim.x * DN_THREADS) {
        const int v = view[k], p = pixel[k];
        float wx = 0.0f, wy = 0.0f, wz = 0.0f;                   // an index outside its range reads nothing and gives 0
        if (v >= 0 && v < n_views && p >= 0 && p < npix[v])
            cf_world_normal(cams + (long)v * PSCV_GEO_CAM_FLOATS, nrm[v] + 3 * (long)p, wx, wy, wz);
        *(reinterpret_cast<DnF3*>(out) + k) = DnF3{wx, wy, wz};
    }
}

}  // namespace pscv

extern "C" int pscv_depth_normals(const float* const* depth, const int* hw, int n_views, const float* cams, int radius,
                                  double rel_gate, int min_support, float* const* normal, int* const* support, void* stream) {
    using namespace pscv;
    const char* what = "pscv_depth_normals";
    PSCV_CHECK_ARG(depth && hw && cams && normal, "%s: null pointer argument", what);
    if (check_view_count(what, n_views, 1)) return -1;
    PSCV_CHECK_ARG(radius >= 1 && radius <= DN_MAX_RADIUS, "%s: radius=%d outside [1,%d]", what, radius, DN_MAX_RADIUS);
    PSCV_CHECK_ARG(rel_gate > 0.0 && rel_gate <= DBL_MAX, "%s: rel_gate=%g must be positive and finite", what, rel_gate);
    const int window = (2 * radius + 1) * (2 * radius + 1);
    PSCV_CHECK_ARG(min_support >= 3 && min_support <= window, "%s: min_support=%d outside [3,%d]", what, min_support, window);
    DnArgs a;
    if (fill_views(a, what, depth, hw, n_views) || fill_view_ptrs(a.normal, what, normal, n_views) ||
        fill_view_ptrs(a.support, what, support, n_views))
        return -1;
    long max_tiles = 0;
    for (int v = 0; v < n_views; ++v) {
        const long tiles = (long)((a.h[v] + DN_TH - 1) / DN_TH) * ((a.w[v] + DN_TW - 1) / DN_TW);
        if (tiles > max_tiles) max_tiles = tiles;
    }
    a.cams = cams;
    a.tau = rel_gate;
    a.min_support = min_support;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)max_tiles, (unsigned)n_views), block(DN_THREADS);
    switch (radius) {
        case 1: return launch(what, depth_normals_kernel<1>, grid, block, 0, st, a);
        case 2: return launch(what, depth_normals_kernel<2>, grid, block, 0, st, a);
        case 3: return launch(what, depth_normals_kernel<3>, grid, block, 0, st, a);
        default: return launch(what, depth_normals_kernel<4>, grid, block, 0, st, a);
    }
}

extern "C" int pscv_point_world_normals(const int* view, const int* pixel, long n_points, const float* const* normal, const int* hw,
                                        int n_views, const float* cams, float* out, void* stream) {
    using namespace pscv;
    const char* what = "pscv_point_world_normals";
    PSCV_CHECK_ARG(n_points >= 0, "%s: n_points=%ld < 0", what, n_points);
    PSCV_CHECK_ARG(normal && hw && cams, "%s: null pointer argument", what);
    if (check_view_count(what, n_views, 1)) return -1;
    PwnArgs a;
    if (fill_view_ptrs(a.normal, what, normal, n_views)) return -1;
    for (int v = 0; v < PSCV_FUSE_MAX_VIEWS; ++v) {
        a.pixels[v] = 0;
        if (v >= n_views) continue;
        if (check_view_size(what, v, hw[2 * v], hw[2 * v + 1])) return -1;
        a.pixels[v] = hw[2 * v] * hw[2 * v + 1];
    }
    if (n_points == 0) return 0;
    PSCV_CHECK_ARG(view && pixel && out, "%s: null pointer argument", what);
    const long blocks = (n_points + DN_THREADS - 1) / DN_THREADS;
    return launch(what, point_world_normals_kernel, dim3((unsigned)(blocks < 65535 ? blocks : 65535)), dim3(DN_THREADS), 0,
                  reinterpret_cast<hipStream_t>(stream), a, view, pixel, cams, out, n_points, n_views);
}
