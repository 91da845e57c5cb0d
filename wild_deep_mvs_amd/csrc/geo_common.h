// Shared pieces of the evaluation kernels.  Included by geo_filter, depth_fusion, colmap_fusion, view_covis, depth_normals, patch_match,
// point_metrics and, through tsdf_dev.h, tsdf_fusion and tsdf_bricks.  gfx950.
#pragma once
#include "pscv_common.h"

namespace pscv {

// ---- the camera block of ops.geo_filter_cams: PSCV_GEO_CAM_FLOATS floats, K, K^-1, R (row-major 3x3 each), t ----------------
constexpr int CAM_K = 0, CAM_KINV = 9, CAM_R = 18, CAM_T = 27;

// M v, accumulated k = 0, 1, 2 like a 3-wide GEMM row (explicit fmaf: callers that recompute a projection get the same bits)
__device__ __forceinline__ void mat_vec(const float* M, float x, float y, float z, float& ox, float& oy, float& oz) {
    ox = fmaf(M[2], z, fmaf(M[1], y, M[0] * x));
    oy = fmaf(M[5], z, fmaf(M[4], y, M[3] * x));
    oz = fmaf(M[8], z, fmaf(M[7], y, M[6] * x));
}
// M^T v
__device__ __forceinline__ void matT_vec(const float* M, float x, float y, float z, float& ox, float& oy, float& oz) {
    ox = fmaf(M[6], z, fmaf(M[3], y, M[0] * x));
    oy = fmaf(M[7], z, fmaf(M[4], y, M[1] * x));
    oz = fmaf(M[8], z, fmaf(M[5], y, M[2] * x));
}
// R^T (d K^-1 (x, y, 1) - t)
__device__ __forceinline__ void cam_unproject(const float* cam, float x, float y, float d, float& X, float& Y, float& Z) {
    const float* t = cam + CAM_T;
    float ax, ay, az;
    mat_vec(cam + CAM_KINV, x * d, y * d, d, ax, ay, az);
    matT_vec(cam + CAM_R, ax - t[0], ay - t[1], az - t[2], X, Y, Z);
}
// K (R X + t): the homogeneous pixel (not divided by z)
__device__ __forceinline__ void cam_point(const float* cam, float X, float Y, float Z, float& px, float& py, float& pz) {
    const float* t = cam + CAM_T;
    float cx, cy, cz;
    mat_vec(cam + CAM_R, X, Y, Z, cx, cy, cz);
    mat_vec(cam + CAM_K, cx + t[0], cy + t[1], cz + t[2], px, py, pz);
}

// ---- fp64 geometry of the COLMAP-style fusion (colmap_fusion.hip phase A) and of the view covisibility built on it (view_covis.hip):
// pixel (col, row) is the integer pair itself (no half-pixel offset); both files are compiled with -ffp-contract=off ---------------
// R^T (d K^-1 (x, y, 1) - t)
__device__ __forceinline__ void cf_unproject(const float* c, double x, double y, double d, double& X, double& Y, double& Z) {
    const float *Ki = c + CAM_KINV, *R = c + CAM_R, *t = c + CAM_T;
    const double px = x * d, py = y * d, pz = d;
    const double a0 = (double)Ki[0] * px + (double)Ki[1] * py + (double)Ki[2] * pz;
    const double a1 = (double)Ki[3] * px + (double)Ki[4] * py + (double)Ki[5] * pz;
    const double a2 = (double)Ki[6] * px + (double)Ki[7] * py + (double)Ki[8] * pz;
    const double b0 = a0 - (double)t[0], b1 = a1 - (double)t[1], b2 = a2 - (double)t[2];
    X = (double)R[0] * b0 + (double)R[3] * b1 + (double)R[6] * b2;
    Y = (double)R[1] * b0 + (double)R[4] * b1 + (double)R[7] * b2;
    Z = (double)R[2] * b0 + (double)R[5] * b1 + (double)R[8] * b2;
}
// K (R X + t)
__device__ __forceinline__ void cf_project(const float* c, double X, double Y, double Z, double& x, double& y, double& z) {
    const float *K = c + CAM_K, *R = c + CAM_R, *t = c + CAM_T;
    const double e0 = (double)R[0] * X + (double)R[1] * Y + (double)R[2] * Z + (double)t[0];
    const double e1 = (double)R[3] * X + (double)R[4] * Y + (double)R[5] * Z + (double)t[1];
    const double e2 = (double)R[6] * X + (double)R[7] * Y + (double)R[8] * Z + (double)t[2];
    x = (double)K[0] * e0 + (double)K[1] * e1 + (double)K[2] * e2;
    y = (double)K[3] * e0 + (double)K[4] * e1 + (double)K[5] * e2;
    z = (double)K[6] * e0 + (double)K[7] * e1 + (double)K[8] * e2;
}
__device__ __forceinline__ bool cf_depth_ok(float d) { return d > 0.0f && d <= 3.402823466e38f; }   // (false for NaN, inf)
constexpr double CF_PIX_LIMIT = 1073741824.0;   // 2^30: a projection further out is no pixel of any view
// world normal R^T n of the camera-frame normal at n[0..2], each component rounded to fp32 (the fusion's normal test; depth_normals.hip)
__device__ __forceinline__ void cf_world_normal(const float* c, const float* n, float& wx, float& wy, float& wz) {
    const float* R = c + CAM_R;
    const double nx = (double)n[0], ny = (double)n[1], nz = (double)n[2];
    wx = (float)((double)R[0] * nx + (double)R[3] * ny + (double)R[6] * nz);
    wy = (float)((double)R[1] * nx + (double)R[4] * ny + (double)R[7] * nz);
    wz = (float)((double)R[2] * nx + (double)R[5] * ny + (double)R[8] * nz);
}

// ---- one-workgroup exclusive scan ------------------------------------------------------------------------------------------
// (internal linkage: every translation unit keeps its own copy in its own code object)
namespace {
// off[k] = base + count[0] + ... + count[k-1]: with COUNTER, base = *counter and the counter then advances by the total;
// without, base = 0 and counter is not used
template <int THREADS, typename Off, bool COUNTER>
__global__ __launch_bounds__(THREADS) void scan_kernel(const int* __restrict__ count, Off* off, long long* counter, int n) {
    __shared__ long long part[THREADS];
    const int per = (n + THREADS - 1) / THREADS;
    const int b = threadIdx.x * per, e = min(b + per, n);
    long long s = 0;
    for (int k = b; k < e; ++k) s += count[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < THREADS; o <<= 1) {                       // Hillis-Steele, inclusive
        const long long v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    const long long base = COUNTER ? *counter : 0;
    long long run = base + part[threadIdx.x] - s;
    for (int k = b; k < e; ++k) {
        off[k] = (Off)run;
        run += count[k];
    }
    __syncthreads();                                               // every lane has read the counter
    if (COUNTER && threadIdx.x == THREADS - 1) *counter = base + part[threadIdx.x];
}
}  // namespace

// ---- host side ---------------------------------------------------------------------------------------------------------------
inline long align256(long bytes) { return (bytes + 255) / 256 * 256; }

// The view table of a multi-view operator.  An operator that takes up to PSCV_FUSE_MAX_VIEWS views of different sizes carries them
// as kernel arguments: a struct with depth[], h[], w[] (filled by fill_views) and whatever per-view companion pointers it needs
// (fill_view_ptrs).  Each helper returns -1 with the error set.
inline int check_view_count(const char* what, int n, int lo) {
    PSCV_CHECK_ARG(n >= lo && n <= PSCV_FUSE_MAX_VIEWS, "%s: n_views=%d outside [%d,%d]", what, n, lo, PSCV_FUSE_MAX_VIEWS);
    return 0;
}
inline int check_view_size(const char* what, int v, int h, int w) {
    PSCV_CHECK_ARG(h > 0 && w > 0 && (long)h * w < (1L << 31), "%s: view %d has bad size %dx%d", what, v, h, w);
    return 0;
}
// a.depth, a.h, a.w = the views [first, first + n) of depth / hw; the entries past n are null, 1 x 1
template <typename Args>
int fill_views(Args& a, const char* what, const float* const* depth, const int* hw, int n, int first = 0) {
    for (int k = 0; k < PSCV_FUSE_MAX_VIEWS; ++k) {
        const bool on = k < n;
        const int v = first + k;
        a.depth[k] = on ? depth[v] : nullptr;
        a.h[k] = on ? hw[2 * v] : 1;
        a.w[k] = on ? hw[2 * v + 1] : 1;
        if (!on) continue;
        PSCV_CHECK_ARG(depth[v], "%s: view %d has a null pointer", what, v);
        if (check_view_size(what, v, a.h[k], a.w[k])) return -1;
    }
    return 0;
}
// dst = src[0 .. n), null past n; a null src is an optional array that was not given: every entry null
template <typename T>
int fill_view_ptrs(T* (&dst)[PSCV_FUSE_MAX_VIEWS], const char* what, T* const* src, int n, const char* noun = "pointer") {
    for (int v = 0; v < PSCV_FUSE_MAX_VIEWS; ++v) {
        dst[v] = src && v < n ? src[v] : nullptr;
        PSCV_CHECK_ARG(!src || v >= n || src[v], "%s: view %d has a null %s", what, v, noun);
    }
    return 0;
}

}  // namespace pscv
