// Consistency fusion of filtered depth maps into one point cloud (the step AFTER the geometric filter).  gfx950.
//
// One pass per view i (INTEGRATION.md section 2d states the rule).  Each pass is three launches on the caller's stream:
//   fuse    one lane per pixel of view i, 32 x 8 tiles (a wave covers two 32-pixel rows, so neighbouring lanes project to
//           neighbouring pixels of view j and their depth / colour gathers share cache lines): unproject, project into
//           every other view, round to the nearest pixel, gather depth, the disparity test, and for consistent views the
//           unprojected neighbour point and its RGBA8 colour.  A pixel with enough consistent views writes its point into
//           its SEGMENT (one tile row = 32 consecutive pixels of one image row) of a staging buffer, at its rank among
//           the segment's emitting lanes, and marks the pixels it consumed in the other views' used masks (byte stores;
//           the pass reads only used_i and writes only used_j, j != i, so the result does not depend on lane order);
//   scan    one workgroup: exclusive scan of the per-segment counts in row-major segment order, plus the running offset
//           kept on the device (counter), which it then advances;
//   scatter one lane per staging slot: segment s, slot k < count[s] goes to out[offset[s] + k] if that is below capacity.
// Output order is pass-major, then row-major pixel order; nothing depends on atomics or on scheduling.  The counter keeps
// counting past the capacity, so the caller sees an overflow as counter > capacity after the last pass.
//
// Replaces (fdarmon/wild_deep_mvs): evaluation/fusibile.py:160-181, the external CUDA-only `fusibile` binary it runs
// (normal test off: normal_thresh = 360 with fake_gipuma_normal's constant normals).
#include "geo_common.h"

namespace pscv {

constexpr int FUSE_TW = 32, FUSE_TH = 8, FUSE_THREADS = FUSE_TW * FUSE_TH;
constexpr int FUSE_SCAN_THREADS = 1024;

struct FuseArgs {
    const float* depth[PSCV_FUSE_MAX_VIEWS];       // [h_v, w_v]
    const uint32_t* color[PSCV_FUSE_MAX_VIEWS];    // [h_v, w_v] RGBA8 (R in the low byte)
    uint8_t* used[PSCV_FUSE_MAX_VIEWS];            // [h_v, w_v] 0 / 1
    int h[PSCV_FUSE_MAX_VIEWS], w[PSCV_FUSE_MAX_VIEWS];
    const float* cams;                             // [n][PSCV_GEO_CAM_FLOATS]: K, K^-1, R (row-major), t
    int* seg_count;                                // [h_i * nsx]
    float4* stage;                                 // [h_i * nsx * 32]: x, y, z, RGBA8 bits
    int n, i, nsx, need;
    float disp_thresh, depth_min, depth_max;
};

__device__ __forceinline__ bool fu_valid(float d, float lo, float hi) { return d > lo && d < hi; }   // (false for NaN, +-inf)
// K (R X + t) rounded to the nearest pixel of a view of size hj x wj: false when behind the camera or outside
__device__ __forceinline__ bool fu_project(const float* cam, float X, float Y, float Z, int hj, int wj, float& z, int& qx, int& qy) {
    float a, b;
    cam_point(cam, X, Y, Z, a, b, z);
    if (!(z > 0.0f)) return false;
    const float fx = floorf(a / z + 0.5f), fy = floorf(b / z + 0.5f);
    if (!(fx >= 0.0f && fx < (float)wj && fy >= 0.0f && fy < (float)hj)) return false;
    qx = (int)fx; qy = (int)fy;
    return true;
}
__global__ __launch_bounds__(FUSE_THREADS) void fuse_depth_kernel(const FuseArgs a) {
    __shared__ float cam_lds[PSCV_FUSE_MAX_VIEWS * PSCV_GEO_CAM_FLOATS];
    __shared__ float fb_lds[PSCV_FUSE_MAX_VIEWS];       // f_i * |c_i - c_j|
    for (int k = threadIdx.x; k < a.n * PSCV_GEO_CAM_FLOATS; k += FUSE_THREADS) cam_lds[k] = a.cams[k];
    __syncthreads();
    const int i = a.i;
    const float* ci = cam_lds + i * PSCV_GEO_CAM_FLOATS;
    if (threadIdx.x < a.n) {
        const float* cj = cam_lds + threadIdx.x * PSCV_GEO_CAM_FLOATS;
        float xi, yi, zi, xj, yj, zj;                    // -c = R^T t
        matT_vec(ci + CAM_R, ci[CAM_T], ci[CAM_T + 1], ci[CAM_T + 2], xi, yi, zi);
        matT_vec(cj + CAM_R, cj[CAM_T], cj[CAM_T + 1], cj[CAM_T + 2], xj, yj, zj);
        const float dx = xi - xj, dy = yi - yj, dz = zi - zj;
        fb_lds[threadIdx.x] = ci[CAM_K] * sqrtf(dx * dx + dy * dy + dz * dz);
    }
    __syncthreads();

    const int hi = a.h[i], wi = a.w[i];
    const int tx = threadIdx.x % FUSE_TW, ty = threadIdx.x / FUSE_TW;
    const int x = blockIdx.x * FUSE_TW + tx, y = blockIdx.y * FUSE_TH + ty;
    const bool inside = x < wi && y < hi;
    const long pix = (long)y * wi + x;

    bool emit = false;
    float ox = 0.0f, oy = 0.0f, oz = 0.0f;
    uint32_t rgba = 0;
    if (inside) {
        const float d = a.depth[i][pix];
        if (fu_valid(d, a.depth_min, a.depth_max) && a.used[i][pix] == 0) {
            float X, Y, Z;
            cam_unproject(ci, (float)x, (float)y, d, X, Y, Z);
            float sx = 0.0f, sy = 0.0f, sz = 0.0f;
            uint32_t sr = 0, sg = 0, sb = 0;
            int n = 0;
            uint64_t hit = 0;                            // consistent views
            for (int j = 0; j < a.n; ++j) {
                if (j == i) continue;
                const float* cj = cam_lds + j * PSCV_GEO_CAM_FLOATS;
                float z;
                int qx, qy;
                if (!fu_project(cj, X, Y, Z, a.h[j], a.w[j], z, qx, qy)) continue;
                const long q = (long)qy * a.w[j] + qx;
                const float dj = a.depth[j][q];
                if (!fu_valid(dj, a.depth_min, a.depth_max)) continue;
                const float fb = fb_lds[j];
                if (!(fabsf(fb / z - fb / dj) < a.disp_thresh)) continue;
                float Xj, Yj, Zj;
                cam_unproject(cj, (float)qx, (float)qy, dj, Xj, Yj, Zj);
                sx += Xj; sy += Yj; sz += Zj;
                const uint32_t c = a.color[j][q];
                sr += c & 0xffu; sg += (c >> 8) & 0xffu; sb += (c >> 16) & 0xffu;
                ++n;
                hit |= 1ull << j;
            }
            if (n >= a.need) {
                emit = true;
                const float inv = (float)(n + 1);
                ox = (X + sx) / inv; oy = (Y + sy) / inv; oz = (Z + sz) / inv;
                const uint32_t c = a.color[i][pix];
                sr += c & 0xffu; sg += (c >> 8) & 0xffu; sb += (c >> 16) & 0xffu;
                const uint32_t r = (uint32_t)floorf((float)sr / inv + 0.5f);
                const uint32_t g = (uint32_t)floorf((float)sg / inv + 0.5f);
                const uint32_t b = (uint32_t)floorf((float)sb / inv + 0.5f);
                rgba = r | (g << 8) | (b << 16) | ((uint32_t)tx << 24);   // (top byte: column in the tile)
                // mark what the point consumed (same arithmetic as above, so the same pixels)
                while (hit) {
                    const int j = __builtin_ctzll(hit);
                    hit &= hit - 1;
                    float z;
                    int qx, qy;
                    if (fu_project(cam_lds + j * PSCV_GEO_CAM_FLOATS, X, Y, Z, a.h[j], a.w[j], z, qx, qy))
                        a.used[j][(long)qy * a.w[j] + qx] = 1;
                }
            }
        }
    }
    // rank among the emitting lanes of this lane's segment (half a wave = one 32-pixel tile row)
    const uint64_t ball = __ballot(emit);
    const int lane = threadIdx.x & 63;
    const uint64_t half = (lane < 32) ? 0x00000000ffffffffull : 0xffffffff00000000ull;
    const int rank = __popcll(ball & half & ((1ull << lane) - 1ull));
    if (y < hi) {
        const long seg = (long)y * a.nsx + blockIdx.x;
        if (tx == 0) a.seg_count[seg] = __popcll(ball & half);
        if (emit) a.stage[seg * FUSE_TW + rank] = make_float4(ox, oy, oz, __uint_as_float(rgba));
    }
}

__global__ __launch_bounds__(256) void fuse_scatter_kernel(const int* __restrict__ seg_count, const long long* __restrict__ seg_off,
                                                           const float4* __restrict__ stage, long nslot, int view, int nsx, int w,
                                                           long long capacity, float* out_xyz, uint8_t* out_rgb, int* out_view,
                                                           int* out_pixel) {
    const long slot = (long)blockIdx.x * 256 + threadIdx.x;
    if (slot >= nslot) return;
    const long seg = slot / FUSE_TW;
    const int k = (int)(slot - seg * FUSE_TW);
    if (k >= seg_count[seg]) return;
    const long long o = seg_off[seg] + k;
    if (o >= capacity) return;
    const float4 p = stage[slot];
    const uint32_t c = __float_as_uint(p.w);
    out_xyz[3 * o] = p.x; out_xyz[3 * o + 1] = p.y; out_xyz[3 * o + 2] = p.z;
    out_rgb[3 * o] = (uint8_t)(c & 0xffu); out_rgb[3 * o + 1] = (uint8_t)((c >> 8) & 0xffu);
    out_rgb[3 * o + 2] = (uint8_t)((c >> 16) & 0xffu);
    if (out_view) out_view[o] = view;
    if (out_pixel) {                                  // segment (y, tile column) + the column in the tile, kept in the top byte
        const long y = seg / nsx;
        out_pixel[o] = (int)(y * w + (seg - y * nsx) * FUSE_TW + (c >> 24));
    }
}

}  // namespace pscv

namespace {
long fuse_nseg(int h, int w) { return (long)h * ((w + pscv::FUSE_TW - 1) / pscv::FUSE_TW); }
}

extern "C" long pscv_fuse_depth_workspace(int h, int w) {
    if (h <= 0 || w <= 0) return -1;
    const long nseg = fuse_nseg(h, w);
    // counts int32, offsets int64, staging float4 per slot; each part 256-byte aligned
    return pscv::align256(nseg * 4) + pscv::align256(nseg * 8) + pscv::align256(nseg * pscv::FUSE_TW * 16);
}

extern "C" int pscv_fuse_depth_pass(int pass, const float* const* depth, const unsigned int* const* color,
                                    unsigned char* const* used, const int* hw, int n_views, const float* cams, float disp_thresh,
                                    int num_consistent, float depth_min, float depth_max, float* out_xyz, unsigned char* out_rgb,
                                    int* out_view, int* out_pixel, long capacity, long long* counter, void* workspace,
                                    long workspace_bytes, void* stream) {
    using namespace pscv;
    const char* what = "pscv_fuse_depth_pass";
    PSCV_CHECK_ARG(depth && color && used && hw && cams && counter && workspace, "pscv_fuse_depth_pass: null pointer argument");
    if (check_view_count(what, n_views, 2)) return -1;
    PSCV_CHECK_ARG(pass >= 0 && pass < n_views, "pscv_fuse_depth_pass: pass %d outside [0,%d)", pass, n_views);
    PSCV_CHECK_ARG(capacity >= 0 && (capacity == 0 || (out_xyz && out_rgb)), "pscv_fuse_depth_pass: bad output buffer (capacity %ld)",
                   capacity);
    PSCV_CHECK_ARG(num_consistent >= 0, "pscv_fuse_depth_pass: num_consistent=%d < 0", num_consistent);
    FuseArgs a;
    if (fill_views(a, what, depth, hw, n_views) || fill_view_ptrs(a.color, what, color, n_views) ||
        fill_view_ptrs(a.used, what, used, n_views))
        return -1;
    const int h = a.h[pass], w = a.w[pass];
    const long nseg = fuse_nseg(h, w);
    PSCV_CHECK_ARG(workspace_bytes >= pscv_fuse_depth_workspace(h, w), "pscv_fuse_depth_pass: workspace of %ld bytes < %ld",
                   workspace_bytes, pscv_fuse_depth_workspace(h, w));
    char* ws = static_cast<char*>(workspace);
    int* seg_count = reinterpret_cast<int*>(ws);
    long long* seg_off = reinterpret_cast<long long*>(ws + align256(nseg * 4));
    float4* stage = reinterpret_cast<float4*>(ws + align256(nseg * 4) + align256(nseg * 8));
    a.cams = cams;
    a.seg_count = seg_count;
    a.stage = stage;
    a.n = n_views; a.i = pass; a.nsx = (w + FUSE_TW - 1) / FUSE_TW; a.need = num_consistent;
    a.disp_thresh = disp_thresh; a.depth_min = depth_min; a.depth_max = depth_max;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc = launch("pscv_fuse_depth_pass (fuse)", fuse_depth_kernel, dim3((unsigned)a.nsx, (unsigned)((h + FUSE_TH - 1) / FUSE_TH)),
                    dim3(FUSE_THREADS), 0, s, a);
    if (rc) return rc;
    PSCV_CHECK_ARG(nseg < (1L << 31), "pscv_fuse_depth_pass: %ld segments", nseg);
    rc = launch("pscv_fuse_depth_pass (scan)", scan_kernel<FUSE_SCAN_THREADS, long long, true>, dim3(1), dim3(FUSE_SCAN_THREADS), 0, s,
                seg_count, seg_off, counter, (int)nseg);
    if (rc) return rc;
    const long nslot = nseg * FUSE_TW;
    return launch("pscv_fuse_depth_pass (scatter)", fuse_scatter_kernel, dim3((unsigned)((nslot + 255) / 256)), dim3(256), 0, s, seg_count,
                  seg_off, stage, nslot, pass, a.nsx, w, (long long)capacity, out_xyz, out_rgb, out_view, out_pixel);
}
