// View covisibility from depth maps: for every ordered pair (v, u) of V views, how many samples of v's depth map land inside u's
// map ("seen") and how many of those agree with u's depth there ("consistent").  The overlap graph of the COLMAP-style fusion
// without a sparse model ("Overlap without a sparse model").  gfx950.
//
// The rule is phase A of colmap_fusion.hip, read there and shared through geo_common.h (cf_unproject, cf_project, cf_depth_ok,
// CF_PIX_LIMIT), so that "seen" means "phase A would look there":
//   * a pixel is the integer pair (col, row) itself, no half-pixel offset; geometry in fp64 from the fp32 inputs, no contractions
//     (the Makefile builds this file with -ffp-contract=off, like colmap_fusion.hip);
//   * q = K_u (R_u X + t_u); seen when q_z > 0, |q_x / q_z| and |q_y / q_z| < 2^30 and the pixel (round(q_x / q_z), round(q_y / q_z)),
//     C `round` (half away from zero), lies in [0, w_u) x [0, h_u);
//   * consistent when u's depth d_u there is valid (0 < d_u finite) and |(q_z - d_u) / d_u| <= max_depth_error.
//
// Mapping: a workgroup of 256 lanes owns 256 consecutive samples (row-major over the stride grid) of one source view; a lane
// unprojects its sample once and keeps the world point in registers.  The targets are swept in chunks of VC_CHUNK views: the
// chunk's camera blocks and view-table rows are staged in LDS, every lane projects into each target, a wave reduces its two
// counts with a ballot and a population count, lane 0 adds them to an LDS [VC_CHUNK][2] table, and after the chunk 2 x VC_CHUNK
// lanes flush the table with one global atomicAdd per non-zero (v, u, k): 512 contiguous bytes, no per-sample global atomics.
// Integer adds: the result does not depend on their order.  V is bounded only by the grid (2^31 - 1).
//
// The per-view table (depth pointer, h, w) lives in the caller's workspace: V has no cap, so it cannot travel as a kernel argument;
// it is written there PSCV_FUSE_MAX_VIEWS rows at a time by a launch that carries the rows as arguments (stream-ordered, no host
// buffer has to outlive the call).
#include "geo_common.h"

namespace pscv {

constexpr int VC_THREADS = 256;
constexpr int VC_CHUNK = 64;                  // targets in flight: 64 x 30 floats of cameras + 64 table rows + 128 counters = 9 KB of LDS
constexpr int VC_MAX_TILES = 65535;           // gridDim.y

struct VcView {                               // one row of the device view table
    const float* depth;                       // [h, w], 0 = invalid
    int h, w;
};
static_assert(sizeof(VcView) == 16, "a table row is 16 bytes");

struct VcRows {                               // PSCV_FUSE_MAX_VIEWS rows of the table as a kernel argument
    const float* depth[PSCV_FUSE_MAX_VIEWS];
    int h[PSCV_FUSE_MAX_VIEWS], w[PSCV_FUSE_MAX_VIEWS];
};

__global__ __launch_bounds__(PSCV_FUSE_MAX_VIEWS) void covis_table_kernel(const VcRows r, VcView* table, int first, int n) {
    const int k = threadIdx.x;
    if (k < n) table[first + k] = VcView{r.depth[k], r.h[k], r.w[k]};
}

__global__ __launch_bounds__(VC_THREADS) void covis_zero_kernel(int* counts, long n) {
    for (long k = (long)blockIdx.x * VC_THREADS + threadIdx.x; k < n; k += (long)gridDim.x * VC_THREADS) counts[k] = 0;
}

__global__ __launch_bounds__(VC_THREADS) void view_covis_kernel(const VcView* __restrict__ table, const float* __restrict__ cams,
                                                                int* counts, int V, int stride, double max_depth_error) {
    __shared__ float cam[VC_CHUNK * PSCV_GEO_CAM_FLOATS];
    __shared__ VcView tv[VC_CHUNK];
    __shared__ int tab[2 * VC_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63;
    const int v = blockIdx.x;
    const VcView me = table[v];
    const int ns_w = (me.w + stride - 1) / stride, ns_h = (me.h + stride - 1) / stride;
    const long ns = (long)ns_h * ns_w;
    const long s0 = (long)blockIdx.y * VC_THREADS;
    if (s0 >= ns) return;                                         // (the grid is sized for the largest view)
    const long s = s0 + tid;
    bool valid = s < ns;
    double X = 0.0, Y = 0.0, Z = 0.0;
    if (valid) {
        const int row = (int)(s / ns_w) * stride, col = (int)(s % ns_w) * stride;
        const float d = me.depth[(long)row * me.w + col];
        valid = cf_depth_ok(d);
        if (valid) cf_unproject(cams + (long)v * PSCV_GEO_CAM_FLOATS, (double)col, (double)row, (double)d, X, Y, Z);
    }
    if (!__syncthreads_or(valid ? 1 : 0)) return;                 // no sample in this tile: nothing to add

    for (int u0 = 0; u0 < V; u0 += VC_CHUNK) {
        const int nt = min(VC_CHUNK, V - u0);
        const float* src = cams + (long)u0 * PSCV_GEO_CAM_FLOATS;
        for (int k = tid; k < nt * PSCV_GEO_CAM_FLOATS; k += VC_THREADS) cam[k] = src[k];
        if (tid < nt) tv[tid] = table[u0 + tid];
        if (tid < 2 * VC_CHUNK) tab[tid] = 0;
        __syncthreads();
        for (int t = 0; t < nt; ++t) {
            if (u0 + t == v) continue;
            bool seen = false, cons = false;
            if (valid) {
                double x, y, z;
                cf_project(cam + t * PSCV_GEO_CAM_FLOATS, X, Y, Z, x, y, z);
                const double pu = x / z, pv = y / z;
                if (z > 0.0 && fabs(pu) < CF_PIX_LIMIT && fabs(pv) < CF_PIX_LIMIT) {
                    const int col = (int)round(pu), row = (int)round(pv);
                    const int hu = tv[t].h, wu = tv[t].w;
                    if (col >= 0 && col < wu && row >= 0 && row < hu) {
                        seen = true;
                        const float dq = tv[t].depth[(long)row * wu + col];
                        if (cf_depth_ok(dq)) {
                            const double dd = (double)dq;
                            cons = fabs((z - dd) / dd) <= max_depth_error;
                        }
                    }
                }
            }
            const unsigned long long bs = __ballot(seen);
            if (bs != 0ull) {                                     // (wave-uniform)
                const unsigned long long bc = __ballot(cons);
                if (lane == 0) {
                    atomicAdd(&tab[2 * t], __popcll(bs));
                    if (bc != 0ull) atomicAdd(&tab[2 * t + 1], __popcll(bc));
                }
            }
        }
        __syncthreads();
        if (tid < 2 * nt) {
            const int c = tab[tid];
            if (c != 0) atomicAdd(&counts[((long)v * V + u0) * 2 + tid], c);
        }
        __syncthreads();                                          // the next chunk overwrites cam, tv and tab
    }
}

}  // namespace pscv

extern "C" long pscv_view_covisibility_workspace(int n_views) {
    if (n_views < 2) return -1;
    return pscv::align256((long)n_views * (long)sizeof(pscv::VcView));
}

extern "C" int pscv_view_covisibility(const float* const* depth, const int* hw, int n_views, const float* cams, int stride,
                                      float max_depth_error, int* counts, void* workspace, long workspace_bytes, void* stream) {
    using namespace pscv;
    const char* what = "pscv_view_covisibility";
    PSCV_CHECK_ARG(depth && hw && cams && counts && workspace, "%s: null pointer argument", what);
    PSCV_CHECK_ARG(n_views >= 2, "%s: n_views=%d < 2", what, n_views);
    PSCV_CHECK_ARG(stride >= 1, "%s: stride=%d < 1", what, stride);
    PSCV_CHECK_ARG(max_depth_error > 0.0f && max_depth_error < 1.0f, "%s: max_depth_error=%g outside (0,1)", what,
                   (double)max_depth_error);
    PSCV_CHECK_ARG(workspace_bytes >= pscv_view_covisibility_workspace(n_views), "%s: workspace of %ld bytes < %ld", what,
                   workspace_bytes, pscv_view_covisibility_workspace(n_views));
    // The views go through a VcRows PSCV_FUSE_MAX_VIEWS at a time, twice: the first pass checks them and sizes the grid, so that
    // nothing is launched for a bad view; the second uploads the table.
    VcRows r;
    long max_samples = 0;
    for (int first = 0; first < n_views; first += PSCV_FUSE_MAX_VIEWS) {
        const int n = n_views - first < PSCV_FUSE_MAX_VIEWS ? n_views - first : PSCV_FUSE_MAX_VIEWS;
        if (fill_views(r, what, depth, hw, n, first)) return -1;
        for (int k = 0; k < n; ++k) {
            const long ns = (long)((r.h[k] + stride - 1) / stride) * ((r.w[k] + stride - 1) / stride);
            if (ns > max_samples) max_samples = ns;
        }
    }
    const long tiles = (max_samples + VC_THREADS - 1) / VC_THREADS;
    PSCV_CHECK_ARG(tiles <= VC_MAX_TILES, "%s: %ld samples in one view: more than %d tiles of %d (raise the stride)", what,
                   max_samples, VC_MAX_TILES, VC_THREADS);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    VcView* table = static_cast<VcView*>(workspace);
    for (int first = 0; first < n_views; first += PSCV_FUSE_MAX_VIEWS) {
        const int n = n_views - first < PSCV_FUSE_MAX_VIEWS ? n_views - first : PSCV_FUSE_MAX_VIEWS;
        if (fill_views(r, what, depth, hw, n, first)) return -1;
        const int rc = launch(what, covis_table_kernel, dim3(1), dim3(PSCV_FUSE_MAX_VIEWS), 0, st, r, table, first, n);
        if (rc) return rc;
    }
    const long ncount = (long)n_views * n_views * 2;
    const long zb = (ncount + VC_THREADS - 1) / VC_THREADS;
    const int rc = launch(what, covis_zero_kernel, dim3((unsigned)(zb < 4096 ? zb : 4096)), dim3(VC_THREADS), 0, st, counts, ncount);
    if (rc) return rc;
    return launch(what, view_covis_kernel, dim3((unsigned)n_views, (unsigned)tiles), dim3(VC_THREADS), 0, st, table, cams, counts, n_views,
                  stride, (double)max_depth_error);
}
