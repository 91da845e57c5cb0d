// Scene set-up from a COLMAP sparse model: the pair counts behind the source-view selection (utils/colmap_utils.py:
// compute_src_imgs), the per-image depth ranges (compute_min_max_depth_yao), INTEGRATION.md section 2i, and the visible depth
// ranges of image tuples (compute_min_max_depth_visible), section 2j.  gfx950.
//
// ---- pscv_sparse_pair_counts ------------------------------------------------------------------------------------------
// The reference builds, for all N images at once,
//     R_rel[i,j]          = R[j] R[i]^T                      "from i to j"
//     t_rel[i,j]          = t[j] - R_rel[i,j] t[i]
//     rel_opt_center[i,j] = R_rel[i,j]^T t_rel[i,j]          = R[i] R[j]^T t[j] - R[i] R[j]^T R[j] R[i]^T t[i]
// and then, for every 3-D point X with track T (a set of images), for every ORDERED pair (i, j) in T x T
//     adj[i,j]     += 1                                       (the diagonal too: adj[i,i] = the points image i observes)
//     adj_tri[i,j] += 1  when  angle(X, X + rel_opt_center[i,j]) > min_triangulation_angle,
//     angle(u, v) = acos(clip(u.v / |u| / |v|, -1, 1)) 180 / pi.
// This is NOT the triangulation angle at X: it is the angle, seen from the world origin, between the point and the point moved
// by the centre of camera j expressed in camera i's frame (with the sign flipped).  It is restated here as it stands, not
// repaired.  With R[j]^T R[j] = I the second term of rel_opt_center is t[i], so the kernel evaluates
//     c[i,j] = R[i] (R[j]^T t[j]) - t[i]
// per pair, in fp64 from the fp32 R and t (the reference's fp32 products and the rounding of R^T R differ from this by a few
// 1e-7 of |t|, far inside the margin the test fixture asserts around the threshold).  On the diagonal c[i,i] is rounding noise
// and the reference's angle is never above any positive threshold: adj_tri[i,i] is not counted.
// A NaN cosine (X = 0, or X + c = 0) fails the test, as `NaN > x` does in the reference.
//
// Mapping: a workgroup of 256 lanes takes SP_WAVES = 4 consecutive points.  Phase 1: ONE POINT PER WAVE for tracks of at most 64
// images; the 64 lanes walk the L x L ordered pairs k = a L + b with stride 64.  Phase 2: a track longer than 64 images is
// walked by the WHOLE WORKGROUP, stride 256 (a wave alone would take L^2 / 64 rounds while its three neighbours idle).  R and t
// are read from global memory for every pair (N x 48 bytes: cache-resident), nothing of size N x N is precomputed.  Every
// pair ends in one or two global int32 atomicAdd: integers, so the matrices do not depend on the order of the adds.
// Not done, and unmeasured: w = R[j]^T t[j] depends on j alone and could come from an [N,3] fp64 pre-pass instead of 9 loads
// and 9 multiply-adds per pair; it would need a workspace, and the kernel is expected to be bound by its atomics.
//
// ---- pscv_sparse_obs_depths, pscv_segment_percentiles ----------------------------------------------------------------
// utils_3D.project: depth = ((R x + t) K^T)_z + 1e-6 with K's last row (0, 0, 1), i.e. (R x + t).z + 1e-6 in fp64 (x fp64, R and
// t fp32).  One lane per observation writes the 64-bit key (image << 32 | ordered bits of the fp32 depth; image < 2^31, so the keys
// order alike as signed and as unsigned 64-bit integers); the caller sorts the
// keys, after which image i's depths are the ascending run [seg_off[i], seg_off[i+1]).  One lane per image then evaluates
// numpy's percentile (method "linear"): virtual index (n - 1) q, lerp of the two neighbours as numpy's _lerp does.
//
// ---- pscv_tuple_visible_depths ---------------------------------------------------------------------------------------
// compute_min_max_depth_visible for T tuples of V images at once (the MegaDepth tuple mining).  A point
// takes part in tuple k when at least 3 of the tuple's images are in its track; it is then projected into ALL V views,
//     y = R x + t,  u = K y,  depth = u_z + 1e-6,  proj = u_xy / depth      (fp64 from the fp32 K, R, t; no fused multiply-adds)
// and is valid in a view iff 0 <= proj_x < w, 0 <= proj_y < h and depth > 0 (NaN fails).  Per (tuple, view): the smallest and the
// largest valid depth and the LOWEST row of xyz that attains each (numpy's nanargmin / nanargmax over the participating points).
// Mapping: grid (chunks of TVD_THREADS * TVD_ITERS points, T).  A workgroup keeps its tuple's membership bitmask (one bit per
// image, ceil(N / 32) words) and the V cameras in LDS; each lane walks one point's track against the mask and, from 3 hits on,
// projects into the V views.  Pass 1 takes the minimum / maximum of the ORDERED BITS of the fp64 depths: a lane reads the
// workgroup's running value from LDS and issues a 64-bit LDS atomic only when its own key improves it (the value moves one way
// only, so a stale read costs an atomic, never a result), and each workgroup ends with one global 64-bit atomic per view and
// bound.  Pass 2 repeats the walk with the identical arithmetic and takes the minimum ROW among the points whose key equals the
// winner (fp64 depth plus a row do not fit one 64-bit key).  min / max of integers: no result depends on the order of the atomics.
// A lane walks its whole track alone, however long; tracks are short on average and the walk is one LDS read per observation.
#include <vector>

#include "pscv_common.h"

namespace pscv {

constexpr int SP_THREADS = 256;
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr int SP_WAVE_TRACK = 64;             // longest track a single wave walks

__global__ __launch_bounds__(SP_THREADS) void sparse_zero_kernel(int* a, int* b, long n) {
    for (long k = (long)blockIdx.x * SP_THREADS + threadIdx.x; k < n; k += (long)gridDim.x * SP_THREADS) {
        a[k] = 0;
        b[k] = 0;
    }
}

// the ordered pair (ia, ib) of one point: both counters
__device__ __forceinline__ void sp_pair(const double X, const double Y, const double Z, const double n1, int ia, int ib,
                                        const float* __restrict__ R, const float* __restrict__ t, int N, double min_angle,
                                        int* adj, int* adj_tri) {
    if ((unsigned)ia >= (unsigned)N || (unsigned)ib >= (unsigned)N) return;      // (the host checks; never write out of bounds)
    const long o = (long)ia * N + ib;
    atomicAdd(adj + o, 1);
    if (ia == ib) return;
    const float* Ra = R + (long)ia * 9;
    const float* Rb = R + (long)ib * 9;
    const float* ta = t + (long)ia * 3;
    const float* tb = t + (long)ib * 3;
    const double bx = tb[0], by = tb[1], bz = tb[2];
    // w = R[j]^T t[j]
    const double wx = (double)Rb[0] * bx + (double)Rb[3] * by + (double)Rb[6] * bz;
    const double wy = (double)Rb[1] * bx + (double)Rb[4] * by + (double)Rb[7] * bz;
    const double wz = (double)Rb[2] * bx + (double)Rb[5] * by + (double)Rb[8] * bz;
    // ray2 = X + R[i] w - t[i]
    const double rx = X + ((double)Ra[0] * wx + (double)Ra[1] * wy + (double)Ra[2] * wz - (double)ta[0]);
    const double ry = Y + ((double)Ra[3] * wx + (double)Ra[4] * wy + (double)Ra[5] * wz - (double)ta[1]);
    const double rz = Z + ((double)Ra[6] * wx + (double)Ra[7] * wy + (double)Ra[8] * wz - (double)ta[2]);
    const double n2 = sqrt(rx * rx + ry * ry + rz * rz);
    double c = (X * rx + Y * ry + Z * rz) / n1 / n2;
    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);                                   // (NaN stays NaN)
    const double angle = acos(c) / 3.141592653589793 * 180.0;
    if (angle > min_angle) atomicAdd(adj_tri + o, 1);
}

__global__ __launch_bounds__(SP_THREADS) void sparse_pair_counts_kernel(const double* __restrict__ xyz, const long* __restrict__ track_off,
                                                                        const int* __restrict__ track_img, long P, long nnz,
                                                                        const float* __restrict__ R, const float* __restrict__ t, int N,
                                                                        double min_angle, int* adj, int* adj_tri) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long p0 = (long)blockIdx.x * SP_WAVES;
    // phase 1: one short track per wave
    {
        const long p = p0 + wave;
        if (p < P) {
            const long beg = track_off[p], end = track_off[p + 1];
            const long L = end - beg;
            if (beg >= 0 && end <= nnz && L >= 1 && L <= SP_WAVE_TRACK) {
                const double X = xyz[3 * p], Y = xyz[3 * p + 1], Z = xyz[3 * p + 2];
                const double n1 = sqrt(X * X + Y * Y + Z * Z);
                const int l = (int)L;
                const int* tr = track_img + beg;
                for (int k = lane; k < l * l; k += 64) {
                    const int a = k / l, b = k - a * l;
                    sp_pair(X, Y, Z, n1, tr[a], tr[b], R, t, N, min_angle, adj, adj_tri);
                }
            }
        }
    }
    // phase 2: every long track of the four by the whole workgroup (the branch is uniform: it depends on the point alone)
    for (int w = 0; w < SP_WAVES; ++w) {
        const long p = p0 + w;
        if (p >= P) break;
        const long beg = track_off[p], end = track_off[p + 1];
        const long L = end - beg;
        if (beg < 0 || end > nnz || L <= SP_WAVE_TRACK || L > N) continue;     // (L > N: not de-duplicated, skipped)
        const double X = xyz[3 * p], Y = xyz[3 * p + 1], Z = xyz[3 * p + 2];
        const double n1 = sqrt(X * X + Y * Y + Z * Z);
        const int* tr = track_img + beg;
        const int l = (int)L;                                     // l <= N <= 46340: l * l + SP_THREADS fits 32 bits
        for (int k = tid; k < l * l; k += SP_THREADS) {
            const int a = k / l, b = k - a * l;
            sp_pair(X, Y, Z, n1, tr[a], tr[b], R, t, N, min_angle, adj, adj_tri);
        }
    }
}

// fp32 -> 32 bits that order like the values (negative numbers below positive ones)
__device__ __forceinline__ unsigned sp_ordered_bits(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sp_from_ordered_bits(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

__global__ __launch_bounds__(SP_THREADS) void sparse_obs_depths_kernel(const double* __restrict__ xyz, long P, const int* __restrict__ obs_img,
                                                                       const int* __restrict__ obs_pt, long M, const float* __restrict__ R,
                                                                       const float* __restrict__ t, int N, unsigned long long* __restrict__ keys) {
    const long k = (long)blockIdx.x * SP_THREADS + threadIdx.x;
    if (k >= M) return;
    const int i = obs_img[k], p = obs_pt[k];
    unsigned long long key = 0x7fffffffffffffffull;                              // an index out of range: behind every image, signed or unsigned
    if ((unsigned)i < (unsigned)N && p >= 0 && (long)p < P) {
        const float* Ri = R + (long)i * 9;
        const double z = xyz[3 * (long)p] * (double)Ri[6] + xyz[3 * (long)p + 1] * (double)Ri[7] + xyz[3 * (long)p + 2] * (double)Ri[8]
                         + (double)t[(long)i * 3 + 2];
        key = ((unsigned long long)(unsigned)i << 32) | sp_ordered_bits((float)(z + 1e-6));
    }
    keys[k] = key;
}

__device__ __forceinline__ double sp_percentile(const unsigned long long* __restrict__ keys, long beg, long n, double q) {
    const double vi = (double)(n - 1) * q;                                       // numpy's virtual index of method "linear"
    double fl = floor(vi);
    double g = vi - fl;
    long prev = (long)fl;
    if (prev < 0) { prev = 0; g = 0.0; }
    if (prev > n - 1) { prev = n - 1; g = 0.0; }
    const long next = prev + 1 < n ? prev + 1 : n - 1;
    const double a = (double)sp_from_ordered_bits((unsigned)keys[beg + prev]);
    const double b = (double)sp_from_ordered_bits((unsigned)keys[beg + next]);
    const double diff = b - a;
    return g >= 0.5 ? b - diff * (1.0 - g) : a + diff * g;
}

__global__ __launch_bounds__(SP_THREADS) void segment_percentiles_kernel(const unsigned long long* __restrict__ keys, long M,
                                                                         const long* __restrict__ seg_off, int N, double q_lo, double q_hi,
                                                                         double* __restrict__ out_lo, double* __restrict__ out_hi) {
    const int i = blockIdx.x * SP_THREADS + threadIdx.x;
    if (i >= N) return;
    const long beg = seg_off[i], end = seg_off[i + 1];
    double lo = 0.0, hi = 0.0;                                                   // an image without observations: 0, 0
    if (beg >= 0 && end <= M && end > beg) {
        lo = sp_percentile(keys, beg, end - beg, q_lo);
        hi = sp_percentile(keys, beg, end - beg, q_hi);
    }
    out_lo[i] = lo;
    out_hi[i] = hi;
}

// ---- visible depth ranges of tuples ------------------------------------------------------------------------------------------
constexpr int TVD_THREADS = 256;
constexpr int TVD_ITERS = 8;                                   // points per lane: one mask / camera set-up per 2048 points
constexpr int TVD_MAX_VIEWS = 32;
constexpr int TVD_MAX_IMAGES = 46340;
constexpr int TVD_MASK_WORDS = (TVD_MAX_IMAGES + 31) / 32;
constexpr unsigned long long TVD_NONE = ~0ull;                 // "no key yet" of a minimum; a maximum starts at 0

struct TvdCam {
    float K[9], R[9], t[3];
    int ok;                                                    // 0: the tuple's index is out of range (the host checks): no point is valid
    double w, h;
};

// fp64 -> 64 bits that order like the values
__device__ __forceinline__ unsigned long long tvd_ordered_bits(double d) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double tvd_from_ordered_bits(unsigned long long o) {
    return __longlong_as_double((long long)((o >> 63) ? (o & 0x7fffffffffffffffull) : ~o));
}

// depth of x in the view and whether it is valid there; both passes call this, so their depths agree bit for bit
__device__ __forceinline__ bool tvd_project(const TvdCam& c, double X, double Y, double Z, double& depth) {
#pragma clang fp contract(off)
    const double x = (double)c.R[0] * X + (double)c.R[1] * Y + (double)c.R[2] * Z + (double)c.t[0];
    const double y = (double)c.R[3] * X + (double)c.R[4] * Y + (double)c.R[5] * Z + (double)c.t[1];
    const double z = (double)c.R[6] * X + (double)c.R[7] * Y + (double)c.R[8] * Z + (double)c.t[2];
    const double u = (double)c.K[0] * x + (double)c.K[1] * y + (double)c.K[2] * z;
    const double v = (double)c.K[3] * x + (double)c.K[4] * y + (double)c.K[5] * z;
    depth = (double)c.K[6] * x + (double)c.K[7] * y + (double)c.K[8] * z + 1e-6;
    const double px = u / depth, py = v / depth;
    return c.ok && px >= 0.0 && py >= 0.0 && px < c.w && py < c.h && depth > 0.0;    // (a NaN fails every comparison)
}

__device__ __forceinline__ unsigned long long tvd_peek(const unsigned long long* a) {
    return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ws: four planes of T * V 64-bit words -- the minimum's key, the maximum's key, the minimum's row, the maximum's row
__global__ __launch_bounds__(TVD_THREADS) void tuple_visible_init_kernel(unsigned long long* ws, int* n_pts, long TV, int T) {
    const long k = (long)blockIdx.x * TVD_THREADS + threadIdx.x;
    if (k < TV) {
        ws[k] = TVD_NONE;
        ws[TV + k] = 0;
        ws[2 * TV + k] = TVD_NONE;
        ws[3 * TV + k] = TVD_NONE;
    }
    if (k < T) n_pts[k] = 0;
}

template <int PASS>
__global__ __launch_bounds__(TVD_THREADS) void tuple_visible_kernel(const double* __restrict__ xyz, const long* __restrict__ track_off,
                                                                    const int* __restrict__ track_img, long P, long nnz,
                                                                    const int* __restrict__ tuples, const float* __restrict__ K,
                                                                    const float* __restrict__ R, const float* __restrict__ t,
                                                                    const double* __restrict__ sizes, int N, int V,
                                                                    unsigned long long* ws, int* n_pts) {
    __shared__ unsigned mask[TVD_MASK_WORDS];
    __shared__ TvdCam cam[TVD_MAX_VIEWS];
    __shared__ unsigned long long lo[TVD_MAX_VIEWS], hi[TVD_MAX_VIEWS];          // pass 1: keys; pass 2: rows
    __shared__ unsigned long long want_lo[TVD_MAX_VIEWS], want_hi[TVD_MAX_VIEWS];  // pass 2: the winning keys
    __shared__ int cnt;
    const int tid = threadIdx.x;
    const long kv = (long)blockIdx.y * V, TV = (long)gridDim.y * V;
    for (int i = tid; i < ((N + 31) >> 5); i += TVD_THREADS) mask[i] = 0;
    if (tid == 0) cnt = 0;
    __syncthreads();
    if (tid < V) {
        const int idx = tuples[kv + tid];
        TvdCam& c = cam[tid];
        c.ok = (unsigned)idx < (unsigned)N;
        if (c.ok) atomicOr(&mask[idx >> 5], 1u << (idx & 31));
        for (int e = 0; e < 9; ++e) {
            c.K[e] = K[(kv + tid) * 9 + e];
            c.R[e] = c.ok ? R[(long)idx * 9 + e] : 0.f;
        }
        for (int e = 0; e < 3; ++e) c.t[e] = c.ok ? t[(long)idx * 3 + e] : 0.f;
        c.w = sizes[(kv + tid) * 2];
        c.h = sizes[(kv + tid) * 2 + 1];
        lo[tid] = TVD_NONE;
        hi[tid] = PASS == 1 ? 0 : TVD_NONE;
        if (PASS == 2) {
            want_lo[tid] = ws[kv + tid];
            want_hi[tid] = ws[TV + kv + tid];
        }
    }
    __syncthreads();
    const long base = (long)blockIdx.x * (TVD_THREADS * TVD_ITERS);
    int mine = 0;
    for (int it = 0; it < TVD_ITERS; ++it) {
        const long p = base + (long)it * TVD_THREADS + tid;
        if (p >= P) break;
        const long beg = track_off[p], end = track_off[p + 1];
        if (beg < 0 || end > nnz || end - beg < 3) continue;
        int hits = 0;
        for (long q = beg; q < end; ++q) {
            const unsigned i = (unsigned)track_img[q];
            if (i < (unsigned)N) hits += (mask[i >> 5] >> (i & 31)) & 1u;
        }
        if (hits < 3) continue;
        ++mine;
        const double X = xyz[3 * p], Y = xyz[3 * p + 1], Z = xyz[3 * p + 2];
        for (int v = 0; v < V; ++v) {
            double depth;
            if (!tvd_project(cam[v], X, Y, Z, depth)) continue;
            const unsigned long long key = tvd_ordered_bits(depth);
            if (PASS == 1) {
                if (key < tvd_peek(&lo[v])) atomicMin(&lo[v], key);
                if (key > tvd_peek(&hi[v])) atomicMax(&hi[v], key);
            } else {
                const unsigned long long row = (unsigned long long)p;
                if (key == want_lo[v] && row < tvd_peek(&lo[v])) atomicMin(&lo[v], row);
                if (key == want_hi[v] && row < tvd_peek(&hi[v])) atomicMin(&hi[v], row);
            }
        }
    }
    if (PASS == 1 && mine) atomicAdd(&cnt, mine);
    __syncthreads();
    if (tid < V) {
        if (PASS == 1) {
            if (lo[tid] != TVD_NONE) atomicMin(ws + kv + tid, lo[tid]);
            if (hi[tid] != 0) atomicMax(ws + TV + kv + tid, hi[tid]);
        } else {
            if (lo[tid] != TVD_NONE) atomicMin(ws + 2 * TV + kv + tid, lo[tid]);
            if (hi[tid] != TVD_NONE) atomicMin(ws + 3 * TV + kv + tid, hi[tid]);
        }
    }
    if (PASS == 1 && tid == 0 && cnt) atomicAdd(n_pts + blockIdx.y, cnt);
}

__global__ __launch_bounds__(TVD_THREADS) void tuple_visible_finish_kernel(const unsigned long long* __restrict__ ws, long TV,
                                                                           double* __restrict__ min_d, double* __restrict__ max_d,
                                                                           long* __restrict__ min_row, long* __restrict__ max_row) {
    const long k = (long)blockIdx.x * TVD_THREADS + threadIdx.x;
    if (k >= TV) return;
    const bool any = ws[TV + k] != 0 && ws[2 * TV + k] != TVD_NONE && ws[3 * TV + k] != TVD_NONE;     // a view without a valid point
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    min_d[k] = any ? tvd_from_ordered_bits(ws[k]) : nan;
    max_d[k] = any ? tvd_from_ordered_bits(ws[TV + k]) : nan;
    min_row[k] = any ? (long)ws[2 * TV + k] : -1;
    max_row[k] = any ? (long)ws[3 * TV + k] : -1;
}

}  // namespace pscv

extern "C" int pscv_sparse_pair_counts(const double* xyz, const long* track_off, const int* track_img, long n_points, long nnz,
                                       const float* R, const float* t, int n_images, double min_triangulation_angle, int* adj,
                                       int* adj_tri, void* stream) {
    using namespace pscv;
    const char* what = "pscv_sparse_pair_counts";
    PSCV_CHECK_ARG(R && t && adj && adj_tri, "%s: null pointer argument", what);
    PSCV_CHECK_ARG(n_images >= 1 && n_images <= 46340, "%s: n_images=%d outside [1,46340] (an N x N int32 matrix)", what, n_images);
    PSCV_CHECK_ARG(n_points >= 0 && nnz >= 0, "%s: n_points=%ld, nnz=%ld: negative", what, n_points, nnz);
    PSCV_CHECK_ARG(n_points == 0 || (xyz && track_off), "%s: null pointer argument", what);
    PSCV_CHECK_ARG(nnz == 0 || track_img, "%s: null pointer argument", what);
    PSCV_CHECK_ARG(min_triangulation_angle >= 0.0, "%s: min_triangulation_angle=%g < 0 (the diagonal is never counted)", what,
                   min_triangulation_angle);
    const long blocks = (n_points + SP_WAVES - 1) / SP_WAVES;
    PSCV_CHECK_ARG(blocks < (1L << 31), "%s: n_points=%ld: more than 2^31 workgroups", what, n_points);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const long nn = (long)n_images * n_images;
    const long zb = (nn + SP_THREADS - 1) / SP_THREADS;
    int rc = launch(what, sparse_zero_kernel, dim3((unsigned)(zb < 4096 ? zb : 4096)), dim3(SP_THREADS), 0, st, adj, adj_tri, nn);
    if (rc || blocks == 0) return rc;
    return launch(what, sparse_pair_counts_kernel, dim3((unsigned)blocks), dim3(SP_THREADS), 0, st, xyz, track_off, track_img, n_points,
                  nnz, R, t, n_images, min_triangulation_angle, adj, adj_tri);
}

extern "C" int pscv_sparse_obs_depths(const double* xyz, long n_points, const int* obs_img, const int* obs_pt, long n_obs, const float* R,
                                      const float* t, int n_images, unsigned long long* keys, void* stream) {
    using namespace pscv;
    const char* what = "pscv_sparse_obs_depths";
    PSCV_CHECK_ARG(n_images >= 1 && n_points >= 0 && n_obs >= 0, "%s: n_images=%d, n_points=%ld, n_obs=%ld", what, n_images, n_points,
                   n_obs);
    if (n_obs == 0) return 0;
    PSCV_CHECK_ARG(xyz && obs_img && obs_pt && R && t && keys, "%s: null pointer argument", what);
    const long blocks = (n_obs + SP_THREADS - 1) / SP_THREADS;
    PSCV_CHECK_ARG(blocks < (1L << 31), "%s: n_obs=%ld: more than 2^31 workgroups", what, n_obs);
    return launch(what, sparse_obs_depths_kernel, dim3((unsigned)blocks), dim3(SP_THREADS), 0, reinterpret_cast<hipStream_t>(stream), xyz,
                  n_points, obs_img, obs_pt, n_obs, R, t, n_images, keys);
}

extern "C" int pscv_segment_percentiles(const unsigned long long* keys, long n_keys, const long* seg_off, int n_segments, double q_lo,
                                        double q_hi, double* out_lo, double* out_hi, void* stream) {
    using namespace pscv;
    const char* what = "pscv_segment_percentiles";
    PSCV_CHECK_ARG(seg_off && out_lo && out_hi && (keys || n_keys == 0), "%s: null pointer argument", what);
    PSCV_CHECK_ARG(n_segments >= 1 && n_keys >= 0, "%s: n_segments=%d, n_keys=%ld", what, n_segments, n_keys);
    PSCV_CHECK_ARG(q_lo >= 0.0 && q_lo <= 1.0 && q_hi >= 0.0 && q_hi <= 1.0, "%s: quantiles %g, %g outside [0,1]", what, q_lo, q_hi);
    return launch(what, segment_percentiles_kernel, dim3((unsigned)((n_segments + SP_THREADS - 1) / SP_THREADS)), dim3(SP_THREADS), 0,
                  reinterpret_cast<hipStream_t>(stream), keys, n_keys, seg_off, n_segments, q_lo, q_hi, out_lo, out_hi);
}

extern "C" long pscv_tuple_visible_depths_workspace(int n_tuples, int n_views) {
    if (n_tuples < 1 || n_views < 1) return 0;
    return 4L * (long)sizeof(unsigned long long) * n_tuples * n_views;
}

extern "C" int pscv_tuple_visible_depths(const double* xyz, const long* track_off, const int* track_img, long n_points, long nnz,
                                         const int* tuples, const float* K, const float* R, const float* t, const double* sizes,
                                         int n_images, int T, int V, double* min_d, double* max_d, long* min_row, long* max_row,
                                         int* n_pts, void* workspace, void* stream) {
    using namespace pscv;
    const char* what = "pscv_tuple_visible_depths";
    PSCV_CHECK_ARG(V >= 3 && V <= TVD_MAX_VIEWS, "%s: V=%d outside [3,%d] (a point takes part from 3 of the tuple's views on)", what, V,
                   TVD_MAX_VIEWS);
    PSCV_CHECK_ARG(T >= 1 && T <= 65535, "%s: T=%d outside [1,65535] (one grid row per tuple)", what, T);
    PSCV_CHECK_ARG(n_images >= 1 && n_images <= TVD_MAX_IMAGES, "%s: n_images=%d outside [1,%d] (the membership bitmask in LDS)", what,
                   n_images, TVD_MAX_IMAGES);
    PSCV_CHECK_ARG(n_points >= 0 && nnz >= 0, "%s: n_points=%ld, nnz=%ld: negative", what, n_points, nnz);
    PSCV_CHECK_ARG(tuples && K && R && t && sizes && min_d && max_d && min_row && max_row && n_pts && workspace,
                   "%s: null pointer argument", what);
    PSCV_CHECK_ARG(n_points == 0 || (xyz && track_off), "%s: null pointer argument", what);
    PSCV_CHECK_ARG(nnz == 0 || track_img, "%s: null pointer argument", what);
    const long chunk = (long)TVD_THREADS * TVD_ITERS;
    const long blocks = (n_points + chunk - 1) / chunk;
    PSCV_CHECK_ARG(blocks < (1L << 31), "%s: n_points=%ld: more than 2^31 workgroups", what, n_points);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // the tuples are read back once (T * V ints, one synchronisation of the stream): a repeated index would count a point's
    // observation twice, one out of range has no camera
    const long TV = (long)T * V;
    std::vector<int> host(TV);
    hipError_t e = hipMemcpyAsync(host.data(), tuples, sizeof(int) * TV, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        set_error("%s: reading the tuples back failed: %s", what, hipGetErrorString(e));
        return -2;
    }
    for (int k = 0; k < T; ++k)
        for (int a = 0; a < V; ++a) {
            const int ia = host[(long)k * V + a];
            PSCV_CHECK_ARG(ia >= 0 && ia < n_images, "%s: tuples[%d][%d]=%d outside [0,%d)", what, k, a, ia, n_images);
            for (int b = 0; b < a; ++b)
                PSCV_CHECK_ARG(host[(long)k * V + b] != ia, "%s: tuples[%d] names image %d twice", what, k, ia);
        }
    unsigned long long* ws = static_cast<unsigned long long*>(workspace);
    const long most = TV > T ? TV : (long)T;
    int rc = launch(what, tuple_visible_init_kernel, dim3((unsigned)((most + TVD_THREADS - 1) / TVD_THREADS)), dim3(TVD_THREADS), 0, st, ws,
                    n_pts, TV, T);
    if (rc) return rc;
    if (blocks > 0) {
        const dim3 grid((unsigned)blocks, (unsigned)T);
        rc = launch(what, tuple_visible_kernel<1>, grid, dim3(TVD_THREADS), 0, st, xyz, track_off, track_img, n_points, nnz, tuples, K, R,
                    t, sizes, n_images, V, ws, n_pts);
        if (rc) return rc;
        rc = launch(what, tuple_visible_kernel<2>, grid, dim3(TVD_THREADS), 0, st, xyz, track_off, track_img, n_points, nnz, tuples, K, R,
                    t, sizes, n_images, V, ws, n_pts);
        if (rc) return rc;
    }
    return launch(what, tuple_visible_finish_kernel, dim3((unsigned)((TV + TVD_THREADS - 1) / TVD_THREADS)), dim3(TVD_THREADS), 0, st,
                  (const unsigned long long*)ws, TV, min_d, max_d, min_row, max_row);
}
