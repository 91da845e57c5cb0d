// COLMAP-style stereo fusion of depth maps into one point cloud (the YFCC path of the reconstruction pipeline).  gfx950.
//
// One pass per view i, in FindNextImage order (INTEGRATION.md section 2g states the rule).  All seeds of view i (pixels with
// 0 < d finite, not fused) run in parallel in two phases, each one launch of the same kernel template:
//   A  each seed computes its reachability closure against the fused masks as they were at the start of the pass and claims
//      every pixel it reaches with a 64-bit atomicMin of (pass tag, seed index) on the claim map;
//   B  each seed recomputes its closure over the pixels whose claim is its own, marks its seed pixel and that cluster fused, and
//      when the cluster holds at least min_num_pixels pixels stages one point (exact per-coordinate medians) at its seed's slot.
// Then count (per 64-pixel segment), scan (one workgroup, geo_common.h; the running offset stays on the device) and scatter, as
// in depth_fusion.hip.  Output order is pass-major, then row-major seed order; nothing depends on atomics order or scheduling.
//
// Mapping: a wave holds 64 / P seeds, P = next_pow2(n_views) lanes per seed, lane m of a group owns view m.  The lane projects
// the seed's point X_s into view m once and keeps a bitmask of the (2W+1)^2 window pixels around the projection that pass the
// acceptance tests (W = ceil(max_reproj_error) <= 2: at most 25 bits); every accepted node lies in that window, so the traversal
// is a breadth-first closure over these bits.  A BFS level expands its frontier nodes one per group at a time: the group's
// leader lane unprojects its node, broadcasts it with a shuffle, and every lane whose view the node's view overlaps tests the
// rounded projection against its window.  A level ends on a wave ballot.  Medians are exact radix selections over the ordered
// fp32 keys of the cluster's nodes (staged in LDS), the counts of a group summed with xor shuffles.
//
// Geometry is fp64 from the fp32 inputs with no contractions (the Makefile builds this file with -ffp-contract=off), so the
// numpy restatement in tests/_colmap_fusion_ref.py reproduces every value bit for bit.
//
// With normal maps (NORMALS = true, pscv_colmap_fuse_pass_normals; section 2g "with normal maps"): every view brings an fp32
// [h_v, w_v, 3] normal map in its camera frame.  The world normal of a pixel is w = R_m^T n rounded to fp32; phase A also asks
// w_seed . w_pixel >= min_cos of every candidate that passed the depth and reprojection tests (against the SEED, not the parent
// node, so it is a property of the (seed, pixel) pair and sits in the window scan); phase B, after the xyz and colour selections,
// stages the cluster's world normals over nx_/ny_/nz_ (a second walk of the reach bits) and runs the same selection on them.
// NORMALS = false is the network path as before: a constant normal per view, no normal test, its own kernel arguments.
//
// Replaces (fdarmon/wild_deep_mvs): utils/colmap_utils.py:391-400, the external `colmap stereo_fusion` run.
#include "geo_common.h"

namespace pscv {

constexpr int CF_WAVE = 64;
constexpr int CF_SCAN_THREADS = 1024;
constexpr int CF_AUX_THREADS = 256;

struct CfArgs {
    const float* depth[PSCV_FUSE_MAX_VIEWS];            // [h_v, w_v]
    const uint32_t* color[PSCV_FUSE_MAX_VIEWS];         // [h_v, w_v] RGBA8 (R in the low byte)
    uint8_t* fused[PSCV_FUSE_MAX_VIEWS];                // [h_v, w_v] 0 / 1
    unsigned long long* claim[PSCV_FUSE_MAX_VIEWS];     // [h_v, w_v] (pass tag, seed) keys
    int h[PSCV_FUSE_MAX_VIEWS], w[PSCV_FUSE_MAX_VIEWS];
    unsigned long long overlap[PSCV_FUSE_MAX_VIEWS];    // bit m of overlap[k]: m follows k (diagonal cleared)
    const float* cams;                                  // [n][PSCV_GEO_CAM_FLOATS]: K, K^-1, R (row-major), t
    uint8_t* flag;                                      // [h_i * w_i] 1 = the seed emits
    float4* stage;                                      // [h_i * w_i][2]: x, y, z, RGBA8 bits | nx, ny, nz, 0
    unsigned long long processed, key;                  // key: the pass tag in the high word
    int n, i, lg_p, min_pixels, max_td;
    double max_depth_error, r2;
};
struct CfArgsN : CfArgs {                               // NORMALS = true
    const float* normal[PSCV_FUSE_MAX_VIEWS];           // [h_v, w_v, 3] unit normals in the camera frame of view v (0 = filtered)
    double min_cos;                                     // cos(max_normal_error)
};
static_assert(sizeof(CfArgsN) <= 4096, "the kernel-argument segment holds 4 KB");
template <bool NORMALS> struct CfArgsOf { using type = CfArgs; };
template <> struct CfArgsOf<true> { using type = CfArgsN; };

// window bit of round(P_m X) relative to the window at (c0x, c0y), or -1
template <int W>
__device__ __forceinline__ int cf_target(const float* cm, double X, double Y, double Z, int c0x, int c0y) {
    constexpr int S = 2 * W + 1;
    double x, y, z;
    cf_project(cm, X, Y, Z, x, y, z);
    const double u = x / z, v = y / z;
    if (!(fabs(u) < CF_PIX_LIMIT && fabs(v) < CF_PIX_LIMIT)) return -1;
    const int tx = (int)round(u) - c0x + W, ty = (int)round(v) - c0y + W;
    if (tx < 0 || tx >= S || ty < 0 || ty >= S) return -1;
    return ty * S + tx;
}

__device__ __forceinline__ unsigned long long cf_group_sum(unsigned long long v, int p) {
    for (int o = 1; o < p; o <<= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t cf_fkey(float f) {           // IEEE total order as unsigned integers
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cf_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

template <int W, bool PHASE_B, bool NORMALS>
__global__ __launch_bounds__(CF_WAVE) void colmap_fuse_kernel(const typename CfArgsOf<NORMALS>::type a) {
    constexpr int S = 2 * W + 1, NB = S * S;
    __shared__ float cam[PSCV_FUSE_MAX_VIEWS * PSCV_GEO_CAM_FLOATS];
    __shared__ unsigned long long adj[PSCV_FUSE_MAX_VIEWS];
    // phase B: the lane's cluster nodes (x, y, z, RGBA8), slot-major so that a round's reads hit distinct banks
    __shared__ float nx_[PHASE_B ? NB : 1][CF_WAVE], ny_[PHASE_B ? NB : 1][CF_WAVE], nz_[PHASE_B ? NB : 1][CF_WAVE];
    __shared__ uint32_t nc_[PHASE_B ? NB : 1][CF_WAVE];
    const int lane = threadIdx.x;
    for (int k = lane; k < a.n * PSCV_GEO_CAM_FLOATS; k += CF_WAVE) cam[k] = a.cams[k];
    adj[lane] = lane < a.n ? a.overlap[lane] : 0ull;
    __syncthreads();

    const int P = 1 << a.lg_p, m = lane & (P - 1), base = lane - m;
    const int i = a.i, hi = a.h[i], wi = a.w[i];
    const long s = (long)blockIdx.x * (CF_WAVE >> a.lg_p) + (lane >> a.lg_p);    // seed pixel of this group
    const bool in_view = s < (long)hi * wi;
    const int srow = in_view ? (int)(s / wi) : 0, scol = in_view ? (int)(s - (long)srow * wi) : 0;
    float ds = 0.0f;
    bool seed = false;
    if (in_view) {
        ds = a.depth[i][s];
        seed = cf_depth_ok(ds) && a.fused[i][s] == 0;
    }
    double Xs = 0.0, Ys = 0.0, Zs = 0.0;
    if (seed) cf_unproject(cam + i * PSCV_GEO_CAM_FLOATS, (double)scol, (double)srow, (double)ds, Xs, Ys, Zs);
    // the seed's world normal: phase A tests every candidate against it, phase B stages it as the seed node's
    float wsx = 0.0f, wsy = 0.0f, wsz = 0.0f;
    if constexpr (NORMALS) {
        if (seed) cf_world_normal(cam + i * PSCV_GEO_CAM_FLOATS, a.normal[i] + 3 * s, wsx, wsy, wsz);
    }
    const unsigned long long key = a.key | (unsigned long long)s;   // (pass tag, seed index): the lowest seed wins a pixel
    const bool act = seed && m < a.n && m != i && !((a.processed >> m) & 1ull);
    const float* cm = cam + (m < a.n ? m : 0) * PSCV_GEO_CAM_FLOATS;
    const int hm = a.h[m < a.n ? m : 0], wm = a.w[m < a.n ? m : 0];

    // the window of view m around round(P_m X_s) and its candidate pixels
    int c0x = 0, c0y = 0;
    uint32_t cand = 0;
    if (act) {
        double x, y, z;
        cf_project(cm, Xs, Ys, Zs, x, y, z);
        const double u = x / z, v = y / z;
        // max_depth_error < 1: a pixel with d > 0 can pass the depth test only when z > 0
        if (z > 0.0 && fabs(u) < CF_PIX_LIMIT && fabs(v) < CF_PIX_LIMIT) {
            c0x = (int)round(u);
            c0y = (int)round(v);
            for (int b = 0; b < NB; ++b) {
                const int col = c0x - W + b % S, row = c0y - W + b / S;
                if (col < 0 || col >= wm || row < 0 || row >= hm) continue;
                const long q = (long)row * wm + col;
                if (PHASE_B) {                     // a claim of its own implies every test passed in phase A
                    if (a.claim[m][q] == key) cand |= 1u << b;
                    continue;
                }
                if (a.fused[m][q]) continue;
                const float dq = a.depth[m][q];
                if (!cf_depth_ok(dq)) continue;
                const double dd = (double)dq;
                if (!(fabs((z - dd) / dd) <= a.max_depth_error)) continue;
                const double du = u - (double)col, dv = v - (double)row;
                if (!(du * du + dv * dv <= a.r2)) continue;
                if constexpr (NORMALS) {           // against the seed's normal; NaN fails
                    float wx, wy, wz;
                    cf_world_normal(cm, a.normal[m] + 3 * q, wx, wy, wz);
                    if (!((double)wsx * (double)wx + (double)wsy * (double)wy + (double)wsz * (double)wz >= a.min_cos)) continue;
                }
                cand |= 1u << b;
            }
        }
    }

    // breadth-first closure from the seed (depth 0); a node at depth L is expanded when L + 1 <= max_td - 1
    uint32_t reach = 0, front = 0;
    if (a.max_td >= 2 && cand && ((adj[i] >> m) & 1ull)) {
        const int t = cf_target<W>(cm, Xs, Ys, Zs, c0x, c0y);
        if (t >= 0 && ((cand >> t) & 1u)) reach = front = 1u << t;
    }
    for (int lvl = 1; lvl + 1 <= a.max_td - 1; ++lvl) {
        if (__ballot(front != 0) == 0ull) break;
        uint32_t next = 0;
        while (true) {
            const unsigned long long b = __ballot(front != 0);
            if (b == 0ull) break;
            const unsigned long long gb = (b >> base) & (P == 64 ? ~0ull : ((1ull << P) - 1ull));
            const int leader = gb ? base + __builtin_ctzll(gb) : lane;
            double X = 0.0, Y = 0.0, Z = 0.0;
            if (lane == leader && front) {
                const int bit = __builtin_ctz(front);
                front &= front - 1u;
                const int col = c0x - W + bit % S, row = c0y - W + bit / S;
                cf_unproject(cm, (double)col, (double)row, (double)a.depth[m][(long)row * wm + col], X, Y, Z);
            }
            X = __shfl(X, leader);
            Y = __shfl(Y, leader);
            Z = __shfl(Z, leader);
            const int k = leader - base;
            if (gb && cand && ((adj[k] >> m) & 1ull)) {
                const int t = cf_target<W>(cm, X, Y, Z, c0x, c0y);
                if (t >= 0 && ((cand >> t) & 1u) && !((reach >> t) & 1u)) {
                    reach |= 1u << t;
                    next |= 1u << t;
                }
            }
        }
        front = next;
    }

    if (!PHASE_B) {
        for (uint32_t r = reach; r; r &= r - 1u) {
            const int bit = __builtin_ctz(r);
            const int col = c0x - W + bit % S, row = c0y - W + bit / S;
            atomicMin(&a.claim[m][(long)row * wm + col], key);
        }
        return;
    }

    // phase B: mark, count, stage the cluster's nodes
    int cnt = 0;
    if (seed && m == i) {                                     // the seed is the node of lane i (which never holds another)
        nx_[0][lane] = (float)Xs; ny_[0][lane] = (float)Ys; nz_[0][lane] = (float)Zs;
        nc_[0][lane] = a.color[i][s];
        a.fused[i][s] = 1;
        cnt = 1;
    }
    for (uint32_t r = reach; r; r &= r - 1u) {
        const int bit = __builtin_ctz(r);
        const int col = c0x - W + bit % S, row = c0y - W + bit / S;
        const long q = (long)row * wm + col;
        double X, Y, Z;
        cf_unproject(cm, (double)col, (double)row, (double)a.depth[m][q], X, Y, Z);
        nx_[cnt][lane] = (float)X; ny_[cnt][lane] = (float)Y; nz_[cnt][lane] = (float)Z;
        nc_[cnt][lane] = a.color[m][q];
        a.fused[m][q] = 1;
        ++cnt;
    }
    const int total = (int)cf_group_sum((unsigned long long)cnt, P);
    const bool emit = seed && total >= a.min_pixels;
    // the lane's normal: R_m^T (1, 1, 1) / sqrt(3) rounded to fp32 (the constant normal maps of the reference's network path)
    // (with normal maps the lane's nodes bring their own: staged over nx_/ny_/nz_ after the xyz selection below)
    constexpr double INV_SQRT3 = 0.57735026918962573;
    const float* Rm = cm + CAM_R;
    const float nrm[3] = {(float)((double)Rm[0] * INV_SQRT3 + (double)Rm[3] * INV_SQRT3 + (double)Rm[6] * INV_SQRT3),
                          (float)((double)Rm[1] * INV_SQRT3 + (double)Rm[4] * INV_SQRT3 + (double)Rm[7] * INV_SQRT3),
                          (float)((double)Rm[2] * INV_SQRT3 + (double)Rm[5] * INV_SQRT3 + (double)Rm[8] * INV_SQRT3)};
    const bool any_emit = __ballot(emit) != 0ull;
    float med[3] = {0.0f, 0.0f, 0.0f}, mnr[3] = {0.0f, 0.0f, 0.0f};
    uint32_t mcol[3] = {0, 0, 0};
    if (any_emit) {
        const bool even = (total & 1) == 0;
        const int k0 = (total - 1) / 2;
        uint32_t kx[2][3], kn[2][3], kc[2][3];
        for (int e = 0; e < 2; ++e) {
            // select the (k0 + e)-th smallest key of x, y, z (16-bit count fields; a cluster holds <= 1 + 63 * 25 nodes)
            int kk[3] = {k0 + e, k0 + e, k0 + e};
            uint32_t pre[3] = {0, 0, 0};
            for (int bit = 31; bit >= 0; --bit) {
                unsigned long long c = 0;
                for (int j = 0; j < cnt; ++j) {
                    c += (((cf_fkey(nx_[j][lane]) ^ pre[0]) >> bit) == 0u) ? 1ull : 0ull;
                    c += (((cf_fkey(ny_[j][lane]) ^ pre[1]) >> bit) == 0u) ? (1ull << 16) : 0ull;
                    c += (((cf_fkey(nz_[j][lane]) ^ pre[2]) >> bit) == 0u) ? (1ull << 32) : 0ull;
                }
                c = cf_group_sum(c, P);
                for (int d = 0; d < 3; ++d) {
                    const int cd = (int)((c >> (16 * d)) & 0xffffull);
                    if (kk[d] >= cd) { kk[d] -= cd; pre[d] |= 1u << bit; }
                }
            }
            // the same over the lane's normal, held cnt times
            int kn_[3] = {k0 + e, k0 + e, k0 + e};
            uint32_t pn[3] = {0, 0, 0};
            for (int bit = NORMALS ? -1 : 31; bit >= 0; --bit) {
                unsigned long long c = 0;
                for (int d = 0; d < 3; ++d)
                    c += ((((cf_fkey(nrm[d]) ^ pn[d]) >> bit) == 0u) ? (unsigned long long)cnt : 0ull) << (16 * d);
                c = cf_group_sum(c, P);
                for (int d = 0; d < 3; ++d) {
                    const int cd = (int)((c >> (16 * d)) & 0xffffull);
                    if (kn_[d] >= cd) { kn_[d] -= cd; pn[d] |= 1u << bit; }
                }
            }
            // and over the colour bytes
            int kc_[3] = {k0 + e, k0 + e, k0 + e};
            uint32_t pc[3] = {0, 0, 0};
            for (int bit = 7; bit >= 0; --bit) {
                unsigned long long c = 0;
                for (int j = 0; j < cnt; ++j) {
                    const uint32_t rgba = nc_[j][lane];
                    for (int d = 0; d < 3; ++d)
                        c += (((((rgba >> (8 * d)) & 0xffu) ^ pc[d]) >> bit) == 0u) ? (1ull << (16 * d)) : 0ull;
                }
                c = cf_group_sum(c, P);
                for (int d = 0; d < 3; ++d) {
                    const int cd = (int)((c >> (16 * d)) & 0xffffull);
                    if (kc_[d] >= cd) { kc_[d] -= cd; pc[d] |= 1u << bit; }
                }
            }
            for (int d = 0; d < 3; ++d) { kx[e][d] = pre[d]; kn[e][d] = pn[d]; kc[e][d] = pc[d]; }
            if (__ballot(emit && even) == 0ull) {   // no group needs the upper middle value
                for (int d = 0; d < 3; ++d) { kx[1][d] = pre[d]; kn[1][d] = pn[d]; kc[1][d] = pc[d]; }
                break;
            }
        }
        if constexpr (NORMALS) {
            // the nodes' world normals take the place of their positions (slot-major as before, the seed in slot 0 of lane i and
            // the reach bits in the same order; a lane reads and writes its own column only), then the selection of x, y, z again
            int j = 0;
            if (seed && m == i) { nx_[0][lane] = wsx; ny_[0][lane] = wsy; nz_[0][lane] = wsz; j = 1; }
            for (uint32_t r = reach; r; r &= r - 1u) {
                const int bit = __builtin_ctz(r);
                const int col = c0x - W + bit % S, row = c0y - W + bit / S;
                float wx, wy, wz;
                cf_world_normal(cm, a.normal[m] + 3 * ((long)row * wm + col), wx, wy, wz);
                nx_[j][lane] = wx; ny_[j][lane] = wy; nz_[j][lane] = wz;
                ++j;
            }
            for (int e = 0; e < 2; ++e) {
                int kk[3] = {k0 + e, k0 + e, k0 + e};
                uint32_t pre[3] = {0, 0, 0};
                for (int bit = 31; bit >= 0; --bit) {
                    unsigned long long c = 0;
                    for (int jj = 0; jj < cnt; ++jj) {
                        c += (((cf_fkey(nx_[jj][lane]) ^ pre[0]) >> bit) == 0u) ? 1ull : 0ull;
                        c += (((cf_fkey(ny_[jj][lane]) ^ pre[1]) >> bit) == 0u) ? (1ull << 16) : 0ull;
                        c += (((cf_fkey(nz_[jj][lane]) ^ pre[2]) >> bit) == 0u) ? (1ull << 32) : 0ull;
                    }
                    c = cf_group_sum(c, P);
                    for (int d = 0; d < 3; ++d) {
                        const int cd = (int)((c >> (16 * d)) & 0xffffull);
                        if (kk[d] >= cd) { kk[d] -= cd; pre[d] |= 1u << bit; }
                    }
                }
                for (int d = 0; d < 3; ++d) kn[e][d] = pre[d];
                if (__ballot(emit && even) == 0ull) {
                    for (int d = 0; d < 3; ++d) kn[1][d] = pre[d];
                    break;
                }
            }
        }
        for (int d = 0; d < 3; ++d) {
            if (even) {
                med[d] = (cf_unkey(kx[0][d]) + cf_unkey(kx[1][d])) * 0.5f;
                mnr[d] = (cf_unkey(kn[0][d]) + cf_unkey(kn[1][d])) * 0.5f;
                mcol[d] = (kc[0][d] + kc[1][d] + 1u) >> 1;
            } else {
                med[d] = cf_unkey(kx[0][d]);
                mnr[d] = cf_unkey(kn[0][d]);
                mcol[d] = kc[0][d];
            }
        }
    }
    if (m == 0 && in_view) {
        bool out = false;
        if (emit) {
            const double gx = (double)mnr[0], gy = (double)mnr[1], gz = (double)mnr[2];
            const double norm = sqrt(gx * gx + gy * gy + gz * gz);
            if (norm >= 1.1920928955078125e-07) {             // FLT_EPSILON
                out = true;
                const uint32_t rgba = mcol[0] | (mcol[1] << 8) | (mcol[2] << 16);
                a.stage[2 * s] = make_float4(med[0], med[1], med[2], __uint_as_float(rgba));
                a.stage[2 * s + 1] = make_float4((float)(gx / norm), (float)(gy / norm), (float)(gz / norm), 0.0f);
            }
        }
        a.flag[s] = out ? 1 : 0;
    }
}

// per 64-pixel segment: the number of emitting seeds
__global__ __launch_bounds__(CF_AUX_THREADS) void colmap_count_kernel(const uint8_t* __restrict__ flag, long npix, int* seg_count) {
    const long p = (long)blockIdx.x * CF_AUX_THREADS + threadIdx.x;
    const unsigned long long b = __ballot(p < npix && flag[p] != 0);
    if ((threadIdx.x & 63) == 0 && p < npix) seg_count[p >> 6] = __popcll(b);
}

// one lane per pixel of view i: an emitting seed goes to out[offset[segment] + its rank among the segment's emitting seeds]
__global__ __launch_bounds__(CF_AUX_THREADS) void colmap_scatter_kernel(const uint8_t* __restrict__ flag, const long long* __restrict__ seg_off,
                                                                        const float4* __restrict__ stage, long npix, int view,
                                                                        long long capacity, float* out_xyz, float* out_normal,
                                                                        uint8_t* out_rgb, int* out_view, int* out_pixel) {
    const long p = (long)blockIdx.x * CF_AUX_THREADS + threadIdx.x;
    const bool on = p < npix && flag[p] != 0;
    const unsigned long long b = __ballot(on);
    if (!on) return;
    const int lane = threadIdx.x & 63;
    const long long o = seg_off[p >> 6] + __popcll(b & ((1ull << lane) - 1ull));
    if (o >= capacity) return;
    const float4 q0 = stage[2 * p], q1 = stage[2 * p + 1];
    const uint32_t c = __float_as_uint(q0.w);
    out_xyz[3 * o] = q0.x; out_xyz[3 * o + 1] = q0.y; out_xyz[3 * o + 2] = q0.z;
    if (out_normal) { out_normal[3 * o] = q1.x; out_normal[3 * o + 1] = q1.y; out_normal[3 * o + 2] = q1.z; }
    out_rgb[3 * o] = (uint8_t)(c & 0xffu); out_rgb[3 * o + 1] = (uint8_t)((c >> 8) & 0xffu); out_rgb[3 * o + 2] = (uint8_t)((c >> 16) & 0xffu);
    if (out_view) out_view[o] = view;
    if (out_pixel) out_pixel[o] = (int)p;
}

}  // namespace pscv

namespace {
long cf_nseg(long npix) { return (npix + 63) / 64; }
}

extern "C" long pscv_colmap_fuse_workspace(int h, int w) {
    if (h <= 0 || w <= 0) return -1;
    const long npix = (long)h * w, nseg = cf_nseg(npix);
    // flags uint8, counts int32, offsets int64, staging 2 x float4 per pixel; each part 256-byte aligned
    return pscv::align256(npix) + pscv::align256(nseg * 4) + pscv::align256(nseg * 8) + pscv::align256(npix * 32);
}

namespace {
// one pass: `what` names the entry point in messages; NORMALS adds the normal maps and cos(max_normal_error)
template <bool NORMALS>
int cf_pass(const char* what, int view, int tag, const float* const* depth, const unsigned int* const* color,
            unsigned char* const* fused, unsigned long long* const* claim, const int* hw, int n_views, const float* cams,
            const long* overlap, long processed_mask, float max_depth_error, float max_reproj_error, int min_num_pixels,
            int max_traversal_depth, const float* const* normal, float max_normal_error, float* out_xyz, float* out_normal,
            unsigned char* out_rgb, int* out_view, int* out_pixel, long capacity, long long* counter, void* workspace,
            long workspace_bytes, void* stream) {
    using namespace pscv;
    PSCV_CHECK_ARG(depth && color && fused && claim && hw && cams && overlap && counter && workspace,
                   "%s: null pointer argument", what);
    if (check_view_count(what, n_views, 2)) return -1;
    PSCV_CHECK_ARG(view >= 0 && view < n_views, "%s: view %d outside [0,%d)", what, view, n_views);
    const unsigned long long processed = (unsigned long long)processed_mask;
    PSCV_CHECK_ARG(!((processed >> view) & 1ull), "%s: view %d is already processed", what, view);
    PSCV_CHECK_ARG(max_reproj_error > 0.0f && max_reproj_error <= 2.0f, "%s: max_reproj_error=%g outside (0,2]", what,
                   (double)max_reproj_error);
    PSCV_CHECK_ARG(max_depth_error > 0.0f && max_depth_error < 1.0f, "%s: max_depth_error=%g outside (0,1)", what,
                   (double)max_depth_error);
    PSCV_CHECK_ARG(max_traversal_depth >= 1, "%s: max_traversal_depth=%d < 1", what, max_traversal_depth);
    PSCV_CHECK_ARG(tag >= 0, "%s: tag %d < 0", what, tag);
    PSCV_CHECK_ARG(capacity >= 0 && (capacity == 0 || (out_xyz && out_rgb)), "%s: bad output buffer (capacity %ld)", what,
                   capacity);
    typename CfArgsOf<NORMALS>::type a;
    if (fill_views(a, what, depth, hw, n_views) || fill_view_ptrs(a.color, what, color, n_views) ||
        fill_view_ptrs(a.fused, what, fused, n_views) || fill_view_ptrs(a.claim, what, claim, n_views))
        return -1;
    const unsigned long long all = n_views == 64 ? ~0ull : ((1ull << n_views) - 1ull);
    for (int v = 0; v < PSCV_FUSE_MAX_VIEWS; ++v) a.overlap[v] = v < n_views ? ((unsigned long long)overlap[v] & ~(1ull << v)) & all : 0ull;
    if constexpr (NORMALS) {
        PSCV_CHECK_ARG(normal, "%s: null pointer argument", what);
        PSCV_CHECK_ARG(max_normal_error > 0.0f && max_normal_error <= 180.0f, "%s: max_normal_error=%g outside (0,180] degrees", what,
                       (double)max_normal_error);
        if (fill_view_ptrs(a.normal, what, normal, n_views, "normal map")) return -1;
        a.min_cos = cos((double)max_normal_error * 3.14159265358979323846 / 180.0);
    }
    const long npix = (long)a.h[view] * a.w[view], nseg = cf_nseg(npix);
    PSCV_CHECK_ARG(workspace_bytes >= pscv_colmap_fuse_workspace(a.h[view], a.w[view]),
                   "%s: workspace of %ld bytes < %ld", what, workspace_bytes,
                   pscv_colmap_fuse_workspace(a.h[view], a.w[view]));
    char* ws = static_cast<char*>(workspace);
    a.flag = reinterpret_cast<uint8_t*>(ws);
    int* seg_count = reinterpret_cast<int*>(ws + align256(npix));
    long long* seg_off = reinterpret_cast<long long*>(ws + align256(npix) + align256(nseg * 4));
    a.stage = reinterpret_cast<float4*>(ws + align256(npix) + align256(nseg * 4) + align256(nseg * 8));
    a.cams = cams;
    a.processed = processed;
    a.key = ((unsigned long long)(0xffffffffu - (unsigned)tag) << 32);   // an earlier (lower) tag has a larger key and loses every atomicMin
    a.n = n_views; a.i = view;
    a.lg_p = 1;
    while ((1 << a.lg_p) < n_views) ++a.lg_p;
    a.min_pixels = min_num_pixels; a.max_td = max_traversal_depth;
    a.max_depth_error = (double)max_depth_error;
    a.r2 = (double)max_reproj_error * (double)max_reproj_error;
    const bool w2 = max_reproj_error > 1.0f;
    const long groups = (long)CF_WAVE >> a.lg_p;
    const long nblk = (npix + groups - 1) / groups;
    PSCV_CHECK_ARG(nblk < (1L << 31), "%s: %ld blocks", what, nblk);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)nblk), wave(CF_WAVE);
    int rc = w2 ? launch(what, colmap_fuse_kernel<2, false, NORMALS>, grid, wave, 0, st, a)
                : launch(what, colmap_fuse_kernel<1, false, NORMALS>, grid, wave, 0, st, a);
    if (rc) return rc;
    rc = w2 ? launch(what, colmap_fuse_kernel<2, true, NORMALS>, grid, wave, 0, st, a)
            : launch(what, colmap_fuse_kernel<1, true, NORMALS>, grid, wave, 0, st, a);
    if (rc) return rc;
    const dim3 aux((unsigned)((npix + CF_AUX_THREADS - 1) / CF_AUX_THREADS)), aux_threads(CF_AUX_THREADS);
    rc = launch(what, colmap_count_kernel, aux, aux_threads, 0, st, a.flag, npix, seg_count);
    if (rc) return rc;
    rc = launch(what, scan_kernel<CF_SCAN_THREADS, long long, true>, dim3(1), dim3(CF_SCAN_THREADS), 0, st, seg_count, seg_off, counter,
                (int)nseg);
    if (rc) return rc;
    return launch(what, colmap_scatter_kernel, aux, aux_threads, 0, st, a.flag, seg_off, a.stage, npix, view, (long long)capacity, out_xyz,
                  out_normal, out_rgb, out_view, out_pixel);
}
}  // namespace

extern "C" int pscv_colmap_fuse_pass(int view, int tag, const float* const* depth, const unsigned int* const* color,
                                     unsigned char* const* fused, unsigned long long* const* claim, const int* hw, int n_views,
                                     const float* cams, const long* overlap, long processed_mask,
                                     float max_depth_error, float max_reproj_error, int min_num_pixels, int max_traversal_depth,
                                     float* out_xyz, float* out_normal, unsigned char* out_rgb, int* out_view, int* out_pixel,
                                     long capacity, long long* counter, void* workspace, long workspace_bytes, void* stream) {
    return cf_pass<false>("pscv_colmap_fuse_pass", view, tag, depth, color, fused, claim, hw, n_views, cams, overlap, processed_mask,
                          max_depth_error, max_reproj_error, min_num_pixels, max_traversal_depth, nullptr, 0.0f, out_xyz, out_normal,
                          out_rgb, out_view, out_pixel, capacity, counter, workspace, workspace_bytes, stream);
}

extern "C" int pscv_colmap_fuse_pass_normals(int view, int tag, const float* const* depth, const unsigned int* const* color,
                                             unsigned char* const* fused, unsigned long long* const* claim, const int* hw,
                                             int n_views, const float* cams, const long* overlap, long processed_mask,
                                             float max_depth_error, float max_reproj_error, int min_num_pixels,
                                             int max_traversal_depth, const float* const* normal, float max_normal_error,
                                             float* out_xyz, float* out_normal, unsigned char* out_rgb, int* out_view, int* out_pixel,
                                             long capacity, long long* counter, void* workspace, long workspace_bytes, void* stream) {
    return cf_pass<true>("pscv_colmap_fuse_pass_normals", view, tag, depth, color, fused, claim, hw, n_views, cams, overlap,
                         processed_mask, max_depth_error, max_reproj_error, min_num_pixels, max_traversal_depth, normal,
                         max_normal_error, out_xyz, out_normal, out_rgb, out_view, out_pixel, capacity, counter, workspace,
                         workspace_bytes, stream);
}
