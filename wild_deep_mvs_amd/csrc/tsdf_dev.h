// The TSDF rule's device code, written once for the two storage layouts: the dense grid of tsdf_fusion.hip (INTEGRATION.md section
// 2o) and the brick pool of tsdf_bricks.hip (section 2q).  Both files are built with -ffp-contract=off: every product and sum below
// is its own fp64 operation in the order written, which tests/_tsdf_ref.py reproduces bit for bit.
#pragma once
#include "geo_common.h"

#include <float.h>

namespace pscv {

// ---- integration -------------------------------------------------------------------------------------------------------------
struct TsdfArgs {
    const float* depth[PSCV_FUSE_MAX_VIEWS];            // [h_v, w_v]
    const unsigned int* color[PSCV_FUSE_MAX_VIEWS];     // [h_v, w_v] rgba8, red in the low byte
    int h[PSCV_FUSE_MAX_VIEWS], w[PSCV_FUSE_MAX_VIEWS];
    const float* cams;                                  // [n][PSCV_GEO_CAM_FLOATS]
    const float* dmax;                                  // [n]: the largest valid depth of each view (0 when it has none)
    double o0, o1, o2, s, trunc;
    int nx, ny, nz, n_views;
    float* tsdf_sum;
    int* weight;
    float* rgb_sum;
    int* cweight;
};
static_assert(sizeof(TsdfArgs) <= 4096, "the kernel-argument segment holds 4 KB");

struct TsdfF3 { float x, y, z; };

// True only when no lattice point of the box [lo, hi]^3 (coordinates as the lanes compute them; o + i s is monotone in i, so every
// point of the tile lies in the box) can be updated by the view.  x, y, z of cf_project are affine in X, so an affine test that
// holds at the eight corners holds inside; the corners and the lanes round differently, by at most ~20 ulp of S, the sum of the
// absolute values of every term of the projection at the box's largest coordinates.  The margin m = 1e-9 S (1 + max(w, h)) is six
// orders above that and far below a pixel or a voxel:
//   * behind:  z < -m at every corner, so every lane computes z <= 0;
//   * left:    x + z / 2 < -m at every corner: a lane with z > 0 has x / z + 0.5 < -m / (2 z) + |x / z| 2^-52 < 0 (m > 1e-9 |x|),
//              so px < 0; "top" is the same with y;
//   * right:   x + z / 2 - w z > m at every corner: a lane with z > 0 has x / z + 0.5 > w before rounding, >= w after, so px >= w;
//              "bottom" is the same with y and h;
//   * deep:    z > dmax + trunc + m at every corner: every valid d <= dmax gives d - z < -trunc - m / 2, and |d - z| < z <= S puts
//              its rounding far below m / 2, so sd < -trunc.
// A NaN or inf anywhere makes every comparison false: the view is kept.
//
// SHALLOW adds a seventh test, for the brick probe only, which asks whether a view can TOUCH a point (-trunc <= sd <= trunc), not
// whether it can update it (a point in front of every surface is updated, with phi = 1, but not touched):
//   * shallow: z < dmin - trunc - ms at every corner, dmin the view's smallest valid depth (+inf when it has none: such a view
//              touches nothing) and ms = m + 1e-9 trunc.  A lane's z differs from the affine value by less than m / 2, so every valid
//              d >= dmin has d - z > trunc + m / 2 + 1e-9 trunc as real numbers.  sd is that difference rounded once, a relative
//              error of 2^-53: sd > (trunc + 1e-9 trunc) (1 - 2^-53) > trunc.  The 1e-9 trunc term is there because m scales with
//              the projection, not with trunc: without it a truncation many orders above the scene could absorb m in the rounding
//              of dmin - trunc.  A lane with z <= 0 is not updated at all.
template <bool SHALLOW = false>
__device__ __forceinline__ bool tile_culled(const float* c, double w, double h, double dmax, double trunc, const double (&bx)[2],
                                            const double (&by)[2], const double (&bz)[2], double dmin = 0.0) {
    const float *K = c + CAM_K, *R = c + CAM_R, *t = c + CAM_T;
    const double ax = fmax(fabs(bx[0]), fabs(bx[1])), ay = fmax(fabs(by[0]), fabs(by[1])), az = fmax(fabs(bz[0]), fabs(bz[1]));
    double e[3], S = 0.0;
    for (int r = 0; r < 3; ++r)
        e[r] = fabs((double)R[3 * r]) * ax + fabs((double)R[3 * r + 1]) * ay + fabs((double)R[3 * r + 2]) * az + fabs((double)t[r]);
    for (int r = 0; r < 9; ++r) S += fabs((double)K[r]) * e[r % 3];
    const double m = 1e-9 * S * (1.0 + fmax(w, h));
    const double ms = m + 1e-9 * trunc;
    bool behind = true, left = true, right = true, top = true, bottom = true, deep = true, shallow = SHALLOW;
    for (int q = 0; q < 8; ++q) {
        double x, y, z;
        cf_project(c, bx[q & 1], by[q >> 1 & 1], bz[q >> 2], x, y, z);
        const double gx = x + 0.5 * z, gy = y + 0.5 * z;
        behind = behind && z < -m;
        left = left && gx < -m;
        top = top && gy < -m;
        right = right && gx - w * z > m;
        bottom = bottom && gy - h * z > m;
        deep = deep && z > dmax + trunc + m;
        if (SHALLOW) shallow = shallow && z < dmin - trunc - ms;
    }
    return behind || left || right || top || bottom || deep || shallow;
}

// Steps 1-5 of the rule for one lattice point and view: true when the view updates the point, with its signed distance and the
// pixel's offset in the view's maps.
__device__ __forceinline__ bool tsdf_view_sd(const TsdfArgs& a, int v, double X, double Y, double Z, double& sd, long& o) {
    double x, y, z;
    cf_project(a.cams + (long)v * PSCV_GEO_CAM_FLOATS, X, Y, Z, x, y, z);
    if (!(z > 0.0)) return false;
    const double px = floor(x / z + 0.5), py = floor(y / z + 0.5);
    const int w = a.w[v], h = a.h[v];
    if (!(px >= 0.0 && px < (double)w && py >= 0.0 && py < (double)h)) return false;
    o = (long)(int)py * w + (int)px;
    const float d = a.depth[v][o];
    if (!cf_depth_ok(d)) return false;
    sd = (double)d - z;
    return !(sd < -a.trunc);
}

// One lattice point's state, in registers for a whole call (integer colour sums: exact in fp32 below 2^24)
struct TsdfVoxel {
    double S;
    int wgt, cw, cr, cg, cb;
};

// The views of the set `live` (a workgroup-uniform mask, walked through scalar registers), in ascending order: step 6 of the rule
__device__ __forceinline__ void tsdf_walk_views(const TsdfArgs& a, unsigned long long live, double X, double Y, double Z, TsdfVoxel& r) {
    while (live) {
        const int v = __builtin_ctzll(live);
        live &= live - 1;
        double sd;
        long o;
        if (!tsdf_view_sd(a, v, X, Y, Z, sd, o)) continue;
        const double q = sd / a.trunc;
        r.S += q < 1.0 ? q : 1.0;
        r.wgt += 1;
        if (sd <= a.trunc) {
            const unsigned c = a.color[v][o];
            r.cr += (int)(c & 255u);
            r.cg += (int)(c >> 8 & 255u);
            r.cb += (int)(c >> 16 & 255u);
            r.cw += 1;
        }
    }
}

// The state of the voxel at index `lin` of the four arrays (a dense grid's linear index or a pool index), walked and written back
__device__ __forceinline__ void tsdf_update_voxel(const TsdfArgs& a, unsigned long long live, long lin, double X, double Y, double Z) {
    TsdfF3* rgbp = reinterpret_cast<TsdfF3*>(a.rgb_sum) + lin;
    TsdfVoxel r;
    r.S = (double)a.tsdf_sum[lin];
    r.wgt = a.weight[lin], r.cw = a.cweight[lin];
    const TsdfF3 c0 = *rgbp;
    r.cr = (int)c0.x, r.cg = (int)c0.y, r.cb = (int)c0.z;
    tsdf_walk_views(a, live, X, Y, Z, r);
    a.tsdf_sum[lin] = (float)r.S;
    a.weight[lin] = r.wgt;
    *rgbp = TsdfF3{(float)r.cr, (float)r.cg, (float)r.cb};
    a.cweight[lin] = r.cw;
}

// The ballot of wave 0 through LDS into scalar registers: the workgroup's view list (call from every lane; one barrier)
__device__ __forceinline__ unsigned long long tsdf_share_live(unsigned long long& s_live, bool wave0, bool live) {
    if (wave0) {
        const unsigned long long m = __ballot(live);
        if (threadIdx.x == 0) s_live = m;
    }
    __syncthreads();
    const unsigned long long lv = s_live;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)lv), hi = __builtin_amdgcn_readfirstlane((unsigned)(lv >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// ---- extraction: marching tetrahedra ------------------------------------------------------------------------------------------
// Corner c of a cell is p + (c & 1, c >> 1 & 1, c >> 2 & 1); tetrahedron T of the six axis orders (a, b, c) has the corners
// (0, a, a | b, 7) at positions 0..3; its edge between positions u < v is the global edge (p + offset(c_u), c_v ^ c_u).
//
// The case table: entry [T][neg] for the 4-bit set `neg` of negative corner positions = the number of vertices of the cycle (0, 3
// or 4) in bits 0-2 and vertex k's edge in bits 3 + 6 k .. 8 + 6 k as c_u | (c_v ^ c_u) << 3, in the ORIENTED cyclic order of the
// rule: one or three negatives give the three edges at the lone corner, two negatives N0 < N1 and positives P0 < P1 give (N0,P0),
// (N0,P1), (N1,P1), (N1,P0); with every vertex replaced by its edge's midpoint, the cycle is kept when the normal of its first
// three midpoints has a positive dot product with (centroid of the positive corners - centroid of the negative corners), and
// reversed otherwise -- exact in integers (midpoints doubled, centroids scaled by the two counts).  make_tet_table() IS that
// rule, evaluated by the compiler; pscv_tsdf_case_table hands the result to tests/test_tsdf_cpu.py, which checks all 96 entries
// against the rule restated in Python.
struct TetTable { unsigned int e[6 * 16]; };

constexpr int TET_ORDERS[6][3] = {{1, 2, 4}, {1, 4, 2}, {2, 1, 4}, {2, 4, 1}, {4, 1, 2}, {4, 2, 1}};

constexpr TetTable make_tet_table() {
    TetTable tab{};
    for (int T = 0; T < 6; ++T) {
        const int cc[4] = {0, TET_ORDERS[T][0], TET_ORDERS[T][0] | TET_ORDERS[T][1], 7};
        for (int neg = 0; neg < 16; ++neg) {
            int nn = 0, N[4] = {0, 0, 0, 0}, P[4] = {0, 0, 0, 0}, np = 0;
            for (int u = 0; u < 4; ++u) {
                if (neg >> u & 1) N[nn++] = u;
                else P[np++] = u;
            }
            int cnt = 0, eu[4] = {0, 0, 0, 0}, ev[4] = {0, 0, 0, 0};
            if (nn == 1 || nn == 3) {
                const int lone = nn == 1 ? N[0] : P[0];
                for (int u = 0; u < 4; ++u) {
                    if (u == lone) continue;
                    eu[cnt] = u < lone ? u : lone;
                    ev[cnt] = u < lone ? lone : u;
                    ++cnt;
                }
            } else if (nn == 2) {
                const int pairs[4][2] = {{N[0], P[0]}, {N[0], P[1]}, {N[1], P[1]}, {N[1], P[0]}};
                for (int q = 0; q < 4; ++q) {
                    eu[q] = pairs[q][0] < pairs[q][1] ? pairs[q][0] : pairs[q][1];
                    ev[q] = pairs[q][0] < pairs[q][1] ? pairs[q][1] : pairs[q][0];
                }
                cnt = 4;
            }
            unsigned int entry = (unsigned int)cnt;
            if (cnt) {
                int M[3][3] = {};                                            // doubled midpoints of the first three vertices
                for (int q = 0; q < 3; ++q)
                    for (int ax = 0; ax < 3; ++ax) M[q][ax] = (cc[eu[q]] >> ax & 1) + (cc[ev[q]] >> ax & 1);
                const int ux = M[1][0] - M[0][0], uy = M[1][1] - M[0][1], uz = M[1][2] - M[0][2];
                const int vx = M[2][0] - M[0][0], vy = M[2][1] - M[0][1], vz = M[2][2] - M[0][2];
                const int nrm[3] = {uy * vz - uz * vy, uz * vx - ux * vz, ux * vy - uy * vx};
                int dot = 0;
                for (int ax = 0; ax < 3; ++ax) {
                    int sp = 0, sn = 0;
                    for (int u = 0; u < 4; ++u) {
                        if (neg >> u & 1) sn += cc[u] >> ax & 1;
                        else sp += cc[u] >> ax & 1;
                    }
                    dot += nrm[ax] * (nn * sp - np * sn);                    // (centroid difference times nn np > 0)
                }
                for (int q = 0; q < cnt; ++q) {
                    const int src = dot > 0 ? q : cnt - 1 - q;
                    const unsigned int code = (unsigned int)cc[eu[src]] | (unsigned int)(cc[ev[src]] ^ cc[eu[src]]) << 3;
                    entry |= code << (3 + 6 * q);
                }
            }
            tab.e[T * 16 + neg] = entry;
        }
    }
    return tab;
}

constexpr TetTable H_TET_TABLE = make_tet_table();
static __constant__ TetTable d_tet_table = make_tet_table();       // (one copy per translation unit: the library links no device code)

// info = edge mask (bits 0-6: bit d-1 = edge (p, d) carries a vertex) | observed << 8 | negative << 9 |
//        vertex count << 16 | face count of the cell << 24
constexpr unsigned F_OBS = 1u, F_NEG = 2u;

// observed / negative flags of one voxel: weight >= min_weight, f = tsdf_sum / weight < 0
__device__ __forceinline__ unsigned tsdf_flags(float tsdf_sum, int wv, int min_weight) {
    if (wv < min_weight) return 0u;
    const double val = (double)tsdf_sum / (double)wv;
    return F_OBS | (val < 0.0 ? F_NEG : 0u);
}

// info of the voxel at corner 0 from the flags of its cell's eight corners (a corner outside the volume: 0)
__device__ __forceinline__ int tsdf_cell_info(const unsigned (&cf)[8]) {
    unsigned mask = 0;
#pragma unroll
    for (int d = 1; d < 8; ++d)
        if ((cf[0] & cf[d] & F_OBS) && ((cf[0] ^ cf[d]) & F_NEG)) mask |= 1u << (d - 1);
    unsigned faces = 0;
#pragma unroll
    for (int T = 0; T < 6; ++T) {
        const int c1 = TET_ORDERS[T][0], c2 = c1 | TET_ORDERS[T][1];
        if (cf[0] & cf[c1] & cf[c2] & cf[7] & F_OBS) {
            const unsigned nn = (cf[0] >> 1 & 1u) + (cf[c1] >> 1 & 1u) + (cf[c2] >> 1 & 1u) + (cf[7] >> 1 & 1u);
            faces += nn == 2 ? 2u : (nn == 1 || nn == 3) ? 1u : 0u;
        }
    }
    return (int)(mask | cf[0] << 8 | (unsigned)__popc(mask) << 16 | faces << 24);
}

// vertex index of edge (voxel at index lin2 of info / vincl, d): the voxel's exclusive vertex offset + the edges of smaller type it carries
__device__ __forceinline__ int edge_vertex(const int* __restrict__ info, const int* __restrict__ vincl, long lin2, int d) {
    const unsigned f = (unsigned)info[lin2];
    return vincl[lin2] - (int)(f >> 16 & 255u) + __popc(f & ((1u << (d - 1)) - 1u));
}

struct TsdfVal { double f, m[3]; int cw; };

__device__ __forceinline__ TsdfVal load_val(const float* tsdf_sum, const int* weight, const float* rgb_sum, const int* cweight, long lin) {
    TsdfVal r;
    r.f = (double)tsdf_sum[lin] / (double)weight[lin];
    r.cw = cweight[lin];
    for (int c = 0; c < 3; ++c) r.m[c] = r.cw > 0 ? (double)rgb_sum[3 * lin + c] / (double)r.cw : 0.0;
    return r;
}

// Vertex `out` of the edge between P at Xp and Q at Xq: the zero crossing and the colour interpolated with the same t
__device__ __forceinline__ void tsdf_write_vertex(const TsdfVal& P, const TsdfVal& Q, const double (&Xp)[3], const double (&Xq)[3],
                                                  float* __restrict__ xyz, unsigned char* __restrict__ rgb, long out) {
    const double t = P.f / (P.f - Q.f);
    for (int c = 0; c < 3; ++c) {
        xyz[3 * out + c] = (float)(Xp[c] + t * (Xq[c] - Xp[c]));
        double val = 0.0;
        if (P.cw > 0 && Q.cw > 0) val = P.m[c] + t * (Q.m[c] - P.m[c]);
        else if (P.cw > 0) val = P.m[c];
        else if (Q.cw > 0) val = Q.m[c];
        double by = floor(val + 0.5);
        by = by < 0.0 ? 0.0 : by > 255.0 ? 255.0 : by;
        rgb[3 * out + c] = (unsigned char)(int)by;
    }
}

__device__ __forceinline__ int sel4(int k, int a, int b, int c, int d) { return k == 0 ? a : k == 1 ? b : k == 2 ? c : d; }

// The one or two faces of a cycle of cnt = 3 or 4 vertices q, rotated so that the vertex with the smallest key comes first (key[n]
// for n >= cnt must be the key type's largest value); a quad is (q0,q1,q2), (q0,q2,q3).  In the dense layout the vertex index is
// the key's rank, so the index itself serves as key.  Nothing is written at or past n_faces; `out` advances either way.
template <class Key>
__device__ __forceinline__ void tsdf_write_faces(const int (&q)[4], const Key (&key)[4], int cnt, int* __restrict__ faces, long& out,
                                                 long n_faces) {
    int first = 0;
    Key best = key[0];
#pragma unroll
    for (int n = 1; n < 4; ++n)
        if (key[n] < best) best = key[n], first = n;
    const int r1 = first + 1 >= cnt ? first + 1 - cnt : first + 1, r2 = first + 2 >= cnt ? first + 2 - cnt : first + 2;
    const int r3 = first + 3 >= cnt ? first + 3 - cnt : first + 3;
    const int q0 = sel4(first, q[0], q[1], q[2], q[3]), q1 = sel4(r1, q[0], q[1], q[2], q[3]), q2 = sel4(r2, q[0], q[1], q[2], q[3]);
    if (out >= 0 && out < n_faces) {
        faces[3 * out] = q0;
        faces[3 * out + 1] = q1;
        faces[3 * out + 2] = q2;
    }
    ++out;
    if (cnt == 4) {
        const int q3 = sel4(r3, q[0], q[1], q[2], q[3]);
        if (out >= 0 && out < n_faces) {
            faces[3 * out] = q0;
            faces[3 * out + 1] = q2;
            faces[3 * out + 2] = q3;
        }
        ++out;
    }
}

// ---- host side: the checks and the argument block of a call, once for the two layouts ---------------------------------------------
inline int check_grid(const char* what, double o0, double o1, double o2, double voxel) {
    PSCV_CHECK_ARG(fabs(o0) <= DBL_MAX && fabs(o1) <= DBL_MAX && fabs(o2) <= DBL_MAX, "%s: origin (%g, %g, %g) must be finite", what, o0,
                   o1, o2);
    PSCV_CHECK_ARG(voxel > 0.0 && voxel <= DBL_MAX, "%s: voxel=%g must be positive and finite", what, voxel);
    return 0;
}

// the dense grid: a linear voxel index fits int32
inline int check_dims(const char* what, int nx, int ny, int nz) {
    PSCV_CHECK_ARG(nx >= 1 && ny >= 1 && nz >= 1 && (long)nx * ny < (1L << 31) && (long)nx * ny * nz < (1L << 31),
                   "%s: dims %dx%dx%d must be positive with nx ny nz < 2^31", what, nx, ny, nz);
    return 0;
}

// The views and the lattice of an integration or probe call (color null: the probe reads no colour); the state pointers are left
// null for the caller.  `dense` adds check_dims; a brick lattice is checked by its caller, which also derives the brick counts.
inline int tsdf_setup(const char* what, TsdfArgs& a, const float* const* depth, const unsigned int* const* color, const int* hw,
                      int n_views, const float* cams, const float* dmax, double o0, double o1, double o2, double voxel, double trunc,
                      int nx, int ny, int nz, bool dense) {
    if (check_view_count(what, n_views, 1) || check_grid(what, o0, o1, o2, voxel)) return -1;
    PSCV_CHECK_ARG(trunc > 0.0 && trunc <= DBL_MAX, "%s: trunc=%g must be positive and finite", what, trunc);
    if (dense && check_dims(what, nx, ny, nz)) return -1;
    if (fill_views(a, what, depth, hw, n_views) || fill_view_ptrs(a.color, what, color, n_views)) return -1;
    a.cams = cams;
    a.dmax = dmax;
    a.o0 = o0, a.o1 = o1, a.o2 = o2, a.s = voxel, a.trunc = trunc;
    a.nx = nx, a.ny = ny, a.nz = nz, a.n_views = n_views;
    a.tsdf_sum = nullptr, a.weight = nullptr, a.rgb_sum = nullptr, a.cweight = nullptr;
    return 0;
}

}  // namespace pscv
