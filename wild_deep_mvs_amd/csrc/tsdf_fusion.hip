// Depth maps into a dense TSDF volume, and the volume into an indexed triangle mesh by marching tetrahedra: the surface at the end
// of the reconstruction pipeline.  gfx950.
//
// All arithmetic is fp64 on values converted from their fp32 / byte storage; products and sums are separate operations in the
// order written (the Makefile builds this file with -ffp-contract=off, like depth_normals.hip), which tests/_tsdf_ref.py
// reproduces bit for bit.
//
// Grid: lattice point (i, j, k) sits at X = (o0 + i s, o1 + j s, o2 + k s), lin = (k ny + j) nx + i, nx ny nz < 2^31.
// State [nz, ny, nx]: tsdf_sum fp32, weight int32, rgb_sum fp32 [.., 3] (integer sums, exact below 2^24), cweight int32.
//
// Integration, per voxel and view in ascending view order (S, the sums and the weights live in registers for the whole call):
//   (x, y, z) = cf_project(cam, X), skip unless z > 0;  px = floor(x / z + 0.5), py = floor(y / z + 0.5), skip unless
//   0 <= px < w and 0 <= py < h (compared in fp64);  d = depth[py, px], skip unless cf_depth_ok(d);  sd = (double)d - z, skip if
//   sd < -trunc;  S += min(1, sd / trunc), weight += 1;  if sd <= trunc: rgb_sum += the pixel's bytes, cweight += 1.
// tsdf_sum is rounded to fp32 once per call.
//
// Mapping: a workgroup of 256 lanes owns a tile of TI_TX x TI_TY = 64 x 4 lattice points of one z plane, one per lane, x fastest
// (a wave loads and stores 256 contiguous bytes of every state array).  Wave 0 first decides, one view per lane, which views can
// touch the tile at all (tile_culled below: conservative, so it changes no result), the ballot of the survivors is the
// workgroup's view list, and every lane walks it through scalar registers: the 30 camera floats and the view's pointers are
// workgroup-uniform loads.  A tile that no view touches is neither loaded nor stored.
//
// Extraction: pscv_tsdf_mark writes one int32 per voxel (edge mask, flags, vertex count, face count), the caller turns the two
// counts into inclusive prefix sums, and pscv_tsdf_emit_vertices / pscv_tsdf_emit_faces write the mesh in its defined order.
#include "geo_common.h"

#include <float.h>

namespace pscv {

// ---- integration -------------------------------------------------------------------------------------------------------------
constexpr int TI_TX = 64, TI_TY = 4, TI_THREADS = TI_TX * TI_TY;

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
__device__ __forceinline__ bool tile_culled(const float* c, double w, double h, double dmax, double trunc, const double (&bx)[2],
                                            const double (&by)[2], const double (&bz)[2]) {
    const float *K = c + CAM_K, *R = c + CAM_R, *t = c + CAM_T;
    const double ax = fmax(fabs(bx[0]), fabs(bx[1])), ay = fmax(fabs(by[0]), fabs(by[1])), az = fmax(fabs(bz[0]), fabs(bz[1]));
    double e[3], S = 0.0;
    for (int r = 0; r < 3; ++r)
        e[r] = fabs((double)R[3 * r]) * ax + fabs((double)R[3 * r + 1]) * ay + fabs((double)R[3 * r + 2]) * az + fabs((double)t[r]);
    for (int r = 0; r < 9; ++r) S += fabs((double)K[r]) * e[r % 3];
    const double m = 1e-9 * S * (1.0 + fmax(w, h));
    bool behind = true, left = true, right = true, top = true, bottom = true, deep = true;
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
    }
    return behind || left || right || top || bottom || deep;
}

__global__ __launch_bounds__(TI_THREADS) void tsdf_integrate_kernel(const TsdfArgs a) {
    __shared__ unsigned long long s_live;
    const int tid = threadIdx.x;
    const int tiles_x = (a.nx + TI_TX - 1) / TI_TX, tiles_y = (a.ny + TI_TY - 1) / TI_TY;
    const int b = blockIdx.x;
    const int k = b / (tiles_x * tiles_y), rem = b - k * (tiles_x * tiles_y);
    const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
    const int i0 = tx * TI_TX, j0 = ty * TI_TY;
    if (tid < 64) {                                               // wave 0: lane v judges view v
        bool live = false;
        if (tid < a.n_views) {
            const int i1 = min(i0 + TI_TX, a.nx) - 1, j1 = min(j0 + TI_TY, a.ny) - 1;
            const double bx[2] = {a.o0 + (double)i0 * a.s, a.o0 + (double)i1 * a.s};
            const double by[2] = {a.o1 + (double)j0 * a.s, a.o1 + (double)j1 * a.s};
            const double bz[2] = {a.o2 + (double)k * a.s, a.o2 + (double)k * a.s};
            // (a.w[tid], a.h[tid] and the camera row are indexed per lane: the by-value argument struct stays in the kernel-argument
            // segment and these become loads from it.  Indexing a COPY of the struct, or of its arrays, per lane would put it in
            // scratch: check "ScratchSize: 0" in -Rpass-analysis=kernel-resource-usage after any change here)
            live = !tile_culled(a.cams + (long)tid * PSCV_GEO_CAM_FLOATS, (double)a.w[tid], (double)a.h[tid], (double)a.dmax[tid],
                                a.trunc, bx, by, bz);
        }
        const unsigned long long m = __ballot(live);
        if (tid == 0) s_live = m;
    }
    __syncthreads();
    const unsigned long long lv = s_live;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)lv), hi = __builtin_amdgcn_readfirstlane((unsigned)(lv >> 32));
    unsigned long long live = ((unsigned long long)hi << 32) | lo;           // (in scalar registers: the view loop is uniform)
    if (live == 0) return;
    const int i = i0 + (tid & (TI_TX - 1)), j = j0 + tid / TI_TX;
    if (i >= a.nx || j >= a.ny) return;
    const long lin = ((long)k * a.ny + j) * a.nx + i;
    TsdfF3* rgbp = reinterpret_cast<TsdfF3*>(a.rgb_sum) + lin;
    double S = (double)a.tsdf_sum[lin];
    int wgt = a.weight[lin], cw = a.cweight[lin];
    const TsdfF3 c0 = *rgbp;
    int cr = (int)c0.x, cg = (int)c0.y, cb = (int)c0.z;                      // (integer sums: exact in fp32 below 2^24)
    const double X = a.o0 + (double)i * a.s, Y = a.o1 + (double)j * a.s, Z = a.o2 + (double)k * a.s;
    while (live) {
        const int v = __builtin_ctzll(live);
        live &= live - 1;
        double x, y, z;
        cf_project(a.cams + (long)v * PSCV_GEO_CAM_FLOATS, X, Y, Z, x, y, z);
        if (!(z > 0.0)) continue;
        const double px = floor(x / z + 0.5), py = floor(y / z + 0.5);
        const int w = a.w[v], h = a.h[v];
        if (!(px >= 0.0 && px < (double)w && py >= 0.0 && py < (double)h)) continue;
        const long o = (long)(int)py * w + (int)px;
        const float d = a.depth[v][o];
        if (!cf_depth_ok(d)) continue;
        const double sd = (double)d - z;
        if (sd < -a.trunc) continue;
        const double q = sd / a.trunc;
        S += q < 1.0 ? q : 1.0;
        wgt += 1;
        if (sd <= a.trunc) {
            const unsigned c = a.color[v][o];
            cr += (int)(c & 255u);
            cg += (int)(c >> 8 & 255u);
            cb += (int)(c >> 16 & 255u);
            cw += 1;
        }
    }
    a.tsdf_sum[lin] = (float)S;
    a.weight[lin] = wgt;
    *rgbp = TsdfF3{(float)cr, (float)cg, (float)cb};
    a.cweight[lin] = cw;
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
__constant__ TetTable d_tet_table = make_tet_table();

// info[lin] = edge mask (bits 0-6: bit d-1 = edge (p, d) carries a vertex) | observed << 8 | negative << 9 |
//             vertex count << 16 | face count of the cell << 24
constexpr int TM_TX = 32, TM_TY = 4, TM_TZ = 2, TM_THREADS = TM_TX * TM_TY * TM_TZ;
constexpr int TM_PX = TM_TX + 1, TM_PY = TM_TY + 1, TM_PZ = TM_TZ + 1;
constexpr unsigned F_OBS = 1u, F_NEG = 2u;

__device__ __forceinline__ long corner_lin(long lin, int c, int nx, int ny) {
    return lin + (c & 1) + (long)(c >> 1 & 1) * nx + (long)(c >> 2) * nx * ny;
}

__global__ __launch_bounds__(TM_THREADS) void tsdf_mark_kernel(const float* __restrict__ tsdf_sum, const int* __restrict__ weight,
                                                               int nx, int ny, int nz, int min_weight, int* __restrict__ info) {
    __shared__ unsigned char fl[TM_PZ * TM_PY * TM_PX];
    const int tid = threadIdx.x;
    const int tiles_x = (nx + TM_TX - 1) / TM_TX, tiles_y = (ny + TM_TY - 1) / TM_TY;
    const int b = blockIdx.x;
    const int tz = b / (tiles_x * tiles_y), rem = b - tz * (tiles_x * tiles_y);
    const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
    const int i0 = tx * TM_TX, j0 = ty * TM_TY, k0 = tz * TM_TZ;
    for (int n = tid; n < TM_PZ * TM_PY * TM_PX; n += TM_THREADS) {          // the tile and its +1 halo; outside the grid = unobserved
        const int lz = n / (TM_PY * TM_PX), r2 = n - lz * (TM_PY * TM_PX), ly = r2 / TM_PX, lx = r2 - ly * TM_PX;
        const int i = i0 + lx, j = j0 + ly, k = k0 + lz;
        unsigned f = 0;
        if (i < nx && j < ny && k < nz) {
            const long lin = ((long)k * ny + j) * nx + i;
            const int wv = weight[lin];
            if (wv >= min_weight) {
                const double val = (double)tsdf_sum[lin] / (double)wv;
                f = F_OBS | (val < 0.0 ? F_NEG : 0u);
            }
        }
        fl[n] = (unsigned char)f;
    }
    __syncthreads();
    const int lx = tid & (TM_TX - 1), ly = tid / TM_TX & (TM_TY - 1), lz = tid / (TM_TX * TM_TY);
    const int i = i0 + lx, j = j0 + ly, k = k0 + lz;
    if (i >= nx || j >= ny || k >= nz) return;
    unsigned cf[8];                                                          // flags of the cell's eight corners
#pragma unroll
    for (int c = 0; c < 8; ++c) cf[c] = fl[((lz + (c >> 2)) * TM_PY + ly + (c >> 1 & 1)) * TM_PX + lx + (c & 1)];
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
    info[((long)k * ny + j) * nx + i] = (int)(mask | cf[0] << 8 | (unsigned)__popc(mask) << 16 | faces << 24);
}

// vertex index of edge (voxel at lin2, d): the voxel's exclusive vertex offset + the edges of smaller type it carries
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

__global__ __launch_bounds__(256) void tsdf_emit_vertices_kernel(const float* __restrict__ tsdf_sum, const int* __restrict__ weight,
                                                                 const float* __restrict__ rgb_sum, const int* __restrict__ cweight,
                                                                 const int* __restrict__ info, const int* __restrict__ vincl, int nx,
                                                                 int ny, long nvox, double o0, double o1, double o2, double s,
                                                                 float* __restrict__ xyz, unsigned char* __restrict__ rgb,
                                                                 long n_vertices) {
    const long lin = (long)blockIdx.x * 256 + threadIdx.x;
    if (lin >= nvox) return;
    const unsigned f = (unsigned)info[lin];
    const unsigned mask = f & 127u;
    if (!mask) return;
    const int i = (int)(lin % nx), j = (int)(lin / nx % ny), k = (int)(lin / ((long)nx * ny));
    long out = (long)vincl[lin] - (long)(f >> 16 & 255u);
    const TsdfVal P = load_val(tsdf_sum, weight, rgb_sum, cweight, lin);
    const double Xp[3] = {o0 + (double)i * s, o1 + (double)j * s, o2 + (double)k * s};
    for (int d = 1; d < 8; ++d) {
        if (!(mask >> (d - 1) & 1u)) continue;
        const long linq = corner_lin(lin, d, nx, ny);
        if (linq >= nvox) break;                                             // (a mask that is not pscv_tsdf_mark's reads nothing outside)
        const TsdfVal Q = load_val(tsdf_sum, weight, rgb_sum, cweight, linq);
        const double t = P.f / (P.f - Q.f);
        const double Xq[3] = {o0 + (double)(i + (d & 1)) * s, o1 + (double)(j + (d >> 1 & 1)) * s, o2 + (double)(k + (d >> 2)) * s};
        if (out >= 0 && out < n_vertices) {                                  // (prefix sums that do not belong to `info` write nothing)
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
        ++out;
    }
}

__device__ __forceinline__ int sel4(int k, int a, int b, int c, int d) { return k == 0 ? a : k == 1 ? b : k == 2 ? c : d; }

__global__ __launch_bounds__(256) void tsdf_emit_faces_kernel(const int* __restrict__ info, const int* __restrict__ vincl,
                                                              const int* __restrict__ fincl, int nx, int ny, long nvox,
                                                              int* __restrict__ faces, long n_faces) {
    const long lin = (long)blockIdx.x * 256 + threadIdx.x;
    if (lin >= nvox) return;
    const unsigned f0 = (unsigned)info[lin];
    const unsigned nf = f0 >> 24;
    if (!nf) return;
    if (lin % nx + 1 >= nx || lin / nx % ny + 1 >= ny || corner_lin(lin, 7, nx, ny) >= nvox) return;   // (pscv_tsdf_mark counts faces
                                                                             // only where all eight corners are in the grid)
    unsigned obs = 0, neg = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const unsigned fc = (unsigned)info[corner_lin(lin, c, nx, ny)] >> 8;
        obs |= (fc & 1u) << c;
        neg |= (fc >> 1 & 1u) << c;
    }
    long out = (long)fincl[lin] - (long)nf;
#pragma unroll
    for (int T = 0; T < 6; ++T) {
        const int c1 = TET_ORDERS[T][0], c2 = c1 | TET_ORDERS[T][1];
        const unsigned need = 1u | 1u << c1 | 1u << c2 | 1u << 7;
        if ((obs & need) != need) continue;
        const unsigned cs = (neg & 1u) | (neg >> c1 & 1u) << 1 | (neg >> c2 & 1u) << 2 | (neg >> 7 & 1u) << 3;
        const unsigned e = d_tet_table.e[T * 16 + cs];
        const int cnt = (int)(e & 7u);
        if (!cnt) continue;
        int q[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const unsigned code = e >> (3 + 6 * n) & 63u;                     // (n >= cnt: code 0 = the cell's own voxel; not used)
            q[n] = n < cnt ? edge_vertex(info, vincl, corner_lin(lin, (int)(code & 7u), nx, ny), (int)(code >> 3)) : 0x7fffffff;
        }
        int first = 0, best = q[0];
#pragma unroll
        for (int n = 1; n < 4; ++n)
            if (q[n] < best) best = q[n], first = n;
        const int r1 = first + 1 >= cnt ? first + 1 - cnt : first + 1, r2 = first + 2 >= cnt ? first + 2 - cnt : first + 2;
        const int r3 = first + 3 >= cnt ? first + 3 - cnt : first + 3;
        const int q0 = best, q1 = sel4(r1, q[0], q[1], q[2], q[3]), q2 = sel4(r2, q[0], q[1], q[2], q[3]);
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
}

static int check_dims(const char* what, int nx, int ny, int nz) {
    PSCV_CHECK_ARG(nx >= 1 && ny >= 1 && nz >= 1 && (long)nx * ny < (1L << 31) && (long)nx * ny * nz < (1L << 31),
                   "%s: dims %dx%dx%d must be positive with nx ny nz < 2^31", what, nx, ny, nz);
    return 0;
}

}  // namespace pscv

extern "C" int pscv_tsdf_integrate(const float* const* depth, const unsigned int* const* color, const int* hw, int n_views,
                                   const float* cams, const float* dmax, double o0, double o1, double o2, double voxel, double trunc,
                                   int nx, int ny, int nz, float* tsdf_sum, int* weight, float* rgb_sum, int* cweight, void* stream) {
    using namespace pscv;
    const char* what = "pscv_tsdf_integrate";
    PSCV_CHECK_ARG(depth && color && hw && cams && dmax && tsdf_sum && weight && rgb_sum && cweight, "%s: null pointer argument", what);
    PSCV_CHECK_ARG(n_views >= 1 && n_views <= PSCV_FUSE_MAX_VIEWS, "%s: n_views=%d outside [1,%d]", what, n_views, PSCV_FUSE_MAX_VIEWS);
    PSCV_CHECK_ARG(fabs(o0) <= DBL_MAX && fabs(o1) <= DBL_MAX && fabs(o2) <= DBL_MAX, "%s: origin (%g, %g, %g) must be finite", what, o0,
                   o1, o2);
    PSCV_CHECK_ARG(voxel > 0.0 && voxel <= DBL_MAX, "%s: voxel=%g must be positive and finite", what, voxel);
    PSCV_CHECK_ARG(trunc > 0.0 && trunc <= DBL_MAX, "%s: trunc=%g must be positive and finite", what, trunc);
    if (check_dims(what, nx, ny, nz)) return -1;
    TsdfArgs a;
    for (int v = 0; v < PSCV_FUSE_MAX_VIEWS; ++v) {
        const bool on = v < n_views;
        a.depth[v] = on ? depth[v] : nullptr;
        a.color[v] = on ? color[v] : nullptr;
        a.h[v] = on ? hw[2 * v] : 1;
        a.w[v] = on ? hw[2 * v + 1] : 1;
        if (!on) continue;
        PSCV_CHECK_ARG(depth[v] && color[v], "%s: view %d has a null pointer", what, v);
        PSCV_CHECK_ARG(a.h[v] > 0 && a.w[v] > 0 && (long)a.h[v] * a.w[v] < (1L << 31), "%s: view %d has bad size %dx%d", what, v, a.h[v],
                       a.w[v]);
    }
    a.cams = cams;
    a.dmax = dmax;
    a.o0 = o0, a.o1 = o1, a.o2 = o2, a.s = voxel, a.trunc = trunc;
    a.nx = nx, a.ny = ny, a.nz = nz, a.n_views = n_views;
    a.tsdf_sum = tsdf_sum, a.weight = weight, a.rgb_sum = rgb_sum, a.cweight = cweight;
    const long tiles = (long)((nx + TI_TX - 1) / TI_TX) * ((ny + TI_TY - 1) / TI_TY) * nz;
    return launch(what, tsdf_integrate_kernel, dim3((unsigned)tiles), dim3(TI_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
}

extern "C" int pscv_tsdf_mark(const float* tsdf_sum, const int* weight, int nx, int ny, int nz, int min_weight, int* info, void* stream) {
    using namespace pscv;
    const char* what = "pscv_tsdf_mark";
    PSCV_CHECK_ARG(tsdf_sum && weight && info, "%s: null pointer argument", what);
    PSCV_CHECK_ARG(min_weight >= 1, "%s: min_weight=%d must be at least 1", what, min_weight);
    if (check_dims(what, nx, ny, nz)) return -1;
    const long tiles = (long)((nx + TM_TX - 1) / TM_TX) * ((ny + TM_TY - 1) / TM_TY) * ((nz + TM_TZ - 1) / TM_TZ);
    return launch(what, tsdf_mark_kernel, dim3((unsigned)tiles), dim3(TM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), tsdf_sum,
                  weight, nx, ny, nz, min_weight, info);
}

extern "C" int pscv_tsdf_emit_vertices(const float* tsdf_sum, const int* weight, const float* rgb_sum, const int* cweight,
                                       const int* info, const int* vincl, int nx, int ny, int nz, double o0, double o1, double o2,
                                       double voxel, float* xyz, unsigned char* rgb, long n_vertices, void* stream) {
    using namespace pscv;
    const char* what = "pscv_tsdf_emit_vertices";
    PSCV_CHECK_ARG(n_vertices >= 0 && n_vertices < (1L << 31), "%s: n_vertices=%ld outside [0, 2^31)", what, n_vertices);
    PSCV_CHECK_ARG(fabs(o0) <= DBL_MAX && fabs(o1) <= DBL_MAX && fabs(o2) <= DBL_MAX, "%s: origin (%g, %g, %g) must be finite", what, o0,
                   o1, o2);
    PSCV_CHECK_ARG(voxel > 0.0 && voxel <= DBL_MAX, "%s: voxel=%g must be positive and finite", what, voxel);
    if (check_dims(what, nx, ny, nz)) return -1;
    if (n_vertices == 0) return 0;
    PSCV_CHECK_ARG(tsdf_sum && weight && rgb_sum && cweight && info && vincl && xyz && rgb, "%s: null pointer argument", what);
    const long nvox = (long)nx * ny * nz;
    return launch(what, tsdf_emit_vertices_kernel, dim3((unsigned)((nvox + 255) / 256)), dim3(256), 0,
                  reinterpret_cast<hipStream_t>(stream), tsdf_sum, weight, rgb_sum, cweight, info, vincl, nx, ny, nvox, o0, o1, o2, voxel,
                  xyz, rgb, n_vertices);
}

extern "C" int pscv_tsdf_emit_faces(const int* info, const int* vincl, const int* fincl, int nx, int ny, int nz, int* faces,
                                    long n_faces, void* stream) {
    using namespace pscv;
    const char* what = "pscv_tsdf_emit_faces";
    PSCV_CHECK_ARG(n_faces >= 0 && n_faces < (1L << 31), "%s: n_faces=%ld outside [0, 2^31)", what, n_faces);
    if (check_dims(what, nx, ny, nz)) return -1;
    if (n_faces == 0) return 0;
    PSCV_CHECK_ARG(info && vincl && fincl && faces, "%s: null pointer argument", what);
    const long nvox = (long)nx * ny * nz;
    return launch(what, tsdf_emit_faces_kernel, dim3((unsigned)((nvox + 255) / 256)), dim3(256), 0,
                  reinterpret_cast<hipStream_t>(stream), info, vincl, fincl, nx, ny, nvox, faces, n_faces);
}

extern "C" int pscv_tsdf_case_table(unsigned int* table) {
    PSCV_CHECK_ARG(table, "pscv_tsdf_case_table: null pointer argument");
    for (int n = 0; n < 6 * 16; ++n) table[n] = pscv::H_TET_TABLE.e[n];
    return 0;
}
