// The TSDF volume of tsdf_fusion.hip in a second storage layout: a pool of 8 x 8 x 8 bricks, allocated only where the surface can
// be, behind a dense directory of brick slots.  gfx950.  The rule is the dense one (tsdf_dev.h, built
// with -ffp-contract=off like tsdf_fusion.hip); the mesh is the dense mesh, the same vertices, colours and triangles as sets.
//
// Lattice: (nx, ny, nz) points at o + i s with the lattice's own index i, lin = (k ny + j) nx + i in int64 (the lattice may hold
// more than 2^31 points).  Bricks of B = 8: nb* = ceil(n* / 8), nbx nby nbz < 2^31, brick (bx, by, bz) has the linear index
// (bz nby + by) nbx + bx.  directory int32 [nbz][nby][nbx]: the brick's slot in the pool, -1 = not allocated; brick_ids int32 [n]:
// the brick of every slot, ascending; n < 2^22, so a pool voxel index slot 512 + (z 8 + y) 8 + x fits int32.
// Pool: tsdf_sum, weight, cweight [n][8][8][8], rgb_sum [n][8][8][8][3]; pool voxels outside the lattice stay zero.
//
// pscv_tsdf_brick_probe decides, before any view is integrated, where the surface can be: a lattice point is TOUCHED when some
// view updates it with -trunc <= sd <= trunc; a brick is allocated iff it holds a touched point or one of its 26 neighbours.  The
// probe writes per brick a 27-bit mask of the neighbour bricks (itself included) its touched points ask for; the caller ORs the
// shifted masks (torch), numbers the allocated bricks and sizes the pool.
// pscv_tsdf_brick_integrate runs steps 1-6 of the rule on every lattice point of every allocated brick.
// pscv_tsdf_brick_mark / _emit_vertices / _emit_faces are the dense extraction with "in the grid" read as "in the lattice and in
// an allocated brick"; vertices and faces are ordered by pool voxel, and a face starts at its vertex of the smallest KEY
// lin(p) 7 + (d - 1), which in the dense layout is the smallest index: every quad is cut as the dense one.
#include "tsdf_dev.h"

#include <limits.h>

namespace pscv {

constexpr int BRICK = 8, BRICK_VOX = BRICK * BRICK * BRICK;                  // 512
constexpr int MAX_BRICKS = (1 << 22) - 1;

struct BrickGrid {
    const int* directory;       // [nbz][nby][nbx]
    const int* brick_ids;       // [n]
    int n, nbx, nby, nbz;
};

struct TsdfBrickArgs {
    TsdfArgs v;                 // the views and the lattice; the four state pointers are the pool's (null for the probe)
    const float* dmin;          // probe: [n_views] the smallest valid depth of each view (+inf when it has none)
    int* masks;                 // probe: [nbz][nby][nbx]
    const int* brick_ids;       // integrate: [n]
    int nbx, nby, nbz;
};
static_assert(sizeof(TsdfBrickArgs) <= 4096, "the kernel-argument segment holds 4 KB");

// local voxel l = (z 8 + y) 8 + x of brick b -> lattice index; false outside the lattice (or for a brick outside the directory)
__device__ __forceinline__ bool brick_voxel(int b, int l, int nbx, int nby, int nbz, int nx, int ny, int nz, int& i, int& j, int& k) {
    const int bz = b / (nbx * nby), rem = b - bz * (nbx * nby), by = rem / nbx, bx = rem - by * nbx;
    i = bx * BRICK + (l & 7), j = by * BRICK + (l >> 3 & 7), k = bz * BRICK + (l >> 6);
    return b >= 0 && bz < nbz && i < nx && j < ny && k < nz;
}

// pool voxel index of the lattice point (i, j, k), which the caller has checked to lie in the lattice; -1 = its brick is not allocated
__device__ __forceinline__ int pool_index(const BrickGrid& g, int i, int j, int k) {
    const int slot = g.directory[((long)(k >> 3) * g.nby + (j >> 3)) * g.nbx + (i >> 3)];
    if (slot < 0 || slot >= g.n) return -1;                                   // (a directory that is not the pool's reads nothing outside)
    return slot * BRICK_VOX + ((k & 7) * BRICK + (j & 7)) * BRICK + (i & 7);
}

// The brick's box, clipped to the lattice, judged by lane v of wave 0 for view v
template <bool PROBE>
__device__ __forceinline__ bool brick_view_live(const TsdfBrickArgs& a, int b, int v) {
    const TsdfArgs& t = a.v;
    const int bz = b / (a.nbx * a.nby), rem = b - bz * (a.nbx * a.nby), by = rem / a.nbx, bx = rem - by * a.nbx;
    const int i0 = bx * BRICK, j0 = by * BRICK, k0 = bz * BRICK;
    const int i1 = min(i0 + BRICK, t.nx) - 1, j1 = min(j0 + BRICK, t.ny) - 1, k1 = min(k0 + BRICK, t.nz) - 1;
    if (i1 < i0 || j1 < j0 || k1 < k0) return false;                          // (a brick id outside the directory: no lattice point)
    const double gx[2] = {t.o0 + (double)i0 * t.s, t.o0 + (double)i1 * t.s};
    const double gy[2] = {t.o1 + (double)j0 * t.s, t.o1 + (double)j1 * t.s};
    const double gz[2] = {t.o2 + (double)k0 * t.s, t.o2 + (double)k1 * t.s};
    // (per-lane indexing of the by-value argument struct: loads from the kernel-argument segment, as in the dense kernel)
    return !tile_culled<PROBE>(t.cams + (long)v * PSCV_GEO_CAM_FLOATS, (double)t.w[v], (double)t.h[v], (double)t.dmax[v], t.trunc, gx, gy,
                               gz, PROBE ? (double)a.dmin[v] : 0.0);
}

// ---- probe: one workgroup per directory brick, two voxels per lane ---------------------------------------------------------------
constexpr int TP_THREADS = 256;
constexpr long TP_GRID_X = 1L << 22;

// the neighbour bricks a touched voxel at local (x, y, z) asks for: bit (dz+1) 9 + (dy+1) 3 + (dx+1), d* = 0, -1 at 0, +1 at 7
__device__ __forceinline__ unsigned brick_requests(int l) {
    const int x = l & 7, y = l >> 3 & 7, z = l >> 6;
    const unsigned ax = 2u | (x == 0 ? 1u : 0u) | (x == 7 ? 4u : 0u);       // bits over dx + 1
    const unsigned ay = 2u | (y == 0 ? 1u : 0u) | (y == 7 ? 4u : 0u);
    const unsigned az = 2u | (z == 0 ? 1u : 0u) | (z == 7 ? 4u : 0u);
    unsigned row = 0, req = 0;
#pragma unroll
    for (int n = 0; n < 3; ++n)
        if (ay >> n & 1u) row |= ax << (3 * n);
#pragma unroll
    for (int n = 0; n < 3; ++n)
        if (az >> n & 1u) req |= row << (9 * n);
    return req;
}

__global__ __launch_bounds__(TP_THREADS) void tsdf_brick_probe_kernel(const TsdfBrickArgs a) {
    __shared__ unsigned long long s_live;
    __shared__ unsigned s_mask;
    const int tid = threadIdx.x;
    const TsdfArgs& t = a.v;
    const long bl = (long)blockIdx.y * gridDim.x + blockIdx.x;               // (two grid axes: 2^31 bricks of 256 lanes exceed one)
    if (bl >= (long)a.nbx * a.nby * a.nbz) return;
    const int b = (int)bl;
    if (tid == 0) s_mask = 0u;
    const bool keep = tid < t.n_views && brick_view_live<true>(a, b, tid);
    const unsigned long long live = tsdf_share_live(s_live, tid < 64, keep);  // (the barrier also publishes s_mask = 0)
    if (live == 0) return;
    unsigned acc = 0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int l = tid + half * TP_THREADS;
        int i, j, k;
        if (!brick_voxel(b, l, a.nbx, a.nby, a.nbz, t.nx, t.ny, t.nz, i, j, k)) continue;     // outside the lattice: never touched
        const double X = t.o0 + (double)i * t.s, Y = t.o1 + (double)j * t.s, Z = t.o2 + (double)k * t.s;
        unsigned long long left = live;
        while (left) {
            const int v = __builtin_ctzll(left);
            left &= left - 1;
            double sd;
            long o;
            if (tsdf_view_sd(t, v, X, Y, Z, sd, o) && sd <= t.trunc) {
                acc |= brick_requests(l);
                break;                                                        // (a voxel's requests do not grow with a second touch)
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc |= (unsigned)__shfl_xor((int)acc, off);
    if ((tid & 63) == 0 && acc) atomicOr(&s_mask, acc);                       // (LDS)
    __syncthreads();
    if (tid == 0 && s_mask) a.masks[b] |= (int)s_mask;                        // (this workgroup owns masks[b]; calls are stream-ordered)
}

// ---- integration: one workgroup per allocated brick; a wave moves 256 contiguous bytes of every 4-byte array --------------------------
// 512 lanes with one voxel each, or 256 lanes that take the brick's two halves one after the other (PSCV_TSDF_BRICK_LANES, a
// build-time choice: INTEGRATION.md section 2q has the measurement)
#ifndef PSCV_TSDF_BRICK_LANES
#define PSCV_TSDF_BRICK_LANES 512
#endif
constexpr int TB_THREADS = PSCV_TSDF_BRICK_LANES, TB_PER_LANE = BRICK_VOX / TB_THREADS;
static_assert(TB_THREADS == 512 || TB_THREADS == 256, "one or two voxels per lane");

__global__ __launch_bounds__(TB_THREADS) void tsdf_brick_integrate_kernel(const TsdfBrickArgs a) {
    __shared__ unsigned long long s_live;
    const int tid = threadIdx.x, slot = blockIdx.x;
    const TsdfArgs& t = a.v;
    const int b = a.brick_ids[slot];
    const bool keep = tid < t.n_views && brick_view_live<false>(a, b, tid);
    const unsigned long long live = tsdf_share_live(s_live, tid < 64, keep);
    if (live == 0) return;
#pragma unroll
    for (int r = 0; r < TB_PER_LANE; ++r) {
        const int l = tid + r * TB_THREADS;
        int i, j, k;
        if (!brick_voxel(b, l, a.nbx, a.nby, a.nbz, t.nx, t.ny, t.nz, i, j, k)) continue;     // pool voxels outside the lattice stay zero
        tsdf_update_voxel(t, live, (long)slot * BRICK_VOX + l, t.o0 + (double)i * t.s, t.o1 + (double)j * t.s, t.o2 + (double)k * t.s);
    }
}

// ---- extraction ------------------------------------------------------------------------------------------------------------------
constexpr int TK_P = BRICK + 1, TK_HALO = TK_P * TK_P * TK_P;                // 729

__global__ __launch_bounds__(BRICK_VOX) void tsdf_brick_mark_kernel(const float* __restrict__ tsdf_sum, const int* __restrict__ weight,
                                                                    const BrickGrid g, int nx, int ny, int nz, int min_weight,
                                                                    int* __restrict__ info) {
    __shared__ unsigned char fl[TK_HALO];
    const int tid = threadIdx.x, slot = blockIdx.x;
    const int b = g.brick_ids[slot];
    int i0, j0, k0;
    const bool in_dir = brick_voxel(b, 0, g.nbx, g.nby, g.nbz, nx, ny, nz, i0, j0, k0);
    for (int n = tid; n < TK_HALO; n += BRICK_VOX) {             // the brick and its +1 halo; outside the lattice or not allocated = unobserved
        const int lz = n / (TK_P * TK_P), r2 = n - lz * (TK_P * TK_P), ly = r2 / TK_P, lx = r2 - ly * TK_P;
        const int i = i0 + lx, j = j0 + ly, k = k0 + lz;
        unsigned f = 0;
        if (in_dir && i < nx && j < ny && k < nz) {
            const int p = pool_index(g, i, j, k);
            if (p >= 0) f = tsdf_flags(tsdf_sum[p], weight[p], min_weight);
        }
        fl[n] = (unsigned char)f;
    }
    __syncthreads();
    const int lx = tid & 7, ly = tid >> 3 & 7, lz = tid >> 6;
    unsigned cf[8];                                                          // flags of the cell's eight corners
#pragma unroll
    for (int c = 0; c < 8; ++c) cf[c] = fl[((lz + (c >> 2)) * TK_P + ly + (c >> 1 & 1)) * TK_P + lx + (c & 1)];
    info[(long)slot * BRICK_VOX + tid] = tsdf_cell_info(cf);                 // (0 for a pool voxel outside the lattice)
}

__global__ __launch_bounds__(256) void tsdf_brick_emit_vertices_kernel(const float* __restrict__ tsdf_sum, const int* __restrict__ weight,
                                                                       const float* __restrict__ rgb_sum, const int* __restrict__ cweight,
                                                                       const int* __restrict__ info, const int* __restrict__ vincl,
                                                                       const BrickGrid g, int nx, int ny, int nz, double o0, double o1,
                                                                       double o2, double s, float* __restrict__ xyz,
                                                                       unsigned char* __restrict__ rgb, long* __restrict__ keys,
                                                                       long n_vertices) {
    const int p = blockIdx.x * 256 + threadIdx.x;                            // (n 512 < 2^31)
    if (p >= g.n * BRICK_VOX) return;
    const unsigned f = (unsigned)info[p];
    const unsigned mask = f & 127u;
    if (!mask) return;
    int i, j, k;
    if (!brick_voxel(g.brick_ids[p >> 9], p & 511, g.nbx, g.nby, g.nbz, nx, ny, nz, i, j, k)) return;
    long out = (long)vincl[p] - (long)(f >> 16 & 255u);
    const TsdfVal P = load_val(tsdf_sum, weight, rgb_sum, cweight, p);
    const double Xp[3] = {o0 + (double)i * s, o1 + (double)j * s, o2 + (double)k * s};
    const long lin = ((long)k * ny + j) * nx + i;
    for (int d = 1; d < 8; ++d) {
        if (!(mask >> (d - 1) & 1u)) continue;
        const int iq = i + (d & 1), jq = j + (d >> 1 & 1), kq = k + (d >> 2);
        const int pq = iq < nx && jq < ny && kq < nz ? pool_index(g, iq, jq, kq) : -1;
        if (pq >= 0 && out >= 0 && out < n_vertices) {            // (a mask or prefix sums that are not pscv_tsdf_brick_mark's read and write nothing outside)
            const TsdfVal Q = load_val(tsdf_sum, weight, rgb_sum, cweight, pq);
            const double Xq[3] = {o0 + (double)iq * s, o1 + (double)jq * s, o2 + (double)kq * s};
            tsdf_write_vertex(P, Q, Xp, Xq, xyz, rgb, out);
            if (keys) keys[out] = lin * 7 + (d - 1);
        }
        ++out;
    }
}

__global__ __launch_bounds__(256) void tsdf_brick_emit_faces_kernel(const int* __restrict__ info, const int* __restrict__ vincl,
                                                                    const int* __restrict__ fincl, const BrickGrid g, int nx, int ny,
                                                                    int nz, int* __restrict__ faces, long n_faces) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= g.n * BRICK_VOX) return;
    const unsigned nf = (unsigned)info[p] >> 24;
    if (!nf) return;
    int i, j, k;
    if (!brick_voxel(g.brick_ids[p >> 9], p & 511, g.nbx, g.nby, g.nbz, nx, ny, nz, i, j, k)) return;
    if (i + 1 >= nx || j + 1 >= ny || k + 1 >= nz) return;       // (pscv_tsdf_brick_mark counts faces only where all eight corners are in the lattice)
    unsigned obs = 0, neg = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int pc = pool_index(g, i + (c & 1), j + (c >> 1 & 1), k + (c >> 2));
        const unsigned fc = pc >= 0 ? (unsigned)info[pc] >> 8 : 0u;
        obs |= (fc & 1u) << c;
        neg |= (fc >> 1 & 1u) << c;
    }
    const long lin = ((long)k * ny + j) * nx + i;
    long out = (long)fincl[p] - (long)nf;
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
        long key[4];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const unsigned code = e >> (3 + 6 * n) & 63u;                     // (n >= cnt: not used)
            const int c = (int)(code & 7u), d = (int)(code >> 3);
            q[n] = 0x7fffffff, key[n] = LONG_MAX;
            if (n < cnt) {                                                    // (the corner is observed, so its brick is allocated: pc >= 0)
                const int pc = pool_index(g, i + (c & 1), j + (c >> 1 & 1), k + (c >> 2));
                if (pc >= 0) q[n] = edge_vertex(info, vincl, pc, d);
                key[n] = (lin + (c & 1) + (long)(c >> 1 & 1) * nx + (long)(c >> 2) * nx * ny) * 7 + (d - 1);
            }
        }
        tsdf_write_faces(q, key, cnt, faces, out, n_faces);
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static int check_lattice(const char* what, int nx, int ny, int nz, int& nbx, int& nby, int& nbz) {
    PSCV_CHECK_ARG(nx >= 1 && ny >= 1 && nz >= 1 && nx <= INT_MAX - BRICK && ny <= INT_MAX - BRICK && nz <= INT_MAX - BRICK,
                   "%s: dims %dx%dx%d must be positive", what, nx, ny, nz);
    nbx = (nx + BRICK - 1) / BRICK, nby = (ny + BRICK - 1) / BRICK, nbz = (nz + BRICK - 1) / BRICK;
    PSCV_CHECK_ARG((long)nbx * nby < (1L << 31) && (long)nbx * nby * nbz < (1L << 31),
                   "%s: dims %dx%dx%d need %dx%dx%d bricks: nbx nby nbz must stay below 2^31", what, nx, ny, nz, nbx, nby, nbz);
    return 0;
}

static int check_pool(const char* what, int n_bricks) {
    PSCV_CHECK_ARG(n_bricks >= 0 && n_bricks <= MAX_BRICKS, "%s: n_bricks=%d outside [0, 2^22)", what, n_bricks);
    return 0;
}

}  // namespace pscv

extern "C" int pscv_tsdf_brick_probe(const float* const* depth, const int* hw, int n_views, const float* cams, const float* dmax,
                                     const float* dmin, double o0, double o1, double o2, double voxel, double trunc, int nx, int ny,
                                     int nz, int* masks, void* stream) {
    using namespace pscv;
    const char* what = "pscv_tsdf_brick_probe";
    PSCV_CHECK_ARG(depth && hw && cams && dmax && dmin && masks, "%s: null pointer argument", what);
    TsdfBrickArgs a;
    if (check_lattice(what, nx, ny, nz, a.nbx, a.nby, a.nbz)) return -1;
    if (tsdf_setup(what, a.v, depth, nullptr, hw, n_views, cams, dmax, o0, o1, o2, voxel, trunc, nx, ny, nz, false)) return -1;
    a.dmin = dmin, a.masks = masks, a.brick_ids = nullptr;
    const long bricks = (long)a.nbx * a.nby * a.nbz, gx = bricks < TP_GRID_X ? bricks : TP_GRID_X;
    return launch(what, tsdf_brick_probe_kernel, dim3((unsigned)gx, (unsigned)((bricks + gx - 1) / gx)), dim3(TP_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
}

extern "C" int pscv_tsdf_brick_integrate(const float* const* depth, const unsigned int* const* color, const int* hw, int n_views,
                                         const float* cams, const float* dmax, double o0, double o1, double o2, double voxel,
                                         double trunc, int nx, int ny, int nz, const int* brick_ids, int n_bricks, float* tsdf_sum,
                                         int* weight, float* rgb_sum, int* cweight, void* stream) {
    using namespace pscv;
    const char* what = "pscv_tsdf_brick_integrate";
    PSCV_CHECK_ARG(depth && color && hw && cams && dmax, "%s: null pointer argument", what);
    TsdfBrickArgs a;
    if (check_lattice(what, nx, ny, nz, a.nbx, a.nby, a.nbz)) return -1;
    if (check_pool(what, n_bricks)) return -1;
    if (tsdf_setup(what, a.v, depth, color, hw, n_views, cams, dmax, o0, o1, o2, voxel, trunc, nx, ny, nz, false)) return -1;
    if (n_bricks == 0) return 0;
    PSCV_CHECK_ARG(brick_ids && tsdf_sum && weight && rgb_sum && cweight, "%s: null pointer argument", what);
    a.v.tsdf_sum = tsdf_sum, a.v.weight = weight, a.v.rgb_sum = rgb_sum, a.v.cweight = cweight;
    a.dmin = nullptr, a.masks = nullptr, a.brick_ids = brick_ids;
    return launch(what, tsdf_brick_integrate_kernel, dim3((unsigned)n_bricks), dim3(TB_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
}

extern "C" int pscv_tsdf_brick_mark(const float* tsdf_sum, const int* weight, const int* directory, const int* brick_ids, int n_bricks,
                                    int nx, int ny, int nz, int min_weight, int* info, void* stream) {
    using namespace pscv;
    const char* what = "pscv_tsdf_brick_mark";
    BrickGrid g{directory, brick_ids, n_bricks, 0, 0, 0};
    PSCV_CHECK_ARG(min_weight >= 1, "%s: min_weight=%d must be at least 1", what, min_weight);
    if (check_lattice(what, nx, ny, nz, g.nbx, g.nby, g.nbz)) return -1;
    if (check_pool(what, n_bricks)) return -1;
    if (n_bricks == 0) return 0;
    PSCV_CHECK_ARG(tsdf_sum && weight && directory && brick_ids && info, "%s: null pointer argument", what);
    return launch(what, tsdf_brick_mark_kernel, dim3((unsigned)n_bricks), dim3(BRICK_VOX), 0, reinterpret_cast<hipStream_t>(stream),
                  tsdf_sum, weight, g, nx, ny, nz, min_weight, info);
}

extern "C" int pscv_tsdf_brick_emit_vertices(const float* tsdf_sum, const int* weight, const float* rgb_sum, const int* cweight,
                                             const int* info, const int* vincl, const int* directory, const int* brick_ids,
                                             int n_bricks, int nx, int ny, int nz, double o0, double o1, double o2, double voxel,
                                             float* xyz, unsigned char* rgb, long* keys, long n_vertices, void* stream) {
    using namespace pscv;
    const char* what = "pscv_tsdf_brick_emit_vertices";
    BrickGrid g{directory, brick_ids, n_bricks, 0, 0, 0};
    PSCV_CHECK_ARG(n_vertices >= 0 && n_vertices < (1L << 31), "%s: n_vertices=%ld outside [0, 2^31)", what, n_vertices);
    if (check_grid(what, o0, o1, o2, voxel)) return -1;
    if (check_lattice(what, nx, ny, nz, g.nbx, g.nby, g.nbz)) return -1;
    if (check_pool(what, n_bricks)) return -1;
    if (n_vertices == 0 || n_bricks == 0) return 0;
    PSCV_CHECK_ARG(tsdf_sum && weight && rgb_sum && cweight && info && vincl && directory && brick_ids && xyz && rgb,
                   "%s: null pointer argument", what);
    return launch(what, tsdf_brick_emit_vertices_kernel, dim3((unsigned)n_bricks * 2u), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                  tsdf_sum, weight, rgb_sum, cweight, info, vincl, g, nx, ny, nz, o0, o1, o2, voxel, xyz, rgb, keys, n_vertices);
}

extern "C" int pscv_tsdf_brick_emit_faces(const int* info, const int* vincl, const int* fincl, const int* directory,
                                          const int* brick_ids, int n_bricks, int nx, int ny, int nz, int* faces, long n_faces,
                                          void* stream) {
    using namespace pscv;
    const char* what = "pscv_tsdf_brick_emit_faces";
    BrickGrid g{directory, brick_ids, n_bricks, 0, 0, 0};
    PSCV_CHECK_ARG(n_faces >= 0 && n_faces < (1L << 31), "%s: n_faces=%ld outside [0, 2^31)", what, n_faces);
    if (check_lattice(what, nx, ny, nz, g.nbx, g.nby, g.nbz)) return -1;
    if (check_pool(what, n_bricks)) return -1;
    if (n_faces == 0 || n_bricks == 0) return 0;
    PSCV_CHECK_ARG(info && vincl && fincl && directory && brick_ids && faces, "%s: null pointer argument", what);
    return launch(what, tsdf_brick_emit_faces_kernel, dim3((unsigned)n_bricks * 2u), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                  info, vincl, fincl, g, nx, ny, nz, faces, n_faces);
}
