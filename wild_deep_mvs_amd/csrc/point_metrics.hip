// Point-cloud metrics (the step after fusion): sparse uniform grids, bounded nearest-neighbour distances and the radius
// maximal independent set behind reduce_pts.  gfx950.  INTEGRATION.md section 2f states the rules.
//
// Grid of a point set (pscv_point_grid_build): a 64-bit cell key per point (21 bits per axis, cells of `cell` from `origin`)
// goes into an open-addressing hash table (linear probing, integer atomicCAS), the points of a slot are counted with integer
// atomics, the counts are scanned (chunk sums, one-workgroup scan of the chunk sums, local scans) and the points are scattered
// into slot order as float4 (x, y, z, original index bits).  No sort, nothing dense over the bounding box.  The order of the
// points inside a slot depends on scheduling; every result below is a min / an exists / a rank comparison over a cell's
// points, so none depends on it.
//
// Bounded nearest neighbour (pscv_point_nn_dist): rings of the fine grid around the query's cell, stopped as soon as the ring
// radius passes the best squared distance; then the cells of a coarse grid of the same points within `maxdist`, ring by ring,
// each pruned by its box distance.  Distances are fp64 from the fp32 coordinates; a candidate counts when d^2 < maxdist^2
// (strict, as scipy's distance_upper_bound).  The DTU mode adds the reference's 60 mm blocking (metrics.py::chamfer).
//
// Radius MIS (pscv_radius_mis_round): one round reads the previous state of every point and writes the next one:
// an undecided point with a kept neighbour (d <= dst, fp64) becomes removed; otherwise, with no undecided neighbour of lower
// rank, it becomes kept.  The fixed point is the greedy MIS in rank order, which is what metrics.py::reduce_pts computes.
//
// This file is compiled with -ffp-contract=off: the DTU cell bounds must be the reference's fp64 sums, not fused products.
//
// Replaces (fdarmon/wild_deep_mvs): evaluation/metrics.py reduce_pts, chamfer, chamfer_imw (scipy cKDTree).
#include "geo_common.h"

namespace pscv {

constexpr int PM_THREADS = 256;
constexpr int PM_SCAN_PER = 16;
constexpr int PM_CHUNK = PM_THREADS * PM_SCAN_PER;         // items per scan workgroup
constexpr int PM_SCAN1_THREADS = 1024;
constexpr int PM_KEY_BITS = 21;
constexpr long PM_KEY_SPAN = 1L << PM_KEY_BITS;             // cells per axis a grid can address
constexpr unsigned long long PM_EMPTY = ~0ull;              // (a key never has bit 63 set)
constexpr long PM_MAX_POINTS = 1L << 30;                    // (slot indices of the 2n-slot table stay below 2^31)
constexpr double PM_COORD_CLAMP = 1099511627776.0;          // 2^40: query cell coordinates are clamped before the cast

struct GridView {
    const unsigned long long* keys;     // [cap]
    const int2* cells;                  // [cap]: (start, count) in slot order
    const float4* pts;                  // [n]: x, y, z, original index bits
    const int* payload;                 // [n] in slot order
    unsigned long long mask;            // cap - 1
    double ox, oy, oz, cell;
};

__device__ __forceinline__ unsigned long long pm_hash(unsigned long long k) {      // splitmix64 finaliser
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    return k ^ (k >> 31);
}
__device__ __forceinline__ long pm_cell(double v, double o, double cell) {
    const double c = fmin(fmax(floor((v - o) / cell), -PM_COORD_CLAMP), PM_COORD_CLAMP);    // (NaN -> -clamp)
    return (long)c;
}
__device__ __forceinline__ bool pm_in_span(long x, long y, long z) {
    return x >= 0 && x < PM_KEY_SPAN && y >= 0 && y < PM_KEY_SPAN && z >= 0 && z < PM_KEY_SPAN;
}
__device__ __forceinline__ unsigned long long pm_key(long x, long y, long z) {
    return (unsigned long long)x | ((unsigned long long)y << PM_KEY_BITS) | ((unsigned long long)z << (2 * PM_KEY_BITS));
}
// (start, count) of a cell; count 0 when the cell is empty or outside the addressable span
__device__ __forceinline__ int2 pm_lookup(const GridView& g, long x, long y, long z) {
    if (!pm_in_span(x, y, z)) return make_int2(0, 0);
    const unsigned long long key = pm_key(x, y, z);
    unsigned long long h = pm_hash(key) & g.mask;
    for (;;) {
        const unsigned long long k = g.keys[h];
        if (k == key) return g.cells[h];
        if (k == PM_EMPTY) return make_int2(0, 0);
        h = (h + 1) & g.mask;
    }
}
__device__ __forceinline__ double pm_d2(double x, double y, double z, const float4 p) {
    const double dx = x - (double)p.x, dy = y - (double)p.y, dz = z - (double)p.z;
    return dx * dx + dy * dy + dz * dz;
}
// squared distance from (x, y, z) to the box of cell (cx, cy, cz), shrunk by a relative slack (conservative for pruning)
__device__ __forceinline__ double pm_box_d2(const GridView& g, double x, double y, double z, long cx, long cy, long cz) {
    auto gap = [&](double v, double o, long c) {
        const double lo = o + (double)c * g.cell, hi = lo + g.cell;
        return fmax(fmax(lo - v, v - hi), 0.0);
    };
    const double a = gap(x, g.ox, cx), b = gap(y, g.oy, cy), c = gap(z, g.oz, cz);
    return (a * a + b * b + c * c) * (1.0 - 1e-9);
}

// ---------------------------------------------------------------------------------------------------------------------------
// workgroup scan helpers
__device__ __forceinline__ int pm_block_sum(int v, int* lds) {           // sum over PM_THREADS lanes (4 waves)
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    const int s = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return s;
}
__device__ __forceinline__ int pm_block_exclusive(int v, int* lds) {     // exclusive prefix over PM_THREADS lanes, Hillis-Steele
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < PM_THREADS; off <<= 1) {
        const int a = threadIdx.x >= off ? lds[threadIdx.x - off] : 0;
        __syncthreads();
        lds[threadIdx.x] += a;
        __syncthreads();
    }
    const int r = lds[threadIdx.x] - v;
    __syncthreads();
    return r;
}

template <typename T>
__global__ __launch_bounds__(PM_THREADS) void pm_chunk_sum_kernel(const T* __restrict__ in, long n, int* __restrict__ bsum) {
    __shared__ int lds[4];
    const long base = (long)blockIdx.x * PM_CHUNK;
    int s = 0;
    for (int j = 0; j < PM_SCAN_PER; ++j) {
        const long k = base + (long)j * PM_THREADS + threadIdx.x;
        if (k < n) s += (int)in[k];
    }
    s = pm_block_sum(s, lds);
    if (threadIdx.x == 0) bsum[blockIdx.x] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------
// grid build
__global__ __launch_bounds__(PM_THREADS) void pm_insert_kernel(const float* __restrict__ pts, long n, double ox, double oy, double oz,
                                                               double cell, unsigned long long* keys, int* counts, unsigned long long mask,
                                                               int* __restrict__ slot_of, int* __restrict__ pos, unsigned int* occupied) {
    const long i = (long)blockIdx.x * PM_THREADS + threadIdx.x;
    if (i >= n) return;
    const long cx = min(max(pm_cell((double)pts[3 * i], ox, cell), 0L), PM_KEY_SPAN - 1);
    const long cy = min(max(pm_cell((double)pts[3 * i + 1], oy, cell), 0L), PM_KEY_SPAN - 1);
    const long cz = min(max(pm_cell((double)pts[3 * i + 2], oz, cell), 0L), PM_KEY_SPAN - 1);
    const unsigned long long key = pm_key(cx, cy, cz);
    unsigned long long h = pm_hash(key) & mask;
    for (;;) {                        // the table holds at least 2n slots, so a free one exists
        const unsigned long long prev = atomicCAS(&keys[h], PM_EMPTY, key);
        if (prev == PM_EMPTY || prev == key) {
            if (prev == PM_EMPTY) atomicAdd(occupied, 1u);
            break;
        }
        h = (h + 1) & mask;
    }
    slot_of[i] = (int)h;
    pos[i] = atomicAdd(&counts[h], 1);
}

__global__ __launch_bounds__(PM_THREADS) void pm_cells_kernel(const int* __restrict__ counts, long cap, const int* __restrict__ boff,
                                                              int2* __restrict__ cells) {
    __shared__ int lds[PM_THREADS];
    const long base = (long)blockIdx.x * PM_CHUNK + (long)threadIdx.x * PM_SCAN_PER;
    int v[PM_SCAN_PER];
    int s = 0;
    for (int j = 0; j < PM_SCAN_PER; ++j) {
        v[j] = base + j < cap ? counts[base + j] : 0;
        s += v[j];
    }
    int run = boff[blockIdx.x] + pm_block_exclusive(s, lds);
    for (int j = 0; j < PM_SCAN_PER; ++j) {
        if (base + j < cap) cells[base + j] = make_int2(run, v[j]);
        run += v[j];
    }
}

__global__ __launch_bounds__(PM_THREADS) void pm_scatter_kernel(const float* __restrict__ pts, long n, const int* __restrict__ slot_of,
                                                                const int* __restrict__ pos, const int2* __restrict__ cells,
                                                                const int* __restrict__ payload_in, float4* __restrict__ out,
                                                                int* __restrict__ payload) {
    const long i = (long)blockIdx.x * PM_THREADS + threadIdx.x;
    if (i >= n) return;
    const long sp = (long)cells[slot_of[i]].x + pos[i];
    out[sp] = make_float4(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], __int_as_float((int)i));
    if (payload_in) payload[sp] = payload_in[i];
}

// ---------------------------------------------------------------------------------------------------------------------------
// bounded nearest neighbour
struct NNArgs {
    GridView fine, coarse;
    const float* query;
    double* out;
    long m;
    double maxdist, maxdist2;
    int fine_rings, coarse_rings;
    // DTU blocking (dtu != 0): cells [bb0 + x md, bb0 + x md + md) for x in 0..na on each axis; occ [(na+1)^3] flags a target in
    // the cell's expanded box [low - md, high + md)
    int dtu;
    double bb0[3];
    int na[3];
    const int* occ;
};

// the largest x in 0..na with low <= v < high (the reference overwrites earlier cells), or -1
__device__ __forceinline__ int pm_dtu_cell(double v, double b0, double md, int na) {
    const double f = floor((v - b0) / md);
    if (!(f >= -2.0 && f <= (double)na + 2.0)) return -1;
    const int c = (int)f;
    for (int x = min(c + 1, na); x >= max(c - 1, 0); --x) {
        const double low = b0 + (double)x * md, high = low + md;
        if (low <= v && v < high) return x;
    }
    return -1;
}

// scan one cell's points; `best` / `found` keep the smallest d^2 < best (inside the DTU expanded box when `box`)
__device__ __forceinline__ void pm_scan_cell(const GridView& g, int2 se, double x, double y, double z, double& best, bool& found,
                                             bool box, const double* blo, const double* bhi) {
    for (int k = se.x; k < se.x + se.y; ++k) {
        const float4 p = g.pts[k];
        const double d2 = pm_d2(x, y, z, p);
        if (d2 < best) {
            if (box && !((double)p.x >= blo[0] && (double)p.x < bhi[0] && (double)p.y >= blo[1] && (double)p.y < bhi[1] &&
                         (double)p.z >= blo[2] && (double)p.z < bhi[2]))
                continue;
            best = d2;
            found = true;
        }
    }
}

// rings 0..rings of grid g around the query's cell, stopped once the next ring lies beyond `best`
__device__ __forceinline__ bool pm_ring_search(const GridView& g, int rings, double x, double y, double z, double& best, bool& found,
                                               bool box, const double* blo, const double* bhi) {
    const long cx = pm_cell(x, g.ox, g.cell), cy = pm_cell(y, g.oy, g.cell), cz = pm_cell(z, g.oz, g.cell);
    for (int r = 0; r <= rings; ++r) {
        for (int dz = -r; dz <= r; ++dz)
            for (int dy = -r; dy <= r; ++dy)
                for (int dx = -r; dx <= r; ++dx) {
                    if (max(abs(dx), max(abs(dy), abs(dz))) != r) continue;
                    const long ex = cx + dx, ey = cy + dy, ez = cz + dz;
                    if (!pm_in_span(ex, ey, ez)) continue;
                    if (pm_box_d2(g, x, y, z, ex, ey, ez) >= best) continue;
                    const int2 se = pm_lookup(g, ex, ey, ez);
                    if (se.y) pm_scan_cell(g, se, x, y, z, best, found, box, blo, bhi);
                }
        // every point outside rings 0..r lies at least r cells from the query
        const double reach = (double)r * g.cell * (1.0 - 1e-9);
        if (reach * reach >= best) return true;
    }
    return false;
}

__global__ __launch_bounds__(PM_THREADS) void pm_nn_kernel(const NNArgs a) {
    const long i = (long)blockIdx.x * PM_THREADS + threadIdx.x;
    if (i >= a.m) return;
    const double x = (double)a.query[3 * i], y = (double)a.query[3 * i + 1], z = (double)a.query[3 * i + 2];
    double blo[3] = {0.0, 0.0, 0.0}, bhi[3] = {0.0, 0.0, 0.0};
    if (a.dtu) {
        const int c0 = pm_dtu_cell(x, a.bb0[0], a.maxdist, a.na[0]);
        const int c1 = pm_dtu_cell(y, a.bb0[1], a.maxdist, a.na[1]);
        const int c2 = pm_dtu_cell(z, a.bb0[2], a.maxdist, a.na[2]);
        if (c0 < 0 || c1 < 0 || c2 < 0 || a.occ[((long)c0 * (a.na[1] + 1) + c1) * (a.na[2] + 1) + c2] == 0) {
            a.out[i] = a.maxdist;                   // (a) in no cell, (b) no target in the expanded box
            return;
        }
        const int c[3] = {c0, c1, c2};
        for (int d = 0; d < 3; ++d) {
            const double low = a.bb0[d] + (double)c[d] * a.maxdist, high = low + a.maxdist;
            blo[d] = low - a.maxdist;
            bhi[d] = high + a.maxdist;
        }
    }
    double best = a.maxdist2;
    bool found = false;
    if (!pm_ring_search(a.fine, a.fine_rings, x, y, z, best, found, a.dtu != 0, blo, bhi))
        pm_ring_search(a.coarse, a.coarse_rings, x, y, z, best, found, a.dtu != 0, blo, bhi);
    a.out[i] = found ? sqrt(best) : (double)INFINITY;
}

// occ[x][y][z] = 1 when some target lies in the expanded box of DTU cell (x, y, z)
__global__ __launch_bounds__(PM_THREADS) void pm_dtu_occ_kernel(const float* __restrict__ pts, long n, double b00, double b01, double b02,
                                                                double md, int na0, int na1, int na2, int* occ) {
    const long i = (long)blockIdx.x * PM_THREADS + threadIdx.x;
    if (i >= n) return;
    const double b0[3] = {b00, b01, b02};
    const int na[3] = {na0, na1, na2};
    int lo[3], hi[3];
    for (int d = 0; d < 3; ++d) {
        const double v = (double)pts[3 * i + d];
        const double f = floor((v - b0[d]) / md);
        lo[d] = 1; hi[d] = 0;
        if (!(f >= -4.0 && f <= (double)na[d] + 4.0)) return;
        const int c = (int)f;
        for (int x = max(c - 3, 0); x <= min(c + 3, na[d]); ++x) {
            const double low = b0[d] + (double)x * md, high = low + md;
            if (low - md <= v && v < high + md) {      // (the cells that hold v form one run)
                if (lo[d] > hi[d]) lo[d] = x;
                hi[d] = x;
            }
        }
        if (lo[d] > hi[d]) return;
    }
    for (int x = lo[0]; x <= hi[0]; ++x)
        for (int y = lo[1]; y <= hi[1]; ++y)
            for (int z = lo[2]; z <= hi[2]; ++z) {
                int* o = occ + ((long)x * (na1 + 1) + y) * (na2 + 1) + z;
                if (*o == 0) *o = 1;                // (same value from every writer)
            }
}

// ---------------------------------------------------------------------------------------------------------------------------
// radius maximal independent set
constexpr unsigned char MIS_UNDECIDED = 0, MIS_KEPT = 1, MIS_REMOVED = 2;

__global__ __launch_bounds__(PM_THREADS) void pm_mis_round_kernel(const GridView g, long n, double dst2, const unsigned char* __restrict__ sin,
                                                                  unsigned char* __restrict__ sout, unsigned long long* undecided) {
    const long k = (long)blockIdx.x * PM_THREADS + threadIdx.x;
    unsigned char s = k < n ? sin[k] : MIS_KEPT;
    if (s == MIS_UNDECIDED) {
        const float4 p = g.pts[k];
        const int rank = g.payload[k];
        const double x = p.x, y = p.y, z = p.z;
        const long cx = pm_cell(x, g.ox, g.cell), cy = pm_cell(y, g.oy, g.cell), cz = pm_cell(z, g.oz, g.cell);
        bool blocked = false, removed = false;
        for (int dz = -1; dz <= 1 && !removed; ++dz)
            for (int dy = -1; dy <= 1 && !removed; ++dy)
                for (int dx = -1; dx <= 1 && !removed; ++dx) {
                    const int2 se = pm_lookup(g, cx + dx, cy + dy, cz + dz);
                    for (int j = se.x; j < se.x + se.y; ++j) {
                        if (j == k) continue;
                        const unsigned char sj = sin[j];
                        if (sj == MIS_REMOVED) continue;
                        if (sj == MIS_UNDECIDED && (blocked || g.payload[j] > rank)) continue;
                        if (pm_d2(x, y, z, g.pts[j]) <= dst2) {
                            if (sj == MIS_KEPT) {
                                removed = true;
                                break;
                            }
                            blocked = true;
                        }
                    }
                }
        s = removed ? MIS_REMOVED : blocked ? MIS_UNDECIDED : MIS_KEPT;
    }
    if (k < n) sout[k] = s;
    const unsigned long long ball = __ballot(s == MIS_UNDECIDED);
    if ((threadIdx.x & 63) == 0 && ball) atomicAdd(undecided, (unsigned long long)__popcll(ball));
}

// state (slot order) -> mask byte at the point's original index
__global__ __launch_bounds__(PM_THREADS) void pm_mis_mask_kernel(const float4* __restrict__ pts, long n, const unsigned char* __restrict__ state,
                                                                 unsigned char* __restrict__ mask) {
    const long k = (long)blockIdx.x * PM_THREADS + threadIdx.x;
    if (k >= n) return;
    mask[__float_as_int(pts[k].w)] = state[k] == MIS_KEPT ? 1 : 0;
}

__global__ __launch_bounds__(PM_THREADS) void pm_compact_kernel(const unsigned char* __restrict__ mask, long n, const int* __restrict__ boff,
                                                                int* __restrict__ kept) {
    __shared__ int lds[PM_THREADS];
    const long base = (long)blockIdx.x * PM_CHUNK + (long)threadIdx.x * PM_SCAN_PER;
    unsigned v = 0;
    int s = 0;
    for (int j = 0; j < PM_SCAN_PER; ++j)
        if (base + j < n && mask[base + j]) {
            v |= 1u << j;
            ++s;
        }
    int run = boff[blockIdx.x] + pm_block_exclusive(s, lds);
    for (int j = 0; j < PM_SCAN_PER; ++j)
        if (v & (1u << j)) kept[run++] = (int)(base + j);
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
struct GridLayout {
    long cap, nb;
    long hdr, keys, counts, cells, slot_of, pos, pts, payload, bsum, boff, total;
};
inline GridLayout grid_layout(long n) {
    GridLayout L;
    L.cap = 1024;
    while (L.cap < 2 * n) L.cap <<= 1;
    L.nb = (L.cap + PM_CHUNK - 1) / PM_CHUNK;
    long o = 0;
    L.hdr = o; o += 256;
    L.keys = o; o += align256(L.cap * 8);
    L.counts = o; o += align256(L.cap * 4);
    L.cells = o; o += align256(L.cap * 8);
    L.slot_of = o; o += align256(n * 4);
    L.pos = o; o += align256(n * 4);
    L.pts = o; o += align256(n * 16);
    L.payload = o; o += align256(n * 4);
    L.bsum = o; o += align256(L.nb * 4);
    L.boff = o; o += align256(L.nb * 4);
    L.total = o;
    return L;
}
inline GridView grid_view(const void* grid, long n, double ox, double oy, double oz, double cell) {
    const GridLayout L = grid_layout(n);
    const char* b = static_cast<const char*>(grid);
    GridView g;
    g.keys = reinterpret_cast<const unsigned long long*>(b + L.keys);
    g.cells = reinterpret_cast<const int2*>(b + L.cells);
    g.pts = reinterpret_cast<const float4*>(b + L.pts);
    g.payload = reinterpret_cast<const int*>(b + L.payload);
    g.mask = (unsigned long long)(L.cap - 1);
    g.ox = ox; g.oy = oy; g.oz = oz; g.cell = cell;
    return g;
}
inline unsigned pm_blocks(long n) { return (unsigned)((n + PM_THREADS - 1) / PM_THREADS); }
inline long mis_nb(long n) { return (n + PM_CHUNK - 1) / PM_CHUNK; }

}  // namespace pscv

extern "C" long pscv_point_grid_workspace(long n) {
    if (n < 0 || n >= pscv::PM_MAX_POINTS) return -1;
    return pscv::grid_layout(n).total;
}

extern "C" int pscv_point_grid_build(const float* pts, long n, double ox, double oy, double oz, double cell, const int* payload, void* grid,
                                     long grid_bytes, void* stream) {
    using namespace pscv;
    PSCV_CHECK_ARG(grid && (n == 0 || pts), "pscv_point_grid_build: null pointer argument");
    PSCV_CHECK_ARG(n >= 0 && n < PM_MAX_POINTS, "pscv_point_grid_build: n=%ld outside [0, 2^30)", n);
    PSCV_CHECK_ARG(cell > 0.0 && cell < 1e300, "pscv_point_grid_build: cell edge %g must be positive and finite", cell);
    const GridLayout L = grid_layout(n);
    PSCV_CHECK_ARG(grid_bytes >= L.total, "pscv_point_grid_build: grid buffer of %ld bytes < %ld", grid_bytes, L.total);
    char* b = static_cast<char*>(grid);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PSCV_CHECK_ARG(hipMemsetAsync(b + L.hdr, 0, 256, s) == hipSuccess && hipMemsetAsync(b + L.keys, 0xff, L.cap * 8, s) == hipSuccess &&
                       hipMemsetAsync(b + L.counts, 0, L.cap * 4, s) == hipSuccess,
                   "pscv_point_grid_build: memset failed");
    int* counts = reinterpret_cast<int*>(b + L.counts);
    int* slot_of = reinterpret_cast<int*>(b + L.slot_of);
    int* pos = reinterpret_cast<int*>(b + L.pos);
    int* bsum = reinterpret_cast<int*>(b + L.bsum);
    int* boff = reinterpret_cast<int*>(b + L.boff);
    int2* cells = reinterpret_cast<int2*>(b + L.cells);
    if (n > 0) {
        hipLaunchKernelGGL(pm_insert_kernel, dim3(pm_blocks(n)), dim3(PM_THREADS), 0, s, pts, n, ox, oy, oz, cell,
                           reinterpret_cast<unsigned long long*>(b + L.keys), counts, (unsigned long long)(L.cap - 1), slot_of, pos,
                           reinterpret_cast<unsigned int*>(b + L.hdr));
        PSCV_CHECK_LAUNCH("pscv_point_grid_build (insert)");
    }
    hipLaunchKernelGGL(pm_chunk_sum_kernel<int>, dim3((unsigned)L.nb), dim3(PM_THREADS), 0, s, counts, L.cap, bsum);
    PSCV_CHECK_LAUNCH("pscv_point_grid_build (chunk sums)");
    hipLaunchKernelGGL((scan_kernel<PM_SCAN1_THREADS, int, false>), dim3(1), dim3(PM_SCAN1_THREADS), 0, s, bsum, boff, nullptr,
                       (int)L.nb);
    PSCV_CHECK_LAUNCH("pscv_point_grid_build (scan)");
    hipLaunchKernelGGL(pm_cells_kernel, dim3((unsigned)L.nb), dim3(PM_THREADS), 0, s, counts, L.cap, boff, cells);
    PSCV_CHECK_LAUNCH("pscv_point_grid_build (cells)");
    if (n > 0) {
        hipLaunchKernelGGL(pm_scatter_kernel, dim3(pm_blocks(n)), dim3(PM_THREADS), 0, s, pts, n, slot_of, pos, cells, payload,
                           reinterpret_cast<float4*>(b + L.pts), reinterpret_cast<int*>(b + L.payload));
        PSCV_CHECK_LAUNCH("pscv_point_grid_build (scatter)");
    }
    return 0;
}

extern "C" int pscv_point_nn_dist(const float* query, long m, const void* fine, const void* coarse, long n_target, double ox, double oy,
                                  double oz, double fine_cell, double coarse_cell, int fine_rings, int coarse_rings, double maxdist,
                                  const double* bb, const int* occ, double* out, void* stream) {
    using namespace pscv;
    PSCV_CHECK_ARG(fine && coarse && out && (m == 0 || query), "pscv_point_nn_dist: null pointer argument");
    PSCV_CHECK_ARG(m >= 0 && n_target >= 0 && n_target < PM_MAX_POINTS, "pscv_point_nn_dist: bad sizes m=%ld n_target=%ld", m, n_target);
    PSCV_CHECK_ARG(fine_cell > 0.0 && coarse_cell > 0.0, "pscv_point_nn_dist: cell edges must be positive");
    PSCV_CHECK_ARG(fine_rings >= 0 && fine_rings <= 8 && coarse_rings >= 0 && coarse_rings <= 16,
                   "pscv_point_nn_dist: rings fine=%d coarse=%d outside [0,8] / [0,16]", fine_rings, coarse_rings);
    PSCV_CHECK_ARG(maxdist > 0.0 && maxdist < 1e150, "pscv_point_nn_dist: maxdist %g must be positive and finite", maxdist);
    PSCV_CHECK_ARG((double)coarse_rings * coarse_cell >= maxdist + coarse_cell,
                   "pscv_point_nn_dist: %d coarse rings of %g do not cover maxdist %g", coarse_rings, coarse_cell, maxdist);
    NNArgs a;
    a.fine = grid_view(fine, n_target, ox, oy, oz, fine_cell);
    a.coarse = grid_view(coarse, n_target, ox, oy, oz, coarse_cell);
    a.query = query; a.out = out; a.m = m;
    a.maxdist = maxdist; a.maxdist2 = maxdist * maxdist;
    a.fine_rings = fine_rings; a.coarse_rings = coarse_rings;
    a.dtu = bb != nullptr;
    a.occ = occ;
    for (int d = 0; d < 3; ++d) { a.bb0[d] = 0.0; a.na[d] = 0; }
    if (bb) {
        PSCV_CHECK_ARG(occ, "pscv_point_nn_dist: the DTU mode needs the occupancy of pscv_dtu_cell_occupancy");
        for (int d = 0; d < 3; ++d) {
            const double na = floor((bb[3 + d] - bb[d]) / maxdist);
            PSCV_CHECK_ARG(na >= 0.0 && na < 4096.0, "pscv_point_nn_dist: %g cells on axis %d (bb / maxdist)", na + 1.0, d);
            a.bb0[d] = bb[d];
            a.na[d] = (int)na;
        }
    }
    if (m == 0) return 0;
    hipLaunchKernelGGL(pm_nn_kernel, dim3(pm_blocks(m)), dim3(PM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
    PSCV_CHECK_LAUNCH("pscv_point_nn_dist");
    return 0;
}

extern "C" int pscv_dtu_cell_occupancy(const float* pts, long n, const double* bb, double maxdist, int* occ, void* stream) {
    using namespace pscv;
    PSCV_CHECK_ARG(bb && occ && (n == 0 || pts), "pscv_dtu_cell_occupancy: null pointer argument");
    PSCV_CHECK_ARG(maxdist > 0.0 && maxdist < 1e150, "pscv_dtu_cell_occupancy: maxdist %g must be positive and finite", maxdist);
    int na[3];
    for (int d = 0; d < 3; ++d) {
        const double v = floor((bb[3 + d] - bb[d]) / maxdist);
        PSCV_CHECK_ARG(v >= 0.0 && v < 4096.0, "pscv_dtu_cell_occupancy: %g cells on axis %d (bb / maxdist)", v + 1.0, d);
        na[d] = (int)v;
    }
    if (n <= 0) return 0;
    hipLaunchKernelGGL(pm_dtu_occ_kernel, dim3(pm_blocks(n)), dim3(PM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), pts, n, bb[0], bb[1],
                       bb[2], maxdist, na[0], na[1], na[2], occ);
    PSCV_CHECK_LAUNCH("pscv_dtu_cell_occupancy");
    return 0;
}

extern "C" int pscv_radius_mis_round(const void* grid, long n, double ox, double oy, double oz, double cell, double dst,
                                     const unsigned char* state_in, unsigned char* state_out, long long* undecided, void* stream) {
    using namespace pscv;
    PSCV_CHECK_ARG(grid && undecided && (n == 0 || (state_in && state_out)), "pscv_radius_mis_round: null pointer argument");
    PSCV_CHECK_ARG(n >= 0 && n < PM_MAX_POINTS, "pscv_radius_mis_round: n=%ld outside [0, 2^30)", n);
    PSCV_CHECK_ARG(dst >= 0.0 && cell > dst, "pscv_radius_mis_round: the cell edge %g must exceed dst %g", cell, dst);
    if (n == 0) return 0;
    const GridView g = grid_view(grid, n, ox, oy, oz, cell);
    hipLaunchKernelGGL(pm_mis_round_kernel, dim3(pm_blocks(n)), dim3(PM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), g, n, dst * dst,
                       state_in, state_out, reinterpret_cast<unsigned long long*>(undecided));
    PSCV_CHECK_LAUNCH("pscv_radius_mis_round");
    return 0;
}

extern "C" long pscv_radius_mis_workspace(long n) {
    if (n < 0 || n >= pscv::PM_MAX_POINTS) return -1;
    return 2 * pscv::align256(pscv::mis_nb(n) * 4) + 256;
}

extern "C" int pscv_radius_mis_compact(const void* grid, long n, const unsigned char* state, unsigned char* mask, int* kept,
                                       long long* n_kept, void* workspace, long workspace_bytes, void* stream) {
    using namespace pscv;
    PSCV_CHECK_ARG(grid && n_kept && workspace && (n == 0 || (state && mask && kept)), "pscv_radius_mis_compact: null pointer argument");
    PSCV_CHECK_ARG(n >= 0 && n < PM_MAX_POINTS, "pscv_radius_mis_compact: n=%ld outside [0, 2^30)", n);
    PSCV_CHECK_ARG(workspace_bytes >= pscv_radius_mis_workspace(n), "pscv_radius_mis_compact: workspace of %ld bytes < %ld",
                   workspace_bytes, pscv_radius_mis_workspace(n));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // the scan adds the kept count to *n_kept
    PSCV_CHECK_ARG(hipMemsetAsync(n_kept, 0, sizeof(long long), s) == hipSuccess, "pscv_radius_mis_compact: memset failed");
    if (n == 0) return 0;
    const long nb = mis_nb(n);
    int* bsum = static_cast<int*>(workspace);
    int* boff = reinterpret_cast<int*>(static_cast<char*>(workspace) + align256(nb * 4));
    const GridLayout L = grid_layout(n);
    hipLaunchKernelGGL(pm_mis_mask_kernel, dim3(pm_blocks(n)), dim3(PM_THREADS), 0, s,
                       reinterpret_cast<const float4*>(static_cast<const char*>(grid) + L.pts), n, state, mask);
    PSCV_CHECK_LAUNCH("pscv_radius_mis_compact (mask)");
    hipLaunchKernelGGL(pm_chunk_sum_kernel<unsigned char>, dim3((unsigned)nb), dim3(PM_THREADS), 0, s, mask, n, bsum);
    PSCV_CHECK_LAUNCH("pscv_radius_mis_compact (chunk sums)");
    hipLaunchKernelGGL((scan_kernel<PM_SCAN1_THREADS, int, true>), dim3(1), dim3(PM_SCAN1_THREADS), 0, s, bsum, boff, n_kept, (int)nb);
    PSCV_CHECK_LAUNCH("pscv_radius_mis_compact (scan)");
    hipLaunchKernelGGL(pm_compact_kernel, dim3((unsigned)nb), dim3(PM_THREADS), 0, s, mask, n, boff, kept);
    PSCV_CHECK_LAUNCH("pscv_radius_mis_compact (compact)");
    return 0;
}
