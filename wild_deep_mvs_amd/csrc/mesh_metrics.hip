// Mesh metrics (the step after TSDF fusion and mesh clean-up): deterministic surface sampling proportional to area and the exact
// bounded distance from points to the surface of an indexed triangle mesh.  gfx950.  INTEGRATION.md section 2r states the rules.
//
// Sampling (pscv_mesh_sample_count / pscv_mesh_sample_emit): per face the fp64 area, a stochastically rounded sample count from a
// counter-based splitmix64 hash of (seed, face), the exclusive integer scan of the counts across workgroups (chunk sums, a
// one-workgroup scan of the chunk sums, local scans) and one lane per sample, which finds its face by binary search in the
// offsets and draws its barycentric coordinates from the hash of (seed, face, k).  No floating-point scan, no atomics.
//
// Grid of a mesh (pscv_mesh_grid_count / pscv_mesh_grid_build): every valid face is binned into every cell its bounding box
// touches.  Cells per face, integer scan, one lane per (cell, face) pair (binary search in the offsets), then the scheme of
// pscv_point_grid_build: the pair's 64-bit cell key goes into an open-addressing hash table (integer atomicCAS), the pairs of a
// slot are counted with integer atomics, the counts are scanned and the faces are scattered into slot order.  The order of the
// faces inside a slot depends on scheduling; the distance below is a lexicographic minimum over (d^2, face), so it does not.
//
// Bounded distance (pscv_mesh_point_dist): rings of the fine grid around the query's cell, stopped once the ring radius passes
// the best squared distance, then the cells of a coarse grid within `maxdist`, each pruned by its box distance.  A cell is
// skipped, and the rings stop, only when the bound is STRICTLY beyond the best d^2: a face with an equal d^2 and a lower index
// is still found.  Per-face distances are fp64 from the fp32 coordinates in one fixed expression order.
//
// This file is compiled with -ffp-contract=off: tests/_mesh_metrics_ref.py restates every product and sum as its own operation.
// The grid and scan helpers are private copies of the ones in point_metrics.hip (same names with another prefix).
#include "geo_common.h"

namespace pscv {

constexpr int MM_THREADS = 256;
constexpr int MM_SCAN_PER = 16;
constexpr int MM_CHUNK = MM_THREADS * MM_SCAN_PER;          // items per scan workgroup
constexpr int MM_SCAN1_THREADS = 1024;
constexpr int MM_KEY_BITS = 21;
constexpr long MM_KEY_SPAN = 1L << MM_KEY_BITS;              // cells per axis a grid can address
constexpr unsigned long long MM_EMPTY = ~0ull;               // (a key never has bit 63 set)
constexpr double MM_COORD_CLAMP = 1099511627776.0;           // 2^40: query cell coordinates are clamped before the cast
constexpr long MM_MAX_FACES = 715827882;                     // 3 F < 2^31
constexpr long MM_MAX_COUNT = 2147483647;                    // a face's count saturates here; the totals are 64-bit
constexpr unsigned long long MM_GOLDEN = 0x9e3779b97f4a7c15ull;

// ---------------------------------------------------------------------------------------------------------------------------
// hash
__device__ __forceinline__ unsigned long long mm_mix(unsigned long long k) {       // splitmix64 finaliser (pm_hash)
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    return k ^ (k >> 31);
}
// one splitmix64 step from state x: the generator's output after its state advanced from x
__device__ __forceinline__ unsigned long long mm_step(unsigned long long x) { return mm_mix(x + MM_GOLDEN); }
__device__ __forceinline__ double mm_unit(unsigned long long h) { return (double)(h >> 11) * 0x1.0p-53; }
__device__ __forceinline__ unsigned long long mm_face_hash(unsigned long long seed, long f) {
    return mm_step(mm_step(seed) ^ (unsigned long long)f);
}

// ---------------------------------------------------------------------------------------------------------------------------
// faces
struct Tri {
    double a[3], b[3], c[3];
};
__device__ __forceinline__ bool mm_load_face(const float* __restrict__ xyz, const int* __restrict__ faces, long f, long V, Tri& t) {
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return false;
    for (int d = 0; d < 3; ++d) {
        t.a[d] = (double)xyz[3 * (long)i0 + d];
        t.b[d] = (double)xyz[3 * (long)i1 + d];
        t.c[d] = (double)xyz[3 * (long)i2 + d];
    }
    return true;
}
__device__ __forceinline__ void mm_sub(const double* p, const double* q, double* r) {
    r[0] = p[0] - q[0]; r[1] = p[1] - q[1]; r[2] = p[2] - q[2];
}
__device__ __forceinline__ void mm_cross(const double* u, const double* v, double* n) {
    n[0] = u[1] * v[2] - u[2] * v[1];
    n[1] = u[2] * v[0] - u[0] * v[2];
    n[2] = u[0] * v[1] - u[1] * v[0];
}
__device__ __forceinline__ double mm_dot(const double* u, const double* v) { return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]; }

// the largest index f in [0, n) with off[f] <= i (off ascending, off[0] = 0 <= i)
__device__ __forceinline__ long mm_find(const int* __restrict__ off, long n, long i) {
    long lo = 0, hi = n - 1;
    while (lo < hi) {
        const long mid = (lo + hi + 1) >> 1;
        if ((long)off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---------------------------------------------------------------------------------------------------------------------------
// exclusive scan of int32 counts across workgroups, 64-bit sums: count [n] -> off [n] (saturated at 2^31 - 1), *total
__device__ __forceinline__ long long mm_block_exclusive(long long v, long long* lds) {    // over MM_THREADS lanes, Hillis-Steele
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < MM_THREADS; o <<= 1) {
        const long long a = threadIdx.x >= o ? lds[threadIdx.x - o] : 0;
        __syncthreads();
        lds[threadIdx.x] += a;
        __syncthreads();
    }
    const long long r = lds[threadIdx.x] - v;
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(MM_THREADS) void mm_chunk_sum_kernel(const int* __restrict__ in, long n, long long* __restrict__ bsum) {
    __shared__ long long lds[MM_THREADS];
    const long base = (long)blockIdx.x * MM_CHUNK + (long)threadIdx.x * MM_SCAN_PER;
    long long s = 0;
    for (int j = 0; j < MM_SCAN_PER; ++j)
        if (base + j < n) s += in[base + j];
    const long long before = mm_block_exclusive(s, lds);
    if (threadIdx.x == MM_THREADS - 1) bsum[blockIdx.x] = before + s;
}

// one workgroup: boff[k] = bsum[0] + ... + bsum[k-1], *total = the sum of all
__global__ __launch_bounds__(MM_SCAN1_THREADS) void mm_scan_sums_kernel(const long long* __restrict__ bsum, long long* __restrict__ boff,
                                                                        long long* __restrict__ total, long nb) {
    __shared__ long long part[MM_SCAN1_THREADS];
    const long per = (nb + MM_SCAN1_THREADS - 1) / MM_SCAN1_THREADS;
    const long b = (long)threadIdx.x * per, e = min(b + per, nb);
    long long s = 0;
    for (long k = b; k < e; ++k) s += bsum[k];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < MM_SCAN1_THREADS; o <<= 1) {
        const long long v = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    long long run = part[threadIdx.x] - s;
    for (long k = b; k < e; ++k) {
        boff[k] = run;
        run += bsum[k];
    }
    if (threadIdx.x == MM_SCAN1_THREADS - 1) *total = part[threadIdx.x];
}

__global__ __launch_bounds__(MM_THREADS) void mm_offsets_kernel(const int* __restrict__ in, long n, const long long* __restrict__ boff,
                                                                int* __restrict__ off) {
    __shared__ long long lds[MM_THREADS];
    const long base = (long)blockIdx.x * MM_CHUNK + (long)threadIdx.x * MM_SCAN_PER;
    int v[MM_SCAN_PER];
    long long s = 0;
    for (int j = 0; j < MM_SCAN_PER; ++j) {
        v[j] = base + j < n ? in[base + j] : 0;
        s += v[j];
    }
    long long run = boff[blockIdx.x] + mm_block_exclusive(s, lds);
    for (int j = 0; j < MM_SCAN_PER; ++j) {
        if (base + j < n) off[base + j] = (int)min(run, (long long)MM_MAX_COUNT);
        run += v[j];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// sampling
__global__ __launch_bounds__(MM_THREADS) void mm_sample_count_kernel(const float* __restrict__ xyz, const int* __restrict__ faces, long F, long V,
                                                                     double s2, unsigned long long seed, int* __restrict__ count) {
    const long f = (long)blockIdx.x * MM_THREADS + threadIdx.x;
    if (f >= F) return;
    Tri t;
    int n = 0;
    if (mm_load_face(xyz, faces, f, V, t)) {
        double u[3], v[3], c[3];
        mm_sub(t.b, t.a, u);
        mm_sub(t.c, t.a, v);
        mm_cross(u, v, c);
        const double area = 0.5 * sqrt(mm_dot(c, c));
        if (area > 0.0 && area <= 1.7976931348623157e308) {            // (false for NaN and inf)
            const double x = floor(area / s2 + mm_unit(mm_face_hash(seed, f)));
            n = x >= (double)MM_MAX_COUNT ? (int)MM_MAX_COUNT : (int)x;
        }
    }
    count[f] = n;
}

__global__ __launch_bounds__(MM_THREADS) void mm_sample_emit_kernel(const float* __restrict__ xyz, const int* __restrict__ faces,
                                                                    const int* __restrict__ off, long F, long V, unsigned long long seed, long N,
                                                                    float* __restrict__ out, int* __restrict__ face_out) {
    const long i = (long)blockIdx.x * MM_THREADS + threadIdx.x;
    if (i >= N) return;
    const long f = mm_find(off, F, i);
    const long k = i - (long)off[f];
    Tri t;
    if (!mm_load_face(xyz, faces, f, V, t)) return;                     // (never: a face that is not valid has no samples)
    const unsigned long long hk = mm_step(mm_face_hash(seed, f) ^ ((unsigned long long)k + 1ull));
    double u = mm_unit(hk), v = mm_unit(mm_step(hk));
    if (u + v > 1.0) {
        u = 1.0 - u;
        v = 1.0 - v;
    }
    for (int d = 0; d < 3; ++d) {
        const double e1 = t.b[d] - t.a[d], e2 = t.c[d] - t.a[d];
        out[3 * i + d] = (float)((t.a[d] + u * e1) + v * e2);
    }
    if (face_out) face_out[i] = (int)f;
}

// ---------------------------------------------------------------------------------------------------------------------------
// grid of a mesh
struct MeshGridView {
    const unsigned long long* keys;     // [cap]
    const int2* cells;                  // [cap]: (start, count) in slot order
    const int* items;                   // [n_pairs]: face indices in slot order
    unsigned long long mask;            // cap - 1
    double ox, oy, oz, cell;
};

__device__ __forceinline__ long mm_cell(double v, double o, double cell) {
    const double c = fmin(fmax(floor((v - o) / cell), -MM_COORD_CLAMP), MM_COORD_CLAMP);    // (NaN -> -clamp)
    return (long)c;
}
__device__ __forceinline__ long mm_cell_in_span(double v, double o, double cell) {
    return min(max(mm_cell(v, o, cell), 0L), MM_KEY_SPAN - 1);
}
__device__ __forceinline__ bool mm_in_span(long x, long y, long z) {
    return x >= 0 && x < MM_KEY_SPAN && y >= 0 && y < MM_KEY_SPAN && z >= 0 && z < MM_KEY_SPAN;
}
__device__ __forceinline__ unsigned long long mm_key(long x, long y, long z) {
    return (unsigned long long)x | ((unsigned long long)y << MM_KEY_BITS) | ((unsigned long long)z << (2 * MM_KEY_BITS));
}
__device__ __forceinline__ int2 mm_lookup(const MeshGridView& g, long x, long y, long z) {
    const unsigned long long key = mm_key(x, y, z);
    unsigned long long h = mm_mix(key) & g.mask;
    for (;;) {
        const unsigned long long k = g.keys[h];
        if (k == key) return g.cells[h];
        if (k == MM_EMPTY) return make_int2(0, 0);
        h = (h + 1) & g.mask;
    }
}
// squared distance from (x, y, z) to the box of cell (cx, cy, cz), shrunk by a relative slack (conservative for pruning)
__device__ __forceinline__ double mm_box_d2(const MeshGridView& g, double x, double y, double z, long cx, long cy, long cz) {
    auto gap = [&](double v, double o, long c) {
        const double lo = o + (double)c * g.cell, hi = lo + g.cell;
        return fmax(fmax(lo - v, v - hi), 0.0);
    };
    const double a = gap(x, g.ox, cx), b = gap(y, g.oy, cy), c = gap(z, g.oz, cz);
    return (a * a + b * b + c * c) * (1.0 - 1e-9);
}

// the cells the bounding box of face f touches: lo[3] and the extents n[3]; false for a face that is not valid
__device__ __forceinline__ bool mm_face_cells(const float* __restrict__ xyz, const int* __restrict__ faces, long f, long V, double ox, double oy,
                                              double oz, double cell, long* lo, long* n) {
    Tri t;
    if (!mm_load_face(xyz, faces, f, V, t)) return false;
    const double o[3] = {ox, oy, oz};
    for (int d = 0; d < 3; ++d) {
        lo[d] = mm_cell_in_span(fmin(fmin(t.a[d], t.b[d]), t.c[d]), o[d], cell);
        n[d] = mm_cell_in_span(fmax(fmax(t.a[d], t.b[d]), t.c[d]), o[d], cell) - lo[d] + 1;
    }
    return true;
}

__global__ __launch_bounds__(MM_THREADS) void mm_grid_count_kernel(const float* __restrict__ xyz, const int* __restrict__ faces, long F, long V,
                                                                   double ox, double oy, double oz, double cell, int* __restrict__ count) {
    const long f = (long)blockIdx.x * MM_THREADS + threadIdx.x;
    if (f >= F) return;
    long lo[3], n[3];
    int c = 0;
    if (mm_face_cells(xyz, faces, f, V, ox, oy, oz, cell, lo, n)) {
        const double total = (double)n[0] * (double)n[1] * (double)n[2];                     // (each extent <= 2^21: exact)
        c = total >= (double)MM_MAX_COUNT ? (int)MM_MAX_COUNT : (int)total;
    }
    count[f] = c;
}

// one lane per (cell, face) pair: its key into the table, its slot and its position in the slot
__global__ __launch_bounds__(MM_THREADS) void mm_grid_insert_kernel(const float* __restrict__ xyz, const int* __restrict__ faces,
                                                                    const int* __restrict__ poff, long F, long V, long P, double ox, double oy,
                                                                    double oz, double cell, unsigned long long* keys, int* counts,
                                                                    unsigned long long mask, unsigned int* __restrict__ slot_of,
                                                                    int* __restrict__ pos, int* __restrict__ face_of, unsigned int* occupied) {
    const long p = (long)blockIdx.x * MM_THREADS + threadIdx.x;
    if (p >= P) return;
    const long f = mm_find(poff, F, p);
    long j = p - (long)poff[f];
    long lo[3], n[3];
    if (!mm_face_cells(xyz, faces, f, V, ox, oy, oz, cell, lo, n)) return;                  // (never: such a face has no pairs)
    const long cx = lo[0] + j % n[0];
    j /= n[0];
    const long cy = lo[1] + j % n[1], cz = lo[2] + min(j / n[1], n[2] - 1);
    const unsigned long long key = mm_key(cx, cy, cz);
    unsigned long long h = mm_mix(key) & mask;
    for (;;) {                        // the table holds at least 2 P slots, so a free one exists
        const unsigned long long prev = atomicCAS(&keys[h], MM_EMPTY, key);
        if (prev == MM_EMPTY || prev == key) {
            if (prev == MM_EMPTY) atomicAdd(occupied, 1u);
            break;
        }
        h = (h + 1) & mask;
    }
    slot_of[p] = (unsigned int)h;
    pos[p] = atomicAdd(&counts[h], 1);
    face_of[p] = (int)f;
}

__global__ __launch_bounds__(MM_THREADS) void mm_grid_cells_kernel(const int* __restrict__ counts, long cap, const long long* __restrict__ boff,
                                                                   int2* __restrict__ cells) {
    __shared__ long long lds[MM_THREADS];
    const long base = (long)blockIdx.x * MM_CHUNK + (long)threadIdx.x * MM_SCAN_PER;
    int v[MM_SCAN_PER];
    long long s = 0;
    for (int j = 0; j < MM_SCAN_PER; ++j) {
        v[j] = base + j < cap ? counts[base + j] : 0;
        s += v[j];
    }
    long long run = boff[blockIdx.x] + mm_block_exclusive(s, lds);
    for (int j = 0; j < MM_SCAN_PER; ++j) {
        if (base + j < cap) cells[base + j] = make_int2((int)run, v[j]);
        run += v[j];
    }
}

__global__ __launch_bounds__(MM_THREADS) void mm_grid_scatter_kernel(long P, const unsigned int* __restrict__ slot_of, const int* __restrict__ pos,
                                                                     const int* __restrict__ face_of, const int2* __restrict__ cells,
                                                                     int* __restrict__ items) {
    const long p = (long)blockIdx.x * MM_THREADS + threadIdx.x;
    if (p >= P) return;
    items[(long)cells[slot_of[p]].x + pos[p]] = face_of[p];
}

// ---------------------------------------------------------------------------------------------------------------------------
// bounded distance to the surface
// squared distance from q to the segment p0 p1: the parameter clamped to [0, 1]; a segment of length 0 is its end point
__device__ __forceinline__ double mm_segment_d2(const double* q, const double* p0, const double* p1) {
    double d[3], w[3], r[3];
    mm_sub(p1, p0, d);
    mm_sub(q, p0, w);
    const double dd = mm_dot(d, d);
    double t = 0.0;
    if (dd > 0.0) t = fmin(fmax(mm_dot(w, d) / dd, 0.0), 1.0);
    r[0] = w[0] - t * d[0]; r[1] = w[1] - t * d[1]; r[2] = w[2] - t * d[2];
    return mm_dot(r, r);
}
// squared distance from q to triangle a b c (the order of every operation is part of the rule)
__device__ __forceinline__ double mm_face_d2(const double* q, const Tri& t) {
    double e0[3], e1[3], n[3];
    mm_sub(t.b, t.a, e0);
    mm_sub(t.c, t.a, e1);
    mm_cross(e0, e1, n);
    const double nn = mm_dot(n, n);
    if (nn > 0.0) {
        double wa[3], wb[3], wc[3], e[3], x[3];
        mm_sub(q, t.a, wa);
        mm_sub(q, t.b, wb);
        mm_sub(q, t.c, wc);
        mm_cross(e0, wa, x);
        const double s0 = mm_dot(x, n);
        mm_sub(t.c, t.b, e);
        mm_cross(e, wb, x);
        const double s1 = mm_dot(x, n);
        mm_sub(t.a, t.c, e);
        mm_cross(e, wc, x);
        const double s2 = mm_dot(x, n);
        if (s0 >= 0.0 && s1 >= 0.0 && s2 >= 0.0) {
            const double h = mm_dot(wa, n);
            return (h * h) / nn;
        }
    }
    return fmin(fmin(mm_segment_d2(q, t.a, t.b), mm_segment_d2(q, t.b, t.c)), mm_segment_d2(q, t.c, t.a));
}

struct MeshDistArgs {
    MeshGridView fine, coarse;
    const float* query;
    const float* xyz;
    const int* faces;
    double* out;
    int* face_out;
    long m, F, V;
    double maxdist2;
    int fine_rings, coarse_rings;
};

struct MeshBest {
    double d2;
    int face;           // -1: none yet
};

__device__ __forceinline__ void mm_scan_cell(const MeshDistArgs& a, const MeshGridView& g, int2 se, const double* q, MeshBest& best) {
    for (int k = se.x; k < se.x + se.y; ++k) {
        const int f = g.items[k];
        if (f == best.face || f < 0 || f >= a.F) continue;
        Tri t;
        if (!mm_load_face(a.xyz, a.faces, f, a.V, t)) continue;
        const double d2 = mm_face_d2(q, t);
        if (d2 < best.d2 || (d2 == best.d2 && best.face >= 0 && f < best.face)) {
            best.d2 = d2;
            best.face = f;
        }
    }
}

// rings 0..rings of grid g around the query's cell; true once every face outside them lies strictly beyond `best`
__device__ __forceinline__ bool mm_ring_search(const MeshDistArgs& a, const MeshGridView& g, int rings, const double* q, MeshBest& best) {
    const long cx = mm_cell(q[0], g.ox, g.cell), cy = mm_cell(q[1], g.oy, g.cell), cz = mm_cell(q[2], g.oz, g.cell);
    for (int r = 0; r <= rings; ++r) {
        for (int dz = -r; dz <= r; ++dz)
            for (int dy = -r; dy <= r; ++dy)
                for (int dx = -r; dx <= r; ++dx) {
                    if (max(abs(dx), max(abs(dy), abs(dz))) != r) continue;
                    const long ex = cx + dx, ey = cy + dy, ez = cz + dz;
                    if (!mm_in_span(ex, ey, ez)) continue;
                    if (mm_box_d2(g, q[0], q[1], q[2], ex, ey, ez) > best.d2) continue;
                    const int2 se = mm_lookup(g, ex, ey, ez);
                    if (se.y) mm_scan_cell(a, g, se, q, best);
                }
        // the nearest point of a face seen in none of the rings 0..r lies at least r cells from the query
        const double reach = (double)r * g.cell * (1.0 - 1e-9);
        if (reach * reach > best.d2) return true;
    }
    return false;
}

__global__ __launch_bounds__(MM_THREADS) void mm_dist_kernel(const MeshDistArgs a) {
    const long i = (long)blockIdx.x * MM_THREADS + threadIdx.x;
    if (i >= a.m) return;
    const double q[3] = {(double)a.query[3 * i], (double)a.query[3 * i + 1], (double)a.query[3 * i + 2]};
    MeshBest best;
    best.d2 = a.maxdist2;
    best.face = -1;
    if (!mm_ring_search(a, a.fine, a.fine_rings, q, best)) mm_ring_search(a, a.coarse, a.coarse_rings, q, best);
    // (d^2 == maxdist^2 never wins: with no face yet only a strictly smaller d^2 is taken)
    a.out[i] = best.face >= 0 ? sqrt(best.d2) : (double)INFINITY;
    if (a.face_out) a.face_out[i] = best.face;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host side
inline unsigned mm_blocks(long n) { return (unsigned)((n + MM_THREADS - 1) / MM_THREADS); }
inline long mm_chunks(long n) { return (n + MM_CHUNK - 1) / MM_CHUNK; }

// workspace of a scan over n items: the counts, the chunk sums and their offsets
struct ScanLayout {
    long nb, count, bsum, boff, total;
};
inline ScanLayout scan_layout(long n) {
    ScanLayout L;
    L.nb = mm_chunks(n);
    long o = 0;
    L.count = o; o += align256(n * 4);
    L.bsum = o; o += align256(L.nb * 8);
    L.boff = o; o += align256(L.nb * 8);
    L.total = o + 256;
    return L;
}
// count [n] (in the workspace) -> off [n], *total
inline int mm_scan(const char* what, char* ws, const ScanLayout& L, long n, int* off, long long* total, hipStream_t s) {
    const int* count = reinterpret_cast<const int*>(ws + L.count);
    long long* bsum = reinterpret_cast<long long*>(ws + L.bsum);
    long long* boff = reinterpret_cast<long long*>(ws + L.boff);
    hipLaunchKernelGGL(mm_chunk_sum_kernel, dim3((unsigned)L.nb), dim3(MM_THREADS), 0, s, count, n, bsum);
    PSCV_CHECK_LAUNCH(what);
    hipLaunchKernelGGL(mm_scan_sums_kernel, dim3(1), dim3(MM_SCAN1_THREADS), 0, s, bsum, boff, total, L.nb);
    PSCV_CHECK_LAUNCH(what);
    hipLaunchKernelGGL(mm_offsets_kernel, dim3((unsigned)L.nb), dim3(MM_THREADS), 0, s, count, n, boff, off);
    PSCV_CHECK_LAUNCH(what);
    return 0;
}

struct MeshGridLayout {
    long cap, nb;
    long hdr, keys, counts, cells, slot_of, pos, face_of, items, bsum, boff, total_word, total;
};
inline MeshGridLayout mesh_grid_layout(long P) {
    MeshGridLayout L;
    L.cap = 1024;
    while (L.cap < 2 * P) L.cap <<= 1;
    L.nb = mm_chunks(L.cap);
    long o = 0;
    L.hdr = o; o += 256;
    L.keys = o; o += align256(L.cap * 8);
    L.counts = o; o += align256(L.cap * 4);
    L.cells = o; o += align256(L.cap * 8);
    L.slot_of = o; o += align256(P * 4);
    L.pos = o; o += align256(P * 4);
    L.face_of = o; o += align256(P * 4);
    L.items = o; o += align256(P * 4);
    L.bsum = o; o += align256(L.nb * 8);
    L.boff = o; o += align256(L.nb * 8);
    L.total_word = o; o += 256;
    L.total = o;
    return L;
}
inline MeshGridView mesh_grid_view(const void* grid, long P, double ox, double oy, double oz, double cell) {
    const MeshGridLayout L = mesh_grid_layout(P);
    const char* b = static_cast<const char*>(grid);
    MeshGridView g;
    g.keys = reinterpret_cast<const unsigned long long*>(b + L.keys);
    g.cells = reinterpret_cast<const int2*>(b + L.cells);
    g.items = reinterpret_cast<const int*>(b + L.items);
    g.mask = (unsigned long long)(L.cap - 1);
    g.ox = ox; g.oy = oy; g.oz = oz; g.cell = cell;
    return g;
}

inline bool mm_finite(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }

}  // namespace pscv

#define MM_CHECK_MESH(what, xyz, faces, F, V)                                                                        \
    PSCV_CHECK_ARG((F) >= 0 && (F) <= MM_MAX_FACES && (V) >= 0 && (V) < (1L << 31),                                  \
                   what ": n_faces=%ld, n_vertices=%ld outside 3 n_faces < 2^31, n_vertices < 2^31", (long)(F), (long)(V)); \
    PSCV_CHECK_ARG(((F) == 0 || (faces)) && ((V) == 0 || (xyz)), what ": null pointer argument")

extern "C" long pscv_mesh_scan_workspace(long n_faces) {
    if (n_faces < 0 || n_faces > pscv::MM_MAX_FACES) return -1;
    return pscv::scan_layout(n_faces).total;
}

extern "C" int pscv_mesh_sample_count(const float* xyz, const int* faces, long n_faces, long n_vertices, double spacing, long seed,
                                      int* offsets, long long* total, void* workspace, long workspace_bytes, void* stream) {
    using namespace pscv;
    MM_CHECK_MESH("pscv_mesh_sample_count", xyz, faces, n_faces, n_vertices);
    PSCV_CHECK_ARG(total && workspace && (n_faces == 0 || offsets), "pscv_mesh_sample_count: null pointer argument");
    const double s2 = spacing * spacing;
    PSCV_CHECK_ARG(spacing > 0.0 && s2 > 0.0 && mm_finite(s2), "pscv_mesh_sample_count: spacing %g must be positive with a finite, non-zero square",
                   spacing);
    const ScanLayout L = scan_layout(n_faces);
    PSCV_CHECK_ARG(workspace_bytes >= L.total, "pscv_mesh_sample_count: workspace of %ld bytes < %ld", workspace_bytes, L.total);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n_faces == 0) {
        PSCV_CHECK_ARG(hipMemsetAsync(total, 0, sizeof(long long), s) == hipSuccess, "pscv_mesh_sample_count: memset failed");
        return 0;
    }
    char* ws = static_cast<char*>(workspace);
    hipLaunchKernelGGL(mm_sample_count_kernel, dim3(mm_blocks(n_faces)), dim3(MM_THREADS), 0, s, xyz, faces, n_faces, n_vertices, s2,
                       (unsigned long long)seed, reinterpret_cast<int*>(ws + L.count));
    PSCV_CHECK_LAUNCH("pscv_mesh_sample_count (count)");
    return mm_scan("pscv_mesh_sample_count (scan)", ws, L, n_faces, offsets, total, s);
}

extern "C" int pscv_mesh_sample_emit(const float* xyz, const int* faces, const int* offsets, long n_faces, long n_vertices, long seed,
                                     long n_samples, float* out, int* face_out, void* stream) {
    using namespace pscv;
    MM_CHECK_MESH("pscv_mesh_sample_emit", xyz, faces, n_faces, n_vertices);
    PSCV_CHECK_ARG(n_samples >= 0 && n_samples <= MM_MAX_COUNT - 1, "pscv_mesh_sample_emit: n_samples=%ld outside [0, 2^31 - 2]", n_samples);
    PSCV_CHECK_ARG(n_samples == 0 || (n_faces > 0 && offsets && out), "pscv_mesh_sample_emit: %ld samples need faces, offsets and an output",
                   n_samples);
    if (n_samples == 0) return 0;
    hipLaunchKernelGGL(mm_sample_emit_kernel, dim3(mm_blocks(n_samples)), dim3(MM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), xyz, faces,
                       offsets, n_faces, n_vertices, (unsigned long long)seed, n_samples, out, face_out);
    PSCV_CHECK_LAUNCH("pscv_mesh_sample_emit");
    return 0;
}

extern "C" int pscv_mesh_grid_count(const float* xyz, const int* faces, long n_faces, long n_vertices, double ox, double oy, double oz,
                                    double cell, int* pair_off, long long* total, void* workspace, long workspace_bytes, void* stream) {
    using namespace pscv;
    MM_CHECK_MESH("pscv_mesh_grid_count", xyz, faces, n_faces, n_vertices);
    PSCV_CHECK_ARG(total && workspace && (n_faces == 0 || pair_off), "pscv_mesh_grid_count: null pointer argument");
    PSCV_CHECK_ARG(cell > 0.0 && cell < 1e300 && mm_finite(ox) && mm_finite(oy) && mm_finite(oz),
                   "pscv_mesh_grid_count: cell edge %g must be positive and finite, the origin finite", cell);
    const ScanLayout L = scan_layout(n_faces);
    PSCV_CHECK_ARG(workspace_bytes >= L.total, "pscv_mesh_grid_count: workspace of %ld bytes < %ld", workspace_bytes, L.total);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (n_faces == 0) {
        PSCV_CHECK_ARG(hipMemsetAsync(total, 0, sizeof(long long), s) == hipSuccess, "pscv_mesh_grid_count: memset failed");
        return 0;
    }
    char* ws = static_cast<char*>(workspace);
    hipLaunchKernelGGL(mm_grid_count_kernel, dim3(mm_blocks(n_faces)), dim3(MM_THREADS), 0, s, xyz, faces, n_faces, n_vertices, ox, oy, oz, cell,
                       reinterpret_cast<int*>(ws + L.count));
    PSCV_CHECK_LAUNCH("pscv_mesh_grid_count (count)");
    return mm_scan("pscv_mesh_grid_count (scan)", ws, L, n_faces, pair_off, total, s);
}

extern "C" long pscv_mesh_grid_workspace(long n_pairs) {
    if (n_pairs < 0 || n_pairs > pscv::MM_MAX_COUNT) return -1;
    return pscv::mesh_grid_layout(n_pairs).total;
}

extern "C" int pscv_mesh_grid_build(const float* xyz, const int* faces, const int* pair_off, long n_faces, long n_vertices, double ox,
                                    double oy, double oz, double cell, long n_pairs, void* grid, long grid_bytes, void* stream) {
    using namespace pscv;
    MM_CHECK_MESH("pscv_mesh_grid_build", xyz, faces, n_faces, n_vertices);
    PSCV_CHECK_ARG(grid && (n_pairs == 0 || (n_faces > 0 && pair_off)), "pscv_mesh_grid_build: null pointer argument");
    PSCV_CHECK_ARG(n_pairs >= 0 && n_pairs <= MM_MAX_COUNT, "pscv_mesh_grid_build: n_pairs=%ld outside [0, 2^31 - 1]", n_pairs);
    PSCV_CHECK_ARG(cell > 0.0 && cell < 1e300 && mm_finite(ox) && mm_finite(oy) && mm_finite(oz),
                   "pscv_mesh_grid_build: cell edge %g must be positive and finite, the origin finite", cell);
    const MeshGridLayout L = mesh_grid_layout(n_pairs);
    PSCV_CHECK_ARG(grid_bytes >= L.total, "pscv_mesh_grid_build: grid buffer of %ld bytes < %ld", grid_bytes, L.total);
    char* b = static_cast<char*>(grid);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    PSCV_CHECK_ARG(hipMemsetAsync(b + L.hdr, 0, 256, s) == hipSuccess && hipMemsetAsync(b + L.keys, 0xff, L.cap * 8, s) == hipSuccess &&
                       hipMemsetAsync(b + L.counts, 0, L.cap * 4, s) == hipSuccess,
                   "pscv_mesh_grid_build: memset failed");
    int* counts = reinterpret_cast<int*>(b + L.counts);
    unsigned int* slot_of = reinterpret_cast<unsigned int*>(b + L.slot_of);
    int* pos = reinterpret_cast<int*>(b + L.pos);
    int* face_of = reinterpret_cast<int*>(b + L.face_of);
    long long* bsum = reinterpret_cast<long long*>(b + L.bsum);
    long long* boff = reinterpret_cast<long long*>(b + L.boff);
    int2* cells = reinterpret_cast<int2*>(b + L.cells);
    if (n_pairs > 0) {
        hipLaunchKernelGGL(mm_grid_insert_kernel, dim3(mm_blocks(n_pairs)), dim3(MM_THREADS), 0, s, xyz, faces, pair_off, n_faces, n_vertices,
                           n_pairs, ox, oy, oz, cell, reinterpret_cast<unsigned long long*>(b + L.keys), counts,
                           (unsigned long long)(L.cap - 1), slot_of, pos, face_of, reinterpret_cast<unsigned int*>(b + L.hdr));
        PSCV_CHECK_LAUNCH("pscv_mesh_grid_build (insert)");
    }
    hipLaunchKernelGGL(mm_chunk_sum_kernel, dim3((unsigned)L.nb), dim3(MM_THREADS), 0, s, counts, L.cap, bsum);
    PSCV_CHECK_LAUNCH("pscv_mesh_grid_build (chunk sums)");
    hipLaunchKernelGGL(mm_scan_sums_kernel, dim3(1), dim3(MM_SCAN1_THREADS), 0, s, bsum, boff, reinterpret_cast<long long*>(b + L.total_word),
                       L.nb);
    PSCV_CHECK_LAUNCH("pscv_mesh_grid_build (scan)");
    hipLaunchKernelGGL(mm_grid_cells_kernel, dim3((unsigned)L.nb), dim3(MM_THREADS), 0, s, counts, L.cap, boff, cells);
    PSCV_CHECK_LAUNCH("pscv_mesh_grid_build (cells)");
    if (n_pairs > 0) {
        hipLaunchKernelGGL(mm_grid_scatter_kernel, dim3(mm_blocks(n_pairs)), dim3(MM_THREADS), 0, s, n_pairs, slot_of, pos, face_of, cells,
                           reinterpret_cast<int*>(b + L.items));
        PSCV_CHECK_LAUNCH("pscv_mesh_grid_build (scatter)");
    }
    return 0;
}

extern "C" int pscv_mesh_point_dist(const float* query, long m, const float* xyz, const int* faces, long n_faces, long n_vertices,
                                    const void* fine, long fine_pairs, const void* coarse, long coarse_pairs, double ox, double oy, double oz,
                                    double fine_cell, double coarse_cell, int fine_rings, int coarse_rings, double maxdist, double* out,
                                    int* face_out, void* stream) {
    using namespace pscv;
    MM_CHECK_MESH("pscv_mesh_point_dist", xyz, faces, n_faces, n_vertices);
    PSCV_CHECK_ARG(fine && coarse && (m == 0 || (query && out)), "pscv_mesh_point_dist: null pointer argument");
    PSCV_CHECK_ARG(m >= 0 && fine_pairs >= 0 && fine_pairs <= MM_MAX_COUNT && coarse_pairs >= 0 && coarse_pairs <= MM_MAX_COUNT,
                   "pscv_mesh_point_dist: bad sizes m=%ld fine_pairs=%ld coarse_pairs=%ld", m, fine_pairs, coarse_pairs);
    PSCV_CHECK_ARG(fine_cell > 0.0 && coarse_cell > 0.0, "pscv_mesh_point_dist: cell edges must be positive");
    PSCV_CHECK_ARG(fine_rings >= 0 && fine_rings <= 8 && coarse_rings >= 0 && coarse_rings <= 16,
                   "pscv_mesh_point_dist: rings fine=%d coarse=%d outside [0,8] / [0,16]", fine_rings, coarse_rings);
    PSCV_CHECK_ARG(maxdist > 0.0 && maxdist < 1e150, "pscv_mesh_point_dist: maxdist %g must be positive and finite", maxdist);
    PSCV_CHECK_ARG((double)coarse_rings * coarse_cell >= maxdist + coarse_cell,
                   "pscv_mesh_point_dist: %d coarse rings of %g do not cover maxdist %g", coarse_rings, coarse_cell, maxdist);
    MeshDistArgs a;
    a.fine = mesh_grid_view(fine, fine_pairs, ox, oy, oz, fine_cell);
    a.coarse = mesh_grid_view(coarse, coarse_pairs, ox, oy, oz, coarse_cell);
    a.query = query; a.xyz = xyz; a.faces = faces; a.out = out; a.face_out = face_out;
    a.m = m; a.F = n_faces; a.V = n_vertices;
    a.maxdist2 = maxdist * maxdist;
    a.fine_rings = fine_rings; a.coarse_rings = coarse_rings;
    if (m == 0) return 0;
    hipLaunchKernelGGL(mm_dist_kernel, dim3(mm_blocks(m)), dim3(MM_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a);
    PSCV_CHECK_LAUNCH("pscv_mesh_point_dist");
    return 0;
}
