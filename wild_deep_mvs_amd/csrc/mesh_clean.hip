// Clean-up of an indexed triangle mesh: connected components, removal of small components / degenerate faces / unused vertices
// with order-preserving compaction, and area-weighted vertex normals.  gfx950.
//
// Components.  Two vertices are connected when some face contains both; label[v] is the smallest vertex index of v's component.
// A lock-free union-find on the label array itself:
//   * init: label[v] = v;
//   * hook: one lane per face unites (i0, i1) and (i0, i2): find both roots, compare-and-swap the LARGER root under the smaller;
//     a failed swap hands back the value another lane put there, and the lane goes on from it;
//   * flatten: one lane per vertex walks to its root and stores it.
// Invariant: label[x] <= x at all times and a word only ever decreases.  So every walk strictly descends, every retry strictly
// lowers the larger of its two indices, a root is the minimum of its tree, and the final labels are a pure function of the
// faces whatever the schedule.  No lane waits for another: there is no spin, flag or grid barrier.  Every loop still carries a
// trip limit of n_vertices + 1 (the longest strictly descending walk has n_vertices - 1 steps); a lane that exceeds it, or
// reads an index outside [0, n_vertices), adds 1 to status[1] and leaves, so a defect ends as an error at the host's read of
// the status words and not as a hang.  A face with an index outside [0, n_vertices) joins nothing and adds 1 to status[0].
// The words are read and written with relaxed agent-scope atomics (served by L2): a stale value would still be an ancestor,
// a fresh one ends the walk sooner.
//
// Normals and the degenerate test are fp64 on values converted from fp32; products and sums are separate operations in the
// order written (the Makefile builds this file with -ffp-contract=off, like tsdf_fusion.hip), which tests/_mesh_ref.py
// reproduces bit for bit:  u = b - a, v = c - a, n = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0).
#include "pscv_common.h"

namespace pscv {

constexpr int MC_THREADS = 256;
constexpr long MC_MAX = (1L << 31) - 1;

#define MC_LD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

__device__ __forceinline__ bool in_range(int i, int n) { return (unsigned)i < (unsigned)n; }

// The root of x's tree, compressing on the way (path splitting: every visited node is pointed at its grandparent with an atomic
// min, which keeps "a word only decreases").  false: the trip limit or a word outside [0, n) -- status[1] is raised.
__device__ __forceinline__ bool find_root(int* __restrict__ parent, int n, int x, int* __restrict__ status, int& root) {
    int p = MC_LD(parent + x);
    for (int trips = 0; p != x; ++trips) {
        if (trips > n || !in_range(p, n)) {
            atomicAdd(status + 1, 1);
            return false;
        }
        const int gp = MC_LD(parent + p);
        if (gp != p && in_range(gp, n)) __hip_atomic_fetch_min(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = gp;
    }
    root = x;
    return true;
}

__device__ __forceinline__ void unite(int* __restrict__ parent, int n, int a, int b, int* __restrict__ status) {
    for (int trips = 0; a != b; ++trips) {
        if (trips > n) {
            atomicAdd(status + 1, 1);
            return;
        }
        int ra, rb;
        if (!find_root(parent, n, a, status, ra) || !find_root(parent, n, b, status, rb)) return;
        if (ra == rb) return;
        const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        int seen = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return;
        if (!in_range(seen, n)) {
            atomicAdd(status + 1, 1);
            return;
        }
        a = seen;                                                            // hi has a parent now: seen < hi, lo < hi
        b = lo;
    }
}

__global__ __launch_bounds__(MC_THREADS) void mesh_init_kernel(int* __restrict__ label, int n) {
    const long v = (long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v < n) label[v] = (int)v;
}

__global__ __launch_bounds__(MC_THREADS) void mesh_hook_kernel(const int* __restrict__ faces, long n_faces, int n,
                                                               int* __restrict__ parent, int* __restrict__ status) {
    const long f = (long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (f >= n_faces) return;
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (!(in_range(i0, n) && in_range(i1, n) && in_range(i2, n))) {
        atomicAdd(status, 1);
        return;
    }
    unite(parent, n, i0, i1, status);
    unite(parent, n, i0, i2, status);
}

__global__ __launch_bounds__(MC_THREADS) void mesh_flatten_kernel(int* __restrict__ parent, int n, int* __restrict__ status) {
    const long v = (long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v >= n) return;
    int x = (int)v, p = MC_LD(parent + x);
    for (int trips = 0; p != x; ++trips) {
        if (trips > n || !in_range(p, n)) {
            atomicAdd(status + 1, 1);
            return;
        }
        x = p;
        p = MC_LD(parent + x);
    }
    if (x != (int)v) __hip_atomic_store(parent + v, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// cnt[key] += 1 for every lane with `on`, with one atomic per distinct key and not one per lane (a mesh is mostly one component:
// adding lane by lane would queue the whole mesh on one word).  Every lane of the workgroup calls it.  A wave groups its lanes by
// key, at most 64 rounds; the first group's (key, count) goes to the wave's LDS slot, from which one lane per call merges the
// MS_WAVES slots of the workgroup after the barrier; the later groups, rare, are added at once.  Integer sums: exact in any order.
constexpr int MS_THREADS = 1024, MS_WAVES = MS_THREADS / 64;

__device__ __forceinline__ void wave_count(int* __restrict__ cnt, int key, bool on, int* __restrict__ slot_key, int* __restrict__ slot_cnt) {
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    unsigned long long todo = __ballot(on);
    if (lane == 0) slot_cnt[wave] = 0;
    for (bool first = true; todo; first = false) {
        const int leader = __builtin_ctzll(todo);
        const int k = __shfl(key, leader);
        const unsigned long long same = __ballot(on && key == k);
        if (lane == leader) {
            if (first) slot_key[wave] = k, slot_cnt[wave] = (int)__popcll(same);
            else atomicAdd(cnt + k, (int)__popcll(same));
        }
        todo &= ~same;
    }
}

__device__ __forceinline__ void merge_slots(int* __restrict__ cnt, const int* __restrict__ slot_key, const int* __restrict__ slot_cnt) {
    for (int w = 0; w < MS_WAVES; ++w) {
        if (slot_cnt[w] == 0) continue;
        bool merged = false;                                                 // (an earlier slot with this key has taken this one's count)
        for (int e = 0; e < w; ++e) merged = merged || (slot_cnt[e] != 0 && slot_key[e] == slot_key[w]);
        if (merged) continue;
        int sum = slot_cnt[w];
        for (int l = w + 1; l < MS_WAVES; ++l)
            if (slot_cnt[l] != 0 && slot_key[l] == slot_key[w]) sum += slot_cnt[l];
        atomicAdd(cnt + slot_key[w], sum);
    }
}

__global__ __launch_bounds__(MS_THREADS) void mesh_sizes_kernel(const int* __restrict__ label, const int* __restrict__ faces,
                                                                long n_faces, int n, int* __restrict__ fcount,
                                                                int* __restrict__ vcount) {
    __shared__ int s_key[2][MS_WAVES], s_cnt[2][MS_WAVES];
    const long i = (long)blockIdx.x * MS_THREADS + threadIdx.x;
    int lv = 0, lf = 0;
    bool von = false, fon = false;
    if (i < n) {
        lv = label[i];
        von = in_range(lv, n);
    }
    if (i < n_faces) {
        const int i0 = faces[3 * i], i1 = faces[3 * i + 1], i2 = faces[3 * i + 2];
        if (in_range(i0, n) && in_range(i1, n) && in_range(i2, n)) {
            lf = label[i0];
            fon = in_range(lf, n);
        }
    }
    wave_count(vcount, lv, von, s_key[0], s_cnt[0]);
    wave_count(fcount, lf, fon, s_key[1], s_cnt[1]);
    __syncthreads();
    if (threadIdx.x == 0) merge_slots(vcount, s_key[0], s_cnt[0]);
    if (threadIdx.x == 64) merge_slots(fcount, s_key[1], s_cnt[1]);
}

struct MeshF3 { float x, y, z; };
struct MeshB3 { unsigned char x, y, z; };

__device__ __forceinline__ void face_normal(const MeshF3 a, const MeshF3 b, const MeshF3 c, double (&nrm)[3]) {
    const double u0 = (double)b.x - (double)a.x, u1 = (double)b.y - (double)a.y, u2 = (double)b.z - (double)a.z;
    const double v0 = (double)c.x - (double)a.x, v1 = (double)c.y - (double)a.y, v2 = (double)c.z - (double)a.z;
    nrm[0] = u1 * v2 - u2 * v1;
    nrm[1] = u2 * v0 - u0 * v2;
    nrm[2] = u0 * v1 - u1 * v0;
}

__global__ __launch_bounds__(MC_THREADS) void mesh_mark_kernel(const float* __restrict__ xyz, const int* __restrict__ faces,
                                                               const int* __restrict__ label, const unsigned char* __restrict__ keep_comp,
                                                               long n_faces, int n, int drop_degenerate, int* __restrict__ fmark,
                                                               int* __restrict__ vmark) {
    const long f = (long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (f >= n_faces) return;
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    bool keep = in_range(i0, n) && in_range(i1, n) && in_range(i2, n);
    if (keep) {
        const int l = label[i0];
        keep = in_range(l, n) && keep_comp[l] != 0;
    }
    if (keep && drop_degenerate) {
        if (i0 == i1 || i0 == i2 || i1 == i2) {
            keep = false;
        } else {
            const MeshF3* p = reinterpret_cast<const MeshF3*>(xyz);
            double nrm[3];
            face_normal(p[i0], p[i1], p[i2], nrm);
            keep = !(nrm[0] == 0.0 && nrm[1] == 0.0 && nrm[2] == 0.0);
        }
    }
    fmark[f] = keep ? 1 : 0;
    if (keep) vmark[i0] = 1, vmark[i1] = 1, vmark[i2] = 1;                    // (every writer stores the same value)
}

__global__ __launch_bounds__(MC_THREADS) void mesh_compact_kernel(const float* __restrict__ xyz, const unsigned char* __restrict__ rgb,
                                                                  const float* __restrict__ normals, const int* __restrict__ faces,
                                                                  const int* __restrict__ fmark, const int* __restrict__ vmark,
                                                                  const int* __restrict__ fincl, const int* __restrict__ vincl,
                                                                  long n_faces, int n, float* __restrict__ xyz_out,
                                                                  unsigned char* __restrict__ rgb_out, float* __restrict__ normals_out,
                                                                  int* __restrict__ faces_out, long n_faces_out, long n_vertices_out) {
    const long i = (long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (i < n && vmark[i]) {
        const long out = (long)vincl[i] - 1;
        if (out >= 0 && out < n_vertices_out) {                              // (prefix sums that do not belong to the marks write nothing)
            reinterpret_cast<MeshF3*>(xyz_out)[out] = reinterpret_cast<const MeshF3*>(xyz)[i];
            reinterpret_cast<MeshB3*>(rgb_out)[out] = reinterpret_cast<const MeshB3*>(rgb)[i];
            if (normals) reinterpret_cast<MeshF3*>(normals_out)[out] = reinterpret_cast<const MeshF3*>(normals)[i];
        }
    }
    if (i < n_faces && fmark[i]) {
        const long out = (long)fincl[i] - 1;
        const int i0 = faces[3 * i], i1 = faces[3 * i + 1], i2 = faces[3 * i + 2];
        if (out >= 0 && out < n_faces_out && in_range(i0, n) && in_range(i1, n) && in_range(i2, n)) {
            faces_out[3 * out] = vincl[i0] - 1;
            faces_out[3 * out + 1] = vincl[i1] - 1;
            faces_out[3 * out + 2] = vincl[i2] - 1;
        }
    }
}

// One lane per vertex gathers its corners in ascending corner id (corner 3 f + k is vertex faces[f][k]): no float atomics.
__global__ __launch_bounds__(MC_THREADS) void mesh_vertex_normals_kernel(const float* __restrict__ xyz, const int* __restrict__ faces,
                                                                         const int* __restrict__ corner_off,
                                                                         const int* __restrict__ corners, long n_faces, int n,
                                                                         float* __restrict__ normals) {
    const long v = (long)blockIdx.x * MC_THREADS + threadIdx.x;
    if (v >= n) return;
    const MeshF3* p = reinterpret_cast<const MeshF3*>(xyz);
    const long n_corners = 3 * n_faces;
    long beg = corner_off[v], end = corner_off[v + 1];
    if (beg < 0 || end > n_corners) beg = end = 0;                           // (offsets that are not a CSR of the faces read nothing)
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (long c = beg; c < end; ++c) {
        const int cid = corners[c];
        if (cid < 0 || cid >= n_corners) continue;
        const long f = cid / 3;
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        if (!(in_range(i0, n) && in_range(i1, n) && in_range(i2, n))) continue;
        double nrm[3];
        face_normal(p[i0], p[i1], p[i2], nrm);
        s0 += nrm[0];
        s1 += nrm[1];
        s2 += nrm[2];
    }
    const double len = sqrt(s0 * s0 + s1 * s1 + s2 * s2);
    MeshF3 out{0.0f, 0.0f, 0.0f};
    if (len > 0.0 && len <= 1.7976931348623157e308) out = MeshF3{(float)(s0 / len), (float)(s1 / len), (float)(s2 / len)};
    reinterpret_cast<MeshF3*>(normals)[v] = out;
}

static int check_counts(const char* what, long n_faces, long n_vertices) {
    PSCV_CHECK_ARG(n_vertices >= 0 && n_vertices <= MC_MAX, "%s: n_vertices=%ld outside [0, 2^31)", what, n_vertices);
    PSCV_CHECK_ARG(n_faces >= 0 && 3 * n_faces <= MC_MAX, "%s: n_faces=%ld outside [0, 2^31 / 3)", what, n_faces);
    return 0;
}

static dim3 grid_for(long lanes) { return dim3((unsigned)((lanes + MC_THREADS - 1) / MC_THREADS)); }

}  // namespace pscv

extern "C" int pscv_mesh_components(const int* faces, long n_faces, long n_vertices, int* label, int* status, void* stream) {
    using namespace pscv;
    const char* what = "pscv_mesh_components";
    if (check_counts(what, n_faces, n_vertices)) return -1;
    PSCV_CHECK_ARG(status, "%s: null pointer argument", what);
    if (n_vertices == 0) return 0;                                           // (faces of an empty vertex set are counted by the caller)
    PSCV_CHECK_ARG(label && (faces || n_faces == 0), "%s: null pointer argument", what);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int n = (int)n_vertices;
    int rc = launch(what, mesh_init_kernel, grid_for(n_vertices), dim3(MC_THREADS), 0, st, label, n);
    if (rc || n_faces == 0) return rc;
    rc = launch(what, mesh_hook_kernel, grid_for(n_faces), dim3(MC_THREADS), 0, st, faces, n_faces, n, label, status);
    if (rc) return rc;
    return launch(what, mesh_flatten_kernel, grid_for(n_vertices), dim3(MC_THREADS), 0, st, label, n, status);
}

extern "C" int pscv_mesh_component_sizes(const int* label, const int* faces, long n_faces, long n_vertices, int* fcount, int* vcount,
                                         void* stream) {
    using namespace pscv;
    const char* what = "pscv_mesh_component_sizes";
    if (check_counts(what, n_faces, n_vertices)) return -1;
    if (n_vertices == 0) return 0;
    PSCV_CHECK_ARG(label && fcount && vcount && (faces || n_faces == 0), "%s: null pointer argument", what);
    const long lanes = n_faces > n_vertices ? n_faces : n_vertices;
    return launch(what, mesh_sizes_kernel, dim3((unsigned)((lanes + MS_THREADS - 1) / MS_THREADS)), dim3(MS_THREADS), 0,
                  reinterpret_cast<hipStream_t>(stream), label, faces,
                  n_faces, (int)n_vertices, fcount, vcount);
}

extern "C" int pscv_mesh_mark(const float* xyz, const int* faces, const int* label, const unsigned char* keep_comp, long n_faces,
                              long n_vertices, int drop_degenerate, int* fmark, int* vmark, void* stream) {
    using namespace pscv;
    const char* what = "pscv_mesh_mark";
    if (check_counts(what, n_faces, n_vertices)) return -1;
    PSCV_CHECK_ARG(drop_degenerate == 0 || drop_degenerate == 1, "%s: drop_degenerate=%d must be 0 or 1", what, drop_degenerate);
    if (n_faces == 0) return 0;
    PSCV_CHECK_ARG(faces && fmark, "%s: null pointer argument", what);
    PSCV_CHECK_ARG(n_vertices == 0 || (xyz && label && keep_comp && vmark), "%s: null pointer argument", what);
    return launch(what, mesh_mark_kernel, grid_for(n_faces), dim3(MC_THREADS), 0, reinterpret_cast<hipStream_t>(stream), xyz, faces,
                  label, keep_comp, n_faces, (int)n_vertices, drop_degenerate, fmark, vmark);
}

extern "C" int pscv_mesh_compact(const float* xyz, const unsigned char* rgb, const float* normals, const int* faces, const int* fmark,
                                 const int* vmark, const int* fincl, const int* vincl, long n_faces, long n_vertices, float* xyz_out,
                                 unsigned char* rgb_out, float* normals_out, int* faces_out, long n_faces_out, long n_vertices_out,
                                 void* stream) {
    using namespace pscv;
    const char* what = "pscv_mesh_compact";
    if (check_counts(what, n_faces, n_vertices)) return -1;
    PSCV_CHECK_ARG(n_faces_out >= 0 && n_faces_out <= n_faces, "%s: n_faces_out=%ld outside [0, %ld]", what, n_faces_out, n_faces);
    PSCV_CHECK_ARG(n_vertices_out >= 0 && n_vertices_out <= n_vertices, "%s: n_vertices_out=%ld outside [0, %ld]", what, n_vertices_out,
                   n_vertices);
    PSCV_CHECK_ARG((normals == nullptr) == (normals_out == nullptr) || n_vertices_out == 0,
                   "%s: normals and normals_out must be given together", what);
    if (n_vertices_out == 0) return 0;                                       // (no vertex survives: no face does)
    PSCV_CHECK_ARG(xyz && rgb && vmark && vincl && xyz_out && rgb_out, "%s: null pointer argument", what);
    PSCV_CHECK_ARG(n_faces_out == 0 || (faces && fmark && fincl && faces_out), "%s: null pointer argument", what);
    const long nf = n_faces_out == 0 ? 0 : n_faces;
    const long lanes = nf > n_vertices ? nf : n_vertices;
    return launch(what, mesh_compact_kernel, grid_for(lanes), dim3(MC_THREADS), 0, reinterpret_cast<hipStream_t>(stream), xyz, rgb,
                  normals, faces, fmark, vmark, fincl, vincl, nf, (int)n_vertices, xyz_out, rgb_out, normals_out, faces_out, n_faces_out,
                  n_vertices_out);
}

extern "C" int pscv_mesh_vertex_normals(const float* xyz, const int* faces, const int* corner_off, const int* corners, long n_faces,
                                        long n_vertices, float* normals, void* stream) {
    using namespace pscv;
    const char* what = "pscv_mesh_vertex_normals";
    if (check_counts(what, n_faces, n_vertices)) return -1;
    if (n_vertices == 0) return 0;
    PSCV_CHECK_ARG(xyz && corner_off && normals && ((faces && corners) || n_faces == 0), "%s: null pointer argument", what);
    return launch(what, mesh_vertex_normals_kernel, grid_for(n_vertices), dim3(MC_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                  xyz, faces, corner_off, corners, n_faces, (int)n_vertices, normals);
}
