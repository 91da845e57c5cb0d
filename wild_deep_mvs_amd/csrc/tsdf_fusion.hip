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
#include "tsdf_dev.h"

namespace pscv {

// ---- integration (the rule itself: tsdf_dev.h) -----------------------------------------------------------------------------------
constexpr int TI_TX = 64, TI_TY = 4, TI_THREADS = TI_TX * TI_TY;

__global__ __launch_bounds__(TI_THREADS) void tsdf_integrate_kernel(const TsdfArgs a) {
    __shared__ unsigned long long s_live;
    const int tid = threadIdx.x;
    const int tiles_x = (a.nx + TI_TX - 1) / TI_TX, tiles_y = (a.ny + TI_TY - 1) / TI_TY;
    const int b = blockIdx.x;
    const int k = b / (tiles_x * tiles_y), rem = b - k * (tiles_x * tiles_y);
    const int ty = rem / tiles_x, tx = rem - ty * tiles_x;
    const int i0 = tx * TI_TX, j0 = ty * TI_TY;
    bool keep = false;
    if (tid < a.n_views) {                                        // wave 0: lane v judges view v (n_views <= 64)
        const int i1 = min(i0 + TI_TX, a.nx) - 1, j1 = min(j0 + TI_TY, a.ny) - 1;
        const double bx[2] = {a.o0 + (double)i0 * a.s, a.o0 + (double)i1 * a.s};
        const double by[2] = {a.o1 + (double)j0 * a.s, a.o1 + (double)j1 * a.s};
        const double bz[2] = {a.o2 + (double)k * a.s, a.o2 + (double)k * a.s};
        // (a.w[tid], a.h[tid] and the camera row are indexed per lane: the by-value argument struct stays in the kernel-argument
        // segment and these become loads from it.  Indexing a COPY of the struct, or of its arrays, per lane would put it in
        // scratch: check "ScratchSize: 0" in -Rpass-analysis=kernel-resource-usage after any change here)
        keep = !tile_culled(a.cams + (long)tid * PSCV_GEO_CAM_FLOATS, (double)a.w[tid], (double)a.h[tid], (double)a.dmax[tid],
                            a.trunc, bx, by, bz);
    }
    const unsigned long long live = tsdf_share_live(s_live, tid < 64, keep);   // (in scalar registers: the view loop is uniform)
    if (live == 0) return;
    const int i = i0 + (tid & (TI_TX - 1)), j = j0 + tid / TI_TX;
    if (i >= a.nx || j >= a.ny) return;
    const long lin = ((long)k * a.ny + j) * a.nx + i;
    tsdf_update_voxel(a, live, lin, a.o0 + (double)i * a.s, a.o1 + (double)j * a.s, a.o2 + (double)k * a.s);
}

// ---- extraction: marching tetrahedra (the case table, the flags and the vertex and face rules: tsdf_dev.h) -------------------------
constexpr int TM_TX = 32, TM_TY = 4, TM_TZ = 2, TM_THREADS = TM_TX * TM_TY * TM_TZ;
constexpr int TM_PX = TM_TX + 1, TM_PY = TM_TY + 1, TM_PZ = TM_TZ + 1;

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
            f = tsdf_flags(tsdf_sum[lin], weight[lin], min_weight);
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
    info[((long)k * ny + j) * nx + i] = tsdf_cell_info(cf);
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
        const double Xq[3] = {o0 + (double)(i + (d & 1)) * s, o1 + (double)(j + (d >> 1 & 1)) * s, o2 + (double)(k + (d >> 2)) * s};
        if (out >= 0 && out < n_vertices) tsdf_write_vertex(P, Q, Xp, Xq, xyz, rgb, out);   // (prefix sums that do not belong to `info`
                                                                                            // write nothing)
        ++out;
    }
}

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
        tsdf_write_faces(q, q, cnt, faces, out, n_faces);
    }
}

}  // namespace pscv

extern "C" int pscv_tsdf_integrate(const float* const* depth, const unsigned int* const* color, const int* hw, int n_views,
                                   const float* cams, const float* dmax, double o0, double o1, double o2, double voxel, double trunc,
                                   int nx, int ny, int nz, float* tsdf_sum, int* weight, float* rgb_sum, int* cweight, void* stream) {
    using namespace pscv;
    const char* what = "pscv_tsdf_integrate";
    PSCV_CHECK_ARG(depth && color && hw && cams && dmax && tsdf_sum && weight && rgb_sum && cweight, "%s: null pointer argument", what);
    TsdfArgs a;
    if (tsdf_setup(what, a, depth, color, hw, n_views, cams, dmax, o0, o1, o2, voxel, trunc, nx, ny, nz, true)) return -1;
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
    if (check_grid(what, o0, o1, o2, voxel) || check_dims(what, nx, ny, nz)) return -1;
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
