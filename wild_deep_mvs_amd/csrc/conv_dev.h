// Device half shared by the 3-D convolution kernels (conv3d*.hip), next to the host half in conv_common.h: buffer descriptors, the
// plane fetch of the depth sweeps and the 4-channel epilogue.  Forced inline, free functions over the kernels' own locals.  Built
// with them the depth sweeps' instruction streams differ from the in-place code (scheduling, register numbers, a few scalar
// instructions fewer), with equal instruction-class counts and resource rows: scripts/dev/isa_diff.py, profiles/conv_dev_isa.txt.
#pragma once
#include "pscv_common.h"

namespace pscv {

// ---- zero padding through buffer descriptors: THE rule of the conv family ---------------------------------------------
// The hardware compares every lane's byte offset (vector + scalar offset) of a raw buffer instruction with the descriptor's size: a
// load beyond it returns zeros, a store beyond it is dropped.  That is the convolution's zero padding and the ragged-edge mask:
//   * a lane whose voxel lies outside the image (or its tile) carries BUF_OOR as its offset, made once per thread;
//   * a plane (row, volume) outside the tensor gets an EMPTY descriptor (size 0), made from wave-uniform values;
//   * `size` counts from the descriptor's base: a base advanced by a channel offset has that offset taken off its size.
// BUF_OOR is beyond every size the launchers allow (each checks its planes or volumes against 2 GiB) and, a multiple of 16 with 15
// bytes to spare below 2^31, neither comes into range nor wraps within a 16-byte access.
constexpr int BUF_FLAGS = 0x00020000;          // word 3 of a raw buffer descriptor on gfx950: DATA_FORMAT = 32 bits, all else 0
constexpr unsigned BUF_OOR = 0x7ffffff0u;
typedef unsigned buf_u32x2 __attribute__((ext_vector_type(2)));   // payloads of the raw buffer stores
typedef unsigned buf_u32x4 __attribute__((ext_vector_type(4)));

// descriptor of `size` bytes at `p`
template <typename T>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const T* p, int size) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(p), (short)0, size, BUF_FLAGS);
}
// descriptor of plane `plane` of a tensor whose planes lie `stride` elements of T apart and hold `size_bytes` bytes from `base` on;
// an empty one when !valid (wave-uniform: the plane is outside the volume)
template <typename T, typename S>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t plane_rsrc(const T* base, int plane, S stride, unsigned size_bytes, bool valid) {
    static_assert(sizeof(S) == 8, "plane * stride is a 64-bit product: pass the stride as long / unsigned long");
    return buf_rsrc(base + (S)(valid ? plane : 0) * stride, valid ? (int)size_bytes : 0);
}

// The plane fetch of a depth sweep: a thread owns NLD 16-byte chunks at the same in-plane positions of every input plane.  The kernel
// decodes (voxel, chunk) -> goff[i] once (bytes inside a plane, BUF_OOR outside the image); a plane then costs one descriptor and NLD
// loads, no predicate, zero fill or 64-bit address arithmetic per chunk.  Planes outside [0, plane_hi] read as zeros.  base: plane 0
// of the batch item, channel offset applied; stride: elements of T between planes; bytes: of a plane from `base` on.
template <int NLD, typename T, typename S>
__device__ __forceinline__ void plane_fetch(const T* base, S stride, unsigned bytes, int plane_hi, const unsigned (&goff)[NLD], int plane,
                                            uint4 (&reg)[NLD]) {
    const __amdgpu_buffer_rsrc_t rs = plane_rsrc(base, plane, stride, bytes, plane >= 0 && plane <= plane_hi);
#pragma unroll
    for (int i = 0; i < NLD; ++i) reg[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)goff[i], 0, 0));
}
// ... of one chunk per thread
template <typename T, typename S>
__device__ __forceinline__ uint4 plane_fetch(const T* base, S stride, unsigned bytes, int plane_hi, unsigned goff, int plane) {
    const __amdgpu_buffer_rsrc_t rs = plane_rsrc(base, plane, stride, bytes, plane >= 0 && plane <= plane_hi);
    return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)goff, 0, 0));
}

// ---- epilogue ---------------------------------------------------------------------------------------------------------
// y = post(pre(acc * scale + bias) + skip), pre = max(., floor) and post = max(., 0) where the layer's PSCV_EPI_RELU_* flags say so.
// The constants of output channel c: a null pointer is the identity (scale 1, bias 0, floor 0).
__device__ __forceinline__ float epi_scale(const float* scale, int c) { return scale ? scale[c] : 1.0f; }
__device__ __forceinline__ float epi_bias(const float* bias, int c) { return bias ? bias[c] : 0.0f; }
__device__ __forceinline__ float epi_floor(const float* floor, int c) { return floor ? floor[c] : 0.0f; }
// "clamp" form: the ReLU switches folded into the floors (-inf = off: relu_floor never selects it), for epilogues without branches
__device__ __forceinline__ float epi_floor_clamp(const float* floor, int c, int epi) {
    return (epi & PSCV_EPI_RELU_PRE) ? epi_floor(floor, c) : -__builtin_inff();
}
__device__ __forceinline__ float epi_lo_post(int epi) { return (epi & PSCV_EPI_RELU_POST) ? 0.0f : -__builtin_inff(); }
// ... of a lane's four consecutive channels c0 .. c0 + 3; CLAMP: the clamp form of the floors
template <bool CLAMP = false>
__device__ __forceinline__ void epi_load4(float (&sc)[4], float (&bi)[4], float (&fl)[4], const float* scale, const float* bias,
                                          const float* floor, int c0, int epi = 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        sc[k] = epi_scale(scale, c0 + k);
        bi[k] = epi_bias(bias, c0 + k);
        fl[k] = CLAMP ? epi_floor_clamp(floor, c0 + k, epi) : epi_floor(floor, c0 + k);
    }
}
__device__ __forceinline__ void relu4(float (&y)[4], float lo) {
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = relu_floor(y[k], lo);
}

// the residual's four 16-bit values (a lane's 8 bytes of the skip tensor) added to y
template <typename H>
__device__ __forceinline__ void add_skip4(float (&y)[4], const uint2& sv) {
    y[0] += Half16<H>::lo(sv.x); y[1] += Half16<H>::hi(sv.x);
    y[2] += Half16<H>::lo(sv.y); y[3] += Half16<H>::hi(sv.y);
}
// ... added and clamped ("clamp" form)
template <typename H>
__device__ __forceinline__ void add_skip4_clamp(float (&y)[4], const uint2& sv, float lo_post) {
    y[0] = relu_floor(y[0] + Half16<H>::lo(sv.x), lo_post); y[1] = relu_floor(y[1] + Half16<H>::hi(sv.x), lo_post);
    y[2] = relu_floor(y[2] + Half16<H>::lo(sv.y), lo_post); y[3] = relu_floor(y[3] + Half16<H>::hi(sv.y), lo_post);
}
// four channels as they are stored: 16-bit (8 bytes) or fp32
template <typename H>
__device__ __forceinline__ uint2 pack4(const float (&y)[4]) { return make_uint2(Half16<H>::pack(y[0], y[1]), Half16<H>::pack(y[2], y[3])); }
__device__ __forceinline__ float4 pack4_f32(const float (&y)[4]) { return make_float4(y[0], y[1], y[2], y[3]); }

}  // namespace pscv
