/*
 * pscv.h -- C ABI of the MI355X (gfx950) plane-sweep cost-volume engine.
 *
 * The reference (fdarmon/wild_deep_mvs) has no FFI or operator registry: its hot
 * path is a chain of ATen calls inside models/<arch> forward().  This header is
 * the boundary a maintainer would bind instead of those calls (ctypes stub in
 * INTEGRATION.md; the in-tree binding is wild_deep_mvs_amd/_lib.py).  Each entry
 * point names the reference code it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; every tensor pointer is a DEVICE pointer
 *     borrowed for the duration of the call unless marked "host";
 *   - asynchronous on the given hipStream_t (passed as void*); no allocation,
 *     no global mutable state, re-entrant per stream;
 *   - return 0 on success, negative on error; the message is available from
 *     pscv_last_error() (thread-local);
 *   - tensors are channels-last: feature maps [B,h,w,C], volumes [B,D,h,w,C];
 *     dtype codes select fp32, bf16 or fp16 STORAGE, arithmetic is always fp32
 *     (bf16 / fp16 MFMA products accumulate in fp32).
 */
#ifndef PSCV_H
#define PSCV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSCV_ABI_VERSION 14

/* storage dtypes */
#define PSCV_F32 0
#define PSCV_BF16 1
#define PSCV_F16 2 /* IEEE half, stores saturate at +-65504; a NaN is stored as NaN */

/* sampling geometry of the warp */
#define PSCV_GEOM_PROJ 0  /* q = rot*(x,y,1)*d + trans, integer pixel centres, sample at index (u,v):
                             MVSNet models/MVSNet/module.py:127-166, CVP models/CVP_MVSNet/models/modules.py:74-128 */
#define PSCV_GEOM_HOMOG 1 /* hom = A*(x+.5,y+.5,1) - Bm*(..)/(d+1e-9), sample at index u*(W-1)/W:
                             Vis-MVSNet models/VisMVSNet/homography.py:23-120 */

/* cost aggregation fused behind the warp */
#define PSCV_COST_VARIANCE 0     /* sum f^2/N - (sum f)^2/N^2          models/MVSNet/model.py:113-139 */
#define PSCV_COST_VARIANCE_CVP 1 /* sum f^2/N - (sum f / N)^2          models/CVP_MVSNet/models/net.py:129-152, modules.py:229-293 */
#define PSCV_COST_SOFTMIN 2      /* sum_v e diff/(sum_v e + 1e-6)      models/MVSNet/model.py:141-173 */
#define PSCV_COST_GROUPCORR 3    /* per source, 4-channel group dot    models/VisMVSNet/nn_utils.py:473-490 (call model_cas.py:340) */
#define PSCV_COST_WARP_ONLY 4    /* per source warped volume           homo_warping / homography_warping themselves */
#define PSCV_COST_VARIANCE_PARTIAL 5 /* fp32 partial sums (sum f, sum f^2) over the GIVEN views for a source-view shard across GPUs:
                                    out [2][B,D,h,w,C] fp32; ref may be NULL (only one rank adds the reference view).  The ranks'
                                    outputs are all-reduced (RCCL) and pscv_variance_finish turns them into the cost volume */

#define PSCV_MAX_SRC 16
#define PSCV_CAM_FLOATS 18 /* per (source, batch): PROJ = rot[9] trans[3] pad[6]; HOMOG = A[9] Bm[9] */

/* conv3d kinds */
#define PSCV_CONV_S1 0 /* Conv3d k3 s1 p1 (also ConvTranspose3d k3 s1 p1, packed flipped) */
#define PSCV_CONV_S2 1 /* Conv3d k3 s2 p1 */
#define PSCV_CONV_T2 2 /* ConvTranspose3d k3 s2 p1 output_padding 1 */
#define PSCV_CONV_S1P8 3 /* Conv3d k3 s1 p1 (or ConvTranspose3d k3 s1 p1) with c_in = 8, 16 or 32 and c_out = 8, or 16 -> 16, on the depth-sweep
                            kernels (plane-pair packed MFMA rows, register-resident weights); same result as PSCV_CONV_S1, own
                            packed layout */
#define PSCV_CONV_T2P8 5 /* ConvTranspose3d k3 s2 p1 op1 with c_in = 16, c_out = 8 on the parity-pair packed kernel; same
                            result as PSCV_CONV_T2, own packed layout */
#define PSCV_CONV_S1C1 4 /* Conv3d k3 s1 p1 with c_out = 1, c_in = 8 or 16 (the `prob` heads) on the depth-in-rows MFMA
                            kernel (six output planes share one MFMA tile); same result as PSCV_CONV_S1, own packed layout */

/* epilogue flags for pscv_conv3d */
#define PSCV_EPI_RELU_PRE 1  /* y = max(y, 0) before the skip add   (MVSNet/CVP: skip + relu(bn(deconv))) */
#define PSCV_EPI_RELU_POST 2 /* y = max(y, 0) after the skip add    (Vis BasicBlock: relu(bn(conv) + residual)) */

const char* pscv_last_error(void);
int pscv_abi_version(void);

/* Tuning knobs for measurement runs (not part of the reference's surface).  A knob holds ONE process-wide value (a relaxed
 * atomic; every launching host thread reads it, including PyTorch's autograd thread and DataParallel's replica threads) and an
 * optional per-thread override (pscv_set_tuning_thread).  Kernel selection never depends on anything else that is mutable.
 * The knobs themselves (key, symbol, default) are the PSCV_KNOB_TABLE of csrc/pscv_common.h; every key of it has ONE entry here.  Keys:
 *   "warp_q2"   1 (default): 32-channel 16-bit sweeps run on the quad-mapped kernel (one texel per lane quad, two depth
 *               planes per quad); 0: always the generic kernel.  "warp_lpv" != 0 also selects the generic kernel.
 *   "warp_lpv"  lanes sharing one voxel in the generic pscv_warp_cost kernel (1, 2 or 4 for C=32; 0 = default)
 *   "warp_ppd"  depth planes per workgroup in pscv_warp_cost (0 = default: 8 direct kernels, 32 LDS-staged kernel)
 *   "warp_tiled" 1 (default; -1 restores it; 2 = the same): pscv_warp_cost stages the source patches of a reference tile in LDS
 *               as fp32 where it applies (C = 32, 16-bit features, per-batch planes, PROJ geometry, 1-4 source views, variance /
 *               softmin) -- same bits as the direct-gather kernels; 0: always the direct-gather kernels.  "warp_lpv" != 0
 *               also selects the direct kernel.  (The kernel is built without packed fp32 instructions: `v_pk_*_f32` with
 *               the op_sel bit of src1 set is unreliable beside MFMA kernels of another stream)
 *               4: the lane-owns-voxel kernel (csrc/warp_cost_lv.hip; variance costs; same stored bits): 14 % fewer vector-ALU
 *               instructions and 2 % less time than the default on narrow-baseline rigs, ~2x slower where boxes do not fit the
 *               LDS arena (wide baselines) -- an alternative, not the default.
 *   "warp_tile" test / measurement aids (0 = off).  LDS-staged kernel: 1 = no adaptive split (a 32-plane chunk whose source boxes do not
 *               fit the LDS arena is normally swept as two 16-plane halves with their own boxes instead of taking global taps).
 *               Lane-owns-voxel kernel: 2 = the same split (off by default there: slower on narrow baselines); 7 = every block on its general path; ablations: 8 = no stores, 9 = no taps, 10 = neither
 *   "warp_gc_lds" 1 (default): group-wise correlation volumes (C = 32, 16-bit, HOMOG geometry, maps of >= 21 x 21 texels) over PER-BATCH
 *               planes run the LDS-staged kernel (csrc/warp_gc_lv.hip; 1.8x the quad kernel on the stage-1 shape of BASELINE
 *               configuration 5; values equal to one 16-bit ulp); 2: per-pixel planes too (slower when the per-pixel depths of a tile
 *               spread widely: boxes that do not fit the LDS take slow global taps); 0: always the quad kernel
 *   "warp_lds_pad" KiB of LDS the LDS-staged warp kernel requests on top of its need (0 = default): fewer workgroups per CU with
 *               the same code (occupancy / stream co-residency experiments)
 *   "sweep_dc"  depth planes per workgroup of the depth-sweep convs (0 = default heuristic)
 *   "sweepc_slots" resident-workgroup target that sizes the depth chunks of the 8|16 -> 8 depth-sweep conv (0 = 768)
 *   "sweepc_pd" prefetch distance in iterations (1..3) of the same kernel (0 = 1)
 *   "sweep_th16" 1: the 32->8 depth-sweep conv uses 16-row tiles / 512 threads; 0 (default): 8-row tiles / 256 threads (measured 116 us
 *               against 107 us at the headline size: one workgroup per CU hides less latency)
 *   "sweep_kdm" 1: the 32->8 depth-sweep conv runs the kd-in-rows formulation (32x32x16 MFMAs whose rows hold the three depth
 *               taps; one input plane per iteration, 3-slot ring, three workgroups per CU) with depth chunks sized for 768 resident
 *               workgroups; 2: sized for 1024; 0 (default): the plane-pair kernel.  Same products, another fp32 summation order
 *               (1e-4 apart before the 16-bit store).
 *   "sweep_kdm_pd"  planes in flight per workgroup of the kd-in-rows kernel: 2, or 1 (0 = default = 1)
 *   "warp_bwd_direct" 1: pscv_warp_cost_bwd issues one global float atomic per tap; 0 (default): accumulates per-workgroup
 *               LDS patches and flushes them coalesced
 *   "c1_sweep"  1 (default): 1-channel heads with 8 input channels and at least three 6-plane blocks per depth chunk run the
 *               depth-sweep variant; 0: always the brick variant; 2: the sweep at any depth
 *   "c1_nb"     6-plane blocks per workgroup of the 1-channel heads (0 = default: 1 or 2 for the brick variant, one resident round of
 *               workgroups for the depth sweep; values above 2 reach the depth sweep only)
 *   "conv_s2_sweep"  1 (default): stride-2 layers with 8 input channels and <= 32 output channels on volumes of >= 64 Ki output
 *               voxels run the stride-2 depth-sweep kernel; 0: always the brick kernel; 2: the sweep at any size (same packed weights, same result up to
 *               fp32 summation order)
 *   "s2s_slots"  resident-workgroup target that sizes the depth chunks of the stride-2 depth-sweep kernel (0 = 768)
 *   "block8_slots"  low 16 bits: resident-workgroup target that sizes the depth chunks of pscv_conv3d_block8 (0 = 768); the bits
 *               above them are debug flags of that kernel (0 in any normal run)
 *   "conv2d_wlds"  1 (default): 64-channel k3 s1 2-D layers with 32 | 64 output channels and >= 512 tiles run the persistent
 *               kernel that keeps the layer's packed weights in LDS; 0: always conv2d_kernel; 2: at any size (same bits)
 *   "conv_wide"  1 (default): stride-1 3-D layers with 64 input and 32 | 64 output channels on volumes of >= 512 tiles (4 x 4 x 16
 *               voxels) run the persistent 8-wave kernel with the weights through a shared LDS double buffer (csrc/conv3d_wide.hip;
 *               same bits as the brick kernel); 0: always the brick kernel; 2: at any size, and the 32-input layers too
 *   "conv_tall64"  1 (default): on the brick kernel, 64-input stride-1 layers take 4 x 8 x 16 tiles where the grid fills the chip;
 *               0: 4 x 4 x 16; 2: at any size
 *   "tail_nbk"  6-plane blocks per depth chunk of pscv_tail_sweep (0 = default: one resident round of workgroups)
 *   "conv_small_tiles"  1 (default): small volumes use 1x4x16 tiles with the output channels split over
 *               blockIdx.y; 0: always the large-tile variant
 *   "conv_small_nt"  1 | 2 | 4: 16-channel output tiles per workgroup of the small-volume and stride-2 variants (0 = default choice)
 *   "softargmin_small"  1 (default): pscv_softargmin on depth axes of <= 32 planes (fp32 logits, no probability or partial outputs)
 *               runs the one-thread-per-pixel kernel; 0: always the slice kernel
 *   "fuse_c0"   ablation bits for builds made with -DPSCV_ABLATE (measurement only: the conv depth sweep, the weight gradient and
 *               the warp backward each skip a part of their work per bit, and results are wrong with any bit set); no effect on a
 *               normal build */
int pscv_set_tuning(const char* key, int value);

/* The same knobs for the CALLING host thread only (enable = 1: this thread reads `value` instead of the process-wide one;
 * enable = 0: drop the override).  pscv_set_tuning itself is process-wide: launches issued from other host threads -- PyTorch
 * runs autograd's backward on its own thread, nn.DataParallel runs replicas on worker threads -- see it too. */
int pscv_set_tuning_thread(const char* key, int value, int enable);
/* The value the CALLING thread's next launch would use (its override if set, else the process-wide value). */
int pscv_get_tuning(const char* key, int* value);

/*
 * Camera blocks of the PROJ geometry in one launch: for every source view v != reference_frame,
 * rot|trans of P_v * P_ref^-1 (fp64 inside).  Replaces the torch.inverse / matmul pair of
 * models/MVSNet/module.py:128-130 (models/CVP_MVSNet/models/modules.py:89-98).
 *   proj  device fp32 [B,V,4,4] with last rows (0,0,0,1);  cams  device fp32 [V-1][B][PSCV_CAM_FLOATS],
 *   sources in view order with the reference view skipped.
 */
int pscv_proj_cams(const float* proj, int B, int V, int reference_frame, float* cams, void* stream);

/*
 * Camera blocks of the HOMOG geometry (Vis-MVSNet) in one launch: A and Bm of hom(d) = A p - Bm p / (d + 1e-9).
 * Replaces scale_camera + the matrix products of get_homographies (models/VisMVSNet/preproc.py:63-92,
 * models/VisMVSNet/homography.py:23-74; the per-plane 3x3 products disappear into the warp kernel).
 *   ref_cam  device fp32 [B,2,4,4] ([R|t], [K ; .]) as built by Frontend.fill_cam_array (frontend.py:14-24)
 *   src_cams device fp32 [n_src][B,2,4,4];  scale = 1 / s_scale;  cams device fp32 [n_src][B][PSCV_CAM_FLOATS]
 */
int pscv_homog_cams(const float* ref_cam, const float* src_cams, int B, int n_src, float scale, float* cams, void* stream);

/*
 * Fused plane-sweep warp + cost aggregation (one pass, the warped per-view volumes never reach HBM).
 * Replaces: MVSNet.build_cost_volume (models/MVSNet/model.py:109-176) + homo_warping (module.py:111-169);
 *           CVP net.py:129-152 and proj_cost (modules.py:229-293); Vis SingleStage.build_cost_volume +
 *           groupwise_correlation (model_cas.py:176-186,340).
 *
 *   ref     [B,h,w,C]                 reference feature map (unused for WARP_ONLY, may be NULL)
 *   srcs    host array of n_src device pointers, each [B,hs,ws,C]
 *   cams    device [n_src][B][PSCV_CAM_FLOATS] fp32
 *   depth   device fp32; per-batch planes: element (b,d) at depth[b*depth_bstride + d];
 *           per-pixel planes (depth_per_pixel=1): element (b,d,y,x) at depth[b*depth_bstride + (d*h + y)*w + x]
 *   out     VARIANCE*, SOFTMIN: [B,D,h,w,C];  GROUPCORR: [n_src][B,D,h,w,C/4];  WARP_ONLY: [n_src][B,D,h,w,C]
 *   C must be a multiple of 8 with C/8 in {1,2,4,8}; n_src <= PSCV_MAX_SRC.
 */
int pscv_warp_cost(const void* ref, const void* const* srcs, int n_src, const float* cams, const float* depth,
                   long depth_bstride, int depth_per_pixel, int geom, int cost, float temp, void* out, int B, int C,
                   int h, int w, int hs, int ws, int D, int in_dtype, int out_dtype, void* stream);

/*
 * pscv_warp_cost on a ROW SLAB of the reference image (ABI 7; the row-sharded Vis-MVSNet stages of a multi-GPU forward,
 * wild_deep_mvs_amd/models/VisMVSNet/model_cas.py forward_row_shard): `ref`, a per-pixel `depth` and `out` hold rows
 * [ref_y0, ref_y0 + h) of the full reference grid, the cameras are those of the WHOLE image, and every reference pixel is
 * evaluated at the coordinates (x, y + ref_y0) it has there -- the same fp32 operations on the same values as the
 * whole-image launch, so the slab's voxels are bit-identical to the corresponding rows of pscv_warp_cost's output.
 * ref_y0 = 0 is pscv_warp_cost.
 */
int pscv_warp_cost_rows(const void* ref, const void* const* srcs, int n_src, const float* cams, const float* depth,
                        long depth_bstride, int depth_per_pixel, int geom, int cost, float temp, void* out, int B, int C,
                        int h, int w, int hs, int ws, int D, int in_dtype, int out_dtype, int ref_y0, void* stream);

/*
 * Second half of a source-view-sharded variance cost volume (MVSNet / CVP-MVSNet): after the all-reduce of the
 * PSCV_COST_VARIANCE_PARTIAL outputs, out = sum2 / N - (sum / N)^2 in the rounding order of `cost`
 * (PSCV_COST_VARIANCE: models/MVSNet/model.py:134, PSCV_COST_VARIANCE_CVP: models/CVP_MVSNet/models/net.py:148).
 *   sums fp32 [2][n] (n = B*D*h*w*C, a multiple of 8), n_views = total number of views incl. the reference, out [n] in `dtype`.
 */
int pscv_variance_finish(const float* sums, long n, int n_views, int cost, int dtype, void* out, void* stream);

/*
 * Weight packing for pscv_conv3d (host side, done once at model-load time).
 * Replaces nothing in the reference; it is the layout contract between a checkpoint's
 * [C_out,C_in,3,3,3] (Conv3d) / [C_in,C_out,3,3,3] (ConvTranspose3d) fp32 tensors and the MFMA kernel.
 *   kind        PSCV_CONV_*
 *   transposed  1 if `w` is a ConvTranspose3d weight ([C_in,C_out,3,3,3]); required for T2, and with S1 it
 *               packs the spatially flipped kernel (ConvTranspose3d k3 s1 p1 == Conv3d with flipped taps)
 *   dtype       PSCV_BF16 or PSCV_F16: the 16-bit format of the packed weights (= the layer's activation format)
 *   returns the number of 16-bit elements of the packed buffer (call with packed == NULL to query), <0 on error.
 */
long pscv_pack_conv3d_weights(const float* w /*host*/, int c_in, int c_out, int kind, int transposed, int dtype,
                              uint16_t* packed /*host, may be NULL*/);
/* The same packing as one launch on device pointers (fp32 weights in, packed 16-bit out; the element count comes from
 * pscv_pack_conv3d_weights(NULL ...)): no device -> host copy when the weights change every optimizer step. */
int pscv_pack_conv3d_weights_device(const float* w /*device*/, int c_in, int c_out, int kind, int transposed, int dtype,
                                    uint16_t* packed /*device*/, void* stream);

/*
 * 3x3x3 convolution as an MFMA implicit GEMM with fused per-channel affine (folded eval-mode BatchNorm or bias),
 * ReLU and skip-add epilogue.
 * Replaces: ConvBnReLU3D / ConvBn3D (models/MVSNet/module.py:41-58), the Sequential(ConvTranspose3d, BatchNorm3d,
 *           ReLU) blocks and `prob` of CostRegNet (models/MVSNet/model.py:43-84; CVP net.py:50-85) and the conv /
 *           deconv members of the Vis UNet (models/VisMVSNet/nn_utils.py:194-278).
 *
 *   dtype    PSCV_BF16 or PSCV_F16: format of `in`, `skip` and `packed` (one MFMA operand type per launch)
 *   in       [B,Di,Hi,Wi,in_cstride], the layer reads channels [in_coff, in_coff + c_in)
 *   packed   device copy of pscv_pack_conv3d_weights output
 *   scale,bias  device fp32 [c_out]:  y = acc*scale + bias   (scale may be NULL = 1, bias may be NULL = 0)
 *   floor    device fp32 [c_out] or NULL: with PSCV_EPI_RELU_PRE, y = max(y, floor[c]) instead of max(y, 0)
 *            (floor = -inf keeps a channel linear; lets one launch carry ReLU and linear channels)
 *   skip     NULL or [B,Do,Ho,Wo,skip_cstride] read at channel offset skip_coff, added after RELU_PRE
 *   out      [B,Do,Ho,Wo,out_cstride] written at channel offset out_coff; out_dtype = dtype or PSCV_F32
 *   (Do,Ho,Wo) = (Di,Hi,Wi) for S1, ceil(./2) for S2, 2x for T2.
 *   c_in in {8,16,32,64}; c_out in {1,8,16,32,64}.
 */
int pscv_conv3d(const void* in, int dtype, int in_cstride, int in_coff, const uint16_t* packed, const float* scale,
                const float* bias, const float* floor, const void* skip, int skip_cstride, int skip_coff, void* out,
                int out_cstride, int out_coff, int out_dtype, int B, int Di, int Hi, int Wi, int c_in, int c_out,
                int kind, int epi_flags, void* stream);

/*
 * The same stride-1 3x3x3 convolution for a 16-channel input that is the CONCATENATION of two 8-channel slices living in different
 * tensors: channels 0..7 = in_a[..., a_coff : a_coff + 8], channels 8..15 = in_b[..., b_coff : b_coff + 8] -- the
 * `torch.cat([deconv_out, enc], dim=1)` in front of the Vis U-Net's decoder conv (models/VisMVSNet/nn_utils.py:269-272) is never
 * written: its two producers store dense 8-channel volumes (a strided half-voxel store into a 16-channel buffer costs the 8 -> 8
 * sweep 119 us instead of 65 us at 256 x 144 x 200) and this launch gathers them while staging.  `packed` is the PSCV_CONV_S1P8
 * packing of the [c_out, 16, 3, 3, 3] weight; c_out 8 or 16; everything else as pscv_conv3d.
 */
int pscv_conv3d_cat2(const void* in_a, int a_cstride, int a_coff, const void* in_b, int b_cstride, int b_coff, int dtype,
                     const uint16_t* packed, const float* scale, const float* bias, const float* floor, const void* skip,
                     int skip_cstride, int skip_coff, void* out, int out_cstride, int out_coff, int out_dtype, int B, int D, int H,
                     int W, int c_out, int epi_flags, void* stream);

/*
 * Input side of the 2-D extractors: fp32 NCHW images -> [B,H,W,8] 16-bit channels-last pixels (channels C..7 zero: the first
 * layer's padded input), and one level of CVP's image pyramid (FeaturePyramid.forward, models/CVP_MVSNet/models/net.py:34-47:
 * F.interpolate(img, scale_factor=0.5, mode='bilinear') -- with align_corners = False the 2 x 2 mean, computed in ATen's operation
 * order: same bits).  One pass over the image writes any of
 *   out_cl8  [B,H,W,8] 16-bit        the image itself in the extractor layout            (may be null)
 *   half_img [B,C,H/2,W/2] fp32      the half-resolution image (input of the next level)  (may be null)
 *   half_cl8 [B,H/2,W/2,8] 16-bit    the half-resolution image in the extractor layout    (may be null)
 * img device fp32 [B,C,H,W] contiguous, C <= 8; the half-resolution outputs need an even W.
 */
int pscv_image_prep(const float* img, int B, int C, int H, int W, int dtype, void* out_cl8, float* half_img, void* half_cl8, void* stream);

/*
 * Vis-MVSNet's UncertNet (models/VisMVSNet/model_cas.py:77-98) in eval mode, one launch for the entropy maps of all pairs:
 *   t1 = relu(s1 * conv3x3(x; w1) + b1)   1 -> 8      (BatchNorm folded: s = gamma / sqrt(var + eps), b = beta - mean * s)
 *   t2 = relu(s2 * conv3x3(t1; w2) + b2) + x          (x broadcast over the 8 channels, model_cas.py:95)
 *   out = conv3x3(t2; head)               8 -> 1      (head_convs[0]; the reference's live model has one head)
 * every convolution zero-pads its own input (padding 1), fp32 throughout like the reference.
 *   entropy [N, H, W] fp32 -> out [N, H, W] fp32 (the log-uncertainty that weights a pair in pscv_fuse_pairs).
 *   params  752 floats: w1 as [tap][c_out] (72) | s1 (8) | b1 (8) | w2 as [c_in][tap][c_out] (576) | s2 (8) | b2 (8) |
 *           head as [c_in][tap] (72); tap = 3 * ky + kx.
 */
int pscv_uncert_net(const float* entropy, const float* params, float* out, int N, int H, int W, void* stream);

/*
 * A residual block of two 8 -> 8 stride-1 3x3x3 convolutions in ONE depth sweep (Vis-MVSNet's 3-D U-Net: BasicBlock, models/
 * VisMVSNet/nn_utils.py:27-37 -- conv1 + bn1 + relu, conv2 + bn2, + identity, relu):
 *   t   = epi1(scale1 * conv(in; packed1) + bias1)                       kept in LDS as 16-bit planes, never written
 *   out = epi2(scale2 * conv(t; packed2) + bias2 [+ in if residual])
 * Same values as pscv_conv3d(layer 1) followed by pscv_conv3d(layer 2, skip = in): t is rounded to the storage format exactly
 * as the stored volume was, zero outside the volume (layer 2's padding).  packed1 / packed2: PSCV_CONV_S1P8 packing of
 * [8, 8, 3, 3, 3] weights; scale / bias / floor [8] or null; epi flags as pscv_conv3d; out 16-bit (the storage dtype), must not
 * alias in.
 */
int pscv_conv3d_block8(const void* in, int dtype, int in_cstride, int in_coff, const uint16_t* packed1, const float* scale1,
                       const float* bias1, const float* floor1, int epi1, const uint16_t* packed2, const float* scale2,
                       const float* bias2, const float* floor2, int epi2, int residual, void* out, int out_cstride, int out_coff,
                       int B, int D, int H, int W, void* stream);

/*
 * Visibility-weighted fusion of per-pair volumes (Vis-MVSNet, mode 'soft'), one pass:
 *     out = sum_v exp(-uncert_v) * interm_v / sum_v exp(-uncert_v)
 * Replaces the accumulate / divide sequence of models/VisMVSNet/model_cas.py:354-357,385-386.
 *   interm   host array of n_src device pointers, each [B,D,h,w,8] in `dtype` (bf16 / fp16)
 *   uncert   host array of n_src device pointers, each [B,h,w] fp32 (the UncertNet head output)
 *   out      normalise = 1: [B,D,h,w,8] in `dtype`;  normalise = 0: fp32 partial sums [B,D,h,w,8] (for a
 *            source-view shard: all-reduce `out` and `wsum_out` across ranks, then divide)
 *   wsum_out [B,h,w] fp32 sum of the weights, or NULL
 */
int pscv_fuse_pairs(const void* const* interm, const float* const* uncert, int n_src, int dtype, void* out,
                    float* wsum_out, int normalise, int B, int D, int h, int w, void* stream);

/*
 * Second half of a source-view-sharded fusion: out = partial / wsum after the partial sums of all ranks were
 * all-reduced (RCCL).  partial fp32 [B,D,h,w,8], wsum fp32 [B,h,w], out [B,D,h,w,8] in `dtype`.
 */
int pscv_fuse_finish(const float* partial, const float* wsum, int dtype, void* out, int B, int D, int h, int w, void* stream);

/*
 * 2-D convolution over channels-last 16-bit feature maps with a fused per-channel affine (folded BatchNorm) and ReLU:
 * the 2-D feature extractor in front of the path.  Replaces ConvBnReLU / Conv2d of
 * models/MVSNet/module.py:23-38, models/MVSNet/model.py:21-41.  Supported layers: k3 s1 p1 and k5 s2 p2,
 * c_in 8 / 16 / 32 / 64 (a 3-channel image is zero-padded to 8 by the caller), c_out 8 / 16 / 32 / 64.
 *   pscv_pack_conv2d_weights: w fp32 [c_out, c_in, k, k] (PyTorch layout) -> MFMA A-fragment order for a layer whose
 *       input has c_in_padded channels; returns the number of 16-bit elements (packed may be NULL to query).
 *   pscv_conv2d: in [B,Hi,Wi,c_in] (c_in = the padded count), out [B,Ho,Wo,c_out] in `out_dtype` (the storage dtype or
 *       fp32); scale / bias fp32 [c_out] or NULL; v = conv * scale + bias, y = max(v, neg_slope * v): neg_slope 0 = ReLU,
 *       0.1 = LeakyReLU(0.1) (models/CVP_MVSNet/models/modules.py:24-28), 1 = no activation.
 */
long pscv_pack_conv2d_weights(const float* w, int c_in, int c_in_padded, int c_out, int ks, int dtype, uint16_t* packed);
/* The same packing with `w` (fp32 [c_out][c_in][ks][ks]) and `packed` on the device, one launch on `stream`, no host round trip
 * (ABI 6): what a training step uses to rebuild the extractor's forward and adjoint layers after an optimiser step. */
int pscv_pack_conv2d_weights_device(const float* w, int c_in, int c_in_padded, int c_out, int ks, int dtype, uint16_t* packed, void* stream);
/* adjoint = 1: `w` is the FORWARD layer's weight [c_in][c_out][ks][ks] (this layer's input channels are its output channels) and the
 * packed layer is its adjoint -- channel axes swapped, taps flipped: the data gradient of a stride-1 conv runs on the forward kernel. */
int pscv_pack_conv2d_weights_device_ex(const float* w, int c_in, int c_in_padded, int c_out, int ks, int dtype, int adjoint, uint16_t* packed,
                                       void* stream);
int pscv_conv2d(const void* in, int dtype, const uint16_t* packed, const float* scale, const float* bias, void* out,
                int out_dtype, int B, int Hi, int Wi, int c_in, int c_out, int ks, int stride, float neg_slope, void* stream);
/*
 * The general form, used by Vis-MVSNet's FeatExt (models/VisMVSNet/model_cas.py:18-35: a 2-D residual U-Net over
 * nn_utils.py:123-278).  On top of pscv_conv2d:
 *   layers   k3 s1|s2 p1, k5 s2 p2, k1 s1|s2 p0 (the BasicBlock shortcuts), and ks = 2: one of the four 2x2-tap parity
 *            sub-convolutions of ConvTranspose2d(k3, s2, p1, op1) -- parity = 2 * (output row parity) + (output column parity),
 *            weights [c_out, c_in, 2, 2] with tap (ty, tx) applied to input (i + ty, j + tx); output pixel (2 i + row parity,
 *            2 j + column parity) of a [B, 2 Hi, 2 Wi, *] map.  A k3 s1 layer may carry a parity too (the sub-convolutions of
 *            ConvTranspose2d(k5, s2, p2, op1) = the data gradient of a k5 s2 conv: taps at -1, 0, +1 around input (i, j)).
 *            parity = -1 for every other layer.
 *   skip     NULL or [B,Ho,Wo,skip_cstride] read at channel offset skip_coff, added BEFORE the activation
 *            (BasicBlock: relu(bn(conv(x)) + shortcut))
 *   out      [B,Ho,Wo,out_cstride] written at channel offset out_coff (the decoder's cat([deconv, skip]) needs no copy)
 *   c_in up to 128; c_out up to 64, or 128 (output tiles split over blockIdx.y).
 */
int pscv_conv2d_ex(const void* in, int dtype, const uint16_t* packed, const float* scale, const float* bias, const void* skip,
                   int skip_cstride, int skip_coff, void* out, int out_cstride, int out_coff, int out_dtype, int B, int Hi, int Wi,
                   int c_in, int c_out, int ks, int stride, int parity, float neg_slope, void* stream);

/*
 * Geometric-consistency filter of one depth map against its source views (the step after the
 * path).  Replaces the body of evaluation/filtering.py:60-83 (unproject -> project_all -> grid_sample of the source
 * depth -> unproj_all -> project -> reprojection / relative-depth / triangulation-angle tests -> per-pixel vote).
 *   depth      device fp32 [h,w]            reference depth map
 *   src_depth  host array of n_src device pointers, fp32 [src_hw[2i], src_hw[2i+1]] (maps may differ in size)
 *   src_hw     host int array [n_src][2] = (height, width) of each source map
 *   cams       device fp32 [n_src+1][PSCV_GEO_CAM_FLOATS]: K, K^-1, R (row-major 3x3 each), t (3); view 0 = reference;
 *              intrinsics at the resolution of the respective depth map
 *   max_reproj_error (pixels), depth_threshold (relative), min_tri_angle (degrees), num_consistent: the reference's
 *              command-line parameters (pipeline_utils.py:49-52); a pixel passes a test when at least
 *              num_consistent - 1 sources agree
 *   mask_depth, mask_disp, geo_mask   device uint8 [h,w] (0/1), each may be NULL
 *   counts     device int32 [3][h,w] number of agreeing sources per test (depth, disp, geo), or NULL
 */
#define PSCV_GEO_MAX_SRC 32
#define PSCV_GEO_CAM_FLOATS 30
int pscv_geo_filter(const float* depth, const float* const* src_depth, const int* src_hw, int n_src, const float* cams,
                    int h, int w, float max_reproj_error, float depth_threshold, float min_tri_angle, int num_consistent,
                    unsigned char* mask_depth, unsigned char* mask_disp, unsigned char* geo_mask, int* counts, void* stream);

/*
 * Consistency fusion of filtered depth maps into one point cloud (ABI 10; the step after the geometric filter).  Replaces the
 * external fusibile binary that evaluation/fusibile.py:160-181 runs (its normal test off: normal_thresh = 360 with constant normals).
 * One call = one pass i over the pixels of view i; the caller runs passes 0 .. n_views-1 in order on one stream.  Rule (INTEGRATION.md
 * section 2d): a pixel p of view i with a valid depth (finite, depth_min < d < depth_max) and used_i(p) = 0 is unprojected to X; every
 * other view j, in ascending order, projects X to z > 0 and the pixel q = floor(a/z + 0.5, b/z + 0.5) inside view j with a valid depth
 * d_j(q), and is consistent when |f_i B/z - f_i B/d_j(q)| < disp_thresh (f_i = K_i[0,0], B = |c_i - c_j|, c = -R^T t).  With
 * n >= num_consistent consistent views the pass emits the mean of X and their unprojected pixels, the rounded mean colour, and sets
 * used_j(q) = 1 for each of them.
 *   depth       host array of n_views device pointers, fp32 [hw[2v], hw[2v+1]] (sizes may differ); masked pixels hold 0
 *   color       host array of n_views device pointers, RGBA8 packed in 32 bits [h_v, w_v] (red in the low byte; alpha ignored)
 *   used        host array of n_views device pointers, uint8 [h_v, w_v], 0 / 1; pass i reads used_i and writes used_j, j != i
 *   cams        device fp32 [n_views][PSCV_GEO_CAM_FLOATS] (pscv_geo_filter's blocks: K, K^-1, R, t; intrinsics at each map's size)
 *   out_xyz     device fp32 [capacity][3], out_rgb uint8 [capacity][3]; out_view, out_pixel int32 [capacity] (each may be NULL):
 *               the view and the pixel index y w + x the point was emitted from
 *   counter     device int64: running number of points (0 before pass 0).  Points go to out[counter ...] in row-major pixel order;
 *               the counter advances by the pass's full count even past capacity, and nothing at or beyond capacity is written,
 *               so counter > capacity after the last pass means the buffer was too small (the caller's error)
 *   workspace   device scratch of pscv_fuse_depth_workspace(h_i, w_i) bytes (at least that of the largest view for a whole run)
 * No host synchronisation: three launches on `stream` (fuse, scan, scatter); the result is bit-reproducible.
 */
#define PSCV_FUSE_MAX_VIEWS 64
long pscv_fuse_depth_workspace(int h, int w);
int pscv_fuse_depth_pass(int pass, const float* const* depth, const unsigned int* const* color, unsigned char* const* used,
                         const int* hw, int n_views, const float* cams, float disp_thresh, int num_consistent, float depth_min,
                         float depth_max, float* out_xyz, unsigned char* out_rgb, int* out_view, int* out_pixel, long capacity,
                         long long* counter, void* workspace, long workspace_bytes, void* stream);

/*
 * PatchMatch multi-view stereo (ABI 13; the COLMAP baseline of the reconstruction pipeline, where the reference runs the external
 * `colmap patch_match_stereo` from utils/colmap_utils.py:282-322).  The rule is INTEGRATION.md section 2h: per reference pixel p a
 * plane hypothesis (d > 0, unit normal n in the reference frame facing the camera) stored as fp32 state [h][w][4] = (d, nx, ny,
 * nz); per source s the bilateral-weighted NCC over the (2 radius / step + 1)^2 window through the plane's homography, c_s =
 * clamp(1 - NCC, 0, 2), 2 when the centre projects behind or outside s, a weighted variance is < 1e-5 or the triangulation angle
 * is < 1 deg; in geometric mode c_s + 0.3 min(e_s, 3) with e_s the forward-backward error against s's depth map; the aggregated
 * cost is the mean of the top_k smallest.
 *   ref         device fp32 grey [h][w] of the reference view
 *   src         host array of n_src device pointers, fp32 grey [h_s][w_s]; src_hw host int [n_src][2] = (h_s, w_s)
 *   cams        device fp32 [n_src+1][PSCV_GEO_CAM_FLOATS] (K, K^-1, R, t), row 0 = the reference view
 *   src_depth   host array of n_src device pointers, fp32 [h_s][w_s] photometric depth maps; NULL = photometric mode
 *   1 <= n_src <= PSCV_PM_MAX_SRC, 1 <= radius <= PSCV_PM_MAX_RADIUS, 1 <= step <= radius, 1 <= top_k <= min(n_src,
 *   PSCV_PM_MAX_TOPK), 0 < depth_min < depth_max
 * pscv_patch_match_init       state <- candidate 10 at every pixel (iteration word 0xffffffff, colour 0)
 * pscv_patch_match_cost       per-source photometric costs out_cost [n_src][h][w], errors out_err [n_src][h][w] (geometric mode;
 *                             may be NULL) and the aggregated cost out_agg [h][w] (may be NULL) of the hypotheses in state
 * pscv_patch_match_half_step  one red-black half-step in place on the pixels with (row + col) % 2 == colour: candidates 0-10
 *                             (current; planes of the pixels at (0,+-1), (+-1,0), (0,+-3), (+-3,0); perturbation by delta of the
 *                             inverse-depth range and theta radians; random), the lowest cost wins, ties to the lowest index;
 *                             random draws hash (seed, view, pixel, iteration, colour, slot).  out_choice int [h][w] and out_cand
 *                             fp32 [h][w][11][4] (0 = skipped) receive the chosen index and the candidates when not NULL.
 * pscv_patch_match_filter     COLMAP's filter: a pixel is kept when >= 2 sources have c_s <= 0.9, an angle >= 3 deg and e_s <= 1 px
 *                             (src_depth required); out_depth [h][w], out_normal [h][w][3] (0 elsewhere), out_count [h][w] (may
 *                             be NULL) the passing sources.
 * No host synchronisation: one launch each on `stream`.  seed, view, iteration are used as 32-bit unsigned words.
 */
#define PSCV_PM_MAX_SRC 31
#define PSCV_PM_MAX_RADIUS 8
#define PSCV_PM_MAX_TOPK 8
int pscv_patch_match_init(float* state, int h, int w, const float* cams, float depth_min, float depth_max, int seed, int view,
                          void* stream);
int pscv_patch_match_cost(const float* state, const float* ref, int h, int w, const float* const* src, const int* src_hw, int n_src,
                          const float* cams, const float* const* src_depth, int radius, int step, int top_k, float* out_cost,
                          float* out_err, float* out_agg, void* stream);
int pscv_patch_match_half_step(float* state, const float* ref, int h, int w, const float* const* src, const int* src_hw, int n_src,
                               const float* cams, const float* const* src_depth, float depth_min, float depth_max, int radius,
                               int step, int top_k, int seed, int view, int iteration, int colour, float delta, float theta,
                               int* out_choice, float* out_cand, void* stream);
int pscv_patch_match_filter(const float* state, const float* ref, int h, int w, const float* const* src, const int* src_hw,
                            int n_src, const float* cams, const float* const* src_depth, int radius, int step, float* out_depth,
                            float* out_normal, int* out_count, void* stream);

/*
 * COLMAP-style stereo fusion of depth maps into one point cloud (ABI 12; the YFCC path, where the reference runs the external
 * `colmap stereo_fusion` from utils/colmap_utils.py:391-400 with max_normal_error 180, i.e. the normal test off).  One call = the
 * pass of view `view`; the caller runs the views in FindNextImage order on one stream.  Rule: every
 * seed of the view (0 < d finite, fused = 0; X_s = R^T (d K^-1 (col, row, 1) - t), no +0.5) grows the breadth-first closure of
 * the pixels of the other unprocessed views that pass |(z - d) / d| <= max_depth_error and (x/z - col)^2 + (y/z - row)^2 <=
 * max_reproj_error^2 against (x, y, z) = K (R X_s + t), reached through round(P_m X_node) (half away from zero) along `overlap`
 * from nodes at depth <= max_traversal_depth - 2.  Phase A claims every reached pixel with atomicMin((tag, seed)) on `claim`;
 * phase B recomputes each closure over its own claims, marks the seed and that cluster fused, and a cluster of at least
 * min_num_pixels pixels emits the per-coordinate medians of its points, normals R_k^T (1,1,1)/sqrt(3) (normalised; dropped
 * below FLT_EPSILON) and colours.  Geometry is fp64 from the fp32 inputs.
 *   depth, color, hw, cams   as pscv_fuse_depth_pass (color RGBA8, red in the low byte)
 *   fused       host array of n_views device pointers, uint8 [h_v, w_v], 0 / 1, updated in place
 *   claim       host array of n_views device pointers, uint64 [h_v, w_v]: all bits set before the first pass that uses them
 *   tag         >= 0, strictly increasing over the calls that share `claim` (a pass's claims then beat every earlier one)
 *   overlap     host int64 bit masks [n_views]: bit m of overlap[k] when view m follows view k (the diagonal is ignored)
 *   processed   bit mask: bit v set when view v's pass is done (its pixels are never entered; `view` itself must be clear)
 *   max_reproj_error in (0, 2] pixels, max_depth_error in (0, 1) relative, max_traversal_depth >= 1
 *   out_xyz, out_normal fp32 [capacity][3], out_rgb uint8 [capacity][3], out_view, out_pixel int32 [capacity] (normal, view and
 *               pixel may be NULL): the point, the view and the seed pixel y w + x it was emitted from
 *   counter     device int64 running point count, as pscv_fuse_depth_pass (counter > capacity after the last pass = overflow)
 *   workspace   device scratch of pscv_colmap_fuse_workspace(h, w) bytes for the pass's view
 * No host synchronisation: five launches on `stream` (phase A, phase B, count, scan, scatter); the result is bit-reproducible.
 *
 * pscv_colmap_fuse_pass_normals (ABI 14; the COLMAP baseline, where the reference runs `colmap stereo_fusion
 * --StereoFusion.max_normal_error 10` over PatchMatch's own normal maps, utils/colmap_utils.py:377-381, 396): the same pass with
 * the normal test on ("with normal maps").
 *   normal      host array of n_views device pointers, fp32 [h_v, w_v, 3]: unit normals in the camera frame of their view, 0
 *               where the depth is filtered (what pscv_patch_match_filter writes); every pointer non-null
 *   max_normal_error   degrees, in (0, 180]; min_cos = cos(max_normal_error pi / 180) in fp64
 * The world normal of a pixel is w = R^T n, fp64 sums rounded to fp32.  A pixel joins a seed only if it also passes
 * w_seed . w_pixel >= min_cos (fp64, against the seed, neither side normalised, NaN fails); a pixel that fails only this test is
 * neither claimed nor marked.  The emitted normal is the normalised per-component median of w over the cluster, seed included.
 * pscv_colmap_fuse_pass itself is unchanged (constant normals, no normal test).
 */
long pscv_colmap_fuse_workspace(int h, int w);
int pscv_colmap_fuse_pass(int view, int tag, const float* const* depth, const unsigned int* const* color,
                          unsigned char* const* fused, unsigned long long* const* claim, const int* hw, int n_views, const float* cams,
                          const long* overlap, long processed, float max_depth_error,
                          float max_reproj_error, int min_num_pixels, int max_traversal_depth, float* out_xyz, float* out_normal,
                          unsigned char* out_rgb, int* out_view, int* out_pixel, long capacity, long long* counter, void* workspace,
                          long workspace_bytes, void* stream);
int pscv_colmap_fuse_pass_normals(int view, int tag, const float* const* depth, const unsigned int* const* color,
                                  unsigned char* const* fused, unsigned long long* const* claim, const int* hw, int n_views,
                                  const float* cams, const long* overlap, long processed, float max_depth_error,
                                  float max_reproj_error, int min_num_pixels, int max_traversal_depth, const float* const* normal,
                                  float max_normal_error, float* out_xyz, float* out_normal, unsigned char* out_rgb, int* out_view,
                                  int* out_pixel, long capacity, long long* counter, void* workspace, long workspace_bytes,
                                  void* stream);

/*
 * View covisibility from the depth maps (an addition to ABI 14: new exports only, no existing signature changes): the overlap graph of the COLMAP-style fusion without a sparse model
 * ("Overlap without a sparse model").  For every ordered pair (v, u != v) of n_views views
 *   counts[v][u][0] = the samples of v that u sees, counts[v][u][1] = those that are also consistent with u's depth map.
 * A sample is a pixel (col, row) of v with row % stride == 0, col % stride == 0 and a valid depth (0 < d finite).  With
 * X = R_v^T (d K_v^-1 (col, row, 1) - t_v) and q = K_u (R_u X + t_u), all fp64 and exactly as phase A of pscv_colmap_fuse_pass
 * computes them, u sees the sample when q_z > 0 and the pixel (round(q_x / q_z), round(q_y / q_z)) (half away from zero, pixel =
 * the integer pair, no half-pixel offset) lies inside u's map; it is consistent when u's depth d_u there is valid and
 * |(q_z - d_u) / d_u| <= max_depth_error.
 *   depth, hw   as pscv_colmap_fuse_pass (host arrays: n_views device pointers to fp32 [h_v, w_v], 0 = invalid; (h_v, w_v) pairs)
 *   n_views     >= 2, not bounded by PSCV_FUSE_MAX_VIEWS;  cams device fp32 [n_views][PSCV_GEO_CAM_FLOATS]
 *   stride      >= 1;  max_depth_error in (0, 1) relative
 *   counts      device int32 [n_views][n_views][2], zero-filled by the call; the diagonal stays 0
 *   workspace   device scratch of pscv_view_covisibility_workspace(n_views) bytes (the view table)
 * No host synchronisation; integer atomics only, so the result does not depend on the order of the adds.
 */
long pscv_view_covisibility_workspace(int n_views);
int pscv_view_covisibility(const float* const* depth, const int* hw, int n_views, const float* cams, int stride,
                           float max_depth_error, int* counts, void* workspace, long workspace_bytes, void* stream);

/*
 * Normal maps from depth maps (an addition to ABI 14: new exports only, no existing signature changes): the normals of a network
 * reconstruction, for the normal test of pscv_colmap_fuse_pass_normals and for meshing (INTEGRATION.md section 2n,
 * csrc/depth_normals.hip).  Per valid pixel (0 < d finite) a linear least-squares fit of the inverse depth over the
 * (2 radius + 1)^2 window, taps gated by |d_q - d_p| <= rel_gate d_p, all fp64 from the fp32 inputs in a fixed order; a pixel with
 * fewer than min_support taps, collinear taps or a fit that does not face the camera gets the ray towards the camera instead.
 *   depth, hw   host arrays: n_views device pointers to fp32 [h_v, w_v] (0 = invalid) and the (h_v, w_v) pairs
 *   cams        device fp32 [n_views][PSCV_GEO_CAM_FLOATS]; K at each map's size
 *   1 <= n_views <= PSCV_FUSE_MAX_VIEWS, 1 <= radius <= 4, rel_gate > 0 finite, 3 <= min_support <= (2 radius + 1)^2
 *   normal      host array of n_views device pointers, fp32 [h_v, w_v, 3]: unit normals in the camera frame (n^T K^-1 p < 0),
 *               0 at invalid pixels -- the layout pscv_colmap_fuse_pass_normals reads
 *   support     host array of n_views device pointers, int32 [h_v, w_v], or NULL: the tap count, negated where the pixel fell
 *               back to the ray, 0 at invalid pixels
 * One launch for all views on `stream`, no workspace, no host synchronisation, bit-reproducible.
 *
 * pscv_point_world_normals: out[k] = R_v^T n_v[pixel[k]], v = view[k] (fp64 sums rounded to fp32, the world normal of the fusion's
 * normal test) for n_points fused points; view, pixel device int32 [n_points] (pixel = y w_v + x), out device fp32 [n_points][3].
 * An index outside its range reads nothing and gives (0, 0, 0).  normal, hw, n_views, cams as above.
 */
int pscv_depth_normals(const float* const* depth, const int* hw, int n_views, const float* cams, int radius, double rel_gate,
                       int min_support, float* const* normal, int* const* support, void* stream);
int pscv_point_world_normals(const int* view, const int* pixel, long n_points, const float* const* normal, const int* hw,
                             int n_views, const float* cams, float* out, void* stream);

/*
 * TSDF fusion and marching tetrahedra (an addition to ABI 14: new exports only, no existing signature changes): depth maps into a
 * dense truncated-signed-distance volume and the volume into an indexed triangle mesh (INTEGRATION.md section 2o,
 * csrc/tsdf_fusion.hip).  Grid: lattice point (i, j, k) at (o0 + i voxel, o1 + j voxel, o2 + k voxel), linear index
 * (k ny + j) nx + i, nx ny nz < 2^31.  State, device arrays [nz][ny][nx], zero at the start: tsdf_sum fp32, weight int32, rgb_sum
 * fp32 [..][3], cweight int32.  All arithmetic is fp64 in a fixed order: every result is bit-reproducible.  Asynchronous on `stream`.
 *
 * pscv_tsdf_integrate: adds 1 <= n_views <= PSCV_FUSE_MAX_VIEWS views to the state, in view order.  Per voxel X and view:
 * (x, y, z) = K (R X + t), z > 0; pixel (floor(x / z + 0.5), floor(y / z + 0.5)) inside the view; its depth d valid (0 < d finite);
 * sd = d - z >= -trunc: tsdf_sum += min(1, sd / trunc), weight += 1, and where sd <= trunc also rgb_sum += the pixel's bytes,
 * cweight += 1.  tsdf_sum is rounded to fp32 once per call.
 *   depth, color, hw   host arrays: n_views device pointers to fp32 [h_v, w_v] and rgba8 [h_v, w_v] (red in the low byte), and the
 *                      (h_v, w_v) pairs;  cams device fp32 [n_views][PSCV_GEO_CAM_FLOATS]
 *   dmax               device fp32 [n_views]: the largest valid depth of each view (0 for a view without one); the kernel skips
 *                      (tile, view) pairs it proves untouched, which changes no result while dmax is not too small
 *   origin, voxel > 0, trunc > 0 finite
 *
 * pscv_tsdf_mark: f(p) = tsdf_sum / weight, p observed iff weight >= min_weight (>= 1), negative iff f(p) < 0.  Edge (p, d), d =
 * 1..7 (bit 0 = x, 1 = y, 2 = z), joins p and p + bits(d); it carries a vertex iff both ends are observed and exactly one is
 * negative.  info device int32 [nz][ny][nx]: bits 0-6 the edge mask of p (bit d-1), bit 8 observed, bit 9 negative, bits 16-23 the
 * number of vertices, bits 24-31 the number of faces of the cell at p (six tetrahedra (0, a, a|b, 7) over the axis orders).
 *
 * pscv_tsdf_emit_vertices / pscv_tsdf_emit_faces: vincl, fincl device int32 [nx ny nz] are the INCLUSIVE prefix sums of the two
 * counts of info in linear order; n_vertices, n_faces their totals.  Vertices are numbered by (linear index, d): position
 * X(p) + t (X(q) - X(p)) with t = f(p) / (f(p) - f(q)) rounded to fp32 -> xyz [n_vertices][3]; colour interpolated the same way
 * between the ends' mean colours (an end with cweight 0 leaves the other's; neither: 0) -> rgb uint8 [n_vertices][3].  Faces:
 * int32 [n_faces][3], by cell, tetrahedron 0..5, oriented towards the positive side, smallest vertex index first, a quad as
 * (q0,q1,q2), (q0,q2,q3).  A total of 0 launches nothing.
 *
 * pscv_tsdf_case_table: the 6 x 16 orientation table of the face kernel, host memory unsigned [96]: entry [T][negative corner
 * positions] = vertex count in bits 0-2, vertex k's edge in bits 3 + 6 k .. 8 + 6 k as corner | edge type << 3.
 */
int pscv_tsdf_integrate(const float* const* depth, const unsigned int* const* color, const int* hw, int n_views, const float* cams,
                        const float* dmax, double o0, double o1, double o2, double voxel, double trunc, int nx, int ny, int nz,
                        float* tsdf_sum, int* weight, float* rgb_sum, int* cweight, void* stream);
int pscv_tsdf_mark(const float* tsdf_sum, const int* weight, int nx, int ny, int nz, int min_weight, int* info, void* stream);
int pscv_tsdf_emit_vertices(const float* tsdf_sum, const int* weight, const float* rgb_sum, const int* cweight, const int* info,
                            const int* vincl, int nx, int ny, int nz, double o0, double o1, double o2, double voxel, float* xyz,
                            unsigned char* rgb, long n_vertices, void* stream);
int pscv_tsdf_emit_faces(const int* info, const int* vincl, const int* fincl, int nx, int ny, int nz, int* faces, long n_faces,
                         void* stream);
int pscv_tsdf_case_table(unsigned int* table);

/*
 * Brick-sparse TSDF volume (an addition to ABI 14: new exports only, no existing signature changes): the rule above in a second
 * storage layout, a pool of 8 x 8 x 8 bricks behind a dense directory (csrc/tsdf_bricks.hip).  The mesh
 * is the dense mesh: the same vertices, colours and triangles as sets, bit for bit.
 * Lattice (nx, ny, nz), origin and voxel as above, but nx ny nz may exceed 2^31: lin = (k ny + j) nx + i is int64.  Bricks:
 * nb* = ceil(n* / 8), nbx nby nbz < 2^31, brick index (bz nby + by) nbx + bx.  directory device int32 [nbz][nby][nbx]: the brick's
 * pool slot or -1; brick_ids device int32 [n_bricks]: the brick of every slot, ascending; 0 <= n_bricks < 2^22.  Pool, device
 * arrays, zero at the start: tsdf_sum fp32, weight int32, cweight int32 [n_bricks][8][8][8], rgb_sum fp32 [n_bricks][8][8][8][3]
 * (x fastest); pool voxels outside the lattice stay zero.  A call with n_bricks 0 launches nothing.
 *
 * pscv_tsdf_brick_probe: a lattice point is touched when one of the 1 <= n_views <= PSCV_FUSE_MAX_VIEWS views updates it with
 * -trunc <= sd <= trunc.  masks device int32 [nbz][nby][nbx], zero before the first call, OR-ed by every call: a touched point at
 * local (x, y, z) of its brick sets bit (dz+1) 9 + (dy+1) 3 + (dx+1) for dx in {0}, plus -1 if x == 0, plus +1 if x == 7, and
 * likewise dy, dz.  Brick b is to be allocated iff some brick b - (dx, dy, dz) has that bit set (the caller's step).  dmax as above;
 * dmin device fp32 [n_views]: the smallest valid depth of each view, +inf for a view without one.
 *
 * pscv_tsdf_brick_integrate: pscv_tsdf_integrate on every lattice point of every brick of brick_ids.  The allocation must have been
 * decided from all views before the first call.
 *
 * pscv_tsdf_brick_mark / _emit_vertices / _emit_faces: pscv_tsdf_mark / _emit_vertices / _emit_faces with "in the grid" read as "in
 * the lattice and in an allocated brick".  info, vincl, fincl: device int32 [n_bricks][512] in pool order.  Vertices are numbered by
 * (slot, local voxel, d), faces by (slot, local cell, tetrahedron); a face starts at its vertex of the smallest key
 * lin(p) 7 + (d - 1) -- in the dense layout that is the smallest index, so every quad is cut alike.  keys: device int64
 * [n_vertices], the vertices' keys, or null.
 */
int pscv_tsdf_brick_probe(const float* const* depth, const int* hw, int n_views, const float* cams, const float* dmax,
                          const float* dmin, double o0, double o1, double o2, double voxel, double trunc, int nx, int ny, int nz,
                          int* masks, void* stream);
int pscv_tsdf_brick_integrate(const float* const* depth, const unsigned int* const* color, const int* hw, int n_views,
                              const float* cams, const float* dmax, double o0, double o1, double o2, double voxel, double trunc,
                              int nx, int ny, int nz, const int* brick_ids, int n_bricks, float* tsdf_sum, int* weight,
                              float* rgb_sum, int* cweight, void* stream);
int pscv_tsdf_brick_mark(const float* tsdf_sum, const int* weight, const int* directory, const int* brick_ids, int n_bricks, int nx,
                         int ny, int nz, int min_weight, int* info, void* stream);
int pscv_tsdf_brick_emit_vertices(const float* tsdf_sum, const int* weight, const float* rgb_sum, const int* cweight, const int* info,
                                  const int* vincl, const int* directory, const int* brick_ids, int n_bricks, int nx, int ny, int nz,
                                  double o0, double o1, double o2, double voxel, float* xyz, unsigned char* rgb, long* keys,
                                  long n_vertices, void* stream);
int pscv_tsdf_brick_emit_faces(const int* info, const int* vincl, const int* fincl, const int* directory, const int* brick_ids,
                               int n_bricks, int nx, int ny, int nz, int* faces, long n_faces, void* stream);

/*
 * Mesh clean-up (an addition to ABI 14: new exports only, no existing signature changes): connected components of an indexed
 * triangle mesh, removal of small components / degenerate faces / unused vertices with order-preserving compaction, and
 * area-weighted vertex normals (csrc/mesh_clean.hip).  faces device int32 [n_faces][3], vertex arrays
 * device [n_vertices][..]; n_vertices < 2^31, 3 n_faces < 2^31; either may be 0 (nothing is launched on an empty grid).  A face
 * with an index outside [0, n_vertices) is never followed: it joins nothing, is counted nowhere and survives nothing.  All calls
 * are asynchronous on `stream`, need no workspace and are bit-reproducible (integer atomics; one lane per output elsewhere).
 *
 * pscv_mesh_components: two vertices are connected when some face contains both; label[v] = the smallest vertex index of v's
 * component (a vertex in no face is its own).  Lock-free union-find on `label` (init, hook with compare-and-swap of the larger
 * root under the smaller, flatten): label[x] <= x throughout, so every walk descends, no lane waits for another, and the result
 * does not depend on the schedule.  status device int32 [2], ZEROED BY THE CALLER: [0] += the faces with an index out of range,
 * [1] += the lanes that left a loop at its trip limit (n_vertices + 1: never, unless the kernel is defective).  A face with a
 * repeated index is legal.
 *
 * pscv_mesh_component_sizes: fcount, vcount device int32 [n_vertices], ZEROED BY THE CALLER: fcount[r] += the faces whose first
 * vertex has label r, vcount[r] += the vertices with label r (so both stay 0 except at roots).
 *
 * pscv_mesh_mark: face f survives iff keep_comp[label[faces[f][0]]] != 0 (device uint8 [n_vertices], indexed by label) and, with
 * drop_degenerate = 1, it is not degenerate: no repeated index, and the fp64 cross product n = (b - a) x (c - a) of its fp32
 * corners (differences, products and sums each rounded once, n = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0)) is not exactly
 * (0, 0, 0).  fmark device int32 [n_faces] = 0 / 1; vmark device int32 [n_vertices], ZEROED BY THE CALLER, = 1 where a surviving
 * face uses the vertex.
 *
 * pscv_mesh_compact: fincl, vincl are the INCLUSIVE int32 prefix sums of fmark, vmark and n_faces_out, n_vertices_out their totals.
 * Surviving vertex v goes to row vincl[v] - 1 of xyz_out fp32 [..][3], rgb_out uint8 [..][3] and, when `normals` is given,
 * normals_out fp32 [..][3]; surviving face f to row fincl[f] - 1 of faces_out with its indices renumbered the same way: both keep
 * their relative order.  A row outside the totals is not written.
 *
 * pscv_mesh_vertex_normals: corner 3 f + k is vertex faces[f][k]; corner_off device int32 [n_vertices + 1] and corners device int32
 * [3 n_faces] are the vertex -> corner adjacency in CSR form, every vertex's corners in ASCENDING corner id.  Per vertex the fp64
 * sum s of the cross products n (above) of its corners' faces, component by component in that order from 0 (a face that names
 * the vertex twice counts twice), len = sqrt(s0 s0 + s1 s1 + s2 s2), normals[v] = s / len rounded to fp32, (0, 0, 0) when len is 0
 * or not finite.  |n| is twice the face's area, so the sum is area-weighted; faces oriented to free space give such normals.
 */
int pscv_mesh_components(const int* faces, long n_faces, long n_vertices, int* label, int* status, void* stream);
int pscv_mesh_component_sizes(const int* label, const int* faces, long n_faces, long n_vertices, int* fcount, int* vcount,
                              void* stream);
int pscv_mesh_mark(const float* xyz, const int* faces, const int* label, const unsigned char* keep_comp, long n_faces,
                   long n_vertices, int drop_degenerate, int* fmark, int* vmark, void* stream);
int pscv_mesh_compact(const float* xyz, const unsigned char* rgb, const float* normals, const int* faces, const int* fmark,
                      const int* vmark, const int* fincl, const int* vincl, long n_faces, long n_vertices, float* xyz_out,
                      unsigned char* rgb_out, float* normals_out, int* faces_out, long n_faces_out, long n_vertices_out, void* stream);
int pscv_mesh_vertex_normals(const float* xyz, const int* faces, const int* corner_off, const int* corners, long n_faces,
                             long n_vertices, float* normals, void* stream);

/*
 * Mesh metrics (an addition to ABI 14: new exports only, no existing signature changes): surface samples proportional to area and
 * the exact bounded distance from points to the surface of an indexed triangle mesh, the step that lets evaluation/metrics.py
 * score a mesh against a ground-truth cloud (csrc/mesh_metrics.hip).  xyz device fp32 [n_vertices][3],
 * faces device int32 [n_faces][3]; n_vertices < 2^31, 3 n_faces < 2^31; either may be 0.  A face with an index outside
 * [0, n_vertices) is never followed: it gives no sample and no distance.  Every value is fp64 from the fp32 coordinates, every
 * product and sum rounded once in the order section 2r writes down.  All calls are asynchronous on `stream`; every result is
 * bit-reproducible (the only atomics are the integer ones of the grid build, and no result depends on their order).
 *
 * Hash: mix(k) is the splitmix64 finaliser, step(x) = mix(x + 0x9e3779b97f4a7c15) on 64-bit words, unit(h) = (h >> 11) * 2^-53.
 * h_f = step(step(seed) ^ f);  h_fk = step(h_f ^ (k + 1)).
 *
 * pscv_mesh_sample_count: n_f = floor(A_f / spacing^2 + unit(h_f)) with A_f = 0.5 * sqrt(n . n), n = (b - a) x (c - a); 0 for a
 *   face that is not valid or whose area is 0 or not finite; saturated at 2^31 - 1.  offsets device int32 [n_faces] = the
 *   exclusive scan of n_f (saturated at 2^31 - 1; exact whenever the total fits), *total device int64 = the sum.
 *   workspace: pscv_mesh_scan_workspace(n_faces) bytes.  `seed` carries 64 bits.
 * pscv_mesh_sample_emit: sample i (face-major, k ascending inside a face; its face found by binary search in `offsets`) is
 *   a + u (b - a) + v (c - a) rounded to fp32, u = unit(h_fk), v = unit(step(h_fk)), both replaced by 1 - u, 1 - v when
 *   u + v > 1.  out device fp32 [n_samples][3]; face_out device int32 [n_samples] or NULL.  n_samples = *total <= 2^31 - 2.
 *
 * Grid of a mesh: every valid face is binned into every cell (edge `cell`, from the origin, 21 bits per axis; the caller keeps
 * the vertices within 2^21 cells of the origin) that its bounding box touches.
 * pscv_mesh_grid_count: pair_off device int32 [n_faces] = the exclusive scan of the cells per face, *total device int64 = the
 *   number of (cell, face) pairs.  workspace: pscv_mesh_scan_workspace(n_faces) bytes.
 * pscv_mesh_grid_build: groups the n_pairs = *total <= 2^31 - 1 pairs by cell as pscv_point_grid_build groups points (hash table
 *   of >= 2 n_pairs slots, counts, scan, scatter) into `grid`, a device buffer of pscv_mesh_grid_workspace(n_pairs) bytes whose
 *   first 4 bytes hold the number of occupied cells (uint32).  Same origin and cell as the count.
 *
 * pscv_mesh_point_dist: out[i] = sqrt(d2) and face_out[i] (may be NULL) = f for the lexicographically smallest (d2, f) over the
 *   valid faces with d2 < maxdist^2 (strict), d2 the squared distance from query i to face f; +inf and -1 when there is none.
 *   Per face: with n = (b - a) x (c - a) and n . n > 0, when the three edge functions ((b - a) x (q - a)) . n,
 *   ((c - b) x (q - b)) . n, ((a - c) x (q - c)) . n are all >= 0, d2 = ((q - a) . n)^2 / (n . n); otherwise the minimum over
 *   the edges ab, bc, ca of |w - t d|^2, d = p1 - p0, w = q - p0, t = clamp((w . d) / (d . d), 0, 1), t = 0 when d . d = 0.
 *   The search visits rings 0..fine_rings of the fine grid, then rings 0..coarse_rings of the coarse grid of the same mesh (same
 *   origin; coarse_rings * coarse_cell >= maxdist + coarse_cell); a cell is skipped and the rings stop only when the bound lies
 *   strictly beyond the best d2, so no result depends on the cell sizes.  query device fp32 [m][3], finite.
 */
long pscv_mesh_scan_workspace(long n_faces);
int pscv_mesh_sample_count(const float* xyz, const int* faces, long n_faces, long n_vertices, double spacing, long seed,
                           int* offsets, long long* total, void* workspace, long workspace_bytes, void* stream);
int pscv_mesh_sample_emit(const float* xyz, const int* faces, const int* offsets, long n_faces, long n_vertices, long seed,
                          long n_samples, float* out, int* face_out, void* stream);
int pscv_mesh_grid_count(const float* xyz, const int* faces, long n_faces, long n_vertices, double ox, double oy, double oz,
                         double cell, int* pair_off, long long* total, void* workspace, long workspace_bytes, void* stream);
long pscv_mesh_grid_workspace(long n_pairs);
int pscv_mesh_grid_build(const float* xyz, const int* faces, const int* pair_off, long n_faces, long n_vertices, double ox,
                         double oy, double oz, double cell, long n_pairs, void* grid, long grid_bytes, void* stream);
int pscv_mesh_point_dist(const float* query, long m, const float* xyz, const int* faces, long n_faces, long n_vertices,
                         const void* fine, long fine_pairs, const void* coarse, long coarse_pairs, double ox, double oy, double oz,
                         double fine_cell, double coarse_cell, int fine_rings, int coarse_rings, double maxdist, double* out,
                         int* face_out, void* stream);

/*
 * Scene set-up from a COLMAP sparse model (an addition to ABI 14: new exports only, no existing signature changes): what
 * utils/colmap_utils.py:compute_src_imgs and compute_min_max_depth_yao compute for every YFCC scene (INTEGRATION.md section 2i,
 * csrc/scene_setup.hip).  All arrays are device memory; all calls are asynchronous on `stream`, need no workspace and are
 * bit-reproducible (integer atomics; one lane per output elsewhere).
 *
 * pscv_sparse_pair_counts: for every point p and every ordered pair (i, j) of its track
 *   adj[i][j] += 1 (the diagonal included), and for i != j
 *   adj_tri[i][j] += 1 when the angle between xyz_p and xyz_p + c[i][j], c[i][j] = R_i (R_j^T t_j) - t_i, acos of the clipped
 *   cosine in degrees, all fp64 from the fp32 R and t, is > min_triangulation_angle (the reference's rel_opt_center; NaN fails).
 *   xyz         fp64 [n_points][3]
 *   track_off   int64 [n_points + 1], track_img int32 [nnz]: the tracks in CSR form, IMAGE INDICES in [0, n_images), sorted and
 *               without duplicates per point (an index out of range, offsets outside [0, nnz], or a track of more than
 *               n_images entries are skipped, never followed)
 *   R, t        fp32 [n_images][3][3], [n_images][3];  1 <= n_images <= 46340;  min_triangulation_angle >= 0, degrees
 *   adj, adj_tri  int32 [n_images][n_images], zero-filled by the call
 *
 * pscv_sparse_obs_depths: one 64-bit sort key per observation k of point obs_pt[k] by image obs_img[k]:
 *   keys[k] = obs_img[k] << 32 | ordered(fp32((R_i x + t_i).z + 1e-6)), the depth of utils_3D.project in fp64 rounded to fp32;
 *   ordered() maps fp32 to 32 bits that compare like the values.  An index out of range gives the key 2^63 - 1, behind every
 *   image's keys whether they are sorted as signed or as unsigned integers (image indices are below 2^31).  Sorted
 *   ascending (the caller's job), the keys of image i are the run [seg_off[i], seg_off[i+1]) of its depths in ascending order.
 *
 * pscv_segment_percentiles: out_lo[s], out_hi[s] = the q_lo and q_hi quantiles (fractions in [0,1]) of the depths in the sorted
 *   keys' run [seg_off[s], seg_off[s+1]), numpy.percentile's linear interpolation in fp64; an empty run gives 0, 0.
 *   seg_off     int64 [n_segments + 1];  out_lo, out_hi  fp64 [n_segments]
 */
int pscv_sparse_pair_counts(const double* xyz, const long* track_off, const int* track_img, long n_points, long nnz,
                            const float* R, const float* t, int n_images, double min_triangulation_angle, int* adj, int* adj_tri,
                            void* stream);
int pscv_sparse_obs_depths(const double* xyz, long n_points, const int* obs_img, const int* obs_pt, long n_obs, const float* R,
                           const float* t, int n_images, unsigned long long* keys, void* stream);
int pscv_segment_percentiles(const unsigned long long* keys, long n_keys, const long* seg_off, int n_segments, double q_lo,
                             double q_hi, double* out_lo, double* out_hi, void* stream);

/*
 * Visible depth ranges of image tuples (an addition to ABI 14: new exports only): utils/colmap_utils.py:
 * compute_min_max_depth_visible for T tuples of V images in one call, the depth range of a MegaDepth training tuple
 * (csrc/scene_setup.hip).  For tuple k with views v = 0..V-1 (image indices tuples[k][v]):
 *   a point takes part when at least 3 of the tuple's images are in its track; n_pts[k] counts those points;
 *   it is projected into every view, all in fp64 without fused multiply-adds from the fp32 K, R, t and the fp64 xyz:
 *     y = R x + t,  u = K y,  depth = u_z + 1e-6,  proj = u_xy / depth;
 *   it is valid in view v iff proj_x >= 0 && proj_y >= 0 && proj_x < w && proj_y < h && depth > 0 (a NaN fails);
 *   min_d[k][v], max_d[k][v] are the smallest and largest valid depth, min_row[k][v], max_row[k][v] the LOWEST row of xyz that
 *   attains each (numpy's nanargmin / nanargmax over the participating points); a view without a valid point gives NaN depths
 *   and rows of -1.
 *   xyz, track_off, track_img   as pscv_sparse_pair_counts (no image twice in a track)
 *   tuples      int32 [T][V] image indices in [0, n_images), distinct within a tuple.  The call copies them to the host and checks
 *               this before it launches: ONE synchronisation of `stream`, the only one of this header's scene set-up calls
 *   K           fp32 [T][V][3][3] the views' intrinsics (per tuple: the miner rescales them);  R, t fp32 [n_images][3][3], [n_images][3]
 *   sizes       fp64 [T][V][2] = (w, h)
 *   3 <= V <= 32;  1 <= T <= 65535;  1 <= n_images <= 46340
 *   min_d, max_d fp64 [T][V];  min_row, max_row int64 [T][V];  n_pts int32 [T]
 *   workspace   device scratch of pscv_tuple_visible_depths_workspace(T, V) bytes, initialised by the call
 * Integer minima and maxima (of the ordered bits of the depths, then of the rows): exact fp64 depths, and no result depends on the
 * order of the atomics.
 */
long pscv_tuple_visible_depths_workspace(int n_tuples, int n_views);
int pscv_tuple_visible_depths(const double* xyz, const long* track_off, const int* track_img, long n_points, long nnz,
                              const int* tuples, const float* K, const float* R, const float* t, const double* sizes, int n_images,
                              int T, int V, double* min_d, double* max_d, long* min_row, long* max_row, int* n_pts, void* workspace,
                              void* stream);

/*
 * Point-cloud metrics (ABI 11; the step after fusion).  Replaces the scipy cKDTree calls of evaluation/metrics.py: reduce_pts,
 * chamfer, chamfer_imw.  The rules are INTEGRATION.md section 2f.  Points are fp32 [n][3]; distances are fp64 from those
 * coordinates.  All calls are asynchronous on `stream`; every result is bit-reproducible.
 *
 * Sparse uniform grid of n points (n < 2^30): cell (floor((x - ox) / cell), ...) with 21 bits per axis (the caller keeps the
 * points within 2^21 cells of the origin; points outside are clamped into the edge cells), an open-addressing hash table of
 * >= 2n slots (integer atomicCAS), per-slot counts, a scan and a scatter into slot order.  No sort, nothing dense.
 *   grid       device buffer of pscv_point_grid_workspace(n) bytes; its first 4 bytes hold the number of occupied cells (uint32)
 *   payload    optional device int32 [n] carried into slot order (the ranks of pscv_radius_mis_round), may be NULL
 * A grid is used with the same n, origin and cell it was built with.
 */
long pscv_point_grid_workspace(long n);
int pscv_point_grid_build(const float* pts, long n, double ox, double oy, double oz, double cell, const int* payload, void* grid,
                          long grid_bytes, void* stream);

/*
 * Bounded nearest-neighbour distance of m query points to the n_target points of two grids of the same set (same origin): out[i]
 * = |q_i - p| of the nearest target p with |q_i - p|^2 < maxdist^2 (strict), +inf when there is none.  The search visits rings
 * 0..fine_rings of the fine grid, then rings 0..coarse_rings of the coarse grid (coarse_rings * coarse_cell >= maxdist +
 * coarse_cell), pruned by the best distance so far.
 * bb != NULL selects the DTU blocking of metrics.py::chamfer: host double[6] = bb0 xyz, bb1 xyz; cells [bb0 + x maxdist,
 * bb0 + x maxdist + maxdist) for x in 0..floor((bb1 - bb0) / maxdist) per axis; a query in no cell, or in a cell whose
 * occupancy (pscv_dtu_cell_occupancy) is 0, gets maxdist; otherwise only targets in the cell's expanded box count.
 */
int pscv_point_nn_dist(const float* query, long m, const void* fine, const void* coarse, long n_target, double ox, double oy,
                       double oz, double fine_cell, double coarse_cell, int fine_rings, int coarse_rings, double maxdist,
                       const double* bb, const int* occ, double* out, void* stream);
/* occ: device int32 [(na_x+1)(na_y+1)(na_z+1)], zeroed by the caller; set to 1 where a target lies in the cell's expanded box
   [low - maxdist, high + maxdist) (bb: host double[6] as above) */
int pscv_dtu_cell_occupancy(const float* pts, long n, const double* bb, double maxdist, int* occ, void* stream);

/*
 * One round of the radius maximal independent set (metrics.py::reduce_pts as the greedy MIS in rank order) over the points of
 * a grid built with payload = rank (unique ints; lower goes first) and cell > dst.  state_in / state_out: uint8 [n] in slot
 * order, 0 undecided / 1 kept / 2 removed (all 0 before round 0).  An undecided point with a kept neighbour (|p - q| <= dst in
 * fp64) becomes removed; with no kept and no lower-ranked undecided neighbour it becomes kept.  *undecided (device int64,
 * zeroed by the caller) gains the number of points still undecided after the round.
 */
int pscv_radius_mis_round(const void* grid, long n, double ox, double oy, double oz, double cell, double dst,
                          const unsigned char* state_in, unsigned char* state_out, long long* undecided, void* stream);
/* Final state -> mask uint8 [n] in the points' original order (1 = kept) and kept int32 [n]: the kept indices in increasing
   order, *n_kept (device int64) of them.  workspace: pscv_radius_mis_workspace(n) bytes. */
long pscv_radius_mis_workspace(long n);
int pscv_radius_mis_compact(const void* grid, long n, const unsigned char* state, unsigned char* mask, int* kept,
                            long long* n_kept, void* workspace, long workspace_bytes, void* stream);

/*
 * Softmax over the depth axis + expectation(s), fused.
 * Replaces: F.softmax + depth_regression + photometric confidence (models/MVSNet/model.py:207-215, module.py:174-178;
 *           CVP net.py:161-162,203-219) and soft_argmin / entropy (models/VisMVSNet/nn_utils.py:453-470).
 *
 *   logits        [B,D,h,w] fp32, bf16 or fp16 (logit_dtype)
 *   depth         same addressing as pscv_warp_cost (per-batch or per-pixel planes); may be NULL (then out_depth must be NULL)
 *   out_depth     [B,h,w] fp32  sum_d p_d depth_d                         (NULL to skip)
 *   out_index     [B,h,w] fp32  sum_d p_d d                               (NULL to skip)
 *   out_conf      [B,h,w] fp32  window probability (NULL to skip):
 *                   conf_mode 0: p[i-1]+p[i]+p[i+1]+p[i+2], i = trunc(E[index])   (MVSNet / CVP)
 *                   conf_mode 1: sum of p_d with |d - E[index]| <= window         (Vis soft_argmin(window=))
 *   out_entropy   [B,h,w] fp32  -sum p log(clamp(p,1e-9,1))               (NULL to skip)
 *   out_prob      [B,D,h,w] fp32 full probability volume                  (NULL to skip)
 *   out_partials  [B,4,h,w] fp32 (max, sum exp, sum exp*depth, sum exp*index) of THIS depth shard, for the
 *                 cross-GPU log-sum-exp merge (NULL to skip); index counts from index_offset.
 */
int pscv_softargmin(const void* logits, int logit_dtype, const float* depth, long depth_bstride, int depth_per_pixel,
                    float* out_depth, float* out_index, float* out_conf, float* out_entropy, float* out_prob,
                    float* out_partials, int conf_mode, float window, int index_offset, int B, int D, int h, int w,
                    void* stream);
/*
 * Depth-plane shard across GPUs, last step of the window probability (Vis soft_argmin(window=), nn_utils.py:464-465): this
 * shard's part of sum_{|d - E[index]| <= window} p_d under the GLOBALLY merged softmax.  logits fp32 [B,D,h,w] = the shard's
 * planes (global index = d + index_offset), stats fp32 [B,3,h,w] = (global max, global sum of exp, global expected index) from
 * the merged out_partials; out fp32 [B,h,w]; the shards' outputs are summed by one all-reduce.
 */
int pscv_softargmin_window(const float* logits, const float* stats, float* out, float window, int index_offset, int B, int D,
                           int h, int w, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Training path: what loss.backward() needs from the hot path when train.py drives the model
 * (train.py:185-191, models/trainer.py:96-206).  The reference gets all of it from ATen autograd; here each piece
 * is one entry point.  Forward in train() mode = pscv_warp_cost, pscv_conv3d without folded statistics
 * (scale = bias = NULL, no ReLU), pscv_bn_stats, pscv_bn_act, pscv_softargmin.
 * ------------------------------------------------------------------------------------------------------------------ */

/* number of floats of the `workspace` argument of pscv_bn_stats / pscv_bn_bwd_reduce */
long pscv_train_workspace_floats(void);

/*
 * Per-channel batch statistics of a channels-last 16-bit volume: sums[0][c] = sum y, sums[1][c] = sum y^2 over all
 * nvox voxels (BatchNorm3d in train(): models/MVSNet/module.py:41-58 normalise with the statistics of the batch).
 * Two-phase, fixed summation order (bit-reproducible).  sums: device fp32 [2][C].  C in {8,16,32,64,128} (128: ABI 6, the Vis-MVSNet extractor's widest layers).
 */
int pscv_bn_stats(const void* y, int dtype, long nvox, int C, float* workspace, float* sums, void* stream);

/*
 * The per-channel bookkeeping between pscv_bn_stats and pscv_bn_act, one launch (nn.BatchNorm3d.train() semantics): from sums
 * [2][C]: mean = s0 / nvox, var = max(s1 / nvox - mean^2, 0), invstd = 1 / sqrt(var + eps); out fp32 [4][C] = (scale = gamma invstd,
 * bias = beta - mean scale, mean, invstd).  gamma / beta may be NULL (1 / 0).  When running_mean / running_var are given they are
 * updated in place with `momentum` and the unbiased variance, and *num_batches_tracked (int64, may be NULL) is incremented.
 */
int pscv_bn_finalize(const float* sums, long nvox, int C, const float* gamma, const float* beta, float eps, float momentum,
                     float* running_mean, float* running_var, long long* num_batches_tracked, float* out, void* stream);
/*
 * The bookkeeping between pscv_bn_bwd_reduce and pscv_bn_bwd_apply: from sums [2][C] = (sum dz, sum dz y): out fp32 [5][C] =
 * (ca, cb, cc, d gamma, d beta) with dy = ca dz + cb y + cc the BatchNorm input gradient.
 */
int pscv_bn_bwd_coeffs(const float* sums, const float* mean, const float* invstd, const float* gamma, long nvox, int C, float* out,
                       void* stream);

/* out = [relu](y * scale + bias) + skip   (scale / bias fp32 [C] = the batch-statistics affine; skip may be NULL;
 * `skip + relu(bn(deconv(x)))` of models/MVSNet/model.py:79-81).  relu: 0 none, 1 before the skip add, 2 AFTER it
 * (`relu(bn(conv(x)) + shortcut)` of the Vis BasicBlock, models/VisMVSNet/nn_utils.py:123-171). */
int pscv_bn_act(const void* y, int dtype, long nvox, int C, const float* scale, const float* bias, int relu,
                const void* skip, void* out, void* stream);

/* BatchNorm(+ReLU) backward, pass 1: with z = y * scale + bias and dz = dact * [z > 0] (dz = dact when relu = 0),
 * sums[0][c] = sum dz, sums[1][c] = sum dz * y. */
int pscv_bn_bwd_reduce(const void* dact, const void* y, int dtype, long nvox, int C, const float* scale,
                       const float* bias, int relu, float* workspace, float* sums, void* stream);

/* BatchNorm(+ReLU) backward, pass 2: dy = ca[c] * dz + cb[c] * y + cc[c] (the caller folds gamma, 1/std, the batch
 * mean and the two sums of pass 1 into the three per-channel coefficients). */
int pscv_bn_bwd_apply(const void* dact, const void* y, int dtype, long nvox, int C, const float* scale,
                      const float* bias, int relu, const float* ca, const float* cb, const float* cc, void* dy,
                      void* stream);

/*
 * Grouped forms of the six BatchNorm entry points above (ABI 6): the tensor is `groups` consecutive slices of `nvox` voxels, and
 * every slice has its OWN batch statistics and constants -- the views of a 2-D extractor batch, which the reference normalises
 * one view at a time (models/MVSNet/model.py:101-107: `self.feature(img)` per view in train()), in one launch per pass.
 *   pscv_bn_stats_grouped / pscv_bn_bwd_reduce_grouped   sums fp32 [groups][2][C]
 *   pscv_bn_finalize_grouped    out fp32 [groups][4][C] = (scale, bias, mean, invstd) per group; the running statistics are updated
 *                               once per group IN ORDER (the module saw `groups` forward calls), num_batches_tracked += groups
 *   pscv_bn_bwd_coeffs_grouped  out fp32 [groups][5][C]; mean / invstd of group g at mean + g * stat_stride floats
 *   pscv_bn_act_grouped / _bwd_reduce_grouped / _bwd_apply_grouped   constants of group g at scale + g * param_stride floats
 *                               (ca / cb / cc: + g * coeff_stride); with finalize's layout param_stride = 4 C, coeff_stride = 5 C
 * groups = 1 (strides unused) is exactly the plain form; d gamma / d beta of a shared BatchNorm are the sums over the groups.
 */
int pscv_bn_stats_grouped(const void* y, int dtype, long nvox, int groups, int C, float* workspace, float* sums, void* stream);
int pscv_bn_finalize_grouped(const float* sums, long nvox, int groups, int C, const float* gamma, const float* beta, float eps,
                             float momentum, float* running_mean, float* running_var, long long* num_batches_tracked, float* out,
                             void* stream);
int pscv_bn_act_grouped(const void* y, int dtype, long nvox, int groups, int C, const float* scale, const float* bias,
                        int param_stride, int relu, const void* skip, void* out, void* stream);
int pscv_bn_bwd_reduce_grouped(const void* dact, const void* y, int dtype, long nvox, int groups, int C, const float* scale,
                               const float* bias, int param_stride, int relu, float* workspace, float* sums, void* stream);
int pscv_bn_bwd_coeffs_grouped(const float* sums, const float* mean, const float* invstd, int stat_stride, const float* gamma,
                               long nvox, int groups, int C, float* out, void* stream);
int pscv_bn_bwd_apply_grouped(const void* dact, const void* y, int dtype, long nvox, int groups, int C, const float* scale,
                              const float* bias, int param_stride, int relu, const float* ca, const float* cb, const float* cc,
                              int coeff_stride, void* dy, void* stream);

/*
 * Backward of softmax over D + the regression heads (models/MVSNet/model.py:207-209, module.py:174-178;
 * models/VisMVSNet/nn_utils.py:453-470), p = softmax(logits); every upstream gradient is optional (NULL):
 *   grad_depth    of depth   = sum_d p_d depth_d                       (needs the depth planes, as in pscv_softargmin)
 *   grad_index    of index   = sum_d p_d d
 *   grad_entropy  of entropy = -sum_d p_d log clamp(p_d, 1e-9, 1)
 * logits fp32 [B,D,h,w], gradients fp32 [B,h,w]  ->  dlogits8 [B,D,h,w,8] in `dtype` with the gradient in channel 0
 * and zeros in channels 1-7 (the layout the 8-channel MFMA kernels read: the 1-channel heads' backward runs on them).
 */
int pscv_softargmin_bwd(const float* logits, const float* depth, long depth_bstride, int depth_per_pixel,
                        const float* grad_depth, const float* grad_index, const float* grad_entropy, void* dlogits8,
                        int dtype, int B, int D, int h, int w, void* stream);

/* dpre = dout * [out > 0]: backward of a ReLU applied AFTER a residual add (Vis BasicBlock, nn_utils.py:123-171; the
 * forward is pscv_bn_act with relu = 2).  16-bit channels-last volumes, C a multiple of 8. */
int pscv_relu_bwd(const void* dout, const void* out, int dtype, long nvox, int C, void* dpre, void* stream);
/* The same with a negative-side slope (ABI 6): dpre = dout * (out > 0 ? 1 : slope) -- the backward of LeakyReLU(slope), whose output
 * has the sign of its input (CVP-MVSNet's 2-D pyramid: conv + LeakyReLU(0.1), models/CVP_MVSNet/models/modules.py:24-28); slope = 0 is
 * pscv_relu_bwd. */
int pscv_leaky_relu_bwd(const void* dout, const void* out, int dtype, long nvox, int C, float slope, void* dpre, void* stream);
/* The same pass that also returns sums[0][c] = sum over the voxels of the STORED dpre (fp32 [2][C], row 1 = 0): the bias gradient of a
 * conv + bias + LeakyReLU layer without a second read of dpre.  workspace: pscv_train_workspace_floats() floats.  C in {8,...,128}. */
int pscv_leaky_relu_bwd_sum(const void* dout, const void* out, int dtype, long nvox, int C, float slope, void* dpre, float* workspace,
                            float* sums, void* stream);

/*
 * Backward of pscv_fuse_pairs (normalise = 1): d interm_v = G w_v / W, d uncert_v = -w_v / W sum_{d,c} G (interm_v - fused)
 * (models/VisMVSNet/model_cas.py:354-357,385-386 under autograd).  grad_fused [B,D,h,w,8] and dinterm[v] in `dtype`,
 * duncert[v] fp32 [B,h,w]; host arrays of n_src device pointers.
 */
int pscv_fuse_pairs_bwd(const void* const* interm, const float* const* uncert, int n_src, int dtype, const void* grad_fused,
                        void* const* dinterm, float* const* duncert, int B, int D, int h, int w, void* stream);

/*
 * Weight gradient of a 3x3x3 convolution, an MFMA contraction over voxels:
 *     dw[a][b][t] = sum_{n,o} P[n,o,a] * Q[n, stride*o + t - 1, b]        (t = (tz,ty,tx), zero outside Q)
 *   Conv3d weight [C_out,C_in,27]:           P = grad of the layer output (a = c_out), Q = layer input  (b = c_in)
 *   ConvTranspose3d weight [C_in,C_out,27]:  P = layer input (a = c_in),  Q = grad of the layer output (b = c_out)
 * P [B,Dp,Hp,Wp,p_cstride] read at channel offset p_coff; Q [B,stride*Dp,stride*Hp,stride*Wp,q_cstride] at q_coff;
 * both in `dtype` (bf16 / fp16).  ca, cb multiples of 8 in [8,64].  workspace: device fp32,
 * pscv_conv3d_wgrad_workspace(...) floats.  dw: device fp32 [ca][cb][27]; accumulate != 0 adds to it.
 * Fixed summation order (bit-reproducible).
 */
long pscv_conv3d_wgrad_workspace(int B, int Dp, int Hp, int Wp, int ca, int cb, int stride);
int pscv_conv3d_wgrad(const void* p, int p_cstride, int p_coff, int ca, const void* q, int q_cstride, int q_coff, int cb,
                      int dtype, int B, int Dp, int Hp, int Wp, int stride, float* workspace, float* dw, int accumulate,
                      void* stream);

/*
 * Backward of pscv_warp_cost with respect to the feature maps (the sampling grid carries no gradient in the
 * reference: models/MVSNet/module.py:127).  Arguments as pscv_warp_cost; grad_out has the layout of that call's
 * `out` in grad_dtype (the features' 16-bit format or fp32).  dref fp32 [B,h,w,C] (may be NULL for WARP_ONLY),
 * dsrcs host array of n_src device fp32 [B,hs,ws,C], dtemp device fp32 [1] (SOFTMIN, may be NULL): all are
 * ACCUMULATED into with float atomics, the caller zero-fills them.  C in {16, 32}.
 */
int pscv_warp_cost_bwd(const void* ref, const void* const* srcs, int n_src, const float* cams, const float* depth,
                       long depth_bstride, int depth_per_pixel, int geom, int cost, float temp, const void* grad_out,
                       float* dref, float* const* dsrcs, float* dtemp, int B, int C, int h, int w, int hs, int ws, int D,
                       int in_dtype, int grad_dtype, void* stream);

/*
 * CVP-MVSNet refinement hypotheses in eval mode without a host round trip.  Replaces calDepthHypo,
 * models/CVP_MVSNet/models/modules.py:131-226 (a per-batch Python loop in fp64 with a median): per pixel the depth step
 * that moves its projection into the FIRST source view by one pixel along the epipolar line (fp64), the lower median of
 * |step| over the valid pixels (exact radix select), and the planes depth + k * median, k = -4..3.
 *   depth    device fp32 [B,H,W]    the upsampled depth of the previous level
 *   cams     device fp64 [B][39]:   K_ref^-1 (9), rows 0..2 of E_src E_ref^-1 (12), K_src (9),
 *                                   A = (K_ref R_ref)(K_src R_src)^-1 (9); row-major, first source view
 *   fallback device fp32 [B]        (depth_max - depth_min) / 128, the step used when no pixel is valid
 *   keys     device uint64 workspace [B*H*W + B*1040];  steps  device fp64 out [B];  hypos  device fp32 out [B,8,H,W]
 */
int pscv_cvp_depth_hypos(const float* depth, const double* cams, const float* fallback, unsigned long long* keys,
                         double* steps, float* hypos, int B, int H, int W, void* stream);

/*
 * Fused tail of the MVSNet regulariser as ONE depth sweep (ABI 8): transposed 3x3x3 convolution 16 -> 8 (stride 2, output_padding 1)
 * + folded BatchNorm + ReLU + skip add, then the 1-channel 3x3x3 head on the result, which never leaves the CU -- the 8-channel
 * full-resolution volume of the unfused path is neither written nor read.  Same operation chains as pscv_conv3d(kind T2P8)
 * followed by pscv_conv3d(kind S1C1): the logits are bit-identical to the two launches.
 * Replaces: conv11 (Sequential(ConvTranspose3d(16, 8), BatchNorm3d, ReLU)), `conv0 + conv11(x)` and `prob` of CostRegNet.forward,
 *           models/MVSNet/model.py:67-72,81-82.
 *   in        device 16-bit [B,Di,Hi,Wi,in_cstride], channels [in_coff, in_coff + 16)
 *   packed_up device copy of pscv_pack_conv3d_weights(kind PSCV_CONV_T2P8); up_scale / up_bias / up_floor device fp32 [8] or null
 *   skip      null or device 16-bit [B,2Di,2Hi,2Wi,skip_cstride] read at skip_coff (added after the first ReLU)
 *   packed_head device copy of pscv_pack_conv3d_weights(kind PSCV_CONV_S1C1, c_in 8); hd_scale / hd_bias / hd_floor device fp32 [1] or null
 *   logits    device fp32 out [B,2Di,2Hi,2Wi]
 *   depth     null, or device fp32 planes (row b at depth + b * depth_bstride, 2Di entries): the sweep then also keeps the softmax
 *             statistics of its logits per depth chunk and a merge launch writes out_depth [B,2Hi,2Wi] = sum softmax(logits) x depth
 *             and, if out_conf is not null, the 4-plane photometric confidence (models/MVSNet/model.py:207-215) -- the separate
 *             pscv_softargmin pass disappears; workspace: device fp32, pscv_tail_sweep_workspace(B, Di, Hi, Wi) floats
 * Returns 0, or 1 when the shape is not covered (call the two layers), negative on error.
 */
long pscv_tail_sweep_workspace(int B, int Di, int Hi, int Wi);
int pscv_tail_sweep(const void* in, int dtype, int in_cstride, int in_coff, const uint16_t* packed_up, const float* up_scale,
                    const float* up_bias, const float* up_floor, int up_epi, const void* skip, int skip_cstride, int skip_coff,
                    const uint16_t* packed_head, const float* hd_scale, const float* hd_bias, const float* hd_floor, int hd_epi,
                    float* logits, const float* depth, long depth_bstride, float* workspace, long workspace_floats,
                    float* out_depth, float* out_conf, int B, int Di, int Hi, int Wi, void* stream);

/*
 * Fused tail of the MVSNet regulariser: the 1-channel `prob` head (kind S1C1 packing, 8 input channels, depth-sweep variant) writes
 * the fp32 logits AND per-depth-chunk softmax partials; a merge launch gives depth and photometric confidence.  Replaces
 * CostRegNet.prob + F.softmax + depth_regression + the 4-plane confidence (models/MVSNet/model.py:72,82,207-215) -- the separate
 * pscv_softargmin pass over the 15.7 MB logit volume disappears.  Returns -3 (with pscv_last_error) when the layer / size does not
 * qualify (then call pscv_conv3d and pscv_softargmin).
 *   in      device 16-bit [B,D,H,W,in_cstride] (channel slice [in_coff, in_coff + c_in)), packed = S1C1 weights, scale/bias/floor [1]
 *   depth   device fp32 planes, row b at depth + b * depth_bstride, D entries;  logits device fp32 out [B,D,H,W]
 *   workspace device fp32, pscv_prob_softargmin_workspace(B,D,H,W) floats;  out_depth / out_conf device fp32 [B,H,W] (conf may be null)
 */
long pscv_prob_softargmin_workspace(int B, int D, int H, int W);
int pscv_prob_softargmin(const void* in, int dtype, int in_cstride, int in_coff, const uint16_t* packed, const float* scale,
                         const float* bias, const float* floor, int c_in, int epi_flags, const float* depth, long depth_bstride,
                         float* logits, float* workspace, long workspace_floats, float* out_depth, float* out_conf, int B, int D,
                         int H, int W, void* stream);

/*
 * Fused head of a Vis-MVSNet PAIR branch: RegPair.final_conv (8 -> 1, kind S1C1 packing, depth-sweep variant) + soft_argmin's expected
 * plane index + the entropy of the softmax over depth, in one pass over the pair volume.  Replaces RegPair.forward + soft_argmin +
 * entropy (models/VisMVSNet/model_cas.py:55-59,342-348; nn_utils.py:453-470): the pair branch only needs these two maps, so the fp32
 * score volume need not exist (`logits` may be null: 24 -> 16 B of traffic per voxel and one launch instead of two).
 *   entropy = log Z - sum_d e_d (l_d - max) / Z  with e_d = exp(l_d - max), Z = sum e_d: the reference's -sum p log(clamp(p, 1e-9, 1))
 *   without the clamp (planes with p < 1e-9 differ by < 3e-6 in total).
 * Returns -3 when the layer / size does not qualify (then call pscv_conv3d and pscv_softargmin).  Arguments as pscv_prob_softargmin;
 *   workspace pscv_prob_softargmin_workspace(B,D,H,W) floats (used when the depth axis is split into chunks);
 *   out_index / out_entropy device fp32 [B,H,W].
 */
int pscv_head_index_entropy(const void* in, int dtype, int in_cstride, int in_coff, const uint16_t* packed, const float* scale,
                            const float* bias, const float* floor, int c_in, int epi_flags, float* logits, float* workspace,
                            long workspace_floats, float* out_index, float* out_entropy, int B, int D, int H, int W, void* stream);

/*
 * Function-level homography warp: one 3x3 matrix per batch item or per reference pixel.  Replaces homography_warping +
 * interpolate of models/VisMVSNet/homography.py:84-120 for direct callers (inside the model the homographies are built in the
 * fused sweep and never materialised).  Pixel centres at +0.5, z <= 0 -> zero sample, divisor clamped at 1e-9,
 * normalise -> clamp(+-1.1) -> align_corners=True bilinear, zero padding.
 *   image device fp32 [m,hs,ws,c] (channels last);  H device fp32 [m,9] (per_pixel = 0) or [m,h,w,9] (per_pixel = 1), row-major
 *   out   device fp32 [m,h,w,c]
 */
int pscv_homography_warp(const float* image, const float* H, int per_pixel, float* out, int m, int c, int h, int w, int hs, int ws,
                         void* stream);

/*
 * Adjoint of pscv_homography_warp with respect to the image (ABI 9).  The reference evaluates the sample positions under no_grad
 * (models/VisMVSNet/homography.py:110-118) and differentiates only grid_sample's `input` (:101-102): grad_image accumulates
 * grad_out x the four bilinear weights at the taps the forward read.
 *   grad_out   device fp32 [m,h,w,c];  H as in the forward
 *   grad_image device fp32 [m,hs,ws,c], ZEROED by the caller (the kernel adds with fp32 atomics)
 */
int pscv_homography_warp_bwd(const float* grad_out, const float* H, int per_pixel, float* grad_image, int m, int c, int h, int w, int hs,
                             int ws, void* stream);

/*
 * Every camera block of a CVP-MVSNet forward pass in one launch.  Replaces conditionIntrinsics, the per-level projection
 * stacks of homo_warping / proj_cost and the camera products of calDepthHypo (models/CVP_MVSNet/models/modules.py:31-50,
 * 89-98, 229-293, 131-226), which are hundreds of 3x3 tensor ops per forward.
 *   ref_in   device fp32 [B,3,3], src_in [B,N,3,3]      intrinsics at image resolution
 *   ref_ex   device fp32 [B,4,4], src_ex [B,N,4,4]      extrinsics (last row 0 0 0 1)
 *   level_scale HOST fp32 [L]                           image_height / level_height of each pyramid level (L <= 8)
 *   warp_cams device fp32 out [L][N][B][PSCV_CAM_FLOATS]  the pscv_proj_cams block of each level (input of pscv_warp_cost)
 *   hypo_cams device fp64 out [L][B][39] or null          the `cams` of pscv_cvp_depth_hypos of each level (first source view)
 */
int pscv_cvp_cams(const float* ref_in, const float* src_in, const float* ref_ex, const float* src_ex, const float* level_scale,
                  int B, int N, int L, float* warp_cams, double* hypo_cams, void* stream);

/* ---- unsupervised photometric loss (replaces models/trainer.py:209-278 + utils/ssimLoss.py:27-60) ---------
 *
 * pscv_photo_warp: depth map -> flows -> warped source images, the body of Trainer.get_flow_from_depthmap /
 * photometricloss / masked_photometricloss (trainer.py:209-236, 258-266; utils_3D.py:185-208, 243-272):
 *   P3 = inv_ref (x d, y d, d, 1);  q = proj_src P3;  f = q_xy / max(q_z, 1e-6);  g = 2 f / (size - 1) - 1;
 *   g = -10 where q_z <= 0; clamp to +-10; sample = grid_sample(bilinear, zeros, align_corners=False) (index g -> ((g+1) size - 1)/2,
 *   the reference's (size-1)-normalised flows under align_corners=False, reproduced).
 * src_imgs fp32 [B,S,C,h,w] (may be null with C = 0), depth [B,h,w], inv_ref [B,16] = inverse of the reference view's 4x4
 * projection, proj_src [B,S,16]; optional src_depth [B,S,h,w].  Outputs, each optional: warped [B,S,C,h,w], mask [B,S,h,w]
 * (1.0 where |g| < 1 in both axes), z_src [B,S,h,w] (depth in the source view), flows [B,S,h,w,2], warped_depth [B,S,h,w].
 * pscv_photo_warp_bwd: grad_warped [B,S,C,h,w] -> grad_depth [B,h,w] through the sampling position (no gradient where the
 * z <= 0 assignment or the clamp cuts the reference's graph); no atomics, deterministic.
 */
int pscv_photo_warp(const float* src_imgs, const float* depth, const float* inv_ref, const float* proj_src, const float* src_depth,
                    float* warped, float* mask, float* z_src, float* flows, float* warped_depth, int B, int S, int C, int h, int w,
                    void* stream);
int pscv_photo_warp_bwd(const float* src_imgs, const float* depth, const float* inv_ref, const float* proj_src,
                        const float* grad_warped, float* grad_depth, int B, int S, int C, int h, int w, void* stream);
/*
 * SSIM loss map of utils/ssimLoss.py:27-60: out = 1 - SSIM(img1, img2) per channel, 11x11 Gaussian window (sigma 1.5), zero
 * padding.  img1 fp32 [n1,C,h,w], img2 [n1*rep,C,h,w] (item n of img2 is compared with item n / rep of img1: the reference
 * image against its rep warped sources), out [n1*rep,C,h,w].  pscv_ssim_bwd: grad_out -> grad_img2 (img1 is data);
 * workspace 3 * n1*rep*C*h*w floats.
 */
int pscv_ssim(const float* img1, const float* img2, float* out, int n1, int rep, int C, int h, int w, void* stream);
int pscv_ssim_bwd(const float* img1, const float* img2, const float* grad_out, float* workspace, float* grad_img2, int n1, int rep,
                  int C, int h, int w, void* stream);

/*
 * Image preparation (an addition to ABI 14: new exports only, no existing signature changes): what the reference does with PIL
 * before an image reaches a network -- preprocess.py:157-164 and data/MVSDataset.py:read_img, `Image.resize(size, resample=
 * Image.LANCZOS)` on 8-bit images, and the nearest-neighbour resize of the ground-truth depth of data/md_yao.py:99-102,123
 * (csrc/image_resample.hip).  Asynchronous on `stream`, no workspace, integer arithmetic: the bytes are
 * PIL's.
 *
 * pscv_resample_u8_pass: ONE separable pass of PIL's resampling over an interleaved 8-bit image.  A resize is the horizontal pass
 * into an 8-bit intermediate, then the vertical pass; a pass whose length does not change is left out, as PIL does.
 *   axis 0 (horizontal): src = `lines` rows of in_len pixels;  dst [lines][out_count][C];  dst_f32 [C][lines][out_count]
 *   axis 1 (vertical):   src = in_len rows of `lines` pixels;  dst [out_count][lines][C];  dst_f32 [C][out_count][lines]
 *   src_pitch   bytes between two source rows (>= the row's pixels * C: a column window of a wider image is a pointer and a pitch)
 *   C           1 or 3 interleaved channels
 *   coeff       device int32: the weights of every output sample in 22-bit fixed point, zero past the sample's n;
 *               axis 0: TRANSPOSED, [ksize][out_len];  axis 1: [out_len][ksize]
 *   bounds      device int32 [out_len][2] = (first, n): the sample reads source indices first .. first + n - 1, n <= ksize
 *   out_first, out_count   the output samples to produce, [out_first, out_first + out_count) of out_len: a crop computes its window
 *   per sample and channel: acc = 2^21 + sum_k coeff[k] * src[first + k] (int32), out = clamp(acc >> 22, 0, 255)
 *   dst_f32     optional planar fp32 copy of the output, value lut[v];  lut device fp32 [256], the caller's float(v) / 255.0f
 *   coeff == NULL with axis 1 and out_len == in_len: the identity pass, output row o = source row out_first + o (the crop and the
 *               fp32 copy of an image that is not resampled)
 *
 * pscv_depth_nearest_crop: depth fp32 [th][tw] resized to oh x ow by F.interpolate(mode="nearest")'s rule on CPU torch -- per axis
 * src = min((int)floorf(dst * scale), in - 1) with scale = (float)in / (float)out -- of which the window of ch rows from y0 and cw
 * columns from x0 is written: out_depth fp32 [ch][cw], out_mask uint8 [ch][cw] = (d >= min_d) && (d < max_d).
 */
int pscv_resample_u8_pass(const unsigned char* src, long src_pitch, int lines, int in_len, int C, int axis, const int* coeff,
                          const int* bounds, int ksize, int out_len, int out_first, int out_count, unsigned char* dst, float* dst_f32,
                          const float* lut, void* stream);
int pscv_depth_nearest_crop(const float* depth, int th, int tw, int oh, int ow, int y0, int x0, int ch, int cw, float min_d,
                            float max_d, float* out_depth, unsigned char* out_mask, void* stream);

/*
 * Loss reductions and depth-map scores (an addition to ABI 14: new exports only, no existing signature changes): the end of
 * models/trainer.py:step (trainer.py:114-198) and the depth-map protocol of Trainer.test / depthmap_eval.py:104-143
 * (csrc/depth_gt.hip).  fp32 data; a mask is uint8 / bool (valid where non-zero) or fp32 holding 0 or 1
 * (valid where 1 for the ground-truth masks, where non-zero for the given masks).  Asynchronous on `stream`, no host wait, no float
 * atomics: per-block partial sums in the caller's workspace, combined in a fixed order in fp64 -- equal inputs, equal bits.
 *
 * One call takes a table of n_terms <= PSCV_LOSS_MAX_TERMS terms as PARALLEL HOST ARRAYS (entry t describes term t; the arrays are
 * read before the call returns, the table travels in the kernel arguments).  With l the per-pixel loss, m the mask, C = sum m,
 * S_l = sum l m, S_u = sum (l exp(-u) + u) m:
 *   kind                 a          u       gt        mask        interval   l                          term
 *   PSCV_LOSS_GT_PLAIN   d [b,h,w]  -       [b,H,W]   [b,H,W]     [b]        |d - gt_down| / interval_b   S_l / C (NaN when C = 0)
 *   PSCV_LOSS_GT_BAYES   d [b,h,w]  [b,h,w] [b,H,W]   [b,H,W]     [b]        the same                     C != 0 ? (S_u + S_l) / C : S_u + S_l
 *   PSCV_LOSS_L_PLAIN    l [n]      -       -         [n]         -          given                        C != 0 ? S_l / C : S_l
 *   PSCV_LOSS_L_BAYES    l [n]      [n]     -         [n]         -          given                        as GT_BAYES
 *   dims [n_terms][5] (host, long) = (b, h, w, H, W); the L kinds use n = b h w and ignore H, W.  mask_u8[t] != 0: the mask is bytes.
 * gt_down and the down mask are F.interpolate(mode="bilinear", align_corners=False) and `== 1` for INTEGER ratios rh = H / h,
 * rw = W / w (anything else is an error): per axis one tap at r i + (r - 1) / 2 for an odd ratio, the two taps r i + r / 2 - 1
 * and the next, weighing 0.5 each, for an even one; m = 1 iff every tap used is valid; gt_down = 0.5 (0.5 a + 0.5 b) +
 * 0.5 (0.5 c + 0.5 d) in that association; taps of weight zero are not read.
 *
 * pscv_loss_terms: two launches (reduce over the whole table; finish).  Device outputs: loss fp32 [1] = sum_t factors[t] term_t,
 * term fp32 [n_terms], sums fp64 [n_terms][3] = (S_l, S_u, C), norm fp32 [n_terms] = the normaliser the backward needs (1 / C;
 * 1 where the term is un-normalised).  workspace: pscv_loss_terms_workspace(n_terms, dims) bytes, 8-byte aligned.
 * pscv_loss_terms_bwd: one launch; grad_out fp32 [1] is read on the device; per term the gradients asked for are written
 * (grad_a: d d or d l, grad_u; a null entry or a null array = skip), the others recomputed per pixel:
 *   d d = g f n m sign(d - gt_down) / interval_b (x (exp(-u) + 1) for the Bayes kinds; sign(0) = 0),  d u = g f n m (1 - l exp(-u)),
 *   d l = g f n m (x (exp(-u) + 1)).  Exactly 0 where m = 0, except that a GT_PLAIN term with C = 0 has n = 1 / 0: NaN, as torch.
 */
#define PSCV_LOSS_GT_PLAIN 0
#define PSCV_LOSS_GT_BAYES 1
#define PSCV_LOSS_L_PLAIN 2
#define PSCV_LOSS_L_BAYES 3
#define PSCV_LOSS_MAX_TERMS 32
#define PSCV_METRIC_MAX_THRESH 4
#define PSCV_METRIC_SUMS 12
long pscv_loss_terms_workspace(int n_terms, const long* dims);
int pscv_loss_terms(int n_terms, const int* kinds, const void* const* a, const void* const* u, const void* const* gt,
                    const void* const* mask, const void* const* interval, const int* mask_u8, const long* dims, const float* factors,
                    void* workspace, float* loss, float* term, double* sums, float* norm, void* stream);
int pscv_loss_terms_bwd(int n_terms, const int* kinds, const void* const* a, const void* const* u, const void* const* gt,
                        const void* const* mask, const void* const* interval, const int* mask_u8, const long* dims,
                        const float* factors, const float* norm, const float* grad_out, const void* const* grad_a,
                        const void* const* grad_u, void* stream);
/*
 * pscv_depth_metrics: the five metric functions of models/utils.py:138-171 (each under compute_metrics_for_each_image) in one pass.
 * est fp32 [b,h,w] is upsampled bilinearly to (H, W) with torch's fp32 index rule -- src = (in / out) (dst + 0.5) - 0.5 clamped
 * at 0, the neighbour clamped at the edge; any sizes, h = H is a copy --, est and gt [b,H,W] are divided by step[b] (null = 1), a
 * pixel counts where mask [b,H,W] > 0.5 (bytes: non-zero).  thr_abs (host, n_abs <= 4) and thr_rel (host, n_rel <= 4).
 * sums fp64 [b][PSCV_METRIC_SUMS] = (C, sum |e - g|, count |e - g| > thr_abs[0..3], sum |e - g| / g, sum (e - g)^2 / g,
 * count max(e / g, g / e) > thr_rel[0..3]); means fp32 [b + 1][PSCV_METRIC_SUMS - 1] = per image (EPE, fraction above thr_abs[k],
 * Rel, SqRel, 1 - fraction above thr_rel[k]) and, in row b, their mean over the batch.  An empty mask gives NaN.
 * workspace: pscv_depth_metrics_workspace(b, H, W) bytes.  Two launches.
 */
long pscv_depth_metrics_workspace(int b, int H, int W);
int pscv_depth_metrics(const float* est, const float* gt, const void* mask, int mask_u8, const float* step, int b, int h, int w, int H,
                       int W, const float* thr_abs, int n_abs, const float* thr_rel, int n_rel, void* workspace, double* sums,
                       float* means, void* stream);

/*
 * Training-view augmentation (an addition to ABI 14: new exports only, no existing signature changes): the reference's
 * MVSDataset.data_augmentation (data/MVSDataset.py:124-150, BlendedMVS in train mode) -- torchvision's ColorJitter on the PIL image
 * (ImageEnhance.Brightness / Contrast = Image.blend with a degenerate image), then a 3 x 3 directional blur of the fp32 image
 * (csrc/image_augment.hip).  imgs: V <= PSCV_AUG_MAX_VIEWS views of one size, interleaved uint8
 * [V][H][W][3] on the device.  The per-view records are PARALLEL HOST ARRAYS read before the call returns:
 *   ops     int   [V][2]  the two steps in their order, each PSCV_AUG_NONE / _BRIGHTNESS / _CONTRAST; none may be listed twice
 *   factors float [V][2]  the blend factor of each step (ignored for NONE); finite
 *   weights float [V][9]  the blur's 3 x 3 correlation kernel, row-major; finite; a centre of 1 among zeros is "no blur"
 * Per byte and step: t = (float)deg + a * (float)((int)v - (int)deg), product and sum each rounded to fp32; for 0 <= a <= 1 the byte
 * is t truncated, otherwise 0 where t <= 0, 255 where t >= 255, else t truncated.  deg = 0 for brightness; for contrast
 * deg = (2 S + H W) / (2 H W) in integers, S the sum over the WHOLE image, as it stands when the step runs, of
 * (19595 R + 38470 G + 7471 B + 0x8000) >> 16.  Per pixel of the window and channel: the taps of non-zero weight, in row-major
 * order, acc = w lut[byte] for the first and acc = acc + w lut[byte] after it (each product and sum rounded to fp32), neighbours
 * outside the IMAGE (not the window) by BORDER_REFLECT_101 (-1 reads 1, n reads n - 2, a length of 1 reads 0).
 *
 * pscv_augment_workspace: bytes of the workspace (8-byte aligned) for V views; < 0 on error.
 * pscv_augment_grey_sums: S of every view that has a contrast step, into the workspace (cleared on the stream first; integer
 *   atomics, so equal inputs give equal sums).  No launch and no workspace needed when no view has one.
 * pscv_augment_apply: out fp32 [V][3][ch][cw] = the window of ch rows from y0 and cw columns from x0; lut device fp32 [256], the
 *   caller's float(v) / 255.0f; workspace as pscv_augment_grey_sums left it on the same stream (may be null without contrast).
 * Asynchronous on `stream`, no host wait.
 */
#define PSCV_AUG_NONE 0
#define PSCV_AUG_BRIGHTNESS 1
#define PSCV_AUG_CONTRAST 2
#define PSCV_AUG_MAX_VIEWS 16
long pscv_augment_workspace(int V);
int pscv_augment_grey_sums(const unsigned char* imgs, int V, int H, int W, const int* ops, const float* factors, void* workspace,
                           void* stream);
int pscv_augment_apply(const unsigned char* imgs, int V, int H, int W, const int* ops, const float* factors, const float* weights,
                       const void* workspace, int x0, int y0, int cw, int ch, const float* lut, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PSCV_H */
