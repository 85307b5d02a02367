/* clslam_hip.h -- C ABI of libclslam_hip.so, the MI355X (gfx950) native library behind the
 * CL-SLAM depth_pose_prediction hot path.
 *
 * The reference (robot-learning-freiburg/CL-SLAM) is pure Python on PyTorch; its "FFI" for this
 * path is the set of ATen/cuDNN ops it calls.  Each entry point below names the reference
 * call site(s) it replaces (paths relative to the reference root; dpp.py =
 * depth_pose_prediction/depth_pose_prediction.py).  The host-side binding is
 * cl-slam_amd/clslam_hip/_lib.py (ctypes); INTEGRATION.md shows the stub a reference
 * maintainer would add.
 *
 * Conventions: every pointer is a DEVICE pointer to fp32 data unless stated otherwise; tensors
 * inside the library are NHWC (channels last) except the planar NCHW images / depth maps that
 * the reference's sample dict and output dict define.  Functions never allocate, never
 * synchronise, enqueue on `stream` (a hipStream_t passed as void*), and return CLSLAM_OK or a
 * negative error code; clslam_last_error() gives the message.  No exceptions cross the ABI.
 */
#ifndef CLSLAM_HIP_H
#define CLSLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLSLAM_OK 0
#define CLSLAM_ERR_INVALID (-1)
#define CLSLAM_ERR_LAUNCH (-2)

#define CLSLAM_ACT_NONE 0
#define CLSLAM_ACT_RELU 1
#define CLSLAM_ACT_ELU 2
#define CLSLAM_ACT_HSWISH 3   /* x * relu6(x+3) / 6   (MobileNetV3) */
#define CLSLAM_ACT_HSIGMOID 4 /* relu6(x+3) / 6 */

#define CLSLAM_PAD_ZERO 0
#define CLSLAM_PAD_REFLECT 1

/* Library identification / error text (thread-local). */
/* ABI version: 101 = clslam_conv_desc.weight_wino appended, clslam_wino_weight_*; 100 -> 101 also covers the double* dp_partial of
 * the view-synthesis / loss backward and clslam_pose_bwd (round 4); 102 = clslam_conv_desc.cu_limit appended; 103 = clslam_handoff_* added;
 * 104 = per-scale range forms of the four pyramid launches added; 105 = clslam_depth_metrics* added; 106 = clslam_pcl_* added;
 * 107 = the range forms of 104 and the unfused pyramid backward removed; 108 = clslam_store_* added (frame store);
 * 109 = the batched-copy and the fused reduction + Adam entry points removed (DESIGN.md "Retired step paths");
 * 110 = clslam_pose_pair_error, clslam_traj_metrics* added; 111 = clslam_resize_level_u8, clslam_ring_gather added (online ingest).
 * 112 = clslam_pair_loss added (predict_from_images); 113 = clslam_pcl_voxel_* added (voxel-grid downsampling of a cloud).
 * 114 = clslam_demosaic_bilinear, clslam_undistort_lut, clslam_robotcar_rectify added (RobotCar raw frames).
 * 114 also carries clslam_png_* (PNG encoding): purely additive -- no struct, no existing signature changes -- so the number stays;
 * a binding that needs them reports a library built before them by the name of the missing entry point.  The same holds for
 * clslam_viz_* (frame panels): one new descriptor struct of their own, nothing that exists changes.
 * Bindings check it before the first call.                                                                                  */
#define CLSLAM_ABI_VERSION 114
int clslam_version(void);
const char* clslam_last_error(void);
const char* clslam_last_error_string(void); /* = clslam_last_error (the name SURVEY.md 8b lists) */
/* 16 hex digits identifying the kernel sources the library was built from (csrc/build.py source_id()); "unstamped" for a
 * build that did not go through build.py.  bench.py pairs its timings with counter files of the same id only.           */
const char* clslam_build_id(void);
/* 1 when the library was built from the HIP sources for gfx950, 0 for the CPU emulator used
 * by the host-logic tests (tests/emu); the product loader refuses anything but 1. */
int clslam_is_device_build(void);

/* ---------------------------------------------------------------------------------------------
 * clslam_conv2d: fp32 implicit-GEMM convolution on MFMA (3x3 / 1x1, NHWC, OHWI weights).
 * Replaces nn.Conv2d + BatchNorm2d(eval) + ReLU/ELU + residual add + ReflectionPad2d +
 * F.interpolate(nearest) + torch.cat at: networks/resnet_encoder.py:118-125 (torchvision
 * BasicBlock bodies), networks/layers.py:9-48, networks/depth_decoder.py:51-66,
 * networks/pose_decoder.py:40-47; and their autograd data-gradients (dgrad runs the same kernel
 * on transposed weights, see clslam_weight_transpose).
 *   out[b,oy,ox,n] = act(scale[n]*sum_{ky,kx,c} in(b, oy*stride-pad+ky, ox*stride-pad+kx, c)
 *                        * weight[n][ky][kx][c] + shift[n] + residual[b,oy,ox,n])
 *   in(...) = channel-concat of src_a (optionally nearest-2x upsampled) and src_b, padded by
 *   zeros or reflection.                                                                      */
typedef struct clslam_conv_desc {
    const float* src_a;    /* [B][in_h(/2)][in_w(/2)][ch_a]                                   */
    const float* src_b;    /* [B][in_h][in_w][ch_b] or NULL                                   */
    const float* weight;   /* [ch_out][ksize*ksize][ch_a+ch_b]                                */
    const float* scale;    /* [ch_out] or NULL (=1)   folded BatchNorm gamma/sqrt(var+eps)     */
    const float* shift;    /* [ch_out] or NULL (=0)   folded BatchNorm shift / conv bias       */
    const float* residual; /* [B][out_h][out_w][ch_out] or NULL                               */
    float* out;            /* [B][out_h][out_w][ch_out]                                       */
    int32_t batch, in_h, in_w, ch_a, ch_b, out_h, out_w, ch_out;
    int32_t ksize, stride, pad, pad_mode, upsample_a, act;
    int32_t config;        /* tile configuration, -1 = choose                                  */
    /* dgrad epilogue: out *= act'(y) where y = actgrad_src[b,oy,ox,n] is the OUTPUT of the
     * activation being differentiated (ReLU' = y>0, ELU' = y>0 ? 1 : y+1). NULL = off.        */
    const float* actgrad_src;
    int32_t actgrad_kind;
    /* Optional split-K scratch for the small-M 3x3 layers (layer3/4, pose decoder, upconv_4_x at 192x640:
     * fewer output tiles than CUs).  Device memory, ZERO-FILLED ONCE by the caller, private to the
     * stream the conv is launched on (convs on one stream may share it: the first 64 KiB are per-tile
     * arrival counters that every launch leaves at zero).  NULL/0: no split-K.  Results do not depend on
     * which workgroup finishes last: partial tiles are summed in split order.                       */
    void* workspace;
    size_t workspace_bytes;
    /* Optional (ABI version >= 101): the same filter pre-transformed for the Winograd F(2x2,3x3) kernel by
     * clslam_wino_weight_transform (3x3, stride 1, zero padding, one source; needs `workspace`).  NULL: the direct kernels.
     * Frozen weights (the two ResNet encoders) are transformed once per load; `weight` must still be set.  The kernel needs
     * 64 KiB + 64 KiB per workgroup of `workspace` (hand-off flags -- eight per workgroup, holding the launch's epoch, never
     * reset -- and one partial slab each); with config < 0 a launch that does not fit falls back to the direct kernels.   */
    const float* weight_wino;
    /* Optional (ABI version >= 102): how many compute units a PERSISTENT launch (the stream-K and Winograd kernels: one or two
     * resident workgroups per CU that walk the whole layer) may occupy; 0 = all of them.  A caller that runs independent
     * branches on several streams (the depth and the pose network of one step) gives each launch half of the chip: two such
     * launches then run side by side, each workgroup walks twice the units and the per-launch prologue / hand-off / epilogue
     * phases cost half.  Measured on MI355X at 192x640: -2.9 % per step at 5 triplets, +3.7 % at 33.  Results
     * do not depend on it beyond the summation order of the hand-off (fixed per (shape, cu_limit)).                       */
    int32_t cu_limit;
} clslam_conv_desc;
int clslam_conv2d(const clslam_conv_desc* desc, void* stream);
/* the tile configuration clslam_conv2d uses for desc->config < 0 (profiling / reporting) */
int clslam_conv2d_pick_config(const clslam_conv_desc* desc);
/* U = G g G^T of Winograd F(2x2,3x3) for a 3x3 filter w [ch_out][9][ch_in] (ch_in a multiple of 16), formed in double and
 * rounded once, in the layout the kernel stages through LDS: clslam_wino_weight_size(ch_out, ch_in) floats
 * ([ceil(ch_out/64)][ch_in/8][16 positions][64][8], zero beyond ch_out).  Replaces nothing in the reference: cuDNN does the
 * same transformation inside its own Winograd convolution (networks/resnet_encoder.py:118-125 on the GPU).            */
size_t clslam_wino_weight_size(int ch_out, int ch_in);
int clslam_wino_weight_transform(const float* w, float* u, int ch_out, int ch_in, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward of the trainable convolutions -- replaces autograd's convolution_backward,
 * reflection_pad2d_backward, upsample_nearest2d_backward, cat backward, elu/relu backward for
 * networks/depth_decoder.py:51-71, networks/layers.py:9-48, networks/pose_decoder.py:37-54
 * (entered from dpp.py:312 `losses['loss'].backward()`).                                      */

/* wt[ci][taps-1-t][co] = w[co][t][ci] for ci < ch_in_sel: the weights of the dgrad-as-conv.    */
int clslam_weight_transpose(const float* w, float* wt, int ch_out, int taps, int ch_in, int ch_in_sel,
                            void* stream);
/* The same for nitems weight tensors in ONE launch (items is a HOST array, passed to the kernel by value): the eleven
 * dgrad weight sets of a backward pass (nine depth_decoder upconvs, pose_decoder.py:40-47 pose_0 / pose_1) depend on
 * the weights only and are produced together at its start.                                                          */
typedef struct clslam_transpose_item {
    const float* w;
    float* wt;
    int ch_out, taps, ch_in, ch_in_sel;
} clslam_transpose_item;
int clslam_weight_transpose_multi(const clslam_transpose_item* items, int nitems, void* stream);
/* dz = act'(yout) * fold(dxp): dxp is the gradient w.r.t. the PADDED conv input
 * [B][h+2*border][w+2*border][ch_stride]; border=1 folds the reflection border back
 * (ReflectionPad2d backward), pool=1 sums each 2x2 block (nearest-2x upsample backward, output
 * is [B][h/2][w/2][ch]); only channels [0,ch) are used (the skip half of a concat is dead:
 * encoders are frozen, dpp.py:308,813-819); yout may be NULL (no activation).                 */
/* bias_partial (optional) receives [clslam_fold_blocks(...)][ch] per-block column sums of dz, i.e.
 * the bias-gradient partials of the conv that produced yout (reduce with clslam_reduce_partials). */
int clslam_fold_blocks(int batch, int h, int w, int ch, int pool);
/* disp_dz (B,h,w) / disp_w (9,ch), optional (pool = 0, border = 1): additionally adds the data gradient of
 * the dispconv head that reads the same activation (what clslam_dispconv_bwd_data would accumulate into
 * dxp), evaluated per folded position; dxp may then be NULL.                                        */
int clslam_fold_act_grad(const float* dxp, const float* yout, float* dz, float* bias_partial, int batch, int h, int w,
                         int ch, int ch_stride, int border, int pool, int act, const float* disp_dz, const float* disp_w,
                         void* stream);
/* Weight gradient as an MFMA GEMM reducing over pixels; desc = the forward conv's descriptor. */
int clslam_wgrad_splits(const clslam_conv_desc* desc, int target_blocks);
int clslam_conv_wgrad(const clslam_conv_desc* desc, const float* dz, float* partial, int splits, void* stream);
/* Same contract as clslam_conv_wgrad for 3x3 stride-1 convs on images wider than 40 px, with the dZ
 * tile and the input patch resident in LDS (wgrad_patch.hip); splits from clslam_wgrad_patch_splits. */
int clslam_wgrad_patch_supported(const clslam_conv_desc* desc);
int clslam_wgrad_patch_splits(const clslam_conv_desc* desc, int target_blocks);
int clslam_conv_wgrad_patch(const clslam_conv_desc* desc, const float* dz, float* partial, int splits, void* stream);
/* out[i] = scale * sum_s partial[s*n + i] in a fixed order (deterministic).                    */
int clslam_reduce_partials(const float* partial, float* out, size_t n, int splits, float scale, void* stream);
/* Batched clslam_reduce_partials: items_dev is a DEVICE array of nitems records
 * {const float* partial; float* out; uint64_t n; int32_t splits; float scale} (32 bytes each).     */
int clslam_reduce_multi(const void* items_dev, int nitems, int blocks_per_item, void* stream);
/* bias gradient: column sums of x[rows][ch], stage 1 (follow with clslam_reduce_partials).     */
int clslam_colsum_blocks(int rows);
int clslam_colsum(const float* x, float* partial, int rows, int ch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Encoder stem (frozen): (x-0.45)/0.225 -> conv7x7 s2 p3 -> eval BN -> ReLU, and maxpool 3x3 s2 p1.
 * Replaces networks/resnet_encoder.py:117-121.  img_a/img_b: planar (B,3,h,w) frames exactly as
 * the sample dict holds them (img_b = second frame of the pose pair, dpp.py:951-955, or NULL);
 * weight: the conv1 weight (64, 3*num_images, 7, 7), checkpoint OIHW order, re-packed ONCE per load by
 * clslam_stem_pack_weight into clslam_stem_packed_size(num_images) floats; out: NHWC (B,h/2,w/2,64). */
int clslam_stem_packed_size(int num_images);
int clslam_stem_pack_weight(const float* weight, float* packed, int num_images, void* stream);
int clslam_stem_conv(const float* img_a, const float* img_b, const float* weight, const float* scale,
                     const float* shift, float* out, int batch, int h, int w, int num_images, void* stream);
int clslam_maxpool3x3s2(const float* in, float* out, int batch, int h, int w, int ch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Disparity head: reflection-padded 3x3 conv C->1 + sigmoid (networks/depth_decoder.py:67-69) and
 * its backward.  x NHWC (B,h,w,ch); w [9][ch]; disp / dz planar (B,h,w); dz = dL/d(pre-sigmoid).
 * dispconv_bwd_data writes (accumulate=0) or adds (1) into the padded-domain gradient
 * dxp (B,h+2,w+2,ch) that clslam_fold_act_grad consumes.                                        */
int clslam_dispconv_fwd(const float* x, const float* w, const float* bias, float* disp, int batch, int h, int wd,
                        int ch, void* stream);
int clslam_dispconv_bwd_data(const float* dz, const float* w, float* dxp, int batch, int h, int wd, int ch,
                             int accumulate, void* stream);
int clslam_dispconv_wgrad_blocks(int pixels);
int clslam_dispconv_wgrad(const float* dz, const float* x, float* partial, int batch, int h, int wd, int ch,
                          void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pose head: pose_2 (1x1, 256->12) + spatial mean + x0.01 (networks/pose_decoder.py:44-54) and
 * its backward.  x: pose_1 output NHWC (n,hw,256) post-ReLU; pose (n,12); mean (n,256) is kept
 * for the backward; dz1 = dL/d(pre-ReLU pose_1 output).                                         */
int clslam_pose_head_fwd(const float* x, const float* w2, const float* b2, float* mean, float* pose, int n, int hw,
                         void* stream);
int clslam_pose_head_bwd(const float* dpose, const float* x, const float* w2, const float* mean, float* dz1,
                         float* dw2, float* db2, int n, int hw, float grad_scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pose -> matrices, view synthesis (forward and backward).  Replaces
 * depth_pose_prediction/utils.py:34-117 (transformation_from_parameters, invert for frame -1),
 * networks/layers.py:51-104 (BackprojectDepth, Project3D), utils.py:120-142 (disp_to_depth),
 * dpp.py:986-1017 (F.interpolate bilinear + F.grid_sample border/align_corners=True) and autograd.
 * pose (2B,12): row fi*B+b = pose-decoder output of frame idx fi (0: frame -1, 1: frame +1);
 * cam_t_cam (2,B,4,4); proj (2,B,3,4) = (K*T)[:3]; images planar (B,3,H,W); depth (B,H,W);
 * warped / dpred (2,B,3,H,W).  min_depth/max_depth <= 0 stand for None.                          */
int clslam_pose_to_proj(const float* pose, const float* kmat, float* cam_t_cam, float* proj, int batch, void* stream);
int clslam_warp_fwd(const float* disp_s, int h, int w, const float* src_m1, const float* src_p1, const float* inv_k,
                    const float* proj, float* depth, float* warped, int batch, int H, int W, float min_depth,
                    float max_depth, void* stream);
/* Pyramid forms (ONE launch for the four scales): disp = host array of 4 device pointers,
 * disp[s] (B,H>>s,W>>s); depth (4,B,H,W); warped (4,2,B,3,H,W).                                     */
int clslam_warp_fwd_pyramid(const float* const* disp, const float* src_m1, const float* src_p1, const float* inv_k,
                            const float* proj, float* depth, float* warped, int batch, int H, int W, float min_depth,
                            float max_depth, void* stream);
/* Diagnostic (parity tests): the bilinear cell and border-clip flags the path uses per (scale, source frame, sample,
 * pixel) -- what F.grid_sample decides internally at dpp.py:1013-1017.  cells (4,2,B,H,W) int32 =
 * x0 | y0 << 12 | (x not clipped) << 24 | (y not clipped) << 25; same arguments as clslam_warp_fwd_pyramid.          */
int clslam_warp_cells_pyramid(const float* const* disp, const float* inv_k, const float* proj, int* cells, int batch, int H,
                              int W, float min_depth, float max_depth, void* stream);
/* Diagnostic: the sampling positions themselves -- coords (4, 2, batch, H, W, 2) float = (ix, iy) in pixels of the source frame
 * after grid_sample's border clip (the value the four taps are weighted by); same arguments as clslam_warp_cells_pyramid.
 * tests/test_warp_positions.py bounds them against the float64 oracle, which is what the warped-image tolerance derives from. */
int clslam_warp_coords_pyramid(const float* const* disp, const float* inv_k, const float* proj, float* coords, int batch, int H,
                               int W, float min_depth, float max_depth, void* stream);
int clslam_warp_bwd_blocks(int H, int W);
/* ddisp_up (B,H,W) = dL/d(upsampled disparity); dp_partial [B][nblk][24] block sums of dL/dproj */
int clslam_warp_bwd(const float* dpred, const float* disp_s, int h, int w, const float* src_m1, const float* src_p1,
                    const float* inv_k, const float* proj, float* ddisp_up, double* dp_partial, int batch, int H, int W,
                    float min_depth, float max_depth, void* stream);
/* dp_partial [nscale][B][nblk][24]; dpose (2B,12) = dL/d(pose-decoder output) incl. the velocity
 * term (dpp.py:1125-1146; dist0/dist1 = relative_distance(0|1) as float64, sample_w (B)).        */
int clslam_pose_bwd(const double* dp_partial, int nscale, int nblk, const float* pose, const float* kmat,
                    const double* dist0, const double* dist1, const float* sample_w, float vel_scale, float* dpose,
                    int batch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Photometric / smoothness / velocity loss and its backward.  Replaces networks/layers.py:107-137
 * (SSIM), dpp.py:1019-1192 (_compute_loss, _compute_smooth_loss incl. its flattening behaviour,
 * _compute_velocity_loss, _compute_reprojection_loss) and autograd.                               */
/* map[n] = 0.85*mean_c SSIM + 0.15*mean_c L1 of pred image n (npred x (3,H,W)) vs target n % B;
 * coef (npred,9,H,W) or NULL: SSIM derivative coefficients kept for clslam_photo_grad.           */
int clslam_photo_map(const float* pred, const float* target, float* map, float* coef, int npred, int batch, int H,
                     int W, void* stream);
int clslam_automask_blocks(int H, int W);
/* idmap/rpmap (2,B,H,W); noise (B,2,H,W) or NULL; sel (B,H,W) u8 argmin of
 * [id(-1)+noise, id(+1)+noise, reproj(-1), reproj(+1)]; partial [B][nblk] sums of the minimum.  */
int clslam_automask(const float* idmap, const float* noise, const float* rpmap, unsigned char* sel, float* partial,
                    int batch, int H, int W, void* stream);
/* psum [B][clslam_disp_mean_chunks()] partial sums of each sample's disparity map (the mean is
 * formed inside clslam_loss_finalize).                                                            */
int clslam_automask_pyramid(const float* idmap, const float* noise, const float* rpmap, unsigned char* sel, float* partial,
                            int nscale, int batch, int H, int W, void* stream);
int clslam_disp_mean_pyramid(const float* const* disp, float* psum, int batch, int H, int W, void* stream);
/* Fused clslam_photo_map(warped) + clslam_automask over the pyramid: both reprojection maps are evaluated in
 * registers and only the SELECTED frame's 9 SSIM coefficients are stored: coef_sel (4,B,9,H,W) or NULL.      */
int clslam_photo_automask_pyramid(const float* warped, const float* target, const float* idmap, const float* noise,
                                  unsigned char* sel, float* coef_sel, float* partial, int batch, int H, int W,
                                  void* stream);
/* The same with the tie-break noise of dpp.py:1055-1056 drawn INSIDE the kernel (Philox4x32-10 + Box-Muller, x 1e-5):
 * element ((scale * B + b) * H * W + pixel) of draw `offset`, key `seed` (non-zero).  Timing / production runs; parity
 * runs inject captured tensors through clslam_photo_automask_pyramid.  clslam_tie_break_noise writes the pairs
 * (n_id(-1), n_id(+1)) of elements [0, npix) of the same stream to out[2 * npix] (tests, inspection).            */
int clslam_photo_automask_pyramid_rng(const float* warped, const float* target, const float* idmap, unsigned long long seed,
                                      unsigned long long offset, unsigned char* sel, float* coef_sel, float* partial, int batch,
                                      int H, int W, void* stream);
int clslam_tie_break_noise(float* out, size_t npix, unsigned long long seed, unsigned long long offset, void* stream);
/* Opt-in "intended" smoothness (the per-sample edge-aware term of monodepth2 instead of the flattened-batch
 * behaviour of dpp.py:1148-1176 that the default mode reproduces).  fwd: partial[4][B][clslam_smooth_intended_chunks()]
 * sums of |d disp| * exp(-mean_c |d I|) / count over the x and y edges; finalize (after clslam_loss_finalize run with
 * n_smooth = 0): adds sum_b w_b * inv_b * T_b per scale to losses[s*4+1..3] and losses[17], keeps aux[4][B][2] =
 * (1/(mean disp + 1e-7), T); bwd: ADDS the term's gradient (through the mean normalisation and the head's sigmoid) to
 * dz[s] (B,h_s,w_s).  means = the (4,B,clslam_disp_mean_chunks()) output of clslam_disp_mean_pyramid.               */
int clslam_smooth_intended_chunks(void);
int clslam_smooth_intended_fwd(const float* const* disp, const float* const* rgb0, float* partial, int batch, int H, int W,
                               void* stream);
int clslam_smooth_intended_finalize(const float* partial, const float* means, const float* sample_w, float* losses, float* aux,
                                    int batch, int H, int W, float smooth_scale, void* stream);
int clslam_smooth_intended_bwd(const float* const* disp, const float* const* rgb0, const float* aux, const float* sample_w,
                               float* const* dz, int batch, int H, int W, float smooth_scale, void* stream);
/* LDS-tiled fused loss backward on coef_sel; dp_partial [4][B][clslam_loss_bwd2_blocks][24].                */
int clslam_loss_bwd2_blocks(int H, int W);
int clslam_loss_bwd2_pyramid(const float* const* disp, const unsigned char* sel, const float* coef_sel, const float* warped,
                             const float* target, const float* src_m1, const float* src_p1, const float* inv_k,
                             const float* proj, const float* sample_w, float* ddisp_up, double* dp_partial, int batch,
                             int H, int W, float min_depth, float max_depth, void* stream);
int clslam_disp_grad_pyramid(const float* ddisp_up, const float* const* disp, const float* smooth_aux, int n_smooth,
                             float* const* dz, int batch, int H, int W, void* stream);
int clslam_disp_mean_chunks(void);
int clslam_disp_mean(const float* disp, float* psum, int batch, int hw, void* stream);
typedef struct clslam_loss_desc {
    const float* partial[4];  /* automask partials per scale [B][nblk]                             */
    const float* disp[4];     /* ('disp',s) (B,H>>s,W>>s)                                          */
    const float* rgb0[4];     /* ('rgb',0,s) (B,3,H>>s,W>>s)                                       */
    const float* means[4];    /* clslam_disp_mean outputs [B][chunks]                              */
    const float* pose;        /* (2B,12)                                                           */
    const double* dist0;      /* ('relative_distance',0) (B) float64                               */
    const double* dist1;
    const float* sample_w;    /* (B) loss weights of the local samples (dpp.py:1031-1032)          */
    const float* smooth_w;    /* (n_smooth) weights of the smoothness terms                        */
    float* losses;            /* [18]: 4 x {reprojection, smooth, reg, depth_loss/scale}, velocity, total */
    float* smooth_aux;        /* [4][2+2*n_smooth] kept for clslam_disp_grad                        */
    int32_t batch, nblk, H, W, n_smooth;
    float smooth_scale, vel_scale;
} clslam_loss_desc;
int clslam_loss_finalize(const clslam_loss_desc* desc, void* stream);
/* ---- mask_dynamic = True: the masked loss (additive entry points, ABI 114) --------------------------------------------------
 * masks: inputs['mask', 0, s] as (B,h_s,w_s) float planes, one per scale as the dataset builds them.  A pixel is STATIC iff its
 * value != 1.0f ((1 - m).type(torch.bool), dpp.py:1066-1067 and 1081-1082: 0.5 and 2.0 are static, only an exact 1 is dynamic).
 * Reprojection (dpp.py:1063-1076): every scale uses the scale-0 mask; reprojection_loss/scale_s = sum over the static pixels of
 * ALL samples of the per-pixel minimum / N_static; sample_w is NOT applied to it (it still weights smoothness and velocity).
 * Smoothness, default mode (dpp.py:1080-1090 into 1148-1176): masked_select flattens the batch, so term i < B is the i-th static
 * element of the cropped x plane (B,1,h,w-1) plus the i-th static element of the cropped y plane (B,1,h-1,w), weighted by
 * smooth_w[i]; dpp.py:1172-1174 then average that scalar over mask[i]: the scalar itself if sample i has a static element in
 * both cropped planes, NaN otherwise.  Supported layout: all B elements lie in sample 0; otherwise the term is written as NaN
 * (the reference raises IndexError or reads into sample 1 there -- the one divergence).
 * None of these synchronises; no floating-point atomics; counts are unsigned integers converted once.                          */
/* Replaces dpp.py:1038-1069: clslam_photo_automask_pyramid[_rng] with mask0 (B,H,W) = ('mask',0,0).  noise (4,B,2,H,W), or NULL
 * with seed != 0 for the in-kernel draw.  partial (4,B,nblk): tile sums over the static pixels; cnt_partial (B,nblk): static
 * pixels per tile (the same for every scale).  sel / coef_sel as without the mask, for every pixel.                            */
int clslam_photo_automask_pyramid_masked(const float* warped, const float* target, const float* idmap, const float* noise,
                                         unsigned long long seed, unsigned long long offset, const float* mask0,
                                         unsigned char* sel, float* coef_sel, float* partial, unsigned* cnt_partial, int batch,
                                         int H, int W, void* stream);
/* The two masked_select calls of dpp.py:1166-1167 as positions: loc [4][2][2 * batch] int per (scale, direction x / y):
 * [i < batch] = pixel index y * w_s + x of the i-th static element of sample 0's cropped plane, -1 if it has fewer;
 * [batch + b] = 1 if sample b has a static element in that cropped plane, else 0 (dpp.py:1172-1173).                          */
int clslam_smooth_locate(const float* const* mask, int* loc, int batch, int H, int W, void* stream);
/* Replaces dpp.py:1071-1113 under mask_dynamic: clslam_loss_finalize on the masked sums.  Same 18 losses, same smooth_aux; the
 * smoothness terms sit at loc's positions (n_smooth == batch, or 0 with loc NULL when the per-sample smoothness follows).
 * mstat [2] = (1 / N_static, N_static) stays on the device for clslam_loss_bwd2_pyramid_masked.                                */
int clslam_loss_finalize_masked(const clslam_loss_desc* desc, const unsigned* cnt_partial, const int* loc, float* mstat,
                                void* stream);
/* Autograd of dpp.py:1068 + 1075: clslam_loss_bwd2_pyramid where a static pixel's term carries inv_n[0] / 4 = 1 / (4 N_static)
 * in place of sample_w[b] / (H W) / 4 and a dynamic pixel's term carries 0 -- in ddisp_up and in dp_partial alike.             */
int clslam_loss_bwd2_pyramid_masked(const float* const* disp, const unsigned char* sel, const float* coef_sel, const float* warped,
                                    const float* target, const float* src_m1, const float* src_p1, const float* inv_k,
                                    const float* proj, const float* mask0, const float* inv_n, float* ddisp_up, double* dp_partial,
                                    int batch, int H, int W, float min_depth, float max_depth, void* stream);
/* Autograd of the positioned terms of dpp.py:1166-1174: ADDS their gradient (and the mean-normalisation feedback) to dz[s] of
 * sample 0, after clslam_disp_grad_pyramid run with n_smooth = 0.                                                             */
int clslam_smooth_pos_bwd(const float* const* disp, const float* smooth_aux, const int* loc, int n_smooth, float* const* dz,
                          int batch, int H, int W, void* stream);
/* reference_quirks = False under mask_dynamic (the per-sample term dpp.py:1148-1176 evidently meant, on its masks): per sample the
 * mean of the x terms over the static elements of mask[b,:,:,:-1] plus the mean of the y terms over those of mask[b,:,:-1,:].
 * partial / cnt [4][B][clslam_smooth_intended_chunks()][2] (x, y); aux [4][B][4] = (inv, T, 1 / n_x, 1 / n_y).  A sample without
 * a static element in a cropped plane gives NaN.  Otherwise as clslam_smooth_intended_*.                                      */
int clslam_smooth_intended_masked_fwd(const float* const* disp, const float* const* rgb0, const float* const* mask, float* partial,
                                      unsigned* cnt, int batch, int H, int W, void* stream);
int clslam_smooth_intended_masked_finalize(const float* partial, const unsigned* cnt, const float* means, const float* sample_w,
                                           float* losses, float* aux, int batch, int H, int W, float smooth_scale, void* stream);
int clslam_smooth_intended_masked_bwd(const float* const* disp, const float* const* rgb0, const float* const* mask,
                                      const float* aux, const float* sample_w, float* const* dz, int batch, int H, int W,
                                      float smooth_scale, void* stream);
/* Pair loss: the photometric loss of ONE source frame at scale 0, forward only.  Replaces dpp.py:602-620
 * (predict_from_images with return_loss: _reconstruct_images of frame -1, i.e. dpp.py:986-1017 with networks/layers.py:51-104
 * and utils.py:120-142, and _compute_loss(scales=(0,)), dpp.py:1038-1113 with networks/layers.py:107-137).
 * clslam_pair_loss: view synthesis, both photometric maps, the per-pixel minimum and its block sums in one kernel; the
 * warped image stays on chip.  disp (B,H,W) = ('disp', 0) of the target; src / target (B,3,H,W); inv_k (B,4,4); proj (B,3,4)
 * = (K * cam_T_cam(0,-1))[:3]; noise (B,1,H,W), already x 1e-5, or NULL; partial [B][clslam_automask_blocks(H, W)].
 * Optional outputs, each may be NULL: depth (B,H,W); sel (B,H,W) u8, 0 = identity + noise, 1 = reprojection (a tie goes to
 * 0); maps (2,B,H,W) = [identity map without noise, reprojection map].  With all three NULL only `partial` is written.
 * clslam_pair_loss_rng draws the noise in the kernel: the FIRST value of element (b * H * W + pixel) of draw `offset`, key
 * `seed` (non-zero), of the stream clslam_tie_break_noise writes -- out[2 * (b * H * W + pixel)] of that call.         */
int clslam_pair_loss(const float* disp, const float* src, const float* target, const float* inv_k, const float* proj,
                     const float* noise, float* partial, float* depth, unsigned char* sel, float* maps, int batch, int H,
                     int W, float min_depth, float max_depth, void* stream);
int clslam_pair_loss_rng(const float* disp, const float* src, const float* target, const float* inv_k, const float* proj,
                         unsigned long long seed, unsigned long long offset, float* partial, float* depth, unsigned char* sel,
                         float* maps, int batch, int H, int W, float min_depth, float max_depth, void* stream);
/* losses[7] = reprojection_loss/scale_0, smooth_loss/scale_0, reg_loss/scale_0, depth_loss/scale_0, depth_loss
 * (= depth_loss/scale_0 / 4: dpp.py:1101 divides by the configured scales), velocity_loss, loss.  rgb0 = the target frame;
 * pose (B,12) rows [axis_angle, translation(0,-1), ...]; dist (B) float64 = ('relative_distance', 0), needed when
 * vel_scale > 0: velocity_loss = vel_scale * | |translation| - |dist| | (the loop of dpp.py:1125-1146 over frame_ids (0,-1):
 * one frame).  Smoothness as the step forms it at scale 0: intended = 0 -> the n_smooth flattened terms of
 * dpp.py:1148-1176 weighted by smooth_w; intended != 0 -> the per-sample term of clslam_smooth_intended_*.
 * scratch: clslam_pair_loss_scratch(batch) floats.                                                                    */
int clslam_pair_loss_scratch(int batch);
int clslam_pair_loss_finalize(const float* partial, int nblk, const float* disp, const float* rgb0, const float* pose,
                              const double* dist, const float* sample_w, const float* smooth_w, int n_smooth, int intended,
                              float* scratch, float* losses, int batch, int H, int W, float smooth_scale, float vel_scale,
                              void* stream);
/* dpred (2,B,3,H,W) = dL/d(warped images) of one scale.                                          */
int clslam_photo_grad(const unsigned char* sel, const float* coef, const float* pred, const float* target,
                      const float* sample_w, float* dpred, int batch, int H, int W, void* stream);
/* dz (B,h,w) = dL/d(pre-sigmoid disparity logits): transposed bilinear upsample of ddisp_up plus the
 * smoothness gradient (smooth_aux slice of this scale), times sigmoid'.                           */
int clslam_disp_grad(const float* ddisp_up, const float* disp, const float* smooth_aux, int n_smooth, float* dz,
                     int batch, int h, int w, int H, int W, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused Adam over a flat fp32 arena.  Replaces torch.optim.Adam.step() (dpp.py:203,313; torch
 * defaults, same op order as the single-tensor CPU implementation).  grad is multiplied by
 * grad_scale first (1 for single GPU; data-parallel ranks all-reduce with SUM, so it stays 1).
 * guard (device pointer or NULL): when *guard is NaN the launch leaves param and both moments
 * untouched -- the NaN-loss abort of dpp.py:1115-1118 without a host sync between forward and
 * backward (the host checks the loss once per step, after the optimizer launch).               */
int clslam_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, double lr,
                     double beta1, double beta2, double eps, int step, float grad_scale, const float* guard, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Measurement hook (bench.py's roofline leg; no reference counterpart).  Between _begin and _end every
 * clslam_conv2d launch issued by THIS host thread carries its own start/stop timestamps (hipExtLaunchKernel):
 * the kernel's execution time, the quantity `rocprofv3 --kernel-trace` reports -- an event pair recorded around
 * a launch also counts the ~3 us dispatch gap.  _end waits for the launches, writes their durations in
 * milliseconds in launch order (at most `capacity`), stores how many there were in *count and disarms.   */
int clslam_conv_profile_begin(int max_launches);
int clslam_conv_profile_end(float* ms, int capacity, int* count);

/* ---------------------------------------------------------------------------------------------
 * Cross-stream hand-off without a marker packet on the PRODUCER's stream (no reference counterpart: the reference
 * has one stream).  The step's dependency chain (decoder forward, data-gradient chain of the backward) releases work to
 * the side streams ~17 times per step; hipEventRecord() puts a barrier packet between two kernels of the chain every
 * time (measured on MI355X / ROCm 7.2, tools/micro/event_gap.hip: +5.0 us per hand-off on the producer), while an event
 * that IS the producing kernel's completion signal (hipExtLaunchKernel stopEvent) costs +1.3 us.
 *   clslam_handoff_arm(ev):   the next clslam_conv2d / clslam_fold_act_grad launch of THIS host thread completes `ev`
 *   clslam_handoff_wait(ev, producer, consumer):  `consumer` stream waits for `ev`; if no launch has taken the armed
 *                             event since clslam_handoff_arm (an op that does not support it, an empty batch) it is
 *                             recorded on `producer` first -- never a missing dependency.
 * Events come from clslam_handoff_event_create (timing disabled) and may be re-armed once waited on.  Arming while another
 * event is still armed (its launch failed before it went out) replaces that event: the stale one was never recorded.     */
void* clslam_handoff_event_create(void);
void clslam_handoff_event_destroy(void* event);
int clslam_handoff_arm(void* event);
int clslam_handoff_wait(void* event, void* producer_stream, void* consumer_stream);

/* ---------------------------------------------------------------------------------------------
 * Exact inner-product search = what the reference asks of faiss's
 * index_factory(d, 'Flat', METRIC_INNER_PRODUCT): loop_closure_detection/loop_closure_detection.py:35-36
 * (.add :48, .reconstruct/.search(features, 100) :55-57) and slam/replay_buffer.py:96-98 (.search(f, 1) :110,
 * .search(features, ntotal) :121-122,130).  Rows are L2-normalised by the caller (faiss.normalize_L2).
 * clslam_ip_scores: scores[q][i] = <db[i], queries[q]>, db (n,d) / queries (nq,d) / scores (nq,n) row-major.
 * clslam_topk_desc: the k largest per query in descending order, equal scores by ascending position;
 * out_val/out_idx (nq,k), missing entries -FLT_MAX / -1 like faiss.  n > 4096 needs cand_val/cand_idx of
 * nq * clslam_topk_chunks(n) * k elements (and chunks * k <= 4096).                                  */
int clslam_ip_scores(const float* db, const float* queries, float* scores, int n, int d, int nq, void* stream);
int clslam_topk_chunks(int n);
int clslam_topk_desc(const float* scores, int n, int nq, int k, float* cand_val, int* cand_idx, float* out_val,
                     int* out_idx, void* stream);
/* faiss.normalize_L2 on device rows (loop_closure_detection.py:47, replay_buffer.py:102,215): x_i *= 1/sqrt(<x_i,x_i>),
 * zero rows untouched. */
int clslam_l2_normalize_rows(float* x, int n, int d, void* stream);
/* One candidate of the replay buffer's diversity bookkeeping (slam/replay_buffer.py:104-152, maximize_diversity):
 * db (max_slots,d) vectors and sim (ld,ld) similarity matrix in SLOT order, occupied[max_slots] flags, `scores`
 * = clslam_ip_scores(db, query) over the first nslots slots.  Accepts the candidate when its largest similarity to
 * an occupied slot is < threshold (0 for an empty buffer), writes it to the first free slot (or slot nslots) with
 * its row/column of sim, and when more than `capacity` slots are occupied evicts argmax_j(sum_i sim[i][j] -
 * sim[j][j]) (row/column set to -1, slot freed).  result[5] = {accepted, slot written, slot evicted, occupied
 * count, bits of the nearest similarity}; similarity[0] = the nearest stored similarity as a float.  One workgroup; no host decision between the steps. */
int clslam_diversity_commit(float* db, float* sim, int ld, unsigned char* occupied, int nslots, int max_slots, int d,
                            int capacity, float threshold, const float* query, const float* scores, int* result,
                            float* similarity, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Image-pyramid ingest: the reference's datasets resize every pyramid level from the
 * previous one with torchvision.transforms.Resize(LANCZOS) on PIL images (datasets/utils.py:62-66,154-163)
 * = Pillow's ImagingResample 8-bit path, then ToTensor (datasets/utils.py:213-215).  Bit-exact on uint8.
 * clslam_lanczos_plan is a HOST function (double precision + libm, as Pillow): bounds[out][2] = (first tap,
 * tap count), coeffs[out][clslam_lanczos_ksize] 22-bit fixed point.  clslam_resize_pass_u8 runs one
 * separable pass on interleaved uint8 images (B,in_h,in_w,ch<=4) on the device: axis 1 = width -> out_size,
 * axis 0 = height -> out_size (Pillow's order: horizontal first); planar != NULL additionally writes
 * ToTensor(result) as float (B,ch,oh,ow).  clslam_u8_to_planar_f32 is ToTensor alone.                 */
int clslam_lanczos_ksize(int in_size, int out_size);
int clslam_lanczos_plan(int in_size, int out_size, int* bounds, int* coeffs);
int clslam_resize_pass_u8(const unsigned char* src, unsigned char* dst, float* planar, const int* bounds, const int* coeffs,
                          int ksize, int batch, int in_h, int in_w, int ch, int out_size, int axis, void* stream);
int clslam_u8_to_planar_f32(const unsigned char* src, float* planar, int batch, int h, int w, int ch, void* stream);
/* Colour augmentation of the datasets (datasets/utils.py:236-259: torchvision adjust_brightness / _contrast /
 * _saturation / _hue on PIL images, in the order drawn by random.shuffle) with Pillow's exact arithmetic, bit-
 * exact on uint8 RGB (B,h,w,3).  order[n_ops] (0 brightness, 1 contrast, 2 saturation, 3 hue) and factors[4]
 * (doubles as Python draws them, indexed by op id) are HOST arrays; scratch = second image buffer, lsum = batch uint64 device scratch.  */
int clslam_color_jitter_u8(const unsigned char* src, unsigned char* dst, unsigned char* scratch, unsigned long long* lsum,
                           int batch, int h, int w, const int* order, int n_ops, const double* factors, void* stream);

/* The replay buffer's colour jitter (slam/replay_buffer.py:264-265,281-283, enabled by slam/slam.py:98): torchvision's TENSOR code path
 * (transforms/functional_tensor.py 0.11.1: adjust_brightness / _contrast / _saturation / _hue of float images in [0,1]) applied AFTER
 * ToTensor, one drawn transform per replayed sample for its three frames and four scales.  src / dst: n_images planar (3,h,w) float
 * images of one size (dst may be src); params: n_images device records {int32 order[4] (op ids 0 brightness, 1 contrast, 2 saturation,
 * 3 hue in application order, -1 = end); float factor[4] (by op id); float one_minus_factor[4] ((float)(1.0 - factor), formed in
 * double like torch does)} = 48 bytes each; partial: n_images * clslam_color_jitter_f32_blocks(h,w) floats of scratch (the
 * per-image mean gray value of `contrast`, summed in a fixed order).  PARITY UNPINNED against real torchvision (source absent).   */
int clslam_color_jitter_f32_blocks(int h, int w);
int clslam_color_jitter_f32(const float* src, float* dst, const void* params, float* partial, int n_images, int h, int w,
                            void* stream);

/* Frame store: replayed samples kept as bytes in device memory instead of being rebuilt from their image files.  The sample that
 * ReplayBuffer.add receives (slam/replay_buffer.py:82-184) already holds the un-augmented pyramid `_get` builds later
 * (replay_buffer.py:270-279 = datasets/kitti.py:249-259, datasets/utils.py:154-171: Image.open -> LANCZOS level from level ->
 * ToTensor), every value fl32(b / 255) of a byte b.  One SLOT of the store holds one sample: per frame and per level a planar
 * (3, h, w) uint8 block at a fixed offset (a multiple of 16 bytes) inside the slot; table index = frame * n_levels + level.
 *
 * clslam_store_pack (one launch per sample) replaces nothing of the reference -- it is what lets the two entries below skip
 * replay_buffer.py:268-279: plane[k] = the 3 * h * w floats of table entry k (device memory), written to slot + offset[k] as
 * b = (unsigned char)rintf(x * 255); *inexact (device counter) grows by the number of values with (float)b / 255.f != x, which
 * stays 0 for planes a dataset built.
 *
 * clslam_store_gather_jitter replaces, for samples in the store, replay_buffer.py:268-285 (pickle + Image.open + resize chain +
 * ToTensor + colour jitter): image i (sample i / n_frames, frame i % n_frames) is read from slot slot_idx[i] (device array of
 * n_images entries; < 0 or >= capacity: the image is skipped, its rows stay untouched) and written to row row0 + i / n_frames of
 * the caller's (rows, 3, h, w) batch tensors: rgb[k] = byte / 255 (clslam_u8_to_planar_f32's arithmetic), aug[k] = the chain of
 * clslam_color_jitter_f32 on it with params[i] (same 48-byte records), BITWISE what that entry point returns for the same
 * bytes (same partition and order of the contrast mean's sum).  aug[k] == NULL: no jitter for that entry (params, partial may
 * then be NULL).  stride[k]: floats between two rows of entry k.  partial: n_levels * n_images * 64 floats of scratch.  Two
 * launches for all images and levels.                                                                                        */
#define CLSLAM_STORE_MAX_PLANES 16
typedef struct clslam_store_pack_desc {
    const float* plane[CLSLAM_STORE_MAX_PLANES];
    int32_t offset[CLSLAM_STORE_MAX_PLANES]; /* bytes from the slot's start */
    int32_t count[CLSLAM_STORE_MAX_PLANES];  /* 3 * h * w */
    int32_t n_planes;
} clslam_store_pack_desc;
typedef struct clslam_store_gather_desc {
    float* rgb[CLSLAM_STORE_MAX_PLANES];
    float* aug[CLSLAM_STORE_MAX_PLANES];
    int64_t stride[CLSLAM_STORE_MAX_PLANES];
    int32_t offset[CLSLAM_STORE_MAX_PLANES];
    int32_t h[CLSLAM_STORE_MAX_PLANES], w[CLSLAM_STORE_MAX_PLANES]; /* by level */
    int32_t n_frames, n_levels, capacity;                          /* capacity: slots in the store */
    int64_t slot_bytes;
} clslam_store_gather_desc;
int clslam_store_pack(const clslam_store_pack_desc* desc, unsigned char* slot, unsigned long long* inexact, void* stream);
int clslam_store_gather_jitter(const clslam_store_gather_desc* desc, const unsigned char* store, const int* slot_idx,
                               const void* params, float* partial, int n_images, int row0, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Loop-closure feature encoder: MobileNetV3-small forward (loop_closure_detection/encoder.py:13-33:
 * torchvision mobilenet_v3_small cut at 'flatten', ImageNet mean/std normalisation).  The 1x1 convs
 * run through clslam_conv2d (channels zero-padded to multiples of 16); these are the other ops.
 * PARITY UNPINNED: torchvision's source/weights are not available to the build. */
/* normalise + conv3x3 s2 p1 (3->16) + BN + hardswish; img planar (B,3,h,w), weight OIHW (16,3,3,3) */
int clslam_mbv3_stem(const float* img, const float* weight, const float* scale, const float* shift, float* out,
                     int batch, int h, int w, void* stream);
/* depthwise k x k (3|5), stride 1|2, pad k/2, NHWC, weight [k*k][ch], BN scale/shift, activation   */
int clslam_dwconv(const float* x, const float* weight, const float* scale, const float* shift, float* out, int batch,
                  int h, int w, int ch, int ksize, int stride, int act, void* stream);
/* out[b][c] = mean over pixels of x[b][p][c]                                                      */
/* partial (optional): batch * clslam_avgpool_chunks(hw) * ch floats -- two-stage reduction over pixel chunks
 * (deterministic order); NULL = one block per (sample, 64 channels).                                  */
int clslam_avgpool_chunks(int hw);
int clslam_global_avgpool(const float* x, float* out, float* partial, int batch, int hw, int ch, void* stream);
/* squeeze-excitation gates: gate[b][c] = hardsigmoid(w2 * relu(w1 * pool[b] + b1) + b2)            */
int clslam_se_gate(const float* pool, const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                   int batch, int ch, int squeeze, void* stream);
/* x[b][p][c] *= gate[b][c] (in place)                                                             */
int clslam_channel_scale(float* x, const float* gate, int batch, int hw, int ch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SE(3) pose-graph optimisation, fp64 (csrc/pose_graph.hip; conventions in its header): the g2o back end of the reference
 * (slam/pose_graph_optimization.py:1-35,55-77 g2o.SparseOptimizer + BlockSolverSE3 + OptimizationAlgorithmLevenberg over
 * VertexSE3 / EdgeSE3; slam/slam.py:110-115,203-216,241-246 add_vertex / add_edge / optimize(max_iterations=10000)).  The
 * Levenberg control runs on the host (clslam_hip/pose_graph.py).  All pointers are device memory; poses are row-major 4x4
 * doubles indexed by vertex SLOT, edge_v = int32 (from, to) slot pairs, info = the symmetrised 6x6 information matrices,
 * huber_delta[e] <= 0 = no robust kernel.  No floating-point atomics: every result is bitwise reproducible.
 * clslam_pgo_edge_eval: err[ne][6] = toVectorMQT(Z^-1 Xi^-1 Xj), jac_i / jac_j[ne][6][6] = d err / d increment of from / to.
 * clslam_pgo_build_system: linearise every edge into lin[ne][clslam_pgo_lin_stride()], then the block-CSR H (nnzb 6x6 blocks;
 *   block q = sum of the per-edge blocks contrib[cptr[q] .. cptr[q+1]), code = edge*4 + {0 Hii, 1 Hjj, 2 Hij, 3 Hij^T}) and
 *   b[na][6] (from the contributions of the diagonal blocks diag[na]); scal[0] = max diag(H).
 * clslam_pgo_solve: (H + lambda I) delta = -b by PCG in one workgroup, block-tridiagonal preconditioner over consecutive active
 *   rows (tri[na][3] = block index of (k,k-1), (k,k), (k,k+1), -1 = none), factored by block cyclic reduction; stop at relative
 *   residual <= tol or max_iter; work = clslam_pgo_solve_workspace(na) doubles.  scal[1] CG iterations, [2] relative residual,
 *   [3] delta^T (lambda delta - b), [5] 1 if the preconditioner was singular.
 * clslam_pgo_update_score: trial = est * exp(delta[act[v]]) for act[v] >= 0, est elsewhere (delta NULL: score est itself);
 *   scal[out_index] = sum over edges of Huber rho(e^T info e) (robust = 0: plain e^T info e).                            */
int clslam_pgo_edge_eval(const double* est, const int* edge_v, const double* meas, int ne, double* err, double* jac_i,
                         double* jac_j, void* stream);
int clslam_pgo_lin_stride(void);
int clslam_pgo_build_system(const double* est, const int* edge_v, const double* meas, const double* info, const double* huber_delta,
                            int ne, const int* cptr, const int* contrib, const int* diag, int nnzb, int na, double* lin, double* H,
                            double* b, double* scal, void* stream);
int clslam_pgo_solve_workspace(int na);
int clslam_pgo_solve(const double* H, const int* rptr, const int* col, const int* tri, const double* b, double lambda, int na,
                     double tol, int max_iter, double* delta, double* work, double* scal, void* stream);
int clslam_pgo_update_score(const double* est, double* trial, const int* act, int nv, const double* delta, const int* edge_v,
                            const double* meas, const double* info, const double* huber_delta, int ne, int robust, double* scal,
                            int out_index, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Depth-error metrics (csrc/depth_eval.hip).  Replaces slam/utils.py:389-442 (calc_depth_error: cv2.resize, mask, np.median
 * scaling, clamp, the eight np.mean metrics) and the same arithmetic at dpp.py:396-440 inside compute_depth_error, including
 * disp_to_depth(disp, min_depth, None) of dpp.py:405-406 (CLSLAM_DEPTH_EVAL_FROM_DISP: every tap is min_depth / disp BEFORE
 * the interpolation -- the reference resizes depth).
 * pred (n,h,w), gt (n,hg,wg) fp32 planes.  Per image: the prediction is resampled at the ground-truth pixels by OpenCV's
 * INTER_LINEAR rule for float images (source coordinate (d + 0.5) * (src / dst) - 0.5, scale in double, narrowed to float;
 * border cells with fraction 0; horizontal pass first; an equal-size resample is the identity); mask = gt > min_depth [and
 * gt < max_depth]; with MEDIAN_SCALING the prediction is multiplied by median(gt) / median(pred) over the masked pixels (exact
 * order statistics, np.median's mean of the two middle elements for even counts), then clamped to [min_depth, max_depth].
 * out (n,10) = [abs_diff, abs_rel, sq_rel, a1, a2, a3, rmse, rmse_log, ratio (1 without scaling), count of masked pixels];
 * an image without masked pixels gets NaN in the first nine and 0.  Bitwise reproducible (no floating-point atomics).
 * scratch: clslam_depth_metrics_scratch(n, hg, wg) 4-byte words (0 = geometry out of range: a plane is at most 2^24 pixels),
 * 8-byte aligned, contents irrelevant.  Optional outputs for tests and tools: resampled (n,hg,wg), the resampled prediction
 * (0 outside the mask); medians (n,2) = [median gt, median pred] (0 without scaling, NaN for an empty mask).               */
#define CLSLAM_DEPTH_EVAL_MEDIAN_SCALING 1
#define CLSLAM_DEPTH_EVAL_FROM_DISP 2
#define CLSLAM_DEPTH_EVAL_NO_MAX 4 /* max_depth is None: no upper mask bound, no upper clamp */
int clslam_depth_metrics_scratch(int n_images, int hg, int wg);
int clslam_depth_metrics(const float* pred, const float* gt, float* out, void* scratch, float* resampled, float* medians,
                         int n_images, int h, int w, int hg, int wg, float min_depth, float max_depth, int flags, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense mapping (csrc/mapping.hip).  A cloud is (M,6) fp32 rows [x, y, z, r, g, b], 8-byte aligned.  No floating-point atomics:
 * two launches agree bitwise.  Every product and sum named below is rounded on its own (no fma).
 *
 * clslam_pcl_backproject replaces slam/utils.py:25-38 (depth_to_pcl) with BackprojectDepth.forward (layers.py:74-79) in front:
 * depth (n,1,h,w), inv_k (n,4,4), image (n,3,h,w) fp32.  Pixel (x, y) of image i, in row-major order (meshgrid 'xy' flattened),
 * gives cam = depth * ((inv_k[r][0] * x + inv_k[r][1] * y) + inv_k[r][2]) for r = 0..2, in fp32, and the row [cam, r, g, b].
 * It is kept iff sqrt((cx*cx + cy*cy) + cz*cz) < dist_threshold in fp32 (utils.py:35-37; a NaN norm is dropped), or
 * dist_threshold is infinite (np.isinf: keep all); a NaN threshold is an error.  The kept rows of all images follow each other
 * in `points` in image and pixel order (the order-preserving compaction of the reference's boolean mask; count -> scan ->
 * ordered write, no atomic cursor); offsets (n+1) int64 on the device: image i owns rows [offsets[i], offsets[i+1]).  `points`
 * must have room for n*h*w rows.  scratch: clslam_pcl_backproject_scratch(n, h, w) 8-byte words (0 = out of range: 1..65535
 * images, planes of at most 2^30 pixels), contents irrelevant.
 *
 * clslam_pcl_transform replaces slam/utils.py:76-82 (accumulate_pcl): segment f = rows [offsets[f], offsets[f+1]) of `points`
 * (offsets (n_segments+1) int64, non-decreasing, offsets[n_segments] = m; empty segments allowed) is posed by poses[f] (4x4
 * row-major fp64): xyz' = ((R0*x + R1*y) + R2*z) + t per row of the matrix, in fp64 from the fp32 coordinates, rounded once to
 * fp32 (the reference's pcl[:, :3] @ tmat.T, float64 because the poses are); the colours are copied.  out may be `points`.
 *
 * clslam_pcl_splat + clslam_pcl_resolve replace slam/utils.py:41-58 (pcl_to_image: cv2.projectPoints with zero rotation,
 * translation and distortion, restated from OpenCV's source, and the per-point Python loop).  Points [point_base, point_base +
 * count) of `points`, count <= 2^32; with poses != NULL each is first posed as by clslam_pcl_transform (including the rounding
 * to fp32; offsets index the whole cloud).  Then in fp64: zi = z != 0 ? 1/z : 1; u = (x*zi)*fx + cx; v = (y*zi)*fy + cy with
 * fx = K[0], cx = K[2], fy = K[4], cy = K[5] of the 3x3 row-major fp64 K on the device; the pixel is (floor(u), floor(v)) and the
 * point is skipped unless 0 <= floor(v) < rows and 0 <= floor(u) < cols.  Points behind the camera are projected mirrored (the
 * reference's behaviour); has_min_z culls z <= min_z instead.  A point with a non-finite coordinate is skipped (the reference
 * raises on int(nan)).  zbuf (rows*cols 64-bit words, clslam_pcl_splat_scratch; `clear` fills it with all-ones first) takes the
 * minimum of (bits of (float)sqrt((x*x + y*y) + z*z)) << 32 | (index - point_base) by 64-bit integer atomicMin: the closest
 * point by Euclidean distance (utils.py:54), the lowest index among equal distances (the strict < of :55 in loop order).
 * clslam_pcl_resolve: image (rows,cols,3) = the winner's colour, 0 where empty (:48); optional dist (rows,cols) = its distance,
 * +inf where empty; optional index (rows,cols) int64 = its row in `points`, -1 where empty.  merge != 0 (needs dist): the planes
 * hold the result of earlier launches over lower indices and change only where this launch's winner is strictly closer -- how a
 * cloud of more than 2^32 points is rendered in several launches.
 *
 * clslam_pcl_voxel_sort + clslam_pcl_voxel_reduce: the voxel-grid filter, one row per occupied cell.  points (m,6), 1 <= m < 2^31;
 * with poses != NULL each point is first posed as by clslam_pcl_transform (including the rounding to fp32), so the result equals
 * that of the filter on the transformed cloud bitwise.  voxel_size: finite, > 0.  Per axis the cell index is
 * floor((double)c / voxel_size): one IEEE fp64 division and one floor.  A row with a non-finite value among its six (a NaN pose
 * makes its whole segment such) is dropped.  A row with an index outside [-2^20, 2^20 - 1] is dropped and counted: an error for
 * the caller to raise.  key = (iz + 2^20) << 42 | (iy + 2^20) << 21 | (ix + 2^20); the cells come out in ascending key order, those
 * with at least min_points (>= 1) members only.  clslam_pcl_voxel_sort forms the keys, sorts (key, point index) by a stable LSD
 * radix sort of 4-bit digits that skips the digits in which all keys agree, and lists the first position of every kept cell.  It
 * leaves four 64-bit words at scratch + 16 bytes: the number of kept cells, the rows with an index out of range, the radix passes
 * run, the rows dropped (the out-of-range ones included).  The caller reads them back, allocates, and calls
 * clslam_pcl_voxel_reduce with n_cells = the first word and the SAME points, offsets, poses and scratch: rows (n_cells,6) fp32 =
 * per value the fp64 sum of the members' fp32 values divided by their number in fp64, rounded once to fp32; counts (n_cells)
 * int32.  The members are added in an order that depends on their number and their point indices alone (no floating-point
 * atomics): two calls agree bitwise.  scratch: clslam_pcl_voxel_scratch(m) 8-byte words (0 = m out of range), 16-byte aligned:
 * 24 bytes per point (two key and two index buffers) + 1/16 byte per point of histograms + 192 bytes.                          */
int clslam_pcl_backproject_scratch(int n_images, int h, int w);
int clslam_pcl_backproject(const float* depth, const float* inv_k, const float* image, float* points, long long* offsets,
                           void* scratch, int n_images, int h, int w, float dist_threshold, void* stream);
int clslam_pcl_transform(const float* points, const long long* offsets, const double* poses, float* out, long long m,
                         int n_segments, void* stream);
int clslam_pcl_splat_scratch(int rows, int cols);
int clslam_pcl_splat(const float* points, const long long* offsets, const double* poses, int n_segments, const double* K,
                     unsigned long long* zbuf, int rows, int cols, long long point_base, long long count, int has_min_z,
                     double min_z, int clear, void* stream);
int clslam_pcl_resolve(const float* points, const unsigned long long* zbuf, long long point_base, float* image, float* dist,
                       long long* index, int rows, int cols, int merge, void* stream);
size_t clslam_pcl_voxel_scratch(long long m);
int clslam_pcl_voxel_sort(const float* points, const long long* offsets, const double* poses, int n_segments, long long m,
                          double voxel_size, int min_points, void* scratch, void* stream);
int clslam_pcl_voxel_reduce(const float* points, const long long* offsets, const double* poses, int n_segments, long long m,
                            const void* scratch, float* rows, int* counts, long long n_cells, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Trajectory and pose-error metrics (csrc/traj_eval.hip).  Poses are (n,4,4) row-major fp64 on the device, all arithmetic is
 * double, every reduction runs in a fixed order (no floating-point atomics: two launches agree bitwise).  Every 4x4 inverse is
 * a GENERAL inverse (LU with partial pivoting), as np.linalg.inv is in the reference: the rotation blocks need not be
 * orthonormal.  A singular matrix gives non-finite results.  rotation_error(m) = acos(clamp(0.5 * (m00 + m11 + m22 - 1), -1, 1))
 * (slam/utils.py:191-203), translation_error(m) = sqrt(m03^2 + m13^2 + m23^2) (utils.py:206-217).
 *
 * clslam_pose_pair_error: out (n,2) = [translation_error, rotation_error (rad)] of inv(b_i) @ (a_inverted ? inv(a_i) : a_i).
 * a_inverted = 0 is slam.py:257-259 (a = the predicted transformation, b = the ground truth); a_inverted = 1 is dpp.py:505-511
 * (compute_pose_error inverts the prediction first).  n = 0 is a no-op.
 *
 * clslam_traj_metrics replaces slam/utils.py:129-383 (calc_error and everything it calls) for n <= CLSLAM_TRAJ_MAX_POSES poses:
 * out (8) = [ave_t_err, ave_r_err, n_segments, ate, rpe_trans, rpe_rot, scaling, path_length].
 *   dist[i] = the path length of gt up to pose i (utils.py:164-172; a hierarchical sum, serial at every level: non-decreasing).
 *   Segments (utils.py:220-250): for every first_frame = 0, 10, 20, ... < n and length = 100, 200, ..., 800 m, last_frame = the
 *   first i >= first_frame with dist[i] > dist[first_frame] + length; pose_error = inv(inv(pred[first]) @ pred[last]) @
 *   (inv(gt[first]) @ gt[last]).  ave_t_err / ave_r_err = the means of translation_error / length and rotation_error / length
 *   over the segments that have a last frame, (0, 0) when none has (utils.py:292-314); n_segments = their number.
 *   ate = sqrt(mean |gt_xyz - pred_xyz|^2) (utils.py:317-328; NaN for n = 0).  rpe_trans / rpe_rot = the means over i < n-1 of
 *   the two errors of inv(inv(gt[i]) @ gt[i+1]) @ (inv(pred[i]) @ pred[i+1]) (utils.py:331-354; NaN for n < 2).
 *   scaling = sum(pred_xyz * gt_xyz) / sum(pred_xyz^2) (utils.py:151-161), always reported (NaN for n = 0); both sums are added
 *   in the order np.sum adds the contiguous (n,3) arrays (numpy's pairwise summation inside each piece of 8192 elements, the
 *   pieces one after the other; products rounded on their own), so the
 *   factor is the reference's to the last bit -- calc_error prints all its digits.  With optimize_scale != 0 the
 *   translations of pred are multiplied by it for the SEGMENT errors only; ate and rpe use pred as given (utils.py:374,378).
 *   path_length = dist[n-1].
 * Optional outputs: segments (ceil(n/10)*8, 6), one row per (first_frame, length) in the reference's loop order:
 * [first_frame, rotation_error / length, translation_error / length, length, speed = length / (0.1 * (last - first + 1)),
 * last_frame]; a segment without a last frame has last_frame = -1 and NaN in the two errors and the speed.  dist (n).
 * scratch: clslam_traj_metrics_scratch(n) doubles (0 = n out of range), 8-byte aligned, contents irrelevant on entry; after the
 * call its doubles [8, 8 + 2n) hold, for tests and tools, the rows [translation_error, rotation_error] of the RPE pair
 * (i, i+1) (zeros in row n-1).                                                                                                  */
#define CLSLAM_TRAJ_MAX_POSES (1 << 20)
int clslam_pose_pair_error(const double* a, const double* b, int n, int a_inverted, double* out, void* stream);
int clslam_traj_metrics_scratch(int n);
int clslam_traj_metrics(const double* pred, const double* gt, int n, int optimize_scale, double* out, double* segments,
                        double* dist, double* scratch, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Online ingest: the sample the driver takes from its DataLoader in front of every frame (slam/slam.py:141), assembled from a
 * ring of per-frame uint8 pyramids in device memory.  A ring SLOT holds one frame: per level an INTERLEAVED (h, w, 3) uint8 image
 * at a fixed byte offset.
 *
 * clslam_resize_level_u8 replaces one Resize(LANCZOS) of datasets/kitti.py:258 / datasets/utils.py:163 (one pyramid level from the
 * raw frame or from the level above) in ONE launch: src (batch, in_h, in_w, 3) contiguous -> dst (batch, out_h, out_w, 3) with
 * dst_pitch bytes between rows (>= out_w * 3; the bytes between two rows are not touched; image n starts at n * out_h *
 * dst_pitch).  Both Pillow passes run in the kernel, the horizontal one into a uint8 tile in LDS: BITWISE what
 * clslam_resize_pass_u8 (axis 1) followed by clslam_resize_pass_u8 (axis 0) writes.  bounds_* / coeffs_* / ksize_*: the device
 * copies of clslam_lanczos_plan(in_w, out_w) and (in_h, out_h); an axis whose size does not change takes no pass and its tables
 * are not read (may be NULL): in_w == out_w is the vertical pass alone, in_h == out_h the horizontal one, both a copy.  ch must
 * be 3.
 *
 * clslam_ring_gather replaces the ToTensor of datasets/kitti.py:345-347 (datasets/utils.py:213-215) for the 2 * n_frames *
 * n_levels image entries of one sample, in ONE launch: frame f lives in slot[f] (HOST values, each in [0, capacity)), level l at
 * offset[l] bytes inside the slot with h[l] x w[l] pixels; rgb[f * n_levels + l] and aug[f * n_levels + l] (distinct, contiguous
 * (3, h, w) float planes) both receive (float)byte / 255.f, clslam_u8_to_planar_f32's expression.                              */
typedef struct clslam_ring_gather_desc {
    float* rgb[CLSLAM_STORE_MAX_PLANES];
    float* aug[CLSLAM_STORE_MAX_PLANES];
    int64_t offset[CLSLAM_STORE_MAX_PLANES];                        /* by level */
    int32_t h[CLSLAM_STORE_MAX_PLANES], w[CLSLAM_STORE_MAX_PLANES]; /* by level */
    int32_t slot[CLSLAM_STORE_MAX_PLANES];                          /* by frame */
    int32_t n_frames, n_levels, capacity;                           /* capacity: slots in the ring */
    int64_t slot_bytes;
} clslam_ring_gather_desc;
int clslam_resize_level_u8(const unsigned char* src, unsigned char* dst, long long dst_pitch, const int* bounds_h,
                           const int* coeffs_h, int ksize_h, const int* bounds_v, const int* coeffs_v, int ksize_v, int batch,
                           int in_h, int in_w, int ch, int out_h, int out_w, void* stream);
int clslam_ring_gather(const clslam_ring_gather_desc* desc, const unsigned char* ring, void* stream);

/* ---------------------------------------------------------------------------------------------
 * RobotCar raw frames (csrc/robotcar.hip): stereo/centre/<timestamp>.png is a one-channel Bayer mosaic seen through a distorting lens,
 * and the reference reads it only after its offline pass (datasets/robotcar.py:493-548, undistort_images / _load_image) has
 * rewritten the sequence.  Images are contiguous, channels LAST; a launch takes n frames of one size.
 *
 * clslam_demosaic_bilinear replaces colour_demosaicing.demosaicing_CFA_Bayer_bilinear (robotcar.py:544): cfa (n,h,w) uint8 ->
 * out (n,h,w,3) float64, R = conv(CFA * R_m, H_RB), G = conv(CFA * G_m, H_G), B = conv(CFA * B_m, H_RB), H_G = [[0,1,0],[1,4,1],
 * [0,1,0]] / 4, H_RB = [[1,2,1],[2,4,2],[1,2,1]] / 4, with mask[c][y::2, x::2] = 1 for (c, (y, x)) in zip(pattern, [(0,0), (0,1),
 * (1,0), (1,1)]).  Every value is a multiple of 1/4: the result does not depend on the order of the sum.  BORDER: scipy.ndimage.
 * convolve's default 'reflect' (d c b a | a b c d) on the masked planes.  This rule is RESTATED from the libraries' documentation
 * and was NOT COMPARED against colour_demosaicing (not installed where this was written; so was cv2.resize for the depth
 * metrics); only the outermost pixel ring depends on it, and there the result can exceed 255.  n <= 65535.
 *
 * clslam_undistort_lut replaces CameraModel.undistort (robotcar.py:617-642; one scipy.ndimage.map_coordinates(order=1,
 * mode='constant', cval=0) per channel): image, out (n,h,w,c) uint8 (is_f64 = 0) or float64 (is_f64 = 1), distinct; lut (2,h,w)
 * float64 = (row, col) of the source sample of every output pixel, shared by the n frames and read once per element, not once
 * per frame.  Inside iff 0 <= row <= h-1 and 0 <= col <= w-1, else 0.  r0 = floor(row), sy = 1 - (row - r0), ty = 1 - sy (the
 * library's last weight is one minus the others, not row - r0 again), second tap clamped to h-1 (weight 0 there), the same for
 * col;  t = 0; t += (v00*sy)*sx; t += (v01*sy)*tx; t += (v10*ty)*sx; t += (v11*ty)*tx, every operation rounded on its own: scipy's
 * float64 to the last bit.  uint8 output = (int64)t & 255 (truncation
 * toward zero, then the low byte; the reference's astype(np.uint8) of a value above 255 is platform-defined).
 *
 * clslam_robotcar_rectify replaces _load_image(path, model) (robotcar.py:522-548) for n raw frames in ONE launch: cfa (n,h,w) uint8
 * -> out (n,h,w,3) uint8 = clslam_undistort_lut(clslam_demosaic_bilinear(cfa)) converted as above, byte for byte, with the four
 * demosaiced taps of a pixel formed in registers: no float64 image is written.  The table is read once per pixel.
 *
 * h * w * channels <= 2^30.  n = 0 is a no-op.                                                                                  */
#define CLSLAM_BAYER_RGGB 0
#define CLSLAM_BAYER_BGGR 1
#define CLSLAM_BAYER_GRBG 2
#define CLSLAM_BAYER_GBRG 3
int clslam_demosaic_bilinear(const unsigned char* cfa, double* out, int n, int h, int w, int pattern, void* stream);
int clslam_undistort_lut(const void* image, const double* lut, void* out, int n, int h, int w, int c, int is_f64, void* stream);
int clslam_robotcar_rectify(const unsigned char* cfa, const double* lut, unsigned char* out, int n, int h, int w, int pattern,
                            void* stream);

/* ---------------------------------------------------------------------------------------------
 * PNG encoding on the device (csrc/png_encode.hip): n images of one size, uint8, contiguous, (n,h,w) (channels = 1, colour type 0)
 * or (n,h,w,3) (channels = 3, colour type 2), bit depth 8, bpp = channels -> one complete PNG file per image in a caller-allocated
 * device buffer, plus each file's length.  Nothing synchronises; only the n lengths and then the bytes need to reach the host.
 *
 * FILTER (clslam_png_filter).  filtered (n rows of filtered_stride bytes): image i is h scanlines of 1 + w*bpp bytes, the filter type
 * and then the filtered bytes (RFC 2083 section 6: None, Sub, Up, Average, Paeth; the row above row 0 and the bytes left of the first
 * pixel are 0).  filter = CLSLAM_PNG_FILTER_ADAPTIVE keeps, per row, the type with the smallest score sum(min(b, 256 - b)) over the
 * row's filtered bytes, ties to the LOWEST type; filter = 0..4 uses that type on every row.  One launch, one workgroup per row.
 *
 * DEFLATE (clslam_png_deflate) wraps such a filtered stream.  There is no LZ77 matching: the stream is cut into blocks of
 * S = CLSLAM_PNG_BLOCK = 16384 bytes (the last one shorter), and each block is either a DYNAMIC block of literals only -- the
 * length-limited (<= 15 bits) canonical Huffman code of its own histogram of the 256 literals + end-of-block: the optimal code
 * whenever an optimal code of depth <= 15 exists (the two-queue construction prefers leaves on ties, which gives the optimal tree
 * of least depth), else a complete code obtained by moving leaves down; HLIT = 257 codes, HDIST = 1 distance code of length 0
 * (= "literals only"), HCLEN = 19 with the sixteen code-length symbols 0..15 at 4 bits each and no run-length symbols, i.e. a
 * header of 1106 bits -- or a STORED block, whenever the dynamic form would not end before the stored form would at the block's
 * actual bit position.  The last block carries BFINAL.  S: 16 KiB keeps the block's histogram, code table and packed bits in
 * LDS, gives a 960x1280x3 frame 226 independent workgroups, and holds the header at under 1 % of the block.
 *
 * FILE.  signature, IHDR, ONE IDAT = zlib header 78 01 + the deflate stream + Adler-32 of the filtered stream, IEND.  Adler-32 is
 * combined from per-block (a, b) pairs, the IDAT CRC-32 from per-block remainders multiplied by x^(8 * bytes that follow) mod P.
 *
 * clslam_png_bound(h, w, channels): the worst-case file size.  F = h * (1 + w*channels) filtered bytes in B = ceil(F / S) blocks;
 * a block never ends later than its stored form would, and a stored form that starts at or before byte boundary b ends at or before
 * b + 5 + len (3 header bits and padding <= 1 byte further, LEN + NLEN 4 bytes, len bytes of data), so by induction the stream
 * is at most F + 5 B bytes; + 2 (zlib header) + 4 (Adler-32) + 57 (signature 8, IHDR 25, IDAT 12, IEND 12): F + 5 B + 63.  0 for
 * a geometry the library does not take.  out holds n files, file i at out + i * out_stride; out_stride >= the bound, a multiple of
 * 4, out 4-byte aligned (bits are added into zeroed 32-bit words); bytes of a row past lengths[i] are zero or untouched.
 * clslam_png_scratch(n, h, w, channels): bytes of 16-byte-aligned device scratch clslam_png_encode needs (clslam_png_deflate
 * needs no more).  filtered: 16-byte aligned, filtered_stride a multiple of 16 and >= F.
 *
 * h, w >= 1, channels 1 or 3, F <= 2^27, n <= 65535 (n = 0 is a no-op).  Bad arguments are refused before any launch.          */
#define CLSLAM_PNG_BLOCK 16384
#define CLSLAM_PNG_FILTER_ADAPTIVE (-1)
long long clslam_png_bound(int h, int w, int channels);
long long clslam_png_scratch(int n, int h, int w, int channels);
int clslam_png_filter(const unsigned char* image, unsigned char* filtered, long long filtered_stride, int n, int h, int w, int channels,
                      int filter, void* stream);
int clslam_png_deflate(const unsigned char* filtered, long long filtered_stride, unsigned char* out, long long out_stride, int* lengths,
                       void* scratch, long long scratch_bytes, int n, int h, int w, int channels, void* stream);
int clslam_png_encode(const unsigned char* image, unsigned char* out, long long out_stride, int* lengths, void* scratch,
                      long long scratch_bytes, int n, int h, int w, int channels, int filter, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Frame panels on the device (csrc/viz.hip): what slam/utils.py:85-121 generate_figure and dpp.py:1197-1244 save_prediction draw
 * with matplotlib -- the frame, the depth plane as magma_r up to its 95th percentile, the projected map, the x/z trajectory -- as
 * uint8 RGB pixels, without text, axes or legend.  Nothing synchronises and nothing is read back.
 *
 * RANGE (clslam_viz_range; replaces utils.py:100 / dpp.py:1224 `vmax = np.percentile(depth, 95)` and imshow's implicit vmin).
 * planes: n contiguous fp32 planes of npx values.  Only FINITE values take part, m of them (np.percentile would answer NaN).
 * They are ordered by the monotone 32-bit key of the float (sign bit flipped, or all bits flipped for a negative value; -0 below
 * +0), a[0..m-1].  range[2i] = vmin = a[0].  range[2i+1] = vmax: pos = q / 100 * (m - 1) in fp64, k = floor(pos), g = pos - k,
 * vmax = (float)((double)a[k] + ((double)a[min(k+1, m-1)] - (double)a[k]) * g), every fp64 operation rounded, no contraction.
 * The three order statistics are exact (a radix select of 8 bits per pass over the keys).  count[i] = m.  m = 0: vmin = vmax = NaN.
 * 0 <= q <= 100.  Launches: a memset, the digit-0 histogram, three selecting passes, one finishing block per plane.
 * clslam_viz_range_scratch(n): bytes of 8-byte-aligned device scratch for n planes (0: n out of range).
 *
 * COMPOSE (clslam_viz_compose).  One launch writes n_rows rows of h x w pixels, row r into the pixel rows
 * [row0 + r*h, row0 + (r+1)*h) and the columns [0, w) of image i of dst: byte (y, x, c) of image i is at
 * dst + i * dst_image_stride + y * dst_row_stride + 3 * x + c; nothing else of dst is written.  Row kinds:
 *   CHW_F32  (n,3,h,w) fp32 in [0,1]    HWC_F32 / HWC_F64 / HWC_U8  (n,h,w,3)      src_stride: elements between images.
 *            float -> byte: trunc(clamp(x, 0, 1) * 255 + 0.5) in the source's precision, each operation rounded; NaN -> 0
 *            (recovers b from (float)(b / 255.0), the frame store's rule); uint8 is copied.
 *   CMAP     (n,h,w) fp32 through a 256-entry table, matplotlib's arithmetic as Normalize and Colormap carry it out on a float32
 *            plane: r = (float)((double)x - vmin), t = (float)((double)r / ((double)vmax - vmin)) -- the divisor is the exact
 *            difference, the division the correctly rounded IEEE one -- xa = t * 256 in fp32; xa < 0 -> entry 0; xa >= 256 -> entry 255 (256 itself, and the
 *            "over" colour); else entry trunc(xa); x or xa NaN -> (0,0,0) (imshow's masked pixel); vmin == vmax -> entry 0 for
 *            every x that is not NaN (Normalize's rule).  +inf -> entry 255, -inf -> entry 0.  range: (n,2) {vmin, vmax} on the
 *            device, e.g. clslam_viz_range's.  cmap: MAGMA, or MAGMA_R = the same table read backwards;
 *            the table is matplotlib's magma lut * 255 truncated, [0 0 3] .. [251 252 191].
 *   TRAJ     a white row with two polylines of (x, y) fp64 vertices, 1 pixel wide, gt (31,119,180) and over it pred (255,127,14)
 *            (utils.py:113-116).  Vertex -> pixel in fp64: u = floor((x - xlim[0]) / (xlim[1] - xlim[0]) * w),
 *            v = floor((ylim[1] - y) / (ylim[1] - ylim[0]) * h), clamped to +-2^30, then 64-bit integers.  A segment (u0,v0)-(u1,v1)
 *            with n = max(|du|, |dv|) sets, for k = 0..n, the pixel (u0 + floor((2 k du + n) / (2 n)), v0 + floor((2 k dv + n) /
 *            (2 n))) (floor division; n = 0: that pixel); pixels outside the row are dropped.  A segment with a non-finite
 *            vertex is skipped, one vertex draws one pixel, none draws nothing.  k is clipped to the row before anything is
 *            drawn: the work per segment is bounded by the row's size, not by its length -- per BLOCK: every block of the row (a
 *            band of min(8, 8192 / w) pixel rows) walks all segments, so a row costs (h / band) * segments clip tests; meant
 *            for rows of a few hundred pixel rows.  The same polylines go into every image i.
 * 1 <= n_rows <= CLSLAM_VIZ_MAX_ROWS, n <= 65535 (n = 0 is a no-op), 1 <= h <= 2^24, 1 <= w <= CLSLAM_VIZ_MAX_W, h * w <= 2^30,
 * n_gt, n_pred <= 2^24, xlim / ylim finite with distinct ends.  Bad arguments are refused before any launch.                  */
#define CLSLAM_VIZ_MAX_ROWS 4
#define CLSLAM_VIZ_MAX_W 8192
#define CLSLAM_VIZ_ROW_CHW_F32 0
#define CLSLAM_VIZ_ROW_HWC_F32 1
#define CLSLAM_VIZ_ROW_HWC_F64 2
#define CLSLAM_VIZ_ROW_HWC_U8 3
#define CLSLAM_VIZ_ROW_CMAP 4
#define CLSLAM_VIZ_ROW_TRAJ 5
#define CLSLAM_VIZ_CMAP_MAGMA 0
#define CLSLAM_VIZ_CMAP_MAGMA_R 1
typedef struct clslam_viz_row {
    const void* src;         /* image / plane rows; unused by TRAJ */
    const float* range;      /* CMAP: (n,2) vmin, vmax */
    const double* gt_xz;     /* TRAJ: (n_gt,2), may be null when n_gt = 0 */
    const double* pred_xz;   /* TRAJ: (n_pred,2) */
    long long src_stride;
    double xlim[2], ylim[2]; /* TRAJ */
    int kind, cmap, n_gt, n_pred;
} clslam_viz_row;
long long clslam_viz_range_scratch(int n);
int clslam_viz_range(const float* planes, float* range, int* count, void* scratch, long long scratch_bytes, int n, long long npx,
                     double q, void* stream);
int clslam_viz_compose(const clslam_viz_row* rows, int n_rows, unsigned char* dst, long long dst_image_stride,
                       long long dst_row_stride, int row0, int n, int h, int w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLSLAM_HIP_H */
