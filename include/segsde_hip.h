/* segsde_hip.h -- C ABI of libsegsde_hip.so: hand-written gfx950 (MI355X) kernels for the joint
 * segmentation + self-supervised-depth training hot path of
 * lhoyer/improving_segmentation_with_selfsupervised_depth.
 *
 * Boundary rules
 *   - plain pointers + sizes; every pointer is DEVICE memory (the caller -- PyTorch-ROCm in the Python host
 *     layer -- owns allocation); no torch types; `stream` is a hipStream_t passed as void*; nothing syncs.
 *   - return 0 on success, a SEGSDE_ERR_* code (<0) for bad arguments, or a positive hipError_t.
 *   - activations are NHWC fp32 ("rows" = pixels, `ld*` = floats between consecutive pixels, which lets a
 *     tensor be a channel slice of a wider buffer); images / disparities of the loss path are NCHW planar
 *     fp32 exactly as the reference's data loader hands them over.
 *   - workspaces are caller-provided; `*_workspace()` return the bytes needed.
 *
 * The reference is pure Python on torch.nn; it has no FFI.  Each entry point therefore cites the reference
 * call site(s) whose ATen op sequence it replaces (paths relative to /root/reference).  The ctypes binding a
 * maintainer would add is shown in INTEGRATION.md and shipped in
 * improving_segmentation_with_selfsupervised_depth_amd/_lib.py.
 */
#ifndef SEGSDE_HIP_H
#define SEGSDE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEGSDE_ABI_VERSION 26

enum { SEGSDE_ERR_NULL = -1, SEGSDE_ERR_SHAPE = -2, SEGSDE_ERR_WORKSPACE = -3, SEGSDE_ERR_UNSUPPORTED = -4 };
enum { SEGSDE_ACT_NONE = 0, SEGSDE_ACT_RELU = 1, SEGSDE_ACT_ELU = 2, SEGSDE_ACT_SIGMOID = 3 };
enum { SEGSDE_DTYPE_F32 = 0, SEGSDE_DTYPE_I64 = 1, SEGSDE_DTYPE_U8 = 2 };
enum { SEGSDE_PAD_ZERO = 0, SEGSDE_PAD_REFLECT = 1, SEGSDE_PAD_REFLECT_ADJOINT = 2 };

int segsde_abi_version(void);

/* ------------------------------------------------------------------------------------------------ *
 * Convolutions (implicit GEMM on v_mfma_f32_32x32x2_f32)                                           *
 * ------------------------------------------------------------------------------------------------ */
typedef struct segsde_conv_desc {
  int B, H, W;      /* batch; spatial size of the (virtual) conv input: after the optional x2 upsample, before padding */
  int C0, C1;       /* channels of source 0 / source 1 (C1 = 0: single source); the conv sees [src0 | src1]           */
  int ld0, ld1;     /* pixel pitch (floats) of the two sources                                                          */
  int up0;          /* 1: source 0 is stored at (H/2, W/2) and nearest-upsampled x2 on the fly (depth_decoder.py:93-94) */
  int Ho, Wo, Cout; /* output size                                                                                       */
  int ldy, ldy2, nsplit; /* output pitch; optional second destination receiving channels >= nsplit (concat dgrad)       */
  int KH, KW, stride, dil, pad;
  int pad_mode;     /* SEGSDE_PAD_ZERO | SEGSDE_PAD_REFLECT (monodepth_layers.py:133-136) | SEGSDE_PAD_REFLECT_ADJOINT:
                       data-gradient of a reflection-padded 3x3/s1/p1 conv (x0 = dy, dgrad-packed weights, pad = 1)       */
  int in_div;       /* 1; >1 only for data-gradients of strided convs: input coordinate must divide by in_div          */
  int act;          /* fused epilogue activation applied after the bias: SEGSDE_ACT_*                                    */
  int sum2x2;       /* 1 (data-gradient through the x2 upsample): output channels < nsplit are summed over 2x2 pixel
                       blocks in registers and stored to y at (Ho/2, Wo/2); channels >= nsplit go to y2 per pixel.
                       Returns SEGSDE_ERR_UNSUPPORTED when the shape cannot take the fused path.                         */
  int accumulate;   /* 1: y += result instead of y = result (the gradient of a tensor with a second consumer -- a residual
                       block's input -- lands on the gradient that is already there; no separate add pass).  Single
                       destination, no activation; SEGSDE_ERR_UNSUPPORTED when the shape does not take the staged epilogue. */
  int compute;      /* 0: fp32 operands (exact fp32 products, the judged arithmetic).  1: the operands are rounded to fp16
                       inside the kernel and multiplied on v_mfma_f32_32x32x16_f16 with fp32 accumulation -- what
                       torch.cuda.amp.autocast makes of the reference's convolutions under `amp: True` (train.py:468,502).
                       2: split-bf16 operands -- every fp32 operand is split inside the kernel into three bf16 numbers whose sum
                       is the operand exactly (h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), round to nearest even) and the
                       product becomes nine bf16 x bf16 products, each exact in fp32, accumulated in fp32 by
                       v_mfma_f32_32x32x16_bf16: fp32 re-associated, not reduced precision.  A non-finite operand gives a
                       non-finite (NaN) result; operands below 2^-108 lose their low terms (bf16 underflow).
                       3: reserved for the six-product form (h.h, h.m, m.h, h.l, l.h, m.m; the dropped terms are <= 2^-24 of a
                       product each), which missed its error gate on the hardware: every entry point returns
                       SEGSDE_ERR_UNSUPPORTED for it.
                       Launches whose shape does not take the LDS-DMA loop compute in fp32 whatever this says
                       (segsde_conv_compute_taken tells).                                                                  */
} segsde_conv_desc;

/* The operand arithmetic (a value of segsde_conv_desc.compute) the launchers WILL use for d, from the predicates they dispatch
 * on.  direction: which entry point d is meant for -- SEGSDE_DIR_FORWARD / SEGSDE_DIR_DGRAD: segsde_conv2d_forward* /
 * segsde_conv2d_dgrad_actgrad (d as handed to that call), SEGSDE_DIR_WGRAD: segsde_conv2d_wgrad; | SEGSDE_DIR_UPFOLD: the
 * segsde_conv2d_*_upfold call of that direction (d: the forward geometry).  Evaluated for 16-byte aligned tensors with dense rows.
 * d->compute if every implicit-GEMM launch of the call takes it; 0 if any computes in fp32, the call takes another kernel
 * (the one-channel stencils) or rejects d.  Host only: nothing is launched. */
enum { SEGSDE_DIR_FORWARD = 0, SEGSDE_DIR_DGRAD = 1, SEGSDE_DIR_WGRAD = 2, SEGSDE_DIR_UPFOLD = 4 };
int segsde_conv_compute_taken(const segsde_conv_desc* d, int direction);
/* The operand split of the compute = 2 loops applied to an array (tests, probes): h[i], m[i], l[i] = the bf16 bit patterns with
 * float(h[i]) + float(m[i]) + float(l[i]) == x[i] exactly for finite x[i] of magnitude in [2^-108, 2^128 - 2^119). */
int segsde_split_bf16_planes(const float* x, long n, unsigned short* h, unsigned short* m, unsigned short* l, void* stream);

/* y[b,ho,wo,n] = act(bias[n] + sum_{kh,kw,c} x[b, ho*stride-pad+kh*dil, wo*stride-pad+kw*dil, c] * wpack[n][kh][kw][c])
 * Replaces: every nn.Conv2d on the path -- torchvision ResNet convs reached from models/resnet_encoder.py:93-99,
 * Conv3x3 (ReflectionPad2d+Conv2d, models/monodepth_layers.py:127-142) incl. the upsample+torch.cat in front of it
 * (models/depth_decoder.py:93-101), ASPP convs (models/model_parts.py:9-25), SelfAttention convs (:38-39),
 * segmentation heads (models/joint_segmentation_depth_decoder.py:35-53,111-116), PoseDecoder convs
 * (models/pose_decoder.py:29-33).  Run on dgrad-packed weights (segsde_pack_weight(for_dgrad=1)) with
 * pad' = (K-1)*dil - pad, stride 1 and in_div = stride it is the data-gradient of the same convolution. */
int segsde_conv2d_forward(const segsde_conv_desc* d, const float* x0, const float* x1, const float* wpack,
                          const float* bias, float* y, float* y2, void* stream);
/* Same, and additionally leaves the batch statistics of the output (no bias, no activation) as per-tile partials in
 * stats[rows][2][Cout] doubles (rows = segsde_conv2d_stats_rows(d) > 0; sum and sum of squares per row slice of a
 * 128-pixel tile): the statistics of the BatchNorm that follows (models/resnet_encoder.py conv -> bn pairs) without
 * another pass over the tensor.  Finish with segsde_bn_stats_from_partials.  Returns SEGSDE_ERR_UNSUPPORTED when the
 * shape cannot fuse (rows == 0). */
long segsde_conv2d_stats_rows(const segsde_conv_desc* d);
int segsde_conv2d_forward_stats(const segsde_conv_desc* d, const float* x0, const float* x1, const float* wpack,
                                const float* bias, float* y, float* y2, double* stats, void* stream);
/* Data-gradient launch that also applies the backward of the activation which produced the tensor it differentiates with
 * respect to (models/monodepth_layers.py:108-124: ConvBlock = conv -> ELU; the next layer's data-gradient lands on the ELU
 * output): channels < nsplit of y are multiplied by act'(act_out) (act_out = that saved activation output, same row /
 * channel order as y, pitch act_ld, kind SEGSDE_ACT_RELU / ELU / SIGMOID) in the epilogue -- the separate activation-backward
 * pass over the tensor (segsde_act_backward) is not needed.  act_out = NULL: identical to segsde_conv2d_forward_stats.
 * SEGSDE_ERR_UNSUPPORTED when this shape cannot fuse it (the caller then runs segsde_act_backward itself). */
int segsde_conv2d_dgrad_actgrad(const segsde_conv_desc* d, const float* x0, const float* x1, const float* wpack,
                                const float* bias, float* y, float* y2, double* stats, const float* act_out, int act_ld,
                                int act_kind, void* stream);
/* Forward launch with a residual operand: y = act((conv + bias) + res), in that association, d->act any SEGSDE_ACT_*; res is
 * [B,Ho,Wo,Cout] with pixel pitch ldr.  With the weights and bias of segsde_bn_fold it replaces the conv -> frozen BatchNorm ->
 * (+ identity) -> ReLU tail of torchvision's Bottleneck / BasicBlock (reached from models/resnet_encoder.py:93-99) in no-grad
 * forward passes: the segsde_bn_apply pass over the convolution output (one read, one write) is not needed.  res == y with
 * ldr == ldy (in place) is allowed -- every thread loads the residual values of exactly the elements it stores, before it stores
 * them; any other overlap of the two tensors returns SEGSDE_ERR_SHAPE.  The epilogue is shared by every loop of the kernel, so
 * every d->compute mode the launch takes (fp32, fp16, split bf16) carries the residual.  One destination only: a second
 * destination (nsplit / ldy2), sum2x2, in_div > 1, accumulate, SEGSDE_PAD_REFLECT_ADJOINT, Cout == 1 and shapes without the
 * 16-byte epilogue (Cout, ldy, ldr multiples of 4, y and res 16-byte aligned) return SEGSDE_ERR_UNSUPPORTED (the caller then runs
 * segsde_conv2d_forward + segsde_bn_apply).  No statistics partials: a BatchNorm that is folded has none to take. */
int segsde_conv2d_forward_residual(const segsde_conv_desc* d, const float* x0, const float* x1, const float* wpack,
                                   const float* bias, const float* res, int ldr, float* y, void* stream);

/* dW (OIHW, the state_dict layout) of the convolution described by d, given dy [B,Ho,Wo,Cout] (pitch lddy). */
size_t segsde_conv2d_wgrad_workspace(const segsde_conv_desc* d);
int segsde_conv2d_wgrad(const segsde_conv_desc* d, const float* x0, const float* x1, const float* dy, int lddy,
                        float* dw_oihw, float* workspace, size_t workspace_bytes, void* stream);

/* Upsample-folded route of Conv3x3 on [upsample(x0) | x1] (models/depth_decoder.py:93-101 with ReflectionPad2d(1) + 3x3,
 * monodepth_layers.py:127-142; d: up0 = 1, 3x3, stride 1, pad 1, SEGSDE_PAD_REFLECT): on the nearest-upsampled channels the
 * nine taps of an output pixel touch only 2x2 distinct low-resolution pixels, so per output parity class the upsampled half is
 * a 2x2 convolution of the low-resolution tensor with pre-summed weights (4 instead of 9 multiply-adds per upsampled channel;
 * mirrored padding becomes clamping).  Same results as the plain route up to the association of the sums; every entry returns
 * SEGSDE_ERR_UNSUPPORTED for shapes it does not take (the caller then uses the plain entry points).
 *   pack    : w_oihw [Cout][Ctot][3][3] -> wfold [4][Cout][2][2][C0] (forward classes (py, px) = (0,0),(0,1),(1,0),(1,1)) and
 *             wdfold [C0][4][4][Cout] (the 4x4 stride-2 kernel of the low-resolution data-gradient)
 *   forward : wpack = segsde_pack_weight(for_dgrad=0) of the same weight (its skip-channel slice is read in place)
 *   dgrad   : d = the FORWARD geometry; dy [B,H,W,Cout] pitch lddy; wdpack = segsde_pack_weight(for_dgrad=1); dx0
 *             [B,H/2,W/2,C0] dense (nullable), dx1 [B,H,W,C1] dense (nullable; accumulate_dx1 != 0: dx1 already holds
 *             another consumer's gradient of the skip tensor and this one is ADDED to it); act_out (nullable): saved activation output
 *             (pitch act_ld, kind SEGSDE_ACT_*) whose derivative multiplies dx0, as in segsde_conv2d_dgrad_actgrad
 *   wgrad   : dw_oihw [Cout][Ctot][3][3], deterministic (fixed-order reduction of the split partials) */
int segsde_upfold_pack(const float* w_oihw, int Cout, int C0, int Ctot, float* wfold, float* wdfold, void* stream);
int segsde_conv2d_forward_upfold(const segsde_conv_desc* d, const float* x0, const float* x1, const float* wpack,
                                 const float* wfold, const float* bias, float* y, void* stream);
int segsde_conv2d_dgrad_upfold(const segsde_conv_desc* d, const float* dy, int lddy, const float* wdpack, const float* wfold,
                               const float* wdfold, float* dx0, float* dx1, int accumulate_dx1, const float* act_out, int act_ld,
                               int act_kind, void* stream);
size_t segsde_conv2d_wgrad_upfold_workspace(const segsde_conv_desc* d);
int segsde_conv2d_wgrad_upfold(const segsde_conv_desc* d, const float* x0, const float* x1, const float* dy, int lddy,
                               float* dw_oihw, float* workspace, size_t workspace_bytes, void* stream);

/* Network stems: nn.Conv2d(3 * n, 64, 7, stride 2, padding 3, bias=False) of torchvision's ResNet / ResNetMultiImageInput
 * (models/resnet_encoder.py:40-52, 90-93) on the LDS-DMA path.  xpad: the bordered input of segsde_nchw_to_nhwc_bordered with
 * pad_top = 3, pad_left = 3, Hp = H + 6, Wp = W + 8 and cp = 4 (3 planes) or 8 (6 planes) channels per pixel; a 32-float
 * reduction chunk is 8 / 4 neighbouring pixels of one input row ("virtual" 32-channel pixels with the real pixel pitch).
 *   pack     : w_oihw [Cout][C][7][7] -> wstem [Cout][7][8 * cp]  (8 pixels x cp channels per tap row; pixel 7 and channels >= C zero)
 *   forward  : y [B][Ho][Wo][Cout], Ho = (H-1)/2+1; stats (nullable): BatchNorm statistics partials, rows = segsde_stem7x7_stats_rows
 *   wgrad    : dw_oihw [Cout][C][7][7], deterministic; no data-gradient (the input is the image) */
int segsde_stem_pack(const float* w_oihw, int Cout, int C, int cp, float* wstem, void* stream);
long segsde_stem7x7_stats_rows(int B, int Hp, int Wp, int cp, int Cout);
int segsde_stem7x7_forward(const float* xpad, int B, int Hp, int Wp, int cp, const float* wstem, int Cout, float* y, double* stats,
                           void* stream);
/* The stem launch with a bias and an activation, y = act(conv + bias[n]) (bias nullable, act SEGSDE_ACT_*): conv1 -> frozen bn1 ->
 * ReLU of the stem (models/resnet_encoder.py:93-95) as one launch on the weights and bias of segsde_bn_fold; replaces
 * segsde_stem7x7_forward + segsde_bn_apply in no-grad forward passes.  No statistics partials. */
int segsde_stem7x7_forward_bias_act(const float* xpad, int B, int Hp, int Wp, int cp, const float* wstem, int Cout,
                                    const float* bias, int act, float* y, void* stream);
size_t segsde_stem7x7_wgrad_workspace(int B, int Hp, int Wp, int cp, int Cout);
int segsde_stem7x7_wgrad(const float* xpad, int B, int Hp, int Wp, int cp, const float* dy, int lddy, int Cout, int C,
                         float* dw_oihw, float* workspace, size_t workspace_bytes, void* stream);

/* OIHW -> [O][KH][KW][I] (for_dgrad=0) or [I][KH][KW][O] spatially flipped (for_dgrad=1). */
int segsde_pack_weight(const float* w_oihw, float* out, int O, int I, int KH, int KW, int for_dgrad, void* stream);
/* both packs of one weight tensor in a single launch (training forward: the data-gradient pack is kept for backward) */
int segsde_pack_weight_both(const float* w_oihw, float* out_fwd, float* out_dgrad, int O, int I, int KH, int KW,
                            void* stream);
/* The same for many weights in one launch (a training step re-packs every convolution weight of the model).  jobs_device:
 * njobs + 1 entries in DEVICE memory; entry j packs one weight with blocks [block0, next entry's block0) of the launch, the
 * last entry is a sentinel whose block0 is total_blocks.  reserved = 1 selects the transposing path for a weight with at
 * most 9 taps: the job must then own exactly ceil(O/32) * ceil(I/32) blocks (one per 32 x 32 channel block); reserved = 0:
 * any number of blocks, one element per thread and trip. */
typedef struct segsde_pack_job {
  const float* w; float* fwd; float* dgrad;
  int O, I, KH, KW, block0, reserved;
} segsde_pack_job;
int segsde_pack_weight_both_multi(const segsde_pack_job* jobs_device, int njobs, int total_blocks, void* stream);

/* Adds to dx the gradient that entered the mirrored padding cells of a reflection-padded 3x3 stride-1 conv
 * (autograd of nn.ReflectionPad2d(1), models/monodepth_layers.py:134,140); wdpack = segsde_pack_weight(for_dgrad=1).
 * segsde_conv2d_forward(pad_mode = SEGSDE_PAD_REFLECT_ADJOINT) already includes it. */
int segsde_reflect_dgrad_fix(const float* dy, int lddy, const float* wdpack, float* dx, int lddx, float* dx2, int lddx2,
                             int nsplit, int B, int H, int W, int Cin, int Cout, void* stream);

/* ------------------------------------------------------------------------------------------------ *
 * BatchNorm / activations / pooling / resampling (HBM-bound, NHWC)                                 *
 * ------------------------------------------------------------------------------------------------ */
/* Training-mode batch statistics over M rows (nn.BatchNorm2d.forward in train(), every BN on the path):
 * mean[c], invstd[c] = 1/sqrt(biased var + eps); running stats updated with `momentum` using the unbiased var;
 * num_batches_tracked (nullable, device int64 scalar) is incremented by one, as nn.BatchNorm2d does per training forward. */
size_t segsde_bn_stats_workspace(long M, int C);
int segsde_bn_stats(const float* x, int ldx, long M, int C, float* mean, float* invstd, float* running_mean,
                    float* running_var, float momentum, float eps, int64_t* num_batches_tracked, void* workspace,
                    size_t workspace_bytes, void* stream);
/* Eval mode: mean = running_mean, invstd = 1/sqrt(running_var + eps). */
int segsde_bn_eval_stats(const float* running_mean, const float* running_var, int C, float eps, float* mean,
                         float* invstd, void* stream);
/* A frozen (eval-mode) BatchNorm folded into the convolution in front of it, for many (convolution, BatchNorm) pairs in one
 * launch:  w_out[o,i,kh,kw] = w[o,i,kh,kw] * s[o],  b_out[o] = beta[o] - mean[o] * s[o] (+ cb[o] * s[o]),  s[o] = gamma[o] * invstd[o]
 * with invstd[o] = 1/sqrt(var[o] + eps) -- the expression of segsde_bn_eval_stats, bit for bit; plain fp32 in the order written.
 * bn(conv(x, w) + cb) == conv(x, w_out) + b_out up to fp32 re-association: the conv -> bn pairs of models/resnet_encoder.py and
 * models/model_parts.py (ASPP) in eval mode then need no segsde_bn_eval_stats + segsde_bn_apply pass.  cb (the convolution's own
 * bias), gamma and beta are nullable (no bias; affine=False: 1 and 0); any O, I, KH, KW.  jobs_device: njobs + 1 entries in
 * DEVICE memory, job j runs on blocks [block0, next entry's block0) of the launch (at least one; one element per thread and
 * trip), the last entry is a sentinel whose block0 is total_blocks. */
typedef struct segsde_bn_fold_job {
  const float* w; const float* cb; const float* gamma; const float* beta; const float* mean; const float* var;
  float* w_out; float* b_out;
  float eps;
  int O, I, KH, KW, block0, reserved;
} segsde_bn_fold_job;
int segsde_bn_fold(const segsde_bn_fold_job* jobs_device, int njobs, int total_blocks, void* stream);
/* y = dropout(act(gamma*(x-mean)*invstd + beta + residual)); dropout keeps with prob 1-p and scales by 1/(1-p)
 * (nn.Dropout(0.5) in ASPP.project, models/model_parts.py:21-25), mask = hash(seed, element). */
int segsde_bn_apply(const float* x, int ldx, long M, int C, const float* mean, const float* invstd, const float* gamma,
                    const float* beta, const float* residual, int ldr, float* y, int ldy, int act, float drop_p,
                    uint64_t seed, void* stream);
/* Backward of segsde_bn_apply + batch statistics.  Phase 1 reduces dgamma/dbeta (sums[0..C) = sum dz*xhat,
 * sums[C..2C) = sum dz) where dz = dy * dropout_mask * act'(y); phase 2 writes dx (and dres = dz if non-null).
 * batch_stats=0 (eval-mode BN): dx = gamma*invstd*dz. */
/* mean / invstd (+ running-statistics update, exactly as segsde_bn_stats) from the partial sums a
 * segsde_conv2d_forward_stats launch left behind; workspace: segsde_bn_stats_from_partials_workspace(C) bytes. */
size_t segsde_bn_stats_from_partials_workspace(int C);
int segsde_bn_stats_from_partials(const double* partials, long rows, long M, int C, float* mean, float* invstd,
                                  float* running_mean, float* running_var, float momentum, float eps,
                                  int64_t* num_batches_tracked, void* workspace, size_t workspace_bytes, void* stream);
size_t segsde_bn_backward_workspace(long M, int C);
/* y may be NULL ("remask"): for act = none, or act = ReLU with no residual / dropout (then beta is required with gamma),
 * the activation mask is recomputed from x exactly as the forward kernel formed it and the saved output is not read. */
int segsde_bn_backward(const float* dy, int lddy, const float* y, int ldy, const float* x, int ldx, long M, int C,
                       const float* mean, const float* invstd, const float* gamma, const float* beta, int act,
                       float drop_p, uint64_t seed, int batch_stats, float* dgamma, float* dbeta, float* dx, int lddx,
                       float* dres, int lddres, void* workspace, size_t workspace_bytes, void* stream);
/* Packed ReLU mask for the BatchNorms whose mask is not a function of x alone (residual add before the ReLU: bn3 and the
 * downsample BN of a bottleneck, models/resnet_encoder.py).  segsde_bn_apply_mask is segsde_bn_apply plus one bit per element of
 * the logical [M][C] index space: bit (m*C + c) % 32 of word (m*C + c) / 32 is 1 exactly when the stored y > 0;
 * segsde_bn_mask_words(M, C) words, each written whole (zeros past the end), no fill needed.  segsde_bn_backward_mask is
 * segsde_bn_backward with those bits in place of the saved output -- 1/32 B instead of 4 B per element and pass -- and gives
 * bit-identical dx / dres / dgamma / dbeta.  Both need C % 4 == 0, pitches % 4 == 0 and 16-byte aligned tensors (the float4
 * path), no dropout, and the backward act = ReLU: anything else returns SEGSDE_ERR_UNSUPPORTED and the caller keeps y. */
size_t segsde_bn_mask_words(long M, int C);
int segsde_bn_apply_mask(const float* x, int ldx, long M, int C, const float* mean, const float* invstd, const float* gamma,
                         const float* beta, const float* residual, int ldr, float* y, int ldy, int act, float drop_p,
                         uint64_t seed, uint32_t* mask, void* stream);
int segsde_bn_backward_mask(const float* dy, int lddy, const uint32_t* mask, const float* x, int ldx, long M, int C,
                            const float* mean, const float* invstd, const float* gamma, int act, float drop_p,
                            int batch_stats, float* dgamma, float* dbeta, float* dx, int lddx, float* dres, int lddres,
                            void* workspace, size_t workspace_bytes, void* stream);
/* Cross-replica (synchronized) BatchNorm for data-parallel training: the reductions above cut in two, with a seam where the
 * caller's collective sits.  A LOCAL stage reduces this rank's rows to one ROW of doubles, the caller all-gathers the rows of the
 * W ranks (rank order), a GLOBAL stage folds the gathered rows in rank order and finishes.  No atomics, every order fixed: all
 * ranks get the same bits from the same table, and with W = 1 and statistics taken from x the results equal those of
 * segsde_bn_stats / segsde_bn_backward / segsde_bn_backward_mask bit for bit.
 *   ROW layout, segsde_bn_sync_row_bytes(C) = (2 C + 2) * 8 bytes (a multiple of 16), 8-byte aligned:
 *     doubles [0, C)      forward: sum x        backward: sum dz * xhat   (this rank's rows, per channel)
 *     doubles [C, 2 C)    forward: sum x^2      backward: sum dz
 *     double  2 C         this rank's row count M (an integer value)
 *     double  2 C + 1     0 (padding to 16 bytes)
 *   rows: W such rows back to back, as all_gather_into_tensor leaves them.
 * segsde_bn_sync_stats_local: the row from x (workspace: segsde_bn_stats_workspace(M, C)).
 * segsde_bn_sync_stats_local_from_partials: the row from the [rows][2][C] partials of a convolution epilogue (workspace:
 *   segsde_bn_stats_from_partials_workspace(C)), folded as segsde_bn_stats_from_partials folds them (a single gathered row gives
 *   that entry's bits); the same sums as the x source in another order, so the two sources agree to rounding only.
 * segsde_bn_sync_stats_global: mean / invstd / running buffers / num_batches_tracked as segsde_bn_stats computes them, over
 *   M_total = the sum of the gathered counts, which is read on the device (ranks may hold different numbers of rows; M_total == 1
 *   keeps the biased variance in the running update); inv_count[0] = 1 / (float)M_total, a device float for the backward pass.
 * segsde_bn_sync_backward_local: the reduction of segsde_bn_backward (mask == NULL; y == NULL: its remask mode) or of
 *   segsde_bn_backward_mask (mask != NULL, y ignored), with their operand rules and error codes (has_dres: whether the global
 *   stage will write dres -- the remask mode does not allow it); writes this rank's float dgamma / dbeta (the parameter
 *   gradients: local sums, averaged over ranks like every other gradient) and the row (workspace: segsde_bn_backward_workspace).
 * segsde_bn_sync_backward_global: folds the W gathered rows to dgamma_total / dbeta_total (float [C] scratch, written) and
 *   runs the apply pass of segsde_bn_backward with those totals and inv_count in place of 1 / (float)M: dx is the gradient of the
 *   SUM of the ranks' losses with respect to this rank's x; dres = dz.  dx and dres nullable. */
size_t segsde_bn_sync_row_bytes(int C);
int segsde_bn_sync_stats_local(const float* x, int ldx, long M, int C, double* row, void* workspace, size_t workspace_bytes,
                               void* stream);
int segsde_bn_sync_stats_local_from_partials(const double* partials, long rows, long M, int C, double* row, void* workspace,
                                             size_t workspace_bytes, void* stream);
int segsde_bn_sync_stats_global(const double* rows, int W, int C, float* mean, float* invstd, float* running_mean,
                                float* running_var, float momentum, float eps, int64_t* num_batches_tracked, float* inv_count,
                                void* stream);
int segsde_bn_sync_backward_local(const float* dy, int lddy, const float* y, int ldy, const uint32_t* mask, const float* x, int ldx,
                                  long M, int C, const float* mean, const float* invstd, const float* gamma, const float* beta,
                                  int act, float drop_p, uint64_t seed, int has_dres, float* dgamma, float* dbeta, double* row,
                                  void* workspace, size_t workspace_bytes, void* stream);
int segsde_bn_sync_backward_global(const float* dy, int lddy, const float* y, int ldy, const uint32_t* mask, const float* x, int ldx,
                                   long M, int C, const float* mean, const float* invstd, const float* gamma, const float* beta,
                                   int act, float drop_p, uint64_t seed, const double* rows, int W, const float* inv_count,
                                   float* dgamma_total, float* dbeta_total, float* dx, int lddx, float* dres, int lddres,
                                   void* stream);
/* dz = dy * act'(y) (ELU / ReLU / sigmoid via the saved output, as the reference's in-place ops do);
 * dbias[c] = sum_rows dz (nullable).  Replaces autograd of nn.ELU / nn.ReLU / torch.sigmoid + conv bias grad. */
size_t segsde_colsum_workspace(long M, int C);
int segsde_act_backward(const float* dy, int lddy, const float* y, int ldy, long M, int C, int act, float* dz, int lddz,
                        float* dbias, void* workspace, size_t workspace_bytes, void* stream);
int segsde_colsum(const float* x, int ldx, long M, int C, float* out, void* workspace, size_t workspace_bytes,
                  void* stream);

/* Feature distance of the self-supervised pretraining stage (the dec6 configs' feat_dist_lambda term):
 * dist[0] = ||a - b||_2 over two fp32 NHWC tensors of M pixels x C channels with pixel pitches lda / ldb -- torch.dist(
 * outputs["encoder_features"], outputs["imnet_features"], p=2), train.py:480-483.  Deterministic (per-block double partials, a
 * fixed-order one-block finish, no atomics); the result stays on the device.  workspace: segsde_feat_dist_workspace(M, C) bytes.
 * Backward: da = grad[0] * (a - b) / dist[0], 0 where dist[0] == 0 (torch's norm backward); b gets no gradient (it is detached). */
size_t segsde_feat_dist_workspace(long M, int C);
int segsde_feat_dist_forward(const float* a, int lda, const float* b, int ldb, long M, int C, float* dist, void* workspace,
                             size_t workspace_bytes, void* stream);
int segsde_feat_dist_backward(const float* a, int lda, const float* b, int ldb, long M, int C, const float* dist,
                              const float* grad, float* da, int ldda, void* stream);

/* nn.MaxPool2d(3, 2, 1) (models/resnet_encoder.py:96); idx keeps the winning tap (first max in scan order). */
int segsde_maxpool3x3s2_forward(const float* x, int B, int H, int W, int C, float* y, uint8_t* idx, void* stream);
/* accumulate != 0: dx already holds another consumer's gradient of the pooled tensor and this one is added to it */
int segsde_maxpool3x3s2_backward(const float* dy, const uint8_t* idx, int B, int H, int W, int C, float* dx, int accumulate,
                                 void* stream);
/* adjoint of the nearest x2 upsample (models/monodepth_layers.py:202-205): dx[h,w] = sum of the 2x2 block of dy */
int segsde_upsample2x_backward(const float* dy, int lddy, int B, int h, int w, int C, float* dx, int lddx, void* stream);
/* upsample(x) of models/monodepth_layers.py:202-205 as a stand-alone call: x [B,h,w,C] -> y [B,2h,2w,C] */
int segsde_upsample2x_forward(const float* x, int ldx, int B, int h, int w, int C, float* y, int ldy, void* stream);
/* F.interpolate(mode="bilinear") and its adjoint, NHWC (joint_segmentation_depth_decoder.py:64-65,72-73,173-180;
 * torchvision ASPPPooling; loss/loss.py:22-23 with align_corners=1; loss/monodepth_loss.py:72-73 with C=1). */
int segsde_resize_bilinear_forward(const float* x, int ldx, int B, int Hi, int Wi, int C, float* y, int ldy, int Ho, int Wo,
                                   int align_corners, void* stream);
int segsde_resize_bilinear_backward(const float* dy, int lddy, int B, int Hi, int Wi, int C, float* dx, int lddx, int Ho,
                                    int Wo, int align_corners, void* stream);
/* nn.AdaptiveAvgPool2d(1) / out.mean(3).mean(2) (pose_decoder.py:49) and adjoint */
size_t segsde_global_avgpool_workspace(int B, long HW, int C);   /* bytes; 0: the launch needs none */
int segsde_global_avgpool_forward(const float* x, int ldx, int B, long HW, int C, float* y, void* ws, size_t ws_bytes,
                                  void* stream);
int segsde_global_avgpool_backward(const float* dy, int B, long HW, int C, float* dx, int lddx, void* stream);
/* SelfAttention gate y = f * sigmoid(a) (models/model_parts.py:44-46) and adjoint */
int segsde_gate_forward(const float* f, const float* a, long n, float* y, void* stream);
int segsde_gate_backward(const float* dy, const float* f, const float* a, long n, float* df, float* da, void* stream);
/* out = alpha*x + beta*y over n contiguous floats (PAD feature merge :160-161; EMA update train.py:346-358) */
int segsde_axpby(long n, float alpha, const float* x, float beta, const float* y, float* out, void* stream);
/* same with the scalars read from device memory (gradient scaling by upstream 0-dim tensors without a host sync) */
int segsde_axpby_dev(long n, const float* alpha, const float* x, const float* beta, const float* y, float* out, void* stream);
/* channel-slice copy dst[m, 0..C) = src[m, 0..C) (torch.cat of the ASPP branches, models/model_parts.py:31) */
int segsde_copy_channels(const float* src, int lds, float* dst, int ldd, long M, int C, void* stream);
/* nn.Dropout2d inside ConvBlock (models/monodepth_layers.py:117-119, depth_args.dropout > 0): y[b,p,c] = x[b,p,c] * scale[b,c]
 * with scale = 0 or 1/(1-p) per (sample, channel); the same call is its adjoint. */
int segsde_scale_channels(const float* x, int ldx, int B, long HW, int C, const float* scale, float* y, int ldy, void* stream);
/* nn.Dropout(p) on [M, C] rows (JointSegDepthDecoder's layer_dropout on the stacked features,
 * models/joint_segmentation_depth_decoder.py:50): y = x / (1 - p) where the counter-based draw of (seed, element index) keeps the
 * element, else 0; the same call with the same seed on the gradient is its adjoint. */
int segsde_dropout(const float* x, int ldx, long M, int C, float p, uint64_t seed, float* y, int ldy, void* stream);
/* NCHW image -> NHWC with the encoder's input normalisation (x - mean) / std (models/resnet_encoder.py:92);
 * mean = 0, std = 1 gives a plain layout change.  All ldy channels of every pixel are written: channels C..ldy-1 become
 * zero (the 3 / 6-channel network input padded to 4 / 8).  nhwc_to_nchw is the inverse layout change. */
int segsde_nchw_to_nhwc(const float* x, int B, int C, int H, int W, float mean, float std, float* y, int ldy, void* stream);
/* The network-input edge for the stems: (x - mean) / sd of NCHW planes written as 4 / 8-channel pixels (ldy) into the interior of a
 * zero-bordered [B][Hp][Wp][ldy] tensor (interior at (pad_top, pad_left)): the stem's zero padding, materialised, so that
 * segsde_stem7x7_forward needs no padding logic (models/resnet_encoder.py:90-93: normalisation, then conv1 with padding 3). */
int segsde_nchw_to_nhwc_bordered(const float* x, int B, int C, int H, int W, float mean, float sd, float* y, int ldy, int pad_top,
                                 int pad_left, int Hp, int Wp, void* stream);
int segsde_nhwc_to_nchw(const float* x, int ldx, int B, int C, int H, int W, float* y, void* stream);

/* Winograd F(2x2,3x3) route of a stride-1 3x3 convolution with many channels whose padding equals its dilation (the conv2 of
 * every bottleneck, models/resnet_encoder.py:90-101 via torchvision's Bottleneck, dilation 2 in layer4 of the dilated ResNet;
 * the decoder's Conv3x3 on [x | skip] at the bottleneck resolution, models/depth_decoder.py:93-101).  The same call computes
 * the data-gradient of a zero-padded convolution when handed dY, the transposed geometry and the data-gradient pack.
 * segsde_winograd_pack: OIHW -> U = G g G^T as [16][Cout][Cin] (forward) and [16][Cin][Cout] of the flipped kernel
 * (data-gradient); either output may be NULL.  segsde_winograd_pack_multi: the packs of many weights in one launch (device-
 * resident job table; job j owns blocks [block0_j, block0_{j+1}), 2 * ceil(O * I / 256) each).  segsde_conv2d_winograd: input
 * transform (x1 nullable: channels C0.. of the concat), sixteen position GEMMs as one launch of the implicit-GEMM kernel,
 * output transform with bias (nullable) + activation d->act; `stats` (nullable) receives
 * [segsde_conv2d_winograd_stats_rows(d)][2][Cout] doubles for segsde_bn_stats_from_partials.  Zero or mirrored padding (mirrored:
 * dilation 1 only), H and W multiples of 2 * dilation, (C0 + C1) % 32 == 0, C0 % 4 == 0, Cout % 64 == 0; SEGSDE_ERR_UNSUPPORTED
 * otherwise (callers use segsde_conv2d_forward). */
typedef struct segsde_wino_job {
  const float* w;    /* OIHW 3x3 weight */
  float* u_fwd;      /* [16][O][I]  (reserved & 1: the pack of segsde_winograd_fused_pack, flip = 0; O % 64 == 0) */
  float* u_dgrad;    /* [16][I][O]  (reserved & 1: the pack of segsde_winograd_fused_pack, flip = 1; I % 64 == 0) */
  int O, I, block0, reserved;
} segsde_wino_job;
size_t segsde_conv2d_winograd_workspace(const segsde_conv_desc* d);
long segsde_conv2d_winograd_stats_rows(const segsde_conv_desc* d);
int segsde_winograd_pack(const float* w_oihw, int Cout, int Cin, float* u_fwd, float* u_dgrad, void* stream);
int segsde_winograd_pack_multi(const segsde_wino_job* jobs_device, int njobs, int total_blocks, void* stream);
int segsde_conv2d_winograd(const segsde_conv_desc* d, const float* x0, const float* x1, const float* u_pack, const float* bias,
                           float* y, double* stats, float* v_keep, void* workspace, size_t workspace_bytes, void* stream);
/* the weight gradient on the same route: dU_p = V_p^T (A dY A^T)_p as sixteen position GEMMs in one launch of the
 * weight-gradient kernel (split boundaries on the position boundaries), dW = G^T dU G written as OIHW.  d: the FORWARD geometry.
 * v_keep of the forward call (nullable; 16 * Tp * (C0+C1) floats, Tp = B*H/2*W/2 rounded up to a multiple of 128) receives the
 * transformed input; handed back as v_saved
 * (nullable) the weight gradient skips its own input transform. */
size_t segsde_conv2d_wgrad_winograd_workspace(const segsde_conv_desc* d);
int segsde_conv2d_wgrad_winograd(const segsde_conv_desc* d, const float* x0, const float* x1, const float* dy, int lddy,
                                 const float* v_saved, float* dw_oihw, void* workspace, size_t workspace_bytes, void* stream);
/* Winograd F(2x2,3x3) with both transforms inside ONE kernel (no V / M tensors): the 64- and 128-channel conv2 of layer1 / layer2
 * (models/resnet_encoder.py:90-101 via torchvision's Bottleneck / BasicBlock) and the decoder's single-source Conv3x3
 * (models/monodepth_layers.py:127-142, reflect = 1: mirrored padding, forward only) -- 3x3, stride 1, padding 1, one source, H and W
 * even, C % 64 == 0, Cout % 64 == 0.  segsde_winograd_fused_pack: OIHW -> the transformed weights U (16 K N floats) in the layout
 * the kernel reads -- blocked: [transform row][k][block of 64 n][32 lanes][4 positions of the row][2 halves of the block], the
 * eight B operands of a lane and step contiguous; flip = 0: the forward pack
 * (K = Cin, N = Cout), flip = 1: the data-gradient pack of the spatially flipped kernel (K = Cout, N = Cin; call the convolution
 * with x = dY, C = Cout, Cout = Cin).  The layout has no partial block: a pack whose N is not a multiple of 64 is
 * SEGSDE_ERR_UNSUPPORTED (no kernel could read it).  y = act(Y + bias) (bias nullable), or y += Y (accumulate = 1: no bias / activation /
 * statistics; the gradient collector of DESIGN.md 3.2f); stats (nullable):
 * [segsde_winograd_fused_stats_rows(B, H, W)][2][Cout] doubles for segsde_bn_stats_from_partials.  SEGSDE_ERR_UNSUPPORTED outside
 * these shapes (segsde_winograd_fused_ok tells beforehand). */
int segsde_winograd_fused_ok(int B, int H, int W, int C, int Cout);
long segsde_winograd_fused_stats_rows(int B, int H, int W);
int segsde_winograd_fused_pack(const float* w_oihw, int Cout, int Cin, int flip, float* u_kn, void* stream);
int segsde_conv2d_winograd_fused(const float* x, int ldx, int B, int H, int W, int C, int reflect, const float* u_kn, int Cout,
                                 const float* bias, int act, float* y, int ldy, int accumulate, double* stats, void* stream);
/* Round 5.  The same kernel on the decoder's virtual input [up2x?(x0) | x1] (models/depth_decoder.py:88-101: nearest-upsampled
 * previous block, encoder skip): x0 [B, H >> up0, W >> up0, C0], x1 [B, H, W, C1] or NULL; C0 % 64 == 0, (C0 + C1) % 64 == 0 --
 * upsampling, concat and mirrored padding are index arithmetic of the patch loader, all channels at 16 / 36 of the multiply-adds. */
int segsde_conv2d_winograd_fused2(const float* x0, int ld0, int C0, int up0, const float* x1, int ld1, int C1, int B, int H, int W,
                                  int reflect, const float* u_kn, int Cout, const float* bias, int act, float* y, int ldy,
                                  double* stats, void* stream);
/* Data-gradient on the one-kernel route with the direct route's epilogues: dx (+)= conv(dy, flipped pack) * act'(act_out)
 * (act_out nullable: the saved output of the activation that produced this convolution's input, ConvBlock's ELU,
 * monodepth_layers.py:108-125; accumulate: added onto what dx holds).  Zero padding; for the reflection-padded
 * Conv3x3 follow it with segsde_reflect_adjoint_borders2: the gradient that entered the mirrored padding cells, ADDED onto rows
 * 1 / H-2 and columns 1 / W-2 of dx (act_out as above).  ldu: row pitch of ud_kn (Cin; or,
 * for the gradient of ONE source of a two-source convolution -- the decoder's skip input, weight channels [C0, C0 + C1) -- the
 * full pack's width, ud_kn pointing at the slice's first 64-filter block (blocked layout: (first column / 64) * 256 floats into
 * the pack; the slice starts on a multiple of 64); segsde_reflect_adjoint_borders2 takes the matching slice of the forward pack
 * through ldw). */
int segsde_conv2d_winograd_fused_dgrad(const float* dy, int lddy, int B, int H, int W, int Cout, const float* ud_kn, int ldu, int Cin,
                                       float* dx, int lddx, int accumulate, const float* act_out, int act_ld, int act_kind, void* stream);
/* The mirrored-padding terms by a kernel of their own (csrc/winograd_fused.hip: two launches -- row lines, column lines +
 * corners -- of a 32-pixel x Cin MFMA kernel); wpack = the
 * FORWARD pack [Cout][3][3][Cin] of segsde_pack_weight(for_dgrad = 0).  Cin % 32 == 0, Cout % 32 == 0, H, W >= 4. */
int segsde_reflect_adjoint_borders2(const float* dy, int lddy, const float* wpack, int ldw, float* dx, int lddx, const float* act_out,
                                    int act_ld, int act_kind, int B, int H, int W, int Cin, int Cout, void* stream);
/* Weight gradient on the one-kernel Winograd scheme (csrc/winograd_wgrad.hip): dU_p = V_p^T (A dY A^T)_p with both operands formed
 * from the raw input patches and the raw output gradient in LDS, split over tile ranges into slabs, folded deterministically and
 * transformed back (dW = G^T dU G, OIHW).  d as for segsde_conv2d_wgrad: 3x3 / stride 1 / padding 1 / dilation 1, zero or mirrored
 * padding, one or two sources, up0 (the decoder's [upsample(x0) | x1], models/depth_decoder.py:88-101); C0 % 32 == 0, C1 % 32 == 0,
 * Cout % 64 == 0, H and W even.  Workspace 0 = shape not taken. */
size_t segsde_conv2d_wgrad_winograd_fused_workspace(const segsde_conv_desc* d);
int segsde_conv2d_wgrad_winograd_fused(const segsde_conv_desc* d, const float* x0, const float* x1, const float* dy, int lddy,
                                       float* dw_oihw, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------ *
 * Pose: axis-angle + translation -> 4x4 (models/monodepth_layers.py:30-105)                         *
 * ------------------------------------------------------------------------------------------------ */
int segsde_pose_matrix_forward(const float* axisangle, const float* translation, int B, int stride, int invert, float* M,
                               void* stream);
int segsde_pose_matrix_backward(const float* axisangle, const float* translation, const float* dM, int B, int stride,
                                int invert, float* daxisangle, float* dtranslation, void* stream);

/* ------------------------------------------------------------------------------------------------ *
 * Monodepth photometric loss (loss/monodepth_loss.py, models/monodepth_layers.py:18-27,145-254)     *
 * ------------------------------------------------------------------------------------------------ */
/* generate_images_pred for one (scale, frame): bilinear-upsample disp_s (align_corners=False) -> depth ->
 * backproject with inv_K -> project with K*T -> grid_sample(src, bilinear, border, align_corners=True).
 * color: [B,3,H,W]; optional outputs grid [B,H,W,2] (normalised, as outputs[("sample",f,s)]) and depth [B,1,H,W]. */
int segsde_warp_forward(const float* disp, int hs, int ws, const float* inv_K, const float* K, const float* T,
                        const float* src, int B, int H, int W, float min_depth, float max_depth, float* color,
                        float* grid, float* depth, void* stream);
/* adjoint w.r.t. the upsampled disparity (g_disp_up [B,H,W], accumulated +=) and T (gT [B,4,4], accumulated +=). */
size_t segsde_warp_backward_workspace(int B, int H, int W);
int segsde_warp_backward(const float* gcolor, const float* disp, int hs, int ws, const float* inv_K, const float* K,
                         const float* T, const float* src, int B, int H, int W, float min_depth, float max_depth,
                         float* g_disp_up, float* gT, void* workspace, size_t workspace_bytes, void* stream);
/* compute_reprojection_loss: err[b,h,w] = 0.85*mean_c SSIM(pred,target) + 0.15*mean_c|target-pred| (or L1 only).
 * err / gerr are [B,H,W] planes with `bstride` floats between batches (a channel of a [B,n,H,W] tensor). */
int segsde_reprojection_error_forward(const float* pred, const float* target, int B, int H, int W, int no_ssim,
                                      float* err, long err_bstride, void* stream);
size_t segsde_reprojection_error_backward_workspace(int B, int H, int W);
int segsde_reprojection_error_backward(const float* pred, const float* target, const float* gerr, long gerr_bstride, int B,
                                       int H, int W, int no_ssim, float* gpred, void* workspace, size_t workspace_bytes,
                                       void* stream);
/* per-pixel min over [identity(+1e-5*noise) | reprojection] channels (monodepth_loss.py:136-177) for any number of source
 * frames n_reproj (1..8: the loop over frame_ids[1:]): reproj and ident are [B,n_reproj,H,W], noise [B, avg ? 1 : n_reproj, H, W].
 * ident/noise may be NULL (disable_automasking); avg=1 averages the channels of each group first.  n_ident of the adjoint: nonzero
 * if the forward had identity terms.
 * Outputs: sel [B,H,W] uint8 = argmin index in the combined order, identity_selection [B,H,W] float (nullable),
 * sum_out[0] = sum of the minima (the caller divides by B*H*W). */
size_t segsde_automask_workspace(int B, int H, int W);
int segsde_automask_min_forward(const float* ident, const float* noise, const float* reproj, int n_reproj, int avg, int B,
                                int H, int W, uint8_t* sel, float* identity_selection, float* sum_out, void* workspace,
                                size_t workspace_bytes, void* stream);
int segsde_automask_min_backward(const uint8_t* sel, int n_ident, int n_reproj, int avg, int B, int H, int W, float scale,
                                 float* greproj, void* stream);
/* edge-aware smoothness of the mean-normalised disparity (monodepth_loss.py:182-186, monodepth_layers.py:208-221):
 * out[0] = mean|dx d^|e^{-|dx I|} + mean|dy d^|e^{-|dy I|};  mean_disp [B] is kept for the backward. */
size_t segsde_smoothness_workspace(int B, int h, int w);
int segsde_smoothness_forward(const float* disp, const float* img, int B, int h, int w, float* mean_disp, float* out,
                              void* workspace, size_t workspace_bytes, void* stream);
int segsde_smoothness_backward(const float* disp, const float* img, const float* mean_disp, int B, int h, int w,
                               float scale, float* gdisp, void* workspace, size_t workspace_bytes, void* stream);

/* The same layers by themselves, for callers outside the training path (a script that imports them by name from
 * models/monodepth_layers.py): get_smooth_loss WITHOUT the mean normalisation (monodepth_layers.py:208-221; gdisp is
 * accumulated into), SSIM.forward -> the per-channel loss map clamp((1 - SSIM) / 2, 0, 1) and its adjoint w.r.t. both
 * images (:224-254; gx / gy may be NULL), BackprojectDepth.forward -> cam_points [B,4,H*W] (:169-174) and
 * Project3D.forward -> pix_coords [B,H,W,2] in [-1, 1] (:188-199). */
size_t segsde_smooth_loss_workspace(int B, int h, int w);
int segsde_smooth_loss_forward(const float* disp, const float* img, int B, int h, int w, float* out, void* workspace,
                               size_t workspace_bytes, void* stream);
int segsde_smooth_loss_backward(const float* disp, const float* img, int B, int h, int w, float scale, float* gdisp,
                                void* workspace, size_t workspace_bytes, void* stream);
int segsde_ssim_map_forward(const float* x, const float* y, int B, int C, int H, int W, float* out, void* stream);
int segsde_ssim_map_backward(const float* x, const float* y, const float* gout, int B, int C, int H, int W, float* gx,
                             float* gy, void* stream);
int segsde_backproject_depth(const float* depth, const float* inv_K, int B, int H, int W, float* cam_points, void* stream);
int segsde_project3d(const float* points, const float* K, const float* T, int B, int H, int W, float eps, float* pix_coords,
                     void* stream);
/* Their adjoints (the reference layers are plain differentiable torch code, :169-174 / :188-199; the photometric gradient
 * reaches the depth through BackprojectDepth and the pose through Project3D): d depth [B,H*W] from d cam_points [B,4,H*W];
 * d points [B,4,H*W] (nullable) and d T [B,4,4] (nullable; needs the workspace: per-block partial sums in double, folded in
 * block order) from d pix_coords [B,H,W,2].  The intrinsics are data: no gradient for K / inv_K. */
int segsde_backproject_depth_backward(const float* g_cam_points, const float* inv_K, int B, int H, int W, float* g_depth,
                                      void* stream);
size_t segsde_project3d_backward_workspace(int B, int H, int W);
int segsde_project3d_backward(const float* points, const float* K, const float* T, const float* g_pix, int B, int H, int W,
                              float eps, float* g_points, float* g_T, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------ *
 * Segmentation loss and DepthMix / ClassMix (loss/loss.py:17-37, loader/transformsgpu.py:33-47,     *
 * loader/transformmasks.py:27-41, train.py:585-604)                                                 *
 * ------------------------------------------------------------------------------------------------ */
/* F.cross_entropy over NHWC logits (pitch ld) with ignore_index; out[0] = sum_i w_i*nll_i, out[1] = sum_i w_i over
 * non-ignored pixels (w_i = class_weight[t_i] or 1; times pixel_weights[i] if given). */
size_t segsde_cross_entropy_workspace(long M);
int segsde_cross_entropy_forward(const float* logits, int ld, long M, int C, const int64_t* target, int64_t ignore_index,
                                 const float* class_weight, const float* pixel_weights, float* out, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* dlogits[i,c] = scale * w_i * (softmax_c - [c == t_i]) (0 for ignored pixels) */
int segsde_cross_entropy_backward(const float* logits, int ld, long M, int C, const int64_t* target, int64_t ignore_index,
                                  const float* class_weight, const float* pixel_weights, const float* scale,
                                  float* dlogits, int lddl, void* stream);
/* out_i = m_i*x_i + (1-m_i)*x_{(i+1)%B}; mask is int64 or float32 [Bm,H,W] (Bm = B, or B/2: paired-halves branch);
 * element strides let x be NCHW or channels-last.  Bit-exact with the reference's fp32 op sequence. */
int segsde_mix(const void* mask, int mask_is_int64, int Bm, const float* x, int B, int C, int H, int W, long sb, long sc,
               long sh, long sw, float* out, void* stream);
int segsde_mix_labels(const int64_t* mask, const int64_t* target, int B, int H, int W, int64_t* out, void* stream);
/* depthcomp: m_i = (d_i >= d_{(i+1)%B} - margin) * (d_i >= ft_i) -> int64 [B,H,W] (train.py:585-604, generalised partner);
 * ft_i = fg_threshold_per_sample[i] (nullable DEVICE [B]: the per-image draw of train.py:592-599) or fg_threshold for all. */
int segsde_depthcomp_mask(const float* depths, int B, long HW, float margin, float fg_threshold,
                          const float* fg_threshold_per_sample, int64_t* mask, void* stream);
/* generate_depth_mask: depth >= thr (one threshold), or (depth >= min(t)) <= max(t) as the reference writes it */
int segsde_depth_threshold_mask(const float* depth, long n, float t1, float t2, int two_thresholds, float* mask, void* stream);
/* generate_class_mask: N[h,w] = #{k : pred[h,w] == classes[k]} */
int segsde_class_mask(const int64_t* pred, long n, const int64_t* classes, int n_classes, int64_t* mask, void* stream);


/* ---- SURVEY.md 8(f) "next" rows: the trainer-side callers of the path ------------------------------------------------ */
/* One chunk of a multi-tensor operation: n <= 65536 contiguous floats of one tensor. */
typedef struct segsde_mt_chunk { float* dst; const float* src; long n; } segsde_mt_chunk;
/* EMA teacher update, train.py:346-358 (Trainer.update_ema_variables): dst = alpha*dst + one_minus_alpha*src for every
 * chunk of the DEVICE-resident table, one launch for all parameter tensors.  alpha / one_minus_alpha: the fp32 roundings
 * of the reference's Python doubles (min(1 - 1/(iteration+1), alpha_teacher) and 1 minus that). */
int segsde_multi_tensor_lerp(const segsde_mt_chunk* table_dev, int nchunks, float alpha, float one_minus_alpha, void* stream);
/* Pseudo labels of Trainer.calc_pseudo_label_loss, train.py:644-651: label = argmax_c prob (first maximum), ignore_index
 * where the maximum is 0; count[0] = #{max >= threshold}; max_prob (nullable) = the maxima; pixel_weight (nullable) =
 * count/(B*HW) broadcast to every pixel (the reference's unlabeled_weight * ones, without the host round trip). */
int segsde_pseudo_label(const float* prob_nchw, int B, int C, long HW, float threshold, int64_t ignore_index, int64_t* label,
                        float* max_prob, unsigned long long* count, float* pixel_weight, void* stream);
/* runningScore.update / _fast_hist (evaluation/metrics.py:12-25): hist[C*gt + pred] += 1 for every pixel with 0 <= gt < C,
 * accumulated into the DEVICE-resident hist[C*C].  Either pred (int64, as train.py:848 computes it) or logits (then the
 * argmax over the C class planes is fused; element strides sb / sc / sp for batch, class and pixel let the tensor be NCHW
 * or channels-last).  Integer atomics: exact. */
int segsde_confusion_update(const float* logits, long sb, long sc, long sp, const int64_t* pred, const int64_t* gt, int B,
                            long HW, int C, unsigned long long* hist, void* stream);

/* Teacher softmax of the unlabeled step, train.py:666 (torch.softmax(logits_u_w, dim=1)): NHWC logits rows (pitch ld)
 * -> class probabilities in NCHW planar layout, the layout segsde_mix / segsde_pseudo_label read. */
int segsde_softmax_nhwc_to_nchw(const float* logits, int ld, int B, long HW, int C, float* out_nchw, void* stream);
/* mix_use_gt, train.py:667-672 (``softmax_u_w[i] = unlabeled_inputs["onehot_lbl"][i]`` for every sample i of the unlabeled batch
 * whose ``is_labeled[i]`` is set): prob_nchw [B,C,HW] is overwritten IN PLACE with the one-hot planes (the loader's layout and
 * dtype, loader/sequence_segmentation_loader.py:237-246: int64 [C,H,W], all zero on ignored pixels; SEGSDE_DTYPE_*) of the
 * flagged samples; is_labeled is a DEVICE uint8 [B] (no host synchronisation).  Unflagged samples are not touched. */
int segsde_onehot_select(float* prob_nchw, const void* onehot, int onehot_dtype, const uint8_t* is_labeled, int B, int C,
                         long HW, void* stream);
/* Online-depth normalisation for the depthcomp mask, train.py:690-697, and the stored depth estimates of
 * DepthEstimator.prepare_depth_estimates, loader/depth_estimator.py:83-91: per sample b, out = (x - min_b) / (max_b - min_b)
 * (the reference's clamp to [min, max] is the identity); minmax (nullable) receives [B][2] = {min_b, max_b}; out_u8
 * (nullable) receives the 8-bit image ToPILImage makes of it (mul(255).byte()).  At least one of out / out_u8. */
size_t segsde_minmax_normalize_workspace(int B, long HW);
int segsde_minmax_normalize(const float* x, int B, long HW, float* out, float* minmax, uint8_t* out_u8, void* workspace,
                            size_t workspace_bytes, void* stream);
/* Fused photometric loss of one scale, both source frames per launch (loss/monodepth_loss.py:104-177 with
 * models/monodepth_layers.py:224-254): the per-stage entry points above chained through LDS tiles and registers.
 *   identity : err(src_f, target) for f = 0, 1 -> ident [B,2,H,W]  (identical for all scales: computed once, :139-147)
 *   forward  : err(pred_f, target), min over [ident (+ noise * 1e-5) | err] (avg: channel means first, :149-156), first
 *              minimum wins -> sel (uint8 index into the concatenation), identity_selection (nullable, :175-177),
 *              sum_out[0] = sum of the minima.  ident / noise nullable (disable_automasking).
 *   backward : d(scale * sum of minima) / d pred_f is formed in the tile (SSIM window statistics recomputed, reflection
 *              fold included) and pushed straight through the warp adjoint: g_disp_up [B,H,W] is WRITTEN (both frames
 *              summed), gT_f [B,4,4] += weight[0] * dL/dT_f (weight: nullable device scalar = upstream gradient).
 * pred_f are the warped frames [B,3,H,W] (segsde_warp_forward); T_f / src_f the pose and source frame of frame f. */
size_t segsde_photometric_workspace(int B, int H, int W);
int segsde_photometric_identity(const float* src0, const float* src1, const float* target, int B, int H, int W, int no_ssim,
                                float* ident, void* stream);
int segsde_photometric_forward(const float* pred0, const float* pred1, const float* target, const float* ident,
                               const float* noise, int B, int H, int W, int no_ssim, int avg, uint8_t* sel,
                               float* identity_selection, float* sum_out, void* workspace, size_t workspace_bytes,
                               void* stream);
int segsde_photometric_backward(const float* pred0, const float* pred1, const float* target, const uint8_t* sel, int n_ident,
                                const float* disp, int hs, int ws, const float* inv_K, const float* K, const float* T0,
                                const float* T1, const float* src0, const float* src1, int B, int H, int W, float min_depth,
                                float max_depth, int no_ssim, int avg, float scale, const float* weight, float* g_disp_up,
                                float* gT0, float* gT1, void* workspace, size_t workspace_bytes, void* stream);
/* Test-time depth, MonodepthLoss.generate_depth_test_pred, loss/monodepth_loss.py:54-62: bilinear upsample of disp
 * [B,1,hs,ws] to H x W (align_corners=False) and disp_to_depth (monodepth_layers.py:18-27) with the test depth range. */
int segsde_disp_to_depth(const float* disp, int hs, int ws, int B, int H, int W, float min_depth, float max_depth,
                         float* depth, void* stream);

/* strongTransform's colour jitter, loader/transformsgpu.py:10-17 (kornia 0.4.0 ColorJitter(s, s, s, s); third party, parity
 * unpinned): x, y [B,3,HW] planar; params DEVICE [B][4] = {brightness, contrast, saturation, hue} factors; order HOST int[4],
 * a permutation of {0 brightness, 1 contrast, 2 saturation, 3 hue}: clamp(x + (bf - 1)), clamp(x * cf), HSV s *= sf (clamped),
 * HSV h = fmod(h + 2 pi hf, 2 pi). */
int segsde_color_jitter(const float* x, int B, long HW, const float* params, const int* order, float* y, void* stream);
/* strongTransform's blur, loader/transformsgpu.py:20-30 (kornia 0.4.0 GaussianBlur2d, reflect border; parity unpinned):
 * separable -- column pass with the ny (odd) taps wy, then row pass with the nx taps wx -- over `planes` H x W planes;
 * tmp: planes*H*W floats; taps are DEVICE arrays (normalised Gaussian weights, possibly truncated to their non-zero support). */
int segsde_gaussian_blur(const float* x, int planes, int H, int W, const float* wy, int ny, const float* wx, int nx, float* tmp,
                         float* y, void* stream);

/* ------------------------------------------------------------------------------------------------ *
 * Device side of the data loader: decoded uint8 frames -> the training `inputs` tensors            *
 * (loader/sequence_segmentation_loader.py:203-342 + collation; csrc/batchprep.hip).  Bit-identical *
 * to PIL + ToTensor: integer resampling, one correctly rounded division by 255.                    *
 * crop_xy: DEVICE int32 [B][2] = {x1, y1} per sample (null: no crop, ch == H and cw == W required; *
 * offsets outside the frame are clamped); flip: DEVICE uint8 [B] (null: none).  The flip comes     *
 * BEFORE the crop (get_color :148-149, then random_crop :259-267).                                  *
 * ------------------------------------------------------------------------------------------------ */
/* frames [B,H,W,3] uint8 as decoded -> u8_out [B,3,ch,cw] (level 0 of the pyramid, planar) and f32_out [B,3,ch,cw] = u8 / 255
 * (ToTensor, :319). */
int segsde_batchprep_crop(const uint8_t* frames, int B, int H, int W, const int32_t* crop_xy, const uint8_t* flip, int ch, int cw,
                          uint8_t* u8_out, float* f32_out, void* stream);
/* One level of the colour pyramid (:308-309: transforms.Resize((h/2, w/2), Image.ANTIALIAS) of the level above): src
 * [planes,Hs,Ws] uint8 -> u8_out [planes,Hd,Wd] and f32_out = u8 / 255, Pillow's 8-bit Lanczos resampler (horizontal pass,
 * uint8 intermediate, vertical pass).  Exact halving only: SEGSDE_ERR_SHAPE unless Hs == 2 Hd and Ws == 2 Wd.
 * coef: DEVICE int32 [2][7][12], the fixed-point windows of the y axis then of the x axis by Pillow's formula (computed on
 * the host in float64): row r < 3 = output r, the last three rows in use (of min(n, 7)) = the last three outputs, row 3 =
 * every interior output; tap j of output i weighs source pixel 2 i - 5 + j, taps outside the image are zero. */
int segsde_batchprep_pyramid_level(const uint8_t* src, int planes, int Hs, int Ws, const int32_t* coef, int Hd, int Wd,
                                   uint8_t* u8_out, float* f32_out, void* stream);
/* lbl [B,H,W] uint8 label ids -> lbl_out [B,ch,cw] int64 = lut[id] (encode_segmap is a 256-entry table, DEVICE int64 [256];
 * :324-327); samples whose is_labeled (DEVICE uint8 [B], null: all labeled) is 0 get ignore_index everywhere (:227-229).
 * onehot_out (nullable) [B,n_classes,ch,cw] int64: plane c is 1 where the label is c; ignore pixels and unlabeled samples
 * are zero in every plane (:236-248). */
int segsde_batchprep_labels(const uint8_t* lbl, int B, int H, int W, const int32_t* crop_xy, const uint8_t* flip, int ch, int cw,
                            const int64_t* lut, const uint8_t* is_labeled, int64_t ignore_index, int n_classes, int64_t* lbl_out,
                            int64_t* onehot_out, void* stream);
/* one-channel 8-bit image (pseudo_depth, :272-273, :329-330): src [B,H,W] uint8 -> out [B,1,ch,cw] = u8 / 255 */
int segsde_batchprep_plane(const uint8_t* src, int B, int H, int W, const int32_t* crop_xy, const uint8_t* flip, int ch, int cw,
                           float* out, void* stream);
/* color_aug (:297-301, :318-322): torchvision 0.7.0's PIL ColorJitter + ToTensor on the planar level-0 crop that
 * segsde_batchprep_crop writes.  u8 [images,3,h,w] -> f32_out [images,3,h,w]; image i belongs to sample i % B (images = F * B:
 * the frames of a sample share its draw).  Per-sample DEVICE tables: apply uint8 [B] (0: f32_out = u8 / 255), alpha float32
 * [B][3] = the brightness, contrast and saturation factors as C floats, hue_shift int32 [B] in 0..255 = (uint8)(hue_factor *
 * 255), order uint8 [B][4] = the operation ids (0 brightness, 1 contrast, 2 saturation, 3 hue) in the order drawn; only the
 * low two bits of an id are looked at, a row that is no permutation is the caller's to reject.  Pillow's 8-bit arithmetic:
 * every operation reads and writes uint8, contrast blends with the mean L of the image as the operations before it left it
 * (one mean per image).  ops: bit i set = operation i runs (15: all, as ColorJitter does; a cleared bit skips that operation
 * in every sample).  sums: DEVICE uint32 [images] scratch for those means (zeroed here).  SEGSDE_ERR_SHAPE when h * w
 * exceeds SEGSDE_COLOR_JITTER_MAX_PIXELS (the sum of L is kept in 32 bits), images is no multiple of B or ops is outside 0..15. */
#define SEGSDE_COLOR_JITTER_MAX_PIXELS 16843009L /* (2^32 - 1) / 255 */
int segsde_batchprep_color_jitter(const uint8_t* u8, int images, int B, int h, int w, const uint8_t* apply, const float* alpha,
                                  const int32_t* hue_shift, const uint8_t* order, int ops, uint32_t* sums, float* f32_out, void* stream);
/* Colour-coded label maps (loader/mapillary_vistas_loader.py:58-66): lbl [B,H,W,3] uint8 -> lbl_out [B,ch,cw] int64 = the index
 * of the LAST entry of colors (DEVICE int32 [n_colors], r | g << 8 | b << 16) that equals the pixel, 0 when none does; the id
 * ignore_id (Mapillary's "unlabeled", 65; -1: none) becomes ignore_index.  Crop, flip, is_labeled and onehot_out as in
 * segsde_batchprep_labels.  SEGSDE_ERR_SHAPE when n_colors is outside 1..SEGSDE_LABEL_COLORS_MAX. */
#define SEGSDE_LABEL_COLORS_MAX 1024
int segsde_batchprep_labels_rgb(const uint8_t* lbl, int B, int H, int W, const int32_t* crop_xy, const uint8_t* flip, int ch, int cw,
                                const int32_t* colors, int n_colors, int ignore_id, const uint8_t* is_labeled, int64_t ignore_index,
                                int n_classes, int64_t* lbl_out, int64_t* onehot_out, void* stream);

/* pil_loader's resize (loader/loader_utils.py:23-43) in front of the stage above: decoded images of any size -> the working
 * size (csrc/resize.hip).  Samples of one launch may differ in source size; each is described by one row of desc, DEVICE
 * int64 [n][8] = { src, dst, bounds, weights (four DEVICE addresses), in_h, in_w, taps, 0 }.
 *
 * Image.ANTIALIAS (Pillow's 8-bit Lanczos resampler, Resample.c) on HWC RGB images is two passes with a uint8 image between
 * them; a pass whose axis keeps its size is NOT launched (Pillow skips it).  Per axis and (in, out) pair the host supplies, by
 * Pillow's float64 formula, bounds int32 [out][2] = (first source pixel, taps in use) and weights int32 [out][taps] =
 * (int)(w * 2^22 +- 0.5); per output clip8((2^21 + sum_j weights[j] * pix[first + j]) >> 22).
 *   resample_rows: src [in_h][in_w][3] -> dst [in_h][Wd][3] (the horizontal pass); max_rows >= every in_h.
 *   resample_cols: src [in_h][row_bytes] -> dst [Hd][row_bytes] (the vertical pass; row_bytes = 3 * width; in_w is ignored).
 * max_taps >= every row's taps; max_span >= the number of source pixels (rows) from the first window's start to the last
 * window's end over any group of 64 outputs starting at a multiple of 64 (cols: 16 outputs at a multiple of 16).  Both size
 * the LDS stage; bounds that do not fit it, or that leave the source, are pulled back inside, never followed.
 * SEGSDE_ERR_UNSUPPORTED when max_taps exceeds SEGSDE_RESAMPLE_MAX_TAPS (a reduction by more than about 10.3) or the stage
 * does not fit 64 KiB of LDS.
 *
 * Image.NEAREST on maps of 1 or 3 bytes per pixel: src [in_h][in_w][channels] -> dst [Hd][Wd][channels] =
 * src[bounds[y]][weights[x]], the two being the source row of every output row (int32 [Hd]) and the source column of every
 * output column (int32 [Wd]); indices outside the source are clamped. */
#define SEGSDE_RESAMPLE_MAX_TAPS 64
int segsde_batchprep_resample_rows(const void* desc, int n, int max_rows, int Wd, int max_taps, int max_span, void* stream);
int segsde_batchprep_resample_cols(const void* desc, int n, int row_bytes, int Hd, int max_taps, int max_span, void* stream);
int segsde_batchprep_resize_nearest(const void* desc, int n, int Hd, int Wd, int channels, void* stream);

/* ---- label selection (label_selection.py of the reference: uncertainty scores, depth-feature diversity), csrc/labelsel.hip ----
 * All sums are block partials in the workspace folded by a finish pass in a fixed order (no float atomics): every result is a
 * pure function of the inputs.
 *
 * segsde_labelsel_score: the per-image scores of label_selection.py:449-488 in one pass.  logits [B,C,H,W] are read through
 * their element strides (sb, sc, sh, sw: dense NCHW or channels-last); disp_pred / disp_pseudo are dense [B,H,W]; types is a HOST
 * array of T (0..SEGSDE_LABELSEL_MAX_TYPES) SEGSDE_DEPTH_ERR_* codes.  table [B][1+T] (device) receives (mean entropy, mean error
 * of every type); entropy_map [B,H,W] and error_maps [B,T,H,W] are optional (null = not wanted).  Entropy per pixel:
 * -sum p log2(p + 1e-30) / log2(C), p = softmax with the maximum subtracted (loss/loss.py:40-47).  Every error map is multiplied
 * by 1 - dilate(disp_pseudo < 0.07, 7, 3) (the maximum over the 7x7 window, zero padding) and rows >= (int)(0.87 * H) are zero;
 * the means run over all H*W pixels.  2 <= C <= SEGSDE_LABELSEL_MAX_CLASSES, else SEGSDE_ERR_UNSUPPORTED (log2(1) = 0 divides).
 * With T == 0 the two disparity pointers may be null. */
enum { SEGSDE_DEPTH_ERR_ABS = 0, SEGSDE_DEPTH_ERR_ABS_INV_LOG = 1, SEGSDE_DEPTH_ERR_ABS_INV = 2, SEGSDE_DEPTH_ERR_SQ = 3,
       SEGSDE_DEPTH_ERR_ABS_REL = 4, SEGSDE_DEPTH_ERR_SQ_REL = 5, SEGSDE_DEPTH_ERR_ABS_LOG = 6 };
#define SEGSDE_LABELSEL_MAX_TYPES 7
#define SEGSDE_LABELSEL_MAX_CLASSES 160
size_t segsde_labelsel_score_workspace(int B, int H, int W, int T);
int segsde_labelsel_score(const float* logits, long sb, long sc, long sh, long sw, int B, int C, int H, int W,
                          const float* disp_pred, const float* disp_pseudo, const int* types, int T, float* table,
                          float* entropy_map, float* error_maps, void* workspace, size_t workspace_bytes, void* stream);
/* adaptive_avg_pool2d (is_max = 0) / adaptive_max_pool2d (is_max = 1) of x [B,C,H,W] (element strides) to (h, 2h) with PyTorch's
 * bins  start = floor(i * H / oh), end = ceil((i + 1) * H / oh), written to rows [row0, row0 + B) of the float32 bank
 * [N][ld_bank >= C*h*2h] in the element order of an NCHW flatten(1).  transform: SEGSDE_POOL_* applied to every input element
 * first (label_selection.py:417-426: the depth / logdepth feature modes). */
enum { SEGSDE_POOL_NONE = 0, SEGSDE_POOL_INV_CLAMP = 1 /* clamp(1/x, 0.1, 80) */, SEGSDE_POOL_LOG_INV_CLAMP = 2 /* its log */ };
int segsde_labelsel_pool(const float* x, long sb, long sc, long sh, long sw, int B, int C, int H, int W, int h, int is_max,
                         int transform, float* bank, long ld_bank, long N, long row0, void* stream);
/* (f - mean_c) / std_c in place over the bank [N][ld >= C*P] (P = h*2h positions per channel), per channel over the N rows and
 * P positions; std is the unbiased one of torch.std_mean (two passes: the mean, then the squared deviations from it, both
 * accumulated in double).  A constant channel becomes 0/0 = NaN as in the reference. */
size_t segsde_labelsel_normalize_workspace(long N, int C, int P);
int segsde_labelsel_normalize(float* bank, long ld, long N, int C, int P, void* workspace, size_t workspace_bytes, void* stream);
/* The N x N distance matrix of the bank rows (label_selection.py:574-624 without patch_wise): out[i][j] = (sum_k |a_ik - a_jk|^p)^(1/p),
 * p = 2 or 1 (anything else: SEGSDE_ERR_UNSUPPORTED), in the direct form in fp32: the terms of each chunk of 32 features are summed
 * in ascending k and the chunk sums join the total by a compensated (Kahan) addition, so the sources must not be built with
 * fast-math (both build recipes use -ffp-contract=off and no -ffast-math).  Identical rows give exactly 0 and
 * out[i][j] == out[j][i] bit for bit (only the tiles on and above the diagonal are computed; both halves are
 * written).  Then, when bias (device [N], nullable) is given, out[i][j] += bias[j] (a column bias), and the diagonal is set to 0.
 * out has leading dimension ldo >= N; columns >= N of a row are not touched. */
int segsde_labelsel_distance(const float* bank, long ld, int N, int D, int p, const float* bias, float* out, long ldo,
                             void* stream);
/* The patch-wise distances of label_selection.py:582-612 (patch_wise=True), a directed Chamfer distance between images:
 * out[i][j] = (1/P) sum_a min_b (sum_c |f_i[c][a] - f_j[c][b]|^p)^(1/p), a, b in [0, P), p = 2 or 1.  bank is the [N][ld >= C*P]
 * feature bank: patch a of image n is bank[n*ld + c*P + a], c = 0..C-1.  Direct form only; the C terms are summed as in
 * segsde_labelsel_distance (chunks of 32 channels in ascending c, compensated addition of the chunk sums).  The minimum is taken
 * by comparisons on the sums (squared sums for p = 2, one sqrtf per winner) and a NaN operand makes it NaN, as torch.min does;
 * the P minima are added in ascending a and divided by (float)P.  Then + bias[j] (device [N], nullable), and the diagonal is
 * written as 0.  The pair distance is symmetric and evaluated once for out[i][j] and out[j][i], but out is NOT symmetric
 * (except at P = 1, where it is bit for bit).  An image whose patches are a permutation of another's is at distance exactly 0;
 * the order of the patches of image j does not change a bit of column j.  No atomics, no workspace: a pure function of the inputs.
 * Limits (SEGSDE_ERR_UNSUPPORTED otherwise): p in {1, 2}; 1 <= P <= SEGSDE_LABELSEL_PATCH_MAX_P; N*P < 2^31; at most 65535 groups
 * of max(1, 64 / P) images.  Columns >= N of a row of out are not touched. */
#define SEGSDE_LABELSEL_PATCH_MAX_P 128
int segsde_labelsel_patch_distance(const float* bank, long ld, int N, int C, int P, int p, const float* bias, float* out, long ldo,
                                   void* stream);
/* iterative_farthest_point (label_selection.py:627-648) in one launch of one workgroup: the running minimum over the rows of
 * the current samples and one membership byte per sample live in LDS (5 bytes per sample: N <= SEGSDE_LABELSEL_FPS_MAX_N, else
 * SEGSDE_ERR_UNSUPPORTED).  dist: float32 [N][ld]; current: device int32 [n_current] (n_current >= 1, indices in [0, N));
 * preselected: device uint8 [N] mask or null -- columns outside it read as 0 and stay in the competition.  Up to n_new times:
 * the column with the largest running minimum wins (ties: the lowest index); if it is already a current sample the loop stops;
 * otherwise it is recorded with its value, marked, and its row folded into the minimum.  out_idx int32 [n_new], out_dist
 * float32 [n_new], out_count int32 [1] (device).  Comparisons only: bit-exact for a given matrix.  A matrix that holds NaN
 * gives an unspecified selection. */
#define SEGSDE_LABELSEL_FPS_MAX_N 32000
int segsde_labelsel_farthest_point(const float* dist, long ld, int N, const int* current, int n_current,
                                   const uint8_t* preselected, int n_new, int* out_idx, float* out_dist, int* out_count,
                                   void* stream);

/* ---- rendering of inference outputs (inference.py:84-116, train.py:904-923 and _colorize, train.py:137-151, of the reference),
 * csrc/render.hip.  The uint8 images are byte for byte what the reference hands to its file writer; the outputs are DENSE tensors
 * whose base address is a multiple of 4 (else SEGSDE_ERR_UNSUPPORTED).  Integer work and comparisons only, except where stated.
 *
 * segsde_render_labels: class ids -> palette colours, rgb uint8 [B,H,W,3], and optionally the id plane ids_out uint8 [B,H,W]
 * (ids above 255 saturate).  The ids are either the argmax over the C class planes of logits [B,C,H,W], read through their
 * element strides (sb, sc, sh, sw: dense NCHW, channels-last, channel slices, pitched rows) -- first maximum, strict >, which is
 * torch.max(1)[1] on the CPU for finite and infinite values; a pixel whose classes hold NaN is unspecified -- or, when logits is
 * null, the map ids [B,H,W] (dense; ids_dtype SEGSDE_DTYPE_I64 or SEGSDE_DTYPE_U8; read as non-negative).  palette: device uint8
 * [n][3], 1 <= n <= SEGSDE_RENDER_MAX_COLORS.  An id v >= n follows `unmapped`: KEEP writes min(v, 255) into the three channels
 * (Cityscapes.decode_segmap_tocolor starts from a copy of the map and save_image clamps), ZERO writes black (the Mapillary and
 * CamVid decoders start from zeros). */
enum { SEGSDE_RENDER_UNMAPPED_KEEP = 0, SEGSDE_RENDER_UNMAPPED_ZERO = 1 };
#define SEGSDE_RENDER_MAX_COLORS 256
int segsde_render_labels(const float* logits, long sb, long sc, long sh, long sw, const void* ids, int ids_dtype, int B, int C,
                         int H, int W, const uint8_t* palette, int n, int unmapped, uint8_t* rgb, uint8_t* ids_out, void* stream);
/* float32 image x [B,C,H,W] (element strides; C = 1 or 3, else SEGSDE_ERR_UNSUPPORTED) -> out uint8 [B,H,W,C] as torchvision
 * 0.7.0's save_image computes it: x.mul(255).add_(0.5).clamp_(0, 255), then truncation.  The product and the sum are two
 * separately rounded fp32 operations (the sources must not be compiled with floating-point contraction); NaN gives 0, +-inf
 * saturate. */
int segsde_render_unit_image(const float* x, long sb, long sc, long sh, long sw, int B, int C, int H, int W, uint8_t* out,
                             void* stream);
/* _colorize(img, cmap, mask_zero, max_percentile = 100) per image of img [B,H,W] (dense float32) -> out float32 [B,H,W,3].
 * Pass 1 leaves the block partials of np.min / np.max per image in the workspace; pass 2, in fp32 as numpy and matplotlib's
 * Colormap.__call__ do it:  q = clip(x, vmin, vmax) / vmax,  s = q * N,  index = N-1 if s == N, else N (under) if s < 0, else
 * N+1 (over) if s > N, else N+2 (bad) if s is NaN, else trunc(s);  out = lut[index], or (1,1,1) where mask_zero and x <= 0.
 * lut: device float32 [N+3][3], rows 0..N-1 the map, then its under, over and bad colours; 1 <= N <= SEGSDE_COLORIZE_MAX_N.
 * An all-zero image is 0/0 = NaN = the bad colour, as in the reference.  min / max / clip propagate NaN as numpy's do. */
#define SEGSDE_COLORIZE_MAX_N 1024
size_t segsde_colorize_workspace(int B, int H, int W);
int segsde_colorize(const float* img, int B, int H, int W, const float* lut, int N, int mask_zero, float* out, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ---- depth evaluation (the metrics of MonodepthLoss.depth_metric_names: abs_rel, sq_rel, rms, log_rms, a1, a2, a3 with median
 * scaling, the usual monocular-depth protocol), csrc/depthmetrics.hip.  gt, pred: dense float32 [B,H,W] on the device; table:
 * device float64 [B][SEGSDE_DEPTH_ERRORS_COLUMNS].  Comparisons and per-pixel arithmetic in fp32, sums in float64.  Per image:
 *   valid pixel: gt > min_depth, gt < max_depth (a NaN gt is invalid), inside the crop [y0,y1) x [x0,x1) (full image: 0,H,0,W); n
 *   of them.  med_gt, med_pred: the medians of gt and of pred over the valid pixels as np.median gives them for a float32 array
 *   (odd n: the middle element; even n: (lo + hi) / 2 in fp32), bit for bit: an exact radix selection on the float bits in the
 *   IEEE order of finite values (negative and subnormal predictions included).  A NaN prediction at a valid pixel, and which of
 *   -0 / +0 a median is, are unspecified.
 *   ratio = scale * (med_gt / med_pred) if median_scaling, else scale (one fp32 division, one fp32 multiplication).
 *   p = min(max(pred * ratio, min_depth), max_depth), g = gt, t = max(g / p, p / g).
 *   columns 0-6: abs_rel = mean |g - p| / g, sq_rel = mean (g - p)^2 / g, rms = sqrt(mean (g - p)^2), log_rms = sqrt(mean (log g -
 *   log p)^2), a_k = #{t < 1.25^k} / n (k = 1, 2, 3); columns 7-13: n, n_a1, n_a2, n_a3, med_gt, med_pred, ratio.
 *   An image without a valid pixel gets n = 0 and NaN in every other column.
 * No host synchronisation, no copy to the host; launches and grid sizes depend on the arguments only.  Block partials are folded
 * in a fixed order, counts are integer atomics: every result is a pure function of the inputs.
 * SEGSDE_ERR_SHAPE: B, H, W <= 0, an empty crop or one outside the image, !(0 <= min_depth < max_depth).  SEGSDE_ERR_UNSUPPORTED:
 * H * W >= 2^32, B > 65535, a workspace that is not 8-byte aligned.  The workspace size is that of the full image for any crop. */
#define SEGSDE_DEPTH_ERRORS_COLUMNS 14
size_t segsde_depth_errors_workspace(int B, int H, int W);
int segsde_depth_errors(const float* gt, const float* pred, int B, int H, int W, float min_depth, float max_depth,
                        int median_scaling, float scale, int y0, int y1, int x0, int x1, double* table, void* workspace,
                        size_t workspace_bytes, void* stream);

/* ---- segmentation validation at label resolution (train.py:836-851 with loss.py:17-37 as the loss), csrc/segeval.hip.
 * logits: float32 [B,C,Hi,Wi] on the device addressed by four ELEMENT strides (batch, class, row, pixel): dense NCHW,
 * channels-last and slices need no copy; the batch and class offsets are 64-bit.  labels: dense int64 [B,Ht,Wt], any Hi,Wi ->
 * Ht,Wt ratio.  For every label pixel the C logits are interpolated as F.interpolate(mode="bilinear", align_corners=True) does in
 * fp32 (the arithmetic of segsde_resize_bilinear_forward, bit for bit), then
 *   argmax over the classes: strict >, the lowest index wins a tie (segsde_confusion_update's rule; NaN logits: unspecified);
 *   hist[C * label + argmax] += 1                                    where 0 <= label < C          (hist: [C*C], ACCUMULATED);
 *   loss[0] += logsumexp(z) - z[label], loss[1] += 1                 where label != ignore_index and 0 <= label < C
 *                                                                    (fp32 with the maximum subtracted, summed in float64;
 *                                                                    loss: double[2], OVERWRITTEN);
 *   ids[pixel] = argmax                                              (uint8 [B,Ht,Wt]).
 * Each of hist, loss, ids may be null (not all three).  A label outside [0,C) other than ignore_index counts nowhere.
 * One launch (plus a one-block fold of the loss partials), no host synchronisation.  Block-private histograms with integer
 * atomics and block partials folded in a fixed order: two calls give identical bits.
 * SEGSDE_ERR_NULL: logits, labels, all three outputs, or loss without a workspace.  SEGSDE_ERR_SHAPE: B, C, Hi, Wi, Ht, Wt <= 0.
 * SEGSDE_ERR_UNSUPPORTED: a C whose C*C histogram leaves no room for a tile in 64 KB of LDS (C <= 125 works), C > 256 with ids,
 * Ht * Wt >= 2^32, more than 2^31 - 1 tiles, a workspace that is not 8-byte aligned.  SEGSDE_ERR_WORKSPACE: loss asked for and
 * fewer than segsde_seg_eval_workspace(B, Ht, Wt) bytes.
 * segsde_seg_eval_plan: the label rows per tile (16, 8 or 4; tiles are 64 pixels wide) when the tile's source footprint is staged
 * in LDS, 0 when the taps are read straight from memory (the footprint fits at no tile height), or an error code as above. */
size_t segsde_seg_eval_workspace(int B, int Ht, int Wt);
int segsde_seg_eval_plan(int C, int Hi, int Wi, int Ht, int Wt);
int segsde_seg_eval(const float* logits, long sb, long sc, long sh, long sw, int B, int C, int Hi, int Wi, const int64_t* labels,
                    int Ht, int Wt, int64_t ignore_index, unsigned long long* hist, double* loss, unsigned char* ids,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- segmentation evaluation with test-time ensembling at label resolution, csrc/segens.hip (not in the reference, which
 * evaluates one view).  K <= SEGSDE_SEG_ENS_MAX_VIEWS views of the same B images: view k holds float32 logits [B,C,Hi,Wi] on the
 * device, addressed like the logits of segsde_seg_eval by four ELEMENT strides, a flip flag and a weight >= 0.  The array of
 * descriptors is HOST memory; the call copies what it needs into the kernel arguments, so the array may be released on return.
 * For every label pixel, views in the given order (a view of weight 0 is not read, as if it were not in the list):
 *   z = the C logits interpolated as segsde_seg_eval interpolates them (align_corners=True, fp32); a view with flip != 0 is read
 *   at source column Wi - 1 - i for tap column i: the network saw the mirrored image, its output is mirrored back;
 *   p = softmax(z) in fp32: exp(z - max z) / sum;   acc[c] += float(weight / sum of the weights, formed in double) * p[c];
 * then   argmax over acc: strict >, the lowest index wins a tie (NaN logits: unspecified);
 *   hist[C * label + argmax] += 1                                    where 0 <= label < C          (hist: [C*C], ACCUMULATED);
 *   loss[0] += -log(max(acc[label], FLT_MIN)), loss[1] += 1          where label != ignore_index and 0 <= label < C
 *                                                                    (fp32 terms summed in float64; loss: double[2], OVERWRITTEN);
 *   ids[pixel] = argmax                                              (uint8 [B,Ht,Wt]).
 * Each of hist, loss, ids may be null (not all three); labels (dense int64 [B,Ht,Wt]) may be null when only ids are asked for.
 * A label outside [0,C) other than ignore_index counts nowhere.  The resized logits and the probabilities are never written to
 * memory.  One launch whatever K is (plus a one-block fold of the loss partials), no host synchronisation.  Block-private
 * histograms with integer atomics, block partials folded in a fixed order, no float atomics: two calls give identical bits.
 * SEGSDE_ERR_NULL: views, the logits of a view with weight > 0, all three outputs, loss without a workspace, hist or loss without
 * labels.  SEGSDE_ERR_SHAPE: K < 1 or K > SEGSDE_SEG_ENS_MAX_VIEWS, a weight that is negative, NaN or infinite, all weights 0,
 * Hi, Wi, B, C, Ht, Wt <= 0.  SEGSDE_ERR_UNSUPPORTED: C > SEGSDE_SEG_ENS_MAX_CLASSES (the C*C histogram and a one-row tile's
 * accumulator no longer fit the 160 KB of LDS of a workgroup), Ht * Wt >= 2^32, more than 2^31 - 1 tiles, a workspace that is not
 * 8-byte aligned, a device that does not grant the LDS.  SEGSDE_ERR_WORKSPACE: loss asked for and fewer than
 * segsde_seg_ens_workspace(B, Ht, Wt) bytes.
 * segsde_seg_ens_plan: the label rows per tile (16, 8, 4, 2 or 1; tiles are 64 pixels wide) the call would use, or an error code
 * as above; reads Hi, Wi and weight of the descriptors only.  staged (int[K], may be null): per view 1 when the tile's source
 * footprint is staged in LDS, 0 when its taps are read straight from memory (the footprint does not fit, or it holds more source
 * pixels than the tile reads taps: downscaling by more than about two per axis), -1 for a view of weight 0. */
#define SEGSDE_SEG_ENS_MAX_VIEWS 16
#define SEGSDE_SEG_ENS_MAX_CLASSES 171
typedef struct segsde_seg_ens_view {
  const float* logits;
  long sb, sc, sh, sw;
  int Hi, Wi;
  int flip;
  float weight;
} segsde_seg_ens_view;
size_t segsde_seg_ens_workspace(int B, int Ht, int Wt);
int segsde_seg_ens_plan(const segsde_seg_ens_view* views, int K, int C, int Ht, int Wt, int* staged);
int segsde_seg_ens(const segsde_seg_ens_view* views, int K, int B, int C, const int64_t* labels, int Ht, int Wt,
                   int64_t ignore_index, unsigned long long* hist, double* loss, unsigned char* ids, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ---- BerHu pseudo-depth distillation loss (loss.py:5-15; the depth loss of experiments.py:229-301 and a term of every DepthMix
 * validation, train.py:489-496, 870-878), csrc/berhu.hip.  input, target, mask: dense float32 tensors of n elements on the device
 * (mask may be null: all ones).  With apply_log, input and target are replaced by log(1 + .) first.
 *   a = |target - input| * mask * keep,  keep = 1, or with keep_rows >= 0 (the tensors are [.., H, W], H * W divides n): 1 where the
 *   element's row (e / W) % H is < keep_rows, else 0 -- the own-car crop of both callers without a mask tensor;
 *   C = float32(threshold * double(max a));
 *   loss[0] = sum over ALL n elements of (a <= C ? a : (a * a + C * C) / (2 * C)), per element in fp32, summed in double, / n;
 *   state[0] = max a (bit for bit the fp32 maximum), state[1] = C: kept for the backward pass.
 * Backward: dinput = gscale[0] / n * -sign(target - input) * mask * keep * (a <= C ? 1 : a / C), divided by (1 + input) with
 * apply_log; gscale is a DEVICE scalar (the incoming gradient), C a constant as in the reference (it detaches C with .item());
 * exactly 0 wherever a == 0.  max a == 0 gives loss 0 and an all-zero gradient (the reference returns NaN gradients there, the
 * 0/0 of torch.where's unselected branch).  NaN inputs: unspecified.
 * Forward: three launches (block maxima; C and block sums in double; a fixed-order fold), backward: one; no host synchronisation,
 * no atomics: two calls give identical bits.  16-byte accesses when every tensor starts on a 16-byte boundary.
 * SEGSDE_ERR_SHAPE: n <= 0, keep_rows < -1, with keep_rows >= 0: H, W <= 0, keep_rows > H or n % (H * W) != 0 (H, W are not read
 * otherwise), !(0 < threshold < inf).  SEGSDE_ERR_WORKSPACE: fewer than the workspace function's bytes.  SEGSDE_ERR_UNSUPPORTED:
 * a tensor that is not 4-byte aligned, a workspace that is not 8-byte aligned. */
size_t segsde_berhu_workspace(long n);
int segsde_berhu_forward(const float* input, const float* target, const float* mask, long n, int H, int W, int keep_rows,
                         int apply_log, double threshold, float* loss, float* state, void* workspace, size_t workspace_bytes,
                         void* stream);
int segsde_berhu_backward(const float* input, const float* target, const float* mask, long n, int H, int W, int keep_rows,
                          int apply_log, const float* state, const float* gscale, float* dinput, void* stream);

/* ---- Mix masks for a whole batch (Trainer.generate_mix_mask, train.py:573-584 "class", 605-615 "depth", 616-636 "depthhist"),
 * csrc/mixmask.hip.  depth: dense float32 [B][HW]; pred: dense int64 [B][HW]; 1 <= HW < 2^31; B <= 65535.
 * segsde_depth_hist_thresholds: per image i, in order (train.py:616-631):
 *   x = depth (apply_log = 0) or logf(1.0f + depth) (apply_log = 1);
 *   counts, edges = np.histogram(x, bins=100) as numpy 2.2 computes it for float32 data: lo = min x, hi = max x (lo - 0.5, hi + 0.5
 *   when they are equal); edges[k] = float32(k) * ((hi - lo) / 100) + lo in fp32, product and sum rounded separately, edges[100] = hi;
 *   x counts in the bin k with edges[k] <= x < edges[k + 1], the last bin closed on the right;
 *   density[k] = counts[k] / double(edges[k + 1] - edges[k]) / HW, the edge difference in fp32 first;
 *   max_depth = edges[k + 1] of the highest k <= 98 with density[k] > 1.5; min_depth = edges[k] of the first k at which the running
 *   sum of the densities (ascending k, double) divided by their total exceeds 0.4;
 *   thr = u[i] * (max_depth - min_depth) + min_depth in fp32, product and sum rounded separately;
 *   table[i] = {min_depth, max_depth, thr, found}.  found = 1 when a bin qualified for max_depth.  Otherwise found = 0 and max_depth
 *   is that of image i - 1 of the same call, for image 0 its own edges[100] (the reference keeps the stale value of the previous
 *   image without saying so, and fails on the first image).
 * counts: uint32 [B][100] or null (the counters then live in the workspace).  u: device float32 [B].  Three launches (block minima
 * and maxima; histogram in block-private LDS counters flushed with integer atomics; one block for the scans), no host
 * synchronisation, no float atomics: two calls give identical bits.  NaN and depth <= -1 with apply_log: unspecified.
 * segsde_depth_threshold_mask_batch: mask[b][p] = depth[b][p] >= thr[b * thr_stride] ? 1 : 0 (float32), thr in device memory --
 * thr = table + 2, thr_stride = 4 reads the thresholds where the call above left them.  One launch.
 * segsde_class_presence: counts[b][id + 1] = number of pixels of image b with that id, ids -1 .. 254 (slot 0 is the -1 that
 * segsde_pseudo_label writes for ignore_index = -1); other ids are counted nowhere.  counts (uint32 [B][256]) is zeroed by the call.
 * segsde_class_mask_batch: mask[b][p] = selected[b][pred[b][p] + 1] (uint8 [B][256]) for ids -1 .. 254, else 0 -- the
 * generate_class_mask (transformmasks.py:27-30) of every image of the batch against its own class list, one launch.
 * Checks, in this order, before any launch: SEGSDE_ERR_NULL; SEGSDE_ERR_SHAPE (B < 1, HW < 1, HW >= 2^31, thr_stride < 0);
 * SEGSDE_ERR_UNSUPPORTED for B > 65535; SEGSDE_ERR_WORKSPACE (fewer than the workspace function's bytes; 0 for a refused shape);
 * SEGSDE_ERR_UNSUPPORTED for a pointer that is not aligned to its element type. */
size_t segsde_depth_hist_workspace(int B, long HW);
int segsde_depth_hist_thresholds(const float* depth, int B, long HW, int apply_log, const float* u, float* table, unsigned* counts,
                                 void* workspace, size_t workspace_bytes, void* stream);
int segsde_depth_threshold_mask_batch(const float* depth, int B, long HW, const float* thr, long thr_stride, float* mask, void* stream);
int segsde_class_presence(const int64_t* pred, int B, long HW, unsigned* counts, void* stream);
int segsde_class_mask_batch(const int64_t* pred, int B, long HW, const unsigned char* selected, int64_t* mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEGSDE_HIP_H */
