/* os2d_train.h -- C ABI of libos2d_train.so: the backward pass of the OS2D head (reference os2d/modeling/head.py:308-435 under
 * autograd) for the MI355X (gfx950), strict fp32, and - since ABI version 2 - the target assignment and the training
 * objective, hard-patch mining, and the gradient clip + optimiser step (the last sections of this file).
 *
 * The forward of a training step is the "f32" route of libos2d_hip.so, run stage by stage (os2d_fm_sumsq, os2d_corr,
 * os2d_transform_conv x 3, os2d_sample_decode) so that its intermediates stay alive: corr [NB,225,HW], the relu + L2
 * normalised correlation rnorm [NB,226,PLANE], h1 [NB,128,PLANE], h2 [NB,64,PLANE] (after BatchNorm and ReLU) and the
 * transformation parameters params [NB,P,HW].  NB = A*B (image-major pairs), HW = H*W, PLANE = os2d_plane_floats(H,W) of
 * os2d_hip.h: the zero-bordered plane layout of the TransformNet activations (cell (h,w) at BASE + h*(W+3) + w).
 *
 * Conventions as os2d_hip.h: device pointers owned by the caller, fp32, dense; asynchronous on `stream`; 0 on success,
 * negative on error (-1 bad argument, -2 workspace too small, -3 unsupported shape, -4 HIP runtime error), described by
 * os2d_train_last_error() on the calling thread.  Arguments are checked before anything is launched.
 *
 * Arithmetic: fp32 throughout, unless a caller asks the *_ex entry points for the split-fp16 GEMMs.  The matrix-shaped work
 * (the transposed convolutions, the weight gradients, the two correlation GEMMs) runs on v_mfma_f32_16x16x4_f32.  Weight
 * gradients reduce over NB * PLANE positions in split-K partial sums that a second kernel adds in a fixed order:
 * deterministic.  The resampling backward scatters into d corr with fp32 atomicAdd: the order of those additions is not
 * fixed (as in torch's own grid_sample backward), unless the caller takes os2d_train_decode_backward_det, which adds 64-bit
 * integers on a fixed-point grid instead.                                                                                  */
#ifndef OS2D_TRAIN_H
#define OS2D_TRAIN_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OS2D_TRAIN_ABI_VERSION 2

int os2d_train_abi_version(void);
const char* os2d_train_last_error(void);

/* ---- (a) resample + pool + box decode backward (head.py:371-435).  corr [NB,225,HW], params [NB,P,HW] as the forward used
 * them; upstream gradients dcls [NB,HW], dcls_det [NB,HW], dloc [NB,4,HW] (each may be NULL = zero).  dcls + dcls_det are
 * ADDED into dcorr [NB,225,HW] (atomicAdd; the caller zeroes it); dcls and dloc give dparams [NB,P,HW] (written).  The
 * corners carry no gradient (head.py:423).  stride / rec_field as os2d_sample_decode.                                     */
int os2d_train_decode_backward(const float* corr, const float* params, const float* dcls, const float* dcls_det, const float* dloc,
                               int NB, int H, int W, int P, int inverse, int stride, int rec_field, float* dcorr, float* dparams,
                               void* stream);

/* ---- the same stage with an order-independent d corr scatter: two calls on the same inputs give the same bits, and a pair's
 * d corr depends neither on the order in which its addends arrive nor on the other pairs of the batch.  Arguments, dparams
 * (bit for bit) and the contract of dcorr (ADDED into) as os2d_train_decode_backward.  Three launches:
 *   maxima   word[nb] = max over the pair's locations of |dcls + dcls_det| (the fp32 sum), as fp32 bits, by atomicMax;
 *   scatter  every addend (formed in fp32 as in the float kernel) is multiplied by 2^e - exact - rounded to the nearest
 *            integer and added with a 64-bit integer atomic to the cell's sum; e = os2d_train_decode_det_exponent(word[nb], H, W)
 *            puts the pair's maximum m at m 2^e in [2^(60-L), 2^(61-L)), L = ceil(log2(4 H W)): a cell receives at most 4 H W
 *            addends of at most m / 121 each, so no sum reaches 2^62;
 *   convert  dcorr[cell] += (float)((double)sum * 2^-e); a cell whose sum is 0 is left as it is.
 * A pair whose word is zero adds nothing.  A pair whose word is not finite (>= 0x7f800000: a NaN or Inf among its dcls +
 * dcls_det) gets NaN in EVERY cell of its dcorr; other pairs are not affected.  That is the only non-finite input this route
 * reports through dcorr: where the pair's word is finite but an addend is not (a NaN or Inf in params makes the sample
 * coordinates, hence the bilinear weights, NaN), the addend's integer is unspecified and the float entry point's NaN in the
 * touched dcorr cells does not appear; dparams carries that NaN on both routes.  No floating-point atomics.
 * workspace: os2d_train_decode_backward_det_workspace_bytes(NB, H, W) bytes (0 = bad or refused shape), 8-byte aligned; the call
 * clears it and leaves in it  [0, NB*225*HW*8)  the sums, int64 [NB,225,HW] in units of 2^-e of their pair, then NB uint32
 * pair words; the total is rounded up to a multiple of 256 bytes.
 * Refused with -3: NB > 65535, and H*W > 2^21 (L > 23), where the grid step 2^-e could exceed 2^-30 of the pair's largest
 * possible addend m / 121.
 * os2d_train_decode_det_exponent runs on the host and needs no device: e for a finite non-zero word (-90 <= e <= 207), else
 * one of the three values below.                                                                                          */
#define OS2D_TRAIN_DET_ZERO (-1000)        /* the word is zero: the pair adds nothing */
#define OS2D_TRAIN_DET_NONFINITE (-1001)   /* the word is >= 0x7f800000: the pair's dcorr becomes NaN */
#define OS2D_TRAIN_DET_REFUSED (-1002)     /* H, W < 1 or H*W > 2^21 */
size_t os2d_train_decode_backward_det_workspace_bytes(int NB, int H, int W);
int os2d_train_decode_backward_det(const float* corr, const float* params, const float* dcls, const float* dcls_det, const float* dloc,
                                   int NB, int H, int W, int P, int inverse, int stride, int rec_field, float* dcorr, float* dparams,
                                   void* workspace, size_t workspace_bytes, void* stream);
int os2d_train_decode_det_exponent(unsigned max_bits, int H, int W);

/* ---- layer 3 (64 -> P, 5x5, no BatchNorm): dparams [NB,P,HW] -> dy [NB,P,PLANE] (zero-bordered plane layout) and
 * dbias [P] = sum over pairs and positions (written; NULL = not computed).  One grid row per plane: NB * P <= 65535, else -1. */
int os2d_train_params_backward(const float* dparams, int NB, int P, int H, int W, float* dy, float* dbias, void* stream);

/* ---- frozen (eval-mode) BatchNorm + ReLU backward of layer 1 (128 channels) or 2 (64): dh [NB,Cout,PLANE] = gradient of
 * the layer's output h [NB,Cout,PLANE]; gamma / beta / running_var of the BatchNorm, eps its epsilon.  Writes dy
 * [NB,Cout,PLANE] = dh * (h > 0) * gamma / sqrt(var + eps) (the gradient of the convolution output; zero at pad cells) and
 * dgamma, dbeta, dbias [Cout] (each may be NULL: not computed).  dgamma uses (h - beta) / gamma for the normalised
 * pre-activation: a channel with gamma == 0 gets dgamma = 0.  One grid row per plane: NB * Cout <= 65535 (NB <= 511 for layer 1,
 * <= 1023 for layer 2), else -1.                                                                                        */
int os2d_train_bn_relu_backward(int layer, const float* dh, const float* h, const float* gamma, const float* beta,
                                const float* running_var, float eps, int NB, int H, int W, float* dy, float* dgamma, float* dbeta,
                                float* dbias, void* stream);

/* ---- convolution backward, layer 1 (225 -> 128, 7x7), 2 (128 -> 64, 5x5) or 3 (64 -> P, 5x5); w = the layer's raw weights
 * [Cout,Cin,k,k] (not BatchNorm-folded), dy [NB,Cout,PLANE] from the two calls above.
 *   data:   dx [NB,Cin,PLANE] (the transposed convolution; zero at pad cells).  workspace: os2d_train_conv_data_workspace_floats
 *           floats (the flipped, transposed filters).  One grid slice per pair: NB <= 65535, else -1.
 *   weight: dw [Cout,Cin,k,k] = sum over pairs and positions of dy x (written); x = the layer's input as the forward read it
 *           (layer 1: rnorm [NB,226,PLANE]; 2: h1 [NB,128,PLANE]; 3: h2 [NB,64,PLANE]).  The reduction over NB * PLANE is cut
 *           into as many split-K slices as fit `workspace_floats` (at most 64, at least one slice of Cout*Cin*k*k floats).   */
size_t os2d_train_conv_data_workspace_floats(int layer, int P);
int os2d_train_conv_backward_data(int layer, int P, const float* w, const float* dy, int NB, int H, int W, float* dx,
                                  float* workspace, size_t workspace_floats, void* stream);
size_t os2d_train_conv_weight_slice_floats(int layer, int P);
int os2d_train_conv_backward_weight(int layer, int P, const float* x, const float* dy, int NB, int H, int W, float* dw,
                                    float* workspace, size_t workspace_floats, void* stream);

/* ---- relu + L2 over the 225 channels (eps 1e-6, head.py:650) backward: dxn [NB,225,PLANE] = gradient of the normalised
 * tensor; ADDS the gradient of the raw correlation into dcorr [NB,225,HW].                                              */
int os2d_train_norm225_backward(const float* corr, const float* dxn, int NB, int H, int W, float* dcorr, void* stream);

/* ---- correlation + normalisation backward (head.py:339-350, 293): fm [A,C,H,W] raw image features, qp [B,C,256] the class
 * operand of os2d_class_prepare_batch (normalised, x-major channels), dcorr [A*B,225,HW].
 *   dfm [A,C,H,W]   gradient of the raw image features (image L2 over C, eps 1e-5), written; NULL = not computed;
 *   dq  [B,C,225]   gradient of the normalised class maps, x-major channel order (m = x*15 + y), written; NULL = not computed.
 * workspace: os2d_train_corr_workspace_floats(A,C,H,W) floats.                                                          */
size_t os2d_train_corr_workspace_floats(int A, int C, int H, int W);
int os2d_train_corr_backward(const float* fm, const float* qp, const float* dcorr, int A, int B, int C, int H, int W, float* dfm,
                             float* dq, float* workspace, size_t workspace_floats, void* stream);

/* ---- The same three GEMM-shaped entry points with a choice of arithmetic: arith 0 = fp32 (the functions above, bit for bit),
 * 1 = "f16x3": every operand value is multiplied by a power of two, split into fp16 hi + lo where it is staged on chip, and
 * the products hi*hi + hi*lo + lo*hi run on v_mfma_f32_32x32x16_f16 with fp32 accumulation; the result is within fp32
 * rounding of the fp32 route.  The power of two comes from the operand's largest magnitude, found on the device by a short
 * maxima pass per call (no host synchronisation): one per operand a GEMM reduces over as a whole (filters, qp, the normalised
 * image map, both operands of a weight gradient), one per pair for the dy of a data gradient, one per image / per class for the
 * dcorr of the two correlation GEMMs.  An all-zero operand gives exact zeros; a non-finite value reaches every output that
 * depends on it as a non-finite value (with the whole of its slice: the slice is then converted unscaled).  Tensors, layouts
 * and outputs (exact zeros at pad cells; split-K slices added in a fixed order) as above.  The f16x3 route keeps its maxima in
 * the workspace: size it with the _ex functions (arith 0: the sizes above; 0 = bad argument).  Any other arith: -1.         */
size_t os2d_train_conv_data_workspace_floats_ex(int arith, int layer, int P, int NB);
int os2d_train_conv_backward_data_ex(int arith, int layer, int P, const float* w, const float* dy, int NB, int H, int W, float* dx,
                                     float* workspace, size_t workspace_floats, void* stream);
size_t os2d_train_conv_weight_slice_floats_ex(int arith, int layer, int P);
int os2d_train_conv_backward_weight_ex(int arith, int layer, int P, const float* x, const float* dy, int NB, int H, int W, float* dw,
                                       float* workspace, size_t workspace_floats, void* stream);
size_t os2d_train_corr_workspace_floats_ex(int arith, int A, int B, int C, int H, int W);
int os2d_train_corr_backward_ex(int arith, const float* fm, const float* qp, const float* dcorr, int A, int B, int C, int H, int W,
                                float* dfm, float* dq, float* workspace, size_t workspace_floats, void* stream);

/* ==== Batch-statistics ("live") BatchNorm of TransformNet layer 1 (225 -> 128, 7x7) or 2 (128 -> 64, 5x5): what a training
 * forward runs for a layer whose BatchNorm is in training mode, and its backward (csrc_train/bn_live.hip).
 * n = NB*H*W values per channel: the data cells of the planes; pad cells are told by index and never read as data.  Plane tensors
 * 16-byte aligned.  Layer 3 has no BatchNorm: -1.  One grid row per plane: NB * Cout <= 65535, else -1.
 *
 * ---- the raw convolution: z [NB,Cout,PLANE] = conv(x) + bias at data cells, +0.0 at every other cell (no BatchNorm, no ReLU).
 * w [Cout,Cin,k,k] and bias [Cout] as the module holds them; x = rnorm [NB,226,PLANE] (plane 225 is never read) or h1
 * [NB,128,PLANE].  arith 0: the fp32 GEMM of the backward pass; 1: the split-fp16 GEMM (maxima passes on the device: one word for
 * the filters, one per pair of x), within fp32 rounding of it.  workspace: os2d_train_conv_forward_workspace_floats floats
 * (0 = bad argument).                                                                                                       */
size_t os2d_train_conv_forward_workspace_floats(int arith, int layer, int P, int NB);
int os2d_train_conv_forward(int arith, int layer, int P, const float* w, const float* bias, const float* x, int NB, int H, int W, float* z,
                            float* workspace, size_t workspace_floats, void* stream);

/* ---- the statistics of z per channel: mean [C], var [C] (biased: M2 / n) and invstd [C] = 1 / sqrt(var + eps), each rounded
 * once from fp64.  The second moment is centred: a work-group takes the mean of its slice of pairs, then the squared
 * distances to it, and the slices are combined in a fixed order (Chan et al.): the same bits on every run.  n < 2: -1.
 * workspace: os2d_train_bn_workspace_bytes(layer, NB) bytes (0 = bad argument), 16-byte aligned; shared with the backward.  */
size_t os2d_train_bn_workspace_bytes(int layer, int NB);
int os2d_train_bn_stats(int layer, const float* z, int NB, int H, int W, float eps, float* mean, float* var, float* invstd,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- h [NB,C,PLANE] = relu(((z - mean) * invstd) * gamma + beta) at data cells, +0.0 elsewhere.                            */
int os2d_train_bn_relu_forward(int layer, const float* z, const float* gamma, const float* beta, const float* mean, const float* invstd,
                               int NB, int H, int W, float* h, void* stream);

/* ---- the backward through the statistics: g = dh where h > 0 (the forward's own bits), xhat = (z - mean) * invstd;
 *   dbeta [C] = sum g, dgamma [C] = sum g xhat (fp64 sums in a fixed order; each may be NULL: not written);
 *   dy [NB,C,PLANE] = gamma invstd (g - dbeta / n - xhat dgamma / n) at data cells, 0 at pad cells (always written).
 * The gradient of the convolution's bias is exactly zero on such a layer (a constant shift cancels in z - mean): not computed. */
int os2d_train_bn_relu_backward_batch(int layer, const float* dh, const float* z, const float* h, const float* gamma, const float* mean,
                                      const float* invstd, int NB, int H, int W, float* dy, float* dgamma, float* dbeta, void* workspace,
                                      size_t workspace_bytes, void* stream);

/* ---- class map backward, the inverse of os2d_class_prepare_batch (head.py:241-268): q15 [B,C,225] the resized, NOT normalised
 * maps (cell order i*15 + j; os2d_class_prepare_batch with normalize = 0), dq [B,C,225] from os2d_train_corr_backward.  L2 over
 * C (eps 1e-5) backward, then bilinear-resize backward (align_corners = True, zero padding) into dsrcs[b] [C,h_b,w_b]
 * (written), sizes = [B][2] (h, w) on the device.  workspace: B*C*225 floats.                                            */
int os2d_train_class_backward(const float* q15, const float* dq, int B, int C, float* const* dsrcs, const int* sizes,
                              float* workspace, size_t workspace_floats, void* stream);

/* ---- the bridge from a split-fp16 ("f16x3") training forward to the entry points above (csrc_train/shb_planes.hip).  shb is an
 * activation buffer of the f16x3 stage entry points of os2d_hip.h (os2d_corr_f16x3, os2d_transform_conv_f16x3) in the split-half
 * blocked layout: [NB][ceil(channels/8)][hi|lo][PLANE] units of 16 bytes = 8 channels of one plane cell as fp16, channel c
 * stored as x * 2^exp[c]; exp [channels] int32 on the DEVICE (the relu + L2 normalised correlation: 225 times os2d_rnorm_exp();
 * h1 / h2: the layer's out_exp given to os2d_pack_conv_f16x3).  Writes planes [NB,out_channels,PLANE] fp32:
 *   planes[nb][c][n] = (float(hi) + float(lo)) * 2^-exp[c]  at interior cells of the zero-bordered plane layout - exact: the
 *                      halves of a split fp32 value add up to at most 24 bits, the power of two only moves the exponent;
 *   +0.0               at every other cell, whatever shb holds there (pad cells, the unused channels of the last group);
 *   +0.0               in the whole of planes channels .. out_channels-1 (rnorm: channels = 225, out_channels = 226).
 * shb and planes 16-byte aligned.  One grid row per (pair, 8-channel group): NB * ceil(out_channels/8) <= 65535, else -1; also
 * -1: a null pointer, NB / channels / H / W < 1, out_channels < channels, H or W beyond the head's own limits.  One launch.  */
int os2d_train_planes_from_shb(const void* shb, const int* exp, int NB, int channels, int out_channels, int H, int W,
                               float* planes, void* stream);

/* ==== Target assignment and the training objective (csrc_train/objective.hip; reference os2d/modeling/box_coder.py:234-389 and
 * os2d/engine/objective.py:107-313).  A images, B labels, HW = H*W anchors per level, N = A*B*HW elements.  Class targets are
 * int64 (1 positive, 0 negative, -1 ignored), as the reference returns them.  No call synchronises with the host; float sums
 * are reduced in a fixed order (block partials, then one combining block), so two runs on the same input give the same bits. */

/* ---- anchors to ground truth, one thread per (image, label, anchor).  Ground truth arrives packed: gt_boxes [n,4] xyxy,
 * gt_labels [n] int32, gt_difficult [n] bytes, image_offsets [A+1] int32 (the boxes of image a are offsets[a] .. offsets[a+1]-1;
 * num_boxes = n may be 0, then the three gt pointers may be NULL).  Anchors are the closed form of os2d_sample_decode: cell (y,x)
 * centred at ((x+0.5)*stride, (y+0.5)*stride), size rec_field + 14*stride, row-major.  IoU as boxlist_iou in fp32; the best box is
 * the first maximum; torchvision's Matcher(iou_high, iou_low) without low-quality matches (below low: -1, [low, high): -2, a
 * matched difficult box: -2); class target = 1 + clamp(index, -2, 0).
 *   mode 0 (encode):  cls_targets [A,B,HW] int64 and loc_targets [A,B,4,HW] = encode_boxes, weights (10,10,5,5), of the matched box
 *                     against the anchor after clip_to_min_size(1); an unmatched anchor gets the value for the label's FIRST box;
 *                     a label without a box in the image gets zeros.  loc_scores and the two IoU outputs are not used.
 *   mode 1 (remap):   the anchor is replaced by the box decoded from loc_scores [A,B,4,HW] (BoxCoder.decode_single, dw / dh
 *                     clamped at log(1000/16)); writes cls_targets (the remapped targets), ious_anchor (best IoU of the plain
 *                     anchor) and ious_anchor_corrected (best IoU of the decoded box), each [A,B,HW].  loc_targets is not used. */
int os2d_train_assign_targets(int mode, const float* gt_boxes, const int* gt_labels, const unsigned char* gt_difficult,
                              const int* image_offsets, int num_boxes, const float* loc_scores, int A, int B, int H, int W, int stride,
                              int rec_field, float iou_high, float iou_low, float* loc_targets, long long* cls_targets,
                              float* ious_anchor, float* ious_anchor_corrected, void* stream);

/* ---- objective forward.  class_loss 0 = ContrastiveLoss (squared half-margins, then hard-negative mining: the
 * k = neg_to_pos_ratio * num_pos largest losses among the candidates - elements neither positive nor ignored - found by a radix
 * select over the fp32 bit patterns, elements equal to the k-th taken in increasing flat index), 1 = RLL (linear half-margins,
 * positives rescaled by num_pos / num_nontrivial_pos, negatives weighted by exp((l - max_l) * T), T = -log(rll_neg_weight_ratio) /
 * max_l per label, normalised per label and by the number of labels with max_l > 1e-5; no mining: every candidate is used when
 * neg_to_pos_ratio * num_pos > 0, none otherwise).  patch_mining_mode != 0 skips the RLL normalisation and the mining.
 * loc_preds / loc_targets [A,B,4,HW], cls_preds [A,B,HW], cls_targets [A,B,HW] int64; cls_targets_remapped (NULL = none) replaces
 * cls_targets for the class loss, not for the localisation loss; cls_preds_for_neg (NULL = none) replaces cls_preds at negatives.
 * Outputs: losses [5] = loss, loc_smoothL1, cls, cls_pos, cls_neg; cls_loss [N] the per-element class loss; loc_loss [N] the
 * per-element localisation loss (NULL = not written); flags [N] bytes (1 positive, 2 negative used, 4 regression positive,
 * 8 candidate, 16 the element's hinge is active for the gradient: margin_pos - score >= 0 at a positive, score - margin >= 0 at
 * a candidate - torch's clamp(min=0) passes the gradient at 0 too, so a score exactly at its margin has the RLL coefficient of the
 * active side) and coef [N] (d class loss / d score before the count normalisation) for the backward.  The counts
 * (a zero count divides as 1) stay in `workspace`, os2d_train_objective_workspace_floats floats, which the backward reads.   */
size_t os2d_train_objective_workspace_floats(int A, int B, int HW);
int os2d_train_objective_forward(int class_loss, int patch_mining_mode, const float* loc_preds, const float* loc_targets,
                                 const float* cls_preds, const long long* cls_targets, const long long* cls_targets_remapped,
                                 const float* cls_preds_for_neg, int A, int B, int HW, float margin, float margin_pos,
                                 float class_loss_neg_weight, float localization_weight, float neg_to_pos_ratio,
                                 double rll_neg_weight_ratio, float* losses, float* cls_loss, float* loc_loss, unsigned char* flags,
                                 float* coef, float* workspace, size_t workspace_floats, void* stream);

/* ---- objective backward, one kernel: grad_loss is the upstream gradient of losses[0] as a one-element device tensor; flags,
 * coef and workspace as the forward left them.  Writes (each may be NULL = not computed) dloc_preds [A,B,4,HW] = clamp(diff,-1,1)
 * * localization_weight / num_pos_for_regression at regression positives, dcls_preds [A,B,HW] and dcls_preds_for_neg [A,B,HW]:
 * the class term goes to dcls_preds at positives and to dcls_preds_for_neg at the used negatives; without dcls_preds_for_neg
 * both go to dcls_preds.  Zero elsewhere and where a clamp is inactive; the RLL weights and the counts are constants.       */
int os2d_train_objective_backward(const float* grad_loss, const float* loc_preds, const float* loc_targets, const unsigned char* flags,
                                  const float* coef, const float* workspace, int A, int B, int HW, float class_loss_neg_weight,
                                  float localization_weight, float* dloc_preds, float* dcls_preds, float* dcls_preds_for_neg,
                                  void* stream);

/* ---- os2d_train_assign_targets with a box transform chain (hard-patch mining: the level's anchors are compared with ground
 * truth given in the original image).  The chain is op_kinds [nops], op_args [nops][2] on the HOST, OS2D_BOX_OP_* of os2d_hip.h
 * (1 scale, 2 horizontal flip, 3 vertical flip, 4 shift), at most OS2D_BOX_MAX_OPS (6) entries, applied op by op with one
 * rounding per product / difference.
 *   mode 0 (reference box_coder.py:352-354): the anchor goes through the chain before the IoU, clip_to_min_size(1) and encode_boxes;
 *   mode 1 (reference box_coder.py:250-254): the box is decoded from loc_scores against the plain anchor, then the decoded box
 *           and the anchor both go through the chain.
 * Everything else as os2d_train_assign_targets, whose kernel this shares.                                                  */
int os2d_train_assign_targets_ops(int mode, const float* gt_boxes, const int* gt_labels, const unsigned char* gt_difficult,
                                  const int* image_offsets, int num_boxes, const float* loc_scores, int A, int B, int H, int W, int stride,
                                  int rec_field, float iou_high, float iou_low, int nops, const int* op_kinds, const float* op_args,
                                  float* loc_targets, long long* cls_targets, float* ious_anchor, float* ious_anchor_corrected,
                                  void* stream);

/* ==== Hard-patch mining (csrc_train/mining.hip; reference os2d/modeling/box_coder.py:78-166 and os2d/engine/train.py:240-325). */
#define OS2D_MINE_MAX_LEVELS 8
#define OS2D_MINE_MAX_K 64
#define OS2D_MINE_INDEX_INTS 3     /* level, label, anchor */
#define OS2D_MINE_VALUE_FLOATS 19  /* crop xyxy, anchor xyxy, 8 corner values, cls_loss, loc_loss, cls_pred */

/* ---- get_box_to_cut_anchor for one level of H x W anchors (row-major, stride `stride`, size `box_size`) on an image of
 * img_w x img_h: per anchor the stride-aligned crop window of crop_w x crop_h around it (floored to the stride where its corner
 * is positive, else 0; shifted left / up by a whole number of strides when it leaves the image and that fits, else the full width
 * / height from 0) and the anchor box, both through the chain (as above; nops = 0: none).  crop_boxes, anchor_boxes [H*W,4] xyxy. */
int os2d_train_crop_boxes(int H, int W, int stride, int box_size, int img_w, int img_h, int crop_w, int crop_h, int nops,
                          const int* op_kinds, const float* op_args, float* crop_boxes, float* anchor_boxes, void* stream);

/* ---- the K hardest patches per (image, role) over a pyramid of L <= OS2D_MINE_MAX_LEVELS levels.  HOST arrays: level_hw [L][2]
 * (H, W), level_img [L][2] (w, h), level_row_stride [L], op_counts [L], op_kinds [L][OS2D_BOX_MAX_OPS], op_args
 * [L][OS2D_BOX_MAX_OPS][2], and five arrays of L DEVICE pointers: cls_loss, loc_loss, flags (rows of HW_l elements, one per
 * (image, label), level_row_stride[l] >= HW_l elements apart: the level's slice of what os2d_train_objective_forward wrote for
 * the merged pyramid, or a dense [A,B,HW_l]), cls_preds [A,B,HW_l] and corners [A,B,8,HW_l] (dense; `corners` may be NULL).
 * Roles: 0 neg (flag 2, score cls_loss), 1 pos (flag 1, cls_loss), 2 pos_loc (flag 4, loc_loss).  For every (image, role): greedy
 * NMS at iou_thr over the crop windows (os2d_train_crop_boxes) of the flagged candidates by decreasing score, equal scores in
 * increasing (level, label, anchor) order, stopped after K <= OS2D_MINE_MAX_K kept; a candidate whose score is not finite is
 * never selected.  This is greedy NMS over ALL candidates at once, at any number of them.
 * Outputs: out_count [A,3]; out_index [A,3,K,3] (level, label, anchor; -1 in unused records); out_values [A,3,K,19]: crop xyxy,
 * anchor xyxy, the 8 corner values taken as two boxes through the level's chain (zeros without `corners`), cls_loss, loc_loss
 * and cls_preds of the element (zeros in unused records).  workspace: os2d_train_mine_select_workspace_bytes bytes (0 = bad
 * shape), 16-byte aligned.  One launch, A * 3 work-groups; no atomics: two runs give the same bits.                         */
size_t os2d_train_mine_select_workspace_bytes(int A, int B, int L, const int* level_hw);
int os2d_train_mine_select(int A, int B, int L, const int* level_hw, const int* level_img, const int* level_row_stride, int stride,
                           int box_size, const int* op_counts, const int* op_kinds, const float* op_args, const float* const* cls_loss,
                           const float* const* loc_loss, const unsigned char* const* flags, const float* const* cls_preds,
                           const float* const* corners, int crop_w, int crop_h, float iou_thr, int K, int* out_count, int* out_index,
                           float* out_values, void* workspace, size_t workspace_bytes, void* stream);

/* ==== Gradient clip, NaN guard and the SGD / Adam step (csrc_train/optim.hip; torch.nn.utils.clip_grad_norm_ followed by the
 * reference's `if not math.isnan(grad_norm): optimizer.step()`, os2d/engine/train.py:104-108).  fp32
 * parameters, gradients and state, dense.  One launch serves a TABLE of at most OS2D_TRAIN_OPTIM_MAX_TENSORS tensors, passed in the
 * kernel arguments; a work-group owns one chunk of OS2D_TRAIN_OPTIM_CHUNK elements of one tensor.  Chunks are numbered over all
 * the tables of a step: a tensor of numel elements takes os2d_train_optim_chunks chunks from its first_chunk on, and the records
 * of a table follow each other without a gap (checked).  A step is
 *     sumsq (per table)  ->  finalize  ->  [prepare (per table, Adam)]  ->  update (per table)
 * on one stream; nothing synchronises with the host, no floating-point atomics, every sum in a fixed order: two runs on the same
 * input give the same bits.  Every entry point checks its arguments before it launches anything: -1 for a null pointer, a
 * tensor count outside 0 .. OS2D_TRAIN_OPTIM_MAX_TENSORS, a negative numel, records that do not follow each other, an `aligned`
 * mark on pointers that are not 16-byte aligned, max_norm <= 0; -2 for a partials buffer that is too small.                  */
#define OS2D_TRAIN_OPTIM_MAX_TENSORS 60
#define OS2D_TRAIN_OPTIM_CHUNK 4096
#define OS2D_TRAIN_OPTIM_SGD 0
#define OS2D_TRAIN_OPTIM_ADAM 1
typedef struct {
  float* param;        /* [numel] */
  float* grad;         /* [numel]; the update writes grad * coef back */
  float* state1;       /* SGD: momentum_buffer (not read when momentum == 0); Adam: exp_avg; the other methods: the table below */
  float* state2;       /* Adam: exp_avg_sq */
  float* step;         /* every method but SGD: the tensor's step count, one float on the device */
  long long numel;     /* 0 is allowed: no chunk, no access */
  float lr;
  float weight_decay;
  int first_chunk;     /* index of the tensor's first chunk among all chunks of the step */
  int aligned;         /* 1: param, grad and the state pointers are all 16-byte aligned (16-byte accesses); 0: 4-byte accesses */
} os2d_train_optim_tensor;

int os2d_train_optim_max_tensors(void);               /* OS2D_TRAIN_OPTIM_MAX_TENSORS */
size_t os2d_train_optim_chunks(long long numel);      /* ceil(numel / OS2D_TRAIN_OPTIM_CHUNK); 0 for numel <= 0 */

/* ---- partials[first_chunk + j] = the sum of the squares of chunk j of each tensor's grad, in double (an fp32 square is exact in
 * double; per thread, then over the work-group, in a fixed order).  partials holds partials_count doubles: the chunks of ALL tables. */
int os2d_train_optim_sumsq(const os2d_train_optim_tensor* tensors, int n, double* partials, size_t partials_count, void* stream);

/* ---- one work-group adds partials[0 .. partials_count) in index order in double and writes record [4] floats:
 *   record[0] norm = (float)sqrt(sum);
 *   record[1] coef = min(max_norm / (norm + 1e-6f), 1.0f) in fp32 (NaN for a NaN norm); max_norm = +infinity: 1.0f, no clipping;
 *   record[2] skip = 1.0f when norm is NaN, else 0.0f (an infinite norm does not skip);   record[3] = 0.                          */
int os2d_train_optim_finalize(const double* partials, size_t partials_count, float max_norm, float* record, void* stream);

/* ---- Adam, between finalize and update, one thread per tensor of the table: unless record says skip, *step += 1 and
 * factors[2 i] = (float)(lr / bc1), factors[2 i + 1] = (float)sqrt(bc2), bc = 1 - beta^step in double.  factors: 2 n floats.    */
int os2d_train_optim_prepare(const os2d_train_optim_tensor* tensors, int n, const float* record, double beta1, double beta2,
                             float* factors, void* stream);

/* ---- per element g = grad * record[1], written back to grad; then, unless record says skip, in fp32, one rounding per operation,
 * correctly rounded division and square root, d = g + weight_decay * p (d = g when weight_decay == 0):
 *   OS2D_TRAIN_OPTIM_SGD  (dampening 0, no Nesterov; momentum_or_beta1 = momentum, beta2 / eps / factors not used):
 *       buf = momentum * buf + d;  p = p - lr * buf            (momentum == 0: p = p - lr * d, state1 is not touched)
 *   OS2D_TRAIN_OPTIM_ADAM (L2 weight decay, no amsgrad; factors of this table as prepare wrote them):
 *       m = m + (d - m) * (1 - beta1);  v = beta2 * v + ((1 - beta2) * d) * d;
 *       den = sqrt(v) / factors[2 i + 1] + eps;  p = p - factors[2 i] * (m / den)
 * with (float)momentum, (float)beta2, (float)(1 - beta1), (float)(1 - beta2), (float)eps.  On a skipped step parameters and state
 * keep their bits.                                                                                                             */
int os2d_train_optim_update(int method, const os2d_train_optim_tensor* tensors, int n, const float* record, const float* factors,
                            double momentum_or_beta1, double beta2, double eps, void* stream);

/* ---- The reference's other six methods (torch.optim.Adagrad, Adadelta, Adamax, ASGD, RMSprop, Rprop as its create_optimizer
 * builds them: single-tensor arithmetic, no maximize; RMSprop without momentum and not centered).  A step is
 *     sumsq (per table)  ->  finalize  ->  prepare_ex (per table)  ->  update_ex (per table)
 * with the same tables, record, chunk numbering and checks as above.  `hyper` is a HOST array of nhyper doubles, read before the
 * call returns (it travels in the kernel arguments); a method outside 2 .. 7, an nhyper other than the method's, a null hyper, a
 * value outside its range or a null state pointer the method needs: -1 before anything is launched.
 *   method     hyper                                          state1        state2                    factors written by prepare_ex
 *   ADAGRAD    lr_decay, eps                                  sum           -                         clr
 *   ADADELTA   rho, eps                                       square_avg    acc_delta                 -
 *   ADAMAX     beta1, beta2, eps                              exp_avg       exp_inf                   lr / (1 - beta1^step)
 *   ASGD       lambd, alpha, t0                               ax            {eta, mu}: TWO floats     1 - lambd eta, eta, mu
 *   RMSPROP    alpha, eps                                     square_avg    -                         -
 *   RPROP      etaminus, etaplus, step_size_min, _max         prev          step_size                 -
 * The change is additive: OS2D_TRAIN_ABI_VERSION stays 2.                                                                      */
#define OS2D_TRAIN_OPTIM_ADAGRAD 2
#define OS2D_TRAIN_OPTIM_ADADELTA 3
#define OS2D_TRAIN_OPTIM_ADAMAX 4
#define OS2D_TRAIN_OPTIM_ASGD 5
#define OS2D_TRAIN_OPTIM_RMSPROP 6
#define OS2D_TRAIN_OPTIM_RPROP 7
#define OS2D_TRAIN_OPTIM_MAX_HYPER 8      /* no method takes more hyperparameters */
#define OS2D_TRAIN_OPTIM_FACTORS 4        /* floats per tensor that prepare_ex writes */

/* ---- between finalize and update_ex, one thread per tensor of the table: unless record says skip, *step += 1 and
 * factors[4 i ..] = the method's factors above, computed in double from (double)lr and the new step and rounded once (unused
 * entries are 0).  ASGD: the factors are the eta and mu that state2 holds - those the previous step left, lr and 1 before the
 * first - and state2 then receives eta = lr / (1 + lambd lr step)^alpha, mu = 1 / max(1, step - t0) for the next step.  Every
 * record needs `step` (ASGD: and state2), also one without elements.  factors: 4 n floats.                                     */
int os2d_train_optim_prepare_ex(int method, const os2d_train_optim_tensor* tensors, int n, const float* record, const double* hyper,
                                int nhyper, float* factors, void* stream);

/* ---- per element g = grad * record[1], written back to grad; then, unless record says skip, in fp32, one rounding per operation,
 * correctly rounded division and square root, d = g + weight_decay * p (d = g when weight_decay == 0; Rprop: always d = g), with
 * f0 .. f2 the tensor's factors and every hyperparameter (and 1 - rho, 1 - beta1, 1 - alpha) rounded once from double:
 *   ADAGRAD    sum = sum + d * d;  p = p - f0 * (d / (sqrt(sum) + eps))
 *   ADADELTA   sq = rho * sq + ((1 - rho) * d) * d;  delta = sqrt(acc + eps) / sqrt(sq + eps) * d;
 *              acc = rho * acc + ((1 - rho) * delta) * delta;  p = p - lr * delta
 *   ADAMAX     m = m + (d - m) * (1 - beta1);  u = max(beta2 * u, |d| + eps), NaN if either is;  p = p - f0 * (m / u)
 *   ASGD       p = p * f0;  p = p - f1 * d;  ax = ax + (p - ax) * f2 when f2 != 1, else ax = p        (state2 is not touched)
 *   RMSPROP    sq = alpha * sq + ((1 - alpha) * d) * d;  p = p - lr * (d / (sqrt(sq) + eps))
 *   RPROP      s = d * prev;  step_size = clamp(step_size * (etaplus if s > 0, etaminus if s < 0, 1 if s == 0, NaN else), min, max),
 *              a NaN stays;  d = 0 where s < 0;  p = p - sign(d) * step_size (sign(0) = 0, sign(NaN) = NaN);  prev = d
 * On a skipped step parameters and state keep their bits.                                                                       */
int os2d_train_optim_update_ex(int method, const os2d_train_optim_tensor* tensors, int n, const float* record, const float* factors,
                               const double* hyper, int nhyper, void* stream);

/* ---- the range plan of the split-fp16 ("f16x3") packing on the device - what a parameter change makes stale every step: the
 * exponents os2d_pack_conv_f16x3 (include/os2d_hip.h) takes, from the raw fp32 parameters (w1 [128,225,7,7], w2 [64,128,5,5],
 * w3 [P,64,5,5] and the biases of layers 1 and 2; bn<l>_* = NULL for a layer without BatchNorm, all four or none; bn<l>_eps is
 * BatchNorm2d.eps as a DOUBLE).  Eval-mode BatchNorm fold, bounds and exponents in float64 throughout: three dependent launches on
 * `stream`, no host wait, no atomics - two calls on the same parameters give the same bits.
 *   exps   [os2d_train_range_plan_ints() = 520] int32:
 *          wexp1 [128] | e1 [128] | unit_exp [128] | wexp2 [64] | e2 [64] | wexp3 [8] (entries of wexp3 past P are zero)
 *            B1[o] = 7 * ||w1'[o]||_2 + |b1'[o]|                       (w', b': BatchNorm folded; the input has norm <= 1)
 *            B2[o] = min(sum_c B1[c] * ||w2'[o,c]||_1, 5 * ||B1||_2 * ||w2'[o]||_2) + |b2'[o]|
 *            e<l>[o]   = floor(log2(32768 / B<l>[o]))                  the layer's out_exp, the next layer's in_exp
 *            unit_exp  = e1 - 15                                       (bound * 2^unit_exp <= 1)
 *            wexp<l>[o] = floor(log2(16384 / max_c |w<l>'[o,c]| * 2^-in_exp[c]))     (layer 1: in_exp = 12, os2d_rnorm_exp())
 *          each floor(log2) exact (the exponent field), clamped to [-60, 60]; 0 for a zero, NaN or infinite bound / maximum;
 *   bounds [os2d_train_range_plan_doubles() = 192] float64, 8-byte aligned: B1 [128] | B2 [64].
 * The change is additive: OS2D_TRAIN_ABI_VERSION stays 2.                                                                      */
size_t os2d_train_range_plan_ints(void);
size_t os2d_train_range_plan_doubles(void);
int os2d_train_range_plan(int P, const float* w1, const float* b1, const float* bn1_weight, const float* bn1_bias,
                          const float* bn1_running_mean, const float* bn1_running_var, double bn1_eps, const float* w2,
                          const float* b2, const float* bn2_weight, const float* bn2_bias, const float* bn2_running_mean,
                          const float* bn2_running_var, double bn2_eps, const float* w3, int* exps, double* bounds, void* stream);

#ifdef __cplusplus
}
#endif
#endif
