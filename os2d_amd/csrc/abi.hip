// C ABI of libos2d_hip.so (include/os2d_hip.h), the per-stage entry points: an argument check, then the launches of the kernel
// units.  The head call (os2d_head_forward*, os2d_head_workspace_bytes*) is head_call.hip's; the sizes both report and carve
// are in abi_sizes.h.
#include "../../include/os2d_hip.h"
#include "abi_sizes.h"
#include "detect_common.h"

namespace {
// the layer as the packing entry points take it; false for a layer other than 1 .. 3
bool conv_shape(int layer, int P, Os2dLayer* s) {
  if (layer < 1 || layer > 3) return false;
  *s = os2d_layer(layer, P);
  return true;
}
bool bad_P(int P) { return P != 6 && P != 4; }

// shared prologue of os2d_corr_f16x3 / os2d_corr_f16x3_packed: their workspace starts with sumsq | split image features
// (corr_workspace); both are filled
int corr_f16x3_prologue(const float* fm, void* workspace, const CorrWorkspace& w, int A, int C, int H, int W, hipStream_t st, void** fs) {
  float* sumsq = reinterpret_cast<float*>(static_cast<char*>(workspace) + w.sumsq);
  *fs = static_cast<char*>(workspace) + w.fs;
  const int rc = os2d_launch_fm_sumsq(fm, sumsq, A, C, H * W, st);
  return rc ? rc : os2d_launch_split_fm(fm, sumsq, *fs, A, C, H * W, nullptr, 0, Os2dRangeFlag{nullptr, 0}, st);
}
// BatchNorm folding takes all four of weight / bias / running_mean / running_var, or none
bool bn_all_or_none(const float* weight, const float* bias, const float* mean, const float* var) {
  return (weight && bias && mean && var) || !(weight || bias || mean || var);
}
bool bad_bins(int nbins) { return nbins < 8 || (nbins & 7); }
// argument and alignment checks of the per-bin GEMM entry points (`hint`: what the entry point's text adds to the shape)
bool spectral_gemm_args_ok(const char* who, const char* hint, const void* w, const float* X, const float* Y, int NB, int C, int Cout, int nbins,
                           float xscale) {
  if (!w || !X || !Y || NB < 1 || C < 1 || Cout < 1 || Cout > 128 || bad_bins(nbins) || !(xscale > 0.f))
    return OS2D_REFUSE(false, "%s: bad arguments (NB=%d C=%d Cout=%d nbins=%d%s)", who, NB, C, Cout, nbins, hint);
  if (!aligned_to(16, w, X, Y)) return OS2D_REFUSE(false, "%s: buffers must be 16-byte aligned", who);
  return true;
}
// the same for the two weight-spectra builders; P != NULL: the matrix-product family, whose transform length is a multiple of 4
bool spectra_build_args_ok(const char* who, const double* wfold, const double* twP64, const double* twQ64, const void* out,
                           const void* workspace, bool need_workspace, int C, int Cout, int nbins, const int* P) {
  if (!wfold || !twP64 || !twQ64 || !out || (need_workspace && !workspace) || C < 1 || Cout < 1 || Cout > 128 || bad_bins(nbins) || (P && (*P & 3)))
    return P ? OS2D_REFUSE(false, "%s: bad arguments (C=%d Cout=%d P=%d nbins=%d)", who, C, Cout, *P, nbins)
             : OS2D_REFUSE(false, "%s: bad arguments (C=%d Cout=%d nbins=%d)", who, C, Cout, nbins);
  if (!aligned_to(16, out) || !aligned_to(8, workspace)) return OS2D_REFUSE(false, "%s: out must be 16-byte, workspace 8-byte aligned", who);
  return true;
}
// the layers whose inverse transform exists: the 7x7 layer and the 5x5 layer 128 -> 64
bool dft_inverse_args_ok(const float* Y, const float* packed_b, const void* out, const void* matrices, int NB, int Cout, int H, int W) {
  return Y && packed_b && out && matrices && NB >= 1 && (Cout == os2d_layer(1).cout || Cout == os2d_layer(2).cout) && H >= 1 && W >= 1;
}
}  // namespace

extern "C" {

int os2d_abi_version(void) { return OS2D_ABI_VERSION; }
const char* os2d_last_error(void) { return os2d_error_text; }

size_t os2d_packed_conv_floats(int layer) {
  Os2dLayer s;
  if (!conv_shape(layer, 6, &s)) return 0;
  return (size_t)(s.planes() / 2) * s.ks * s.ks * 2 * s.rows;
}
size_t os2d_packed_bias_floats(int layer) {
  Os2dLayer s;
  if (!conv_shape(layer, 6, &s)) return 0;
  return (size_t)3 * s.rows;  // folded bias | per-row 2^-weight_exp | per-row 2^out_exp (f16x3 packing; fp32: first third)
}

int os2d_pack_conv(int layer, int P, const float* w, const float* b, const float* bn_weight, const float* bn_bias,
                   const float* bn_running_mean, const float* bn_running_var, float bn_eps, float* packed_w,
                   float* packed_b, void* stream) {
  Os2dLayer s;
  if (!conv_shape(layer, P, &s) || (layer == 3 && bad_P(P))) return OS2D_REFUSE(-1, "os2d_pack_conv: bad layer %d / P %d", layer, P);
  if (!w || !b || !packed_w || !packed_b) return OS2D_REFUSE(-1, "os2d_pack_conv: null pointer");
  if (!bn_all_or_none(bn_weight, bn_bias, bn_running_mean, bn_running_var))
    return OS2D_REFUSE(-1, "os2d_pack_conv: BatchNorm needs all four of weight/bias/running_mean/running_var");
  return os2d_launch_pack_conv(w, b, bn_weight, bn_bias, bn_running_mean, bn_running_var, bn_eps, s.cout, s.cin, s.ks,
                               s.rows, packed_w, packed_b, os2d_stream(stream));
}

int os2d_class_prepare(const float* src, int C, int h, int w, int normalize, float* q15, float* qp, void* stream) {
  if (!src || !q15 || !qp || C < 1 || h < 1 || w < 1) return OS2D_REFUSE(-1, "os2d_class_prepare: bad arguments (C=%d h=%d w=%d)", C, h, w);
  return os2d_launch_class_prepare(src, C, h, w, normalize, q15, qp, os2d_stream(stream));
}

size_t os2d_class_prepare_workspace_floats(int B, int C) {
  if (B < 1 || C < 1) return 0;
  return (size_t)os2d_class_prepare_partial_floats(B, C);
}

int os2d_class_prepare_batch(const float* const* srcs, const int* sizes, int B, int C, int normalize, float* q15,
                             float* qp, float* workspace, void* stream) {
  if (!srcs || !sizes || !q15 || !qp || !workspace || B < 1 || C < 1 || B > 65535)
    return OS2D_REFUSE(-1, "os2d_class_prepare_batch: bad arguments (B=%d C=%d; at most 65535 classes per call)", B, C);
  return os2d_launch_class_prepare_batch(srcs, sizes, B, C, normalize, q15, qp, workspace, os2d_stream(stream));
}

size_t os2d_plane_floats(int H, int W) { return (size_t)os2d_plane(H, W); }

size_t os2d_shb_bytes(int channels, int H, int W) {
  if (channels < 1 || H < 1 || W < 1) return 0;
  return shb_bytes(channels, H, W);
}

int os2d_fm_sumsq(const float* fm, float* sumsq, int A, int C, int H, int W, void* stream) {
  if (!fm || !sumsq || A < 1 || C < 1 || H < 1 || W < 1) return OS2D_REFUSE(-1, "os2d_fm_sumsq: bad arguments");
  return os2d_launch_fm_sumsq(fm, sumsq, A, C, H * W, os2d_stream(stream));
}

int os2d_corr(const float* fm, const float* qp, const float* sumsq, float* corr, float* rnorm, int A, int B, int C,
              int H, int W, void* stream) {
  if (!fm || !qp || !sumsq || !corr || !rnorm) return OS2D_REFUSE(-1, "os2d_corr: null pointer");
  if (!head_args_ok(A, B, C, H, W, 6)) return -1;
  int rc = os2d_launch_border_zero(rnorm, A * B * OS2D_KP, H, W, os2d_stream(stream));
  if (rc) return rc;
  return os2d_launch_corr(fm, qp, sumsq, corr, rnorm, nullptr, A, B, C, H, W, 0, os2d_stream(stream));
}

size_t os2d_corr_f16x3_workspace_bytes(int A, int C, int H, int W) {
  if (A < 1 || C < 1 || H < 1 || W < 1) return 0;
  return corr_workspace(A, 0, C, H, W).total;
}

int os2d_corr_f16x3(const float* fm, const void* qs, float* corr, void* rshb, int A, int B, int C, int H, int W,
                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!fm || !qs || !corr || !rshb || !workspace) return OS2D_REFUSE(-1, "os2d_corr_f16x3: null pointer");
  if (!head_args_ok(A, B, C, H, W, 6)) return -1;
  const CorrWorkspace w = corr_workspace(A, 0, C, H, W);
  if (workspace_bytes < w.total || !aligned_to(256, workspace)) return OS2D_REFUSE(-2, "os2d_corr_f16x3: workspace too small or not 256-byte aligned");
  void* fs;
  int rc = corr_f16x3_prologue(fm, workspace, w, A, C, H, W, os2d_stream(stream), &fs);
  if (!rc) rc = os2d_launch_border_zero_shb(rshb, A * B, H, W, os2d_stream(stream));
  if (!rc) rc = os2d_launch_corr_f16x3(fs, qs, corr, rshb, nullptr, nullptr, 0, A, B, C, H, W, os2d_stream(stream));
  return rc;
}

size_t os2d_corr_f16x3_packed_workspace_bytes(int A, int B, int C, int H, int W) {
  if (A < 1 || B < 1 || C < 1 || H < 1 || W < 1) return 0;
  return corr_workspace(A, B, C, H, W).total;
}

int os2d_corr_f16x3_packed(const float* fm, const void* qs, float* corr, float* inv_norm, int A, int B, int C, int H, int W,
                           int form, void* workspace, size_t workspace_bytes, void* stream) {
  if (!fm || !qs || !corr || !inv_norm || !workspace) return OS2D_REFUSE(-1, "os2d_corr_f16x3_packed: null pointer");
  if (!head_args_ok(A, B, C, H, W, 6)) return -1;
  if (form < -1 || form > 7 || (form >= 0 && (form & 3) > 1))
    return OS2D_REFUSE(-1, "os2d_corr_f16x3_packed: form %d (0 padded | 1 packed | -1 the head's choice; + 4: no half tiles at the tail)", form);
  const CorrWorkspace w = corr_workspace(A, B, C, H, W);
  if (workspace_bytes < w.total || !aligned_to(256, workspace))
    return OS2D_REFUSE(-2, "os2d_corr_f16x3_packed: workspace too small or not 256-byte aligned");
  void *fs, *sumfx = static_cast<char*>(workspace) + w.sumfx;
  int rc = corr_f16x3_prologue(fm, workspace, w, A, C, H, W, os2d_stream(stream), &fs);
  const bool packed = form < 0 ? os2d_corr_f16x3_use_packed(A, B, H, W) != 0 : (form & 1) != 0;
  if (!rc && packed) rc = os2d_launch_corr_sums_clear(sumfx, A, B, H, W, os2d_stream(stream));
  if (!rc) rc = os2d_launch_corr_f16x3(fs, qs, corr, nullptr, inv_norm, packed ? sumfx : nullptr, (form >= 0 && (form & 4)) ? 2 : 0, A, B, C, H, W, os2d_stream(stream));
  return rc;
}

int os2d_corr_normalize(const float* corr, float* rnorm, int NB, int H, int W, void* stream) {
  if (!corr || !rnorm || NB < 1 || H < 1 || W < 1) return OS2D_REFUSE(-1, "os2d_corr_normalize: bad arguments");
  return os2d_launch_corr_normalize(corr, rnorm, NB, H, W, os2d_stream(stream));
}

int os2d_transform_conv(int layer, const float* in, const float* packed_w, const float* packed_b, float* out, int NB,
                        int P, int H, int W, void* stream) {
  if (!in || !packed_w || !packed_b || !out || NB < 1 || H < 1 || W < 1 || (layer == 3 && bad_P(P)))
    return OS2D_REFUSE(-1, "os2d_transform_conv: bad arguments (layer=%d NB=%d P=%d)", layer, NB, P);
  return os2d_launch_conv(layer, in, packed_w, packed_b, out, NB, P, H, W, os2d_stream(stream));
}

int os2d_sample_decode(const float* corr, const float* params, int NB, int H, int W, int P, int inverse, int stride,
                       int rec_field, float* loc, float* cls, float* corners, void* stream) {
  if (!corr || !params || !loc || !cls || !corners || NB < 1 || H < 1 || W < 1 || bad_P(P)) return OS2D_REFUSE(-1, "os2d_sample_decode: bad arguments");
  return os2d_launch_sample_decode(corr, params, NB, H, W, P, inverse, stride, rec_field, NB, NB, 0, loc, cls,
                                   corners, nullptr, 0, nullptr, os2d_stream(stream));
}

int os2d_decode_boxes(const float* loc, int NB, int H, int W, int stride, int rec_field, float img_w, float img_h,
                      float* boxes, void* stream) {
  if (!loc || !boxes || NB < 1 || H < 1 || W < 1) return OS2D_REFUSE(-1, "os2d_decode_boxes: bad arguments");
  return os2d_launch_decode_boxes(loc, NB, H, W, stride, rec_field, img_w, img_h, boxes, os2d_stream(stream));
}

int os2d_detect_level_supported(int H, int W) { return os2d_detect_level_lds_bytes(H, W) != 0 ? 1 : 0; }

int os2d_detect_level(const float* loc, const float* cls, int B, int H, int W, int stride, int rec_field, float img_w,
                      float img_h, float scale_x, float scale_y, float score_threshold, float iou_threshold,
                      float* out_boxes, float* out_scores, int* out_index, int* out_count, void* stream) {
  if (!loc || !cls || !out_boxes || !out_scores || !out_index || !out_count || B < 1 || H < 1 || W < 1 || stride < 1 || rec_field < 1)
    return OS2D_REFUSE(-1, "os2d_detect_level: bad arguments");
  return os2d_launch_detect_level(loc, cls, B, H, W, stride, rec_field, img_w, img_h, os2d_box_ops_scale<OS2D_BOX_MAX_OPS>(scale_x, scale_y),
                                  score_threshold, iou_threshold, out_boxes, out_scores, out_index, out_count, os2d_stream(stream));
}

int os2d_detect_level_ops(const float* loc, const float* cls, int B, int H, int W, int stride, int rec_field, float img_w,
                          float img_h, int op_count, const int* op_kinds, const float* op_args, float score_threshold,
                          float iou_threshold, float* out_boxes, float* out_scores, int* out_index, int* out_count,
                          void* stream) {
  if (!loc || !cls || !out_boxes || !out_scores || !out_index || !out_count || B < 1 || H < 1 || W < 1 || stride < 1 || rec_field < 1)
    return OS2D_REFUSE(-1, "os2d_detect_level_ops: bad arguments");
  Os2dBoxOps ops;
  if (!os2d_box_ops_from(op_kinds, op_args, op_count, &ops))
    return OS2D_REFUSE(-1, "os2d_detect_level_ops: bad transform chain (at most %d ops of kind 1..4)", OS2D_BOX_MAX_OPS);
  return os2d_launch_detect_level(loc, cls, B, H, W, stride, rec_field, img_w, img_h, ops, score_threshold, iou_threshold,
                                  out_boxes, out_scores, out_index, out_count, os2d_stream(stream));
}

int os2d_nms_workspace_bytes(int NC, int N, size_t* bytes) {
  if (!bytes || NC < 1 || N < 1) return OS2D_REFUSE(-1, "os2d_nms_workspace_bytes: bad arguments");
  *bytes = nms_workspace_bytes(NC, N);
  return 0;
}

int os2d_nms(const float* boxes, const int* counts, int NC, int N, float iou_threshold, unsigned char* keep,
             int* num_keep, void* workspace, size_t workspace_bytes, void* stream) {
  if (!boxes || !counts || !keep || !num_keep || !workspace || NC < 1 || N < 1) return OS2D_REFUSE(-1, "os2d_nms: bad arguments");
  if (!aligned_to(16, boxes, workspace)) return OS2D_REFUSE(-1, "os2d_nms: boxes and workspace must be 16-byte aligned");
  if (workspace_bytes < nms_workspace_bytes(NC, N)) return OS2D_REFUSE(-2, "os2d_nms: workspace too small");
  return os2d_launch_nms(boxes, counts, NC, N, iou_threshold, keep, num_keep, workspace, os2d_stream(stream));
}

size_t os2d_class_split_bytes(int B, int C) {
  if (B < 1 || C < 1) return 0;
  return (size_t)B * class_split_bytes(C);
}

int os2d_class_split(const float* qp, void* qs, int B, int C, void* stream) {
  if (!qp || !qs || B < 1 || C < 1) return OS2D_REFUSE(-1, "os2d_class_split: bad arguments");
  return os2d_launch_split_qp(qp, qs, B, C, os2d_stream(stream));
}

size_t os2d_packed_conv_bytes(int layer, int precision) {
  if (precision == OS2D_PRECISION_F32) return os2d_packed_conv_floats(layer) * sizeof(float);
  if (precision != OS2D_PRECISION_F16X3 && precision != OS2D_PRECISION_F16X2) return 0;
  Os2dLayer s;
  if (!conv_shape(layer, 6, &s)) return 0;
  return (size_t)s.groups * s.steps * 4 * s.rows * 16;  // [groups][padded k-steps][2 half-waves][hi|lo][rows] units of 16 B
}

int os2d_pack_conv_f16x3(int layer, int P, const float* w, const float* b, const float* bn_weight, const float* bn_bias,
                         const float* bn_running_mean, const float* bn_running_var, float bn_eps, const int* weight_exp,
                         const int* in_exp, const int* out_exp, void* packed_w, float* packed_b, void* stream) {
  Os2dLayer s;
  if (!conv_shape(layer, P, &s) || !w || !b || !packed_w || !packed_b || !weight_exp || !in_exp || (layer != 3 && !out_exp) ||
      !bn_all_or_none(bn_weight, bn_bias, bn_running_mean, bn_running_var) || (layer == 3 && bad_P(P)))
    return OS2D_REFUSE(-1, "os2d_pack_conv_f16x3: bad arguments (layer %d, P %d)", layer, P);
  return os2d_launch_pack_conv_f16(w, b, bn_weight, bn_bias, bn_running_mean, bn_running_var, bn_eps, s.cout, s.cin, s.ks, s.rows, s.steps,
                                   weight_exp, in_exp, layer == 3 ? nullptr : out_exp, packed_w, packed_b, os2d_stream(stream));
}

int os2d_rnorm_exp(void) { return OS2D_RNORM_EXP; }

int os2d_corr_normalize_f16x3(const float* corr, void* rshb, int NB, int H, int W, void* stream) {
  if (!corr || !rshb || NB < 1 || H < 1 || W < 1) return OS2D_REFUSE(-1, "os2d_corr_normalize_f16x3: bad arguments");
  return os2d_launch_corr_normalize_shb(corr, rshb, NB, H, W, os2d_stream(stream));
}

int os2d_transform_conv_f16x3(int layer, const void* in, const void* packed_w, const float* packed_b, void* out, int NB,
                              int P, int H, int W, int terms, int* status, void* stream) {
  if (!in || !packed_w || !packed_b || !out || NB < 1 || H < 1 || W < 1 || layer < 1 || layer > 3 || (layer == 3 && bad_P(P)) ||
      (terms != 3 && !(terms == 2 && layer == 1)))
    return OS2D_REFUSE(-1, "os2d_transform_conv_f16x3: bad arguments (layer=%d NB=%d P=%d terms=%d)", layer, NB, P, terms);
  const int max_w = layer == 1 ? OS2D_MAX_W_DIRECT7 : OS2D_MAX_W;
  if (W > max_w) return OS2D_REFUSE(-1, "os2d_transform_conv_f16x3: feature map width %d > %d", W, max_w);
  return os2d_launch_conv_f16x3(layer, in, packed_w, packed_b, Os2dRangeFlag{status, OS2D_STATUS_F16_RANGE}, out, NB, P, H, W, terms, os2d_stream(stream));
}

int os2d_fft_sizes(int H, int W, int* P, int* Q, int* nbins) {
  if (!P || !Q || !nbins) return OS2D_REFUSE(-1, "os2d_fft_sizes: null output");
  if (!os2d_fft_plan(H, W, P, Q, nbins, nullptr)) return OS2D_REFUSE(-3, "os2d_fft_sizes: no transform plan for a %dx%d map", H, W);
  return 0;
}

int os2d_fft_tiles(int H, int W, int* tiles_y, int* tiles_x, int* tile_h, int* tile_w) {
  int t[6];
  if (!tiles_y || !tiles_x || !tile_h || !tile_w) return OS2D_REFUSE(-1, "os2d_fft_tiles: null output");
  if (!os2d_fft_plan(H, W, nullptr, nullptr, nullptr, t)) return OS2D_REFUSE(-3, "os2d_fft_tiles: no transform plan for a %dx%d map", H, W);
  *tiles_y = t[0];
  *tiles_x = t[1];
  *tile_h = t[2];
  *tile_w = t[3];
  return 0;
}

int os2d_fft_forward(const float* corr, const float* inv_norm, float* X, const float* twQ, const float* twP, int NB, int C,
                     int H, int W, void* stream) {
  if (!corr || !inv_norm || !X || !twQ || !twP || NB < 1 || C < 1 || H < 1 || W < 1) return OS2D_REFUSE(-1, "os2d_fft_forward: bad arguments");
  return os2d_launch_fft_forward(corr, inv_norm, X, twQ, twP, NB, C, H, W, os2d_stream(stream));
}

int os2d_fft_inverse_ex(const float* Y, const float* packed_b, void* out, const float* twQ, const float* twP, int NB, int Cout,
                        int H, int W, int* status, int layout, void* stream) {
  constexpr Os2dLayer L1 = os2d_layer(1);
  if (!Y || !packed_b || !out || !twQ || !twP || NB < 1 || Cout != L1.cout || H < 1 || W < 1 || (layout != OS2D_SPECTRA_ROWS && layout != OS2D_SPECTRA_QUADS))
    return OS2D_REFUSE(-1, "os2d_fft_inverse: bad arguments (Cout must be 128: the 7x7 layer)");
  int rc = os2d_launch_border_zero_shb_planes(out, NB * (Cout / 8) * 2, H, W, os2d_stream(stream));
  if (rc) return rc;
  return os2d_launch_fft_inverse(Y, packed_b, L1.rows, out, twQ, twP, NB, Cout, H, W, Os2dRangeFlag{status, OS2D_STATUS_F16_RANGE}, layout, 0, os2d_stream(stream));
}

int os2d_fft_inverse(const float* Y, const float* packed_b, void* out, const float* twQ, const float* twP, int NB, int Cout,
                     int H, int W, int* status, void* stream) {
  return os2d_fft_inverse_ex(Y, packed_b, out, twQ, twP, NB, Cout, H, W, status, OS2D_SPECTRA_ROWS, stream);
}

size_t os2d_spectral_weight_bytes(int C, int Cout, int nbins) {
  if (C < 1 || Cout < 1 || Cout > 128 || bad_bins(nbins)) return 0;
  return os2d_spectral_weight_floats(C, Cout, nbins) * sizeof(float);
}

int os2d_spectral_gemm(const float* wspec, const float* X, float* Y, int NB, int C, int Cout, int nbins, void* stream) {
  if (!spectral_gemm_args_ok("os2d_spectral_gemm", "; nbins must be a multiple of 8", wspec, X, Y, NB, C, Cout, nbins, 1.f)) return -1;
  return os2d_launch_spectral_gemm(wspec, X, Y, NB, C, Cout, nbins, os2d_stream(stream));
}

int os2d_spectral_weights_build(const double* wfold, const double* twP64, const double* twQ64, int C, int Cout, int P, int Q,
                                int nbins, int split, void* out, void* workspace, void* stream) {
  if (!spectra_build_args_ok("os2d_spectral_weights_build", wfold, twP64, twQ64, out, workspace, split != 0, C, Cout, nbins, nullptr)) return -1;
  return os2d_launch_spectra_pack(wfold, twP64, twQ64, C, Cout, P, Q, nbins, split, 0, out, workspace, os2d_stream(stream));
}

size_t os2d_spectral_weight16_bytes(int C, int nbins) {
  if (C < 1 || bad_bins(nbins)) return 0;
  return os2d_spectral_weight16_size(C, nbins);
}

float os2d_spectral_xscale(int H, int W) {
  int t[6];
  if (H < 1 || W < 1 || !os2d_fft_plan(H, W, nullptr, nullptr, nullptr, t)) return 0.f;
  return os2d_spectral_xscale_for(t[4], t[5]);      // samples of one transform window (the whole map, or a tile + its halo)
}

int os2d_spectral_gemm_f16(const void* w16, const float* X, float* Y, int NB, int C, int Cout, int nbins, float xscale,
                           void* stream) {
  if (!spectral_gemm_args_ok("os2d_spectral_gemm_f16", "; nbins must be a multiple of 8", w16, X, Y, NB, C, Cout, nbins, xscale)) return -1;
  return os2d_launch_spectral_gemm_f16(w16, X, Y, NB, C, Cout, nbins, xscale, 0, 0, os2d_stream(stream));
}

/* ---- the transforms of the frequency-domain 7x7 layer as matrix products (dft_mfma.hip; OS2D_PRECISION_FFTX3) */
int os2d_dft_sizes(int H, int W, int* P, int* Q, int* nbins, int* tiles) {
  if (!P || !Q || !nbins) return OS2D_REFUSE(-1, "os2d_dft_sizes: null output");
  if (!os2d_dft_plan(H, W, P, Q, nbins, tiles)) return OS2D_REFUSE(-3, "os2d_dft_sizes: no transform plan for a %dx%d map", H, W);
  return 0;
}

int os2d_dft_channel_stride(int C) { return C == OS2D_K ? OS2D_XSPEC_CPAD : (C + 7) / 8 * 8; }

size_t os2d_dft_matrices_bytes(int P, int Q) {
  if (P < 4 || (P & 3) || Q < 2 || (Q & 1)) return 0;
  return os2d_dft_matrices_size(P, Q);
}

int os2d_dft_matrices_build(const double* twP64, const double* twQ64, int P, int Q, void* out, void* stream) {
  if (!twP64 || !twQ64 || !out || !aligned_to(16, out)) return OS2D_REFUSE(-1, "os2d_dft_matrices_build: bad arguments (out must be 16-byte aligned)");
  return os2d_launch_dft_matrices(twP64, twQ64, P, Q, out, os2d_stream(stream));
}

int os2d_dft_forward(const float* corr, const float* inv_norm, float* X, const void* matrices, int NB, int C, int H, int W,
                     void* stream) {
  if (!corr || !X || !matrices || NB < 1 || C < 1 || H < 1 || W < 1) return OS2D_REFUSE(-1, "os2d_dft_forward: bad arguments");      // inv_norm == NULL: unit norms
  return os2d_launch_dft_forward(corr, inv_norm, X, matrices, NB, C, os2d_dft_channel_stride(C), H, W, os2d_stream(stream));
}

int os2d_dft_inverse(const float* Y, const float* packed_b, void* out, const void* matrices, int NB, int Cout, int H, int W,
                     int* status, void* stream) {
  if (!dft_inverse_args_ok(Y, packed_b, out, matrices, NB, Cout, H, W))
    return OS2D_REFUSE(-1, "os2d_dft_inverse: bad arguments (Cout must be 128 or 64: the 7x7 layer / the 5x5 layer 128 -> 64)");
  return os2d_launch_dft_inverse(Y, packed_b, Cout, out, matrices, NB, Cout, H, W, Os2dRangeFlag{status, OS2D_STATUS_F16_RANGE},
                                 OS2D_DFT_OUT_SHB_BORDERS, os2d_stream(stream));
}

int os2d_dft_inverse_planes(const float* Y, const float* packed_b, float* out, const void* matrices, int NB, int Cout, int H, int W,
                            int* status, void* stream) {
  if (!dft_inverse_args_ok(Y, packed_b, out, matrices, NB, Cout, H, W)) return OS2D_REFUSE(-1, "os2d_dft_inverse_planes: bad arguments (Cout must be 128 or 64)");
  return os2d_launch_dft_inverse(Y, packed_b, Cout, out, matrices, NB, Cout, H, W, Os2dRangeFlag{status, OS2D_STATUS_F16_RANGE},
                                 OS2D_DFT_OUT_PLANES, os2d_stream(stream));
}

int os2d_spectral_weights_build_dft(const double* wfold, const double* twP64, const double* twQ64, int C, int Cout, int P, int Q,
                                    int nbins, void* out, void* workspace, void* stream) {
  if (!spectra_build_args_ok("os2d_spectral_weights_build_dft", wfold, twP64, twQ64, out, workspace, true, C, Cout, nbins, &P)) return -1;
  return os2d_launch_spectra_pack(wfold, twP64, twQ64, C, Cout, P, Q, nbins, 1, 1, out, workspace, os2d_stream(stream));
}

int os2d_spectral_gemm_f16_quads(const void* w16, const float* X, float* Y, int NB, int C, int Cout, int nbins, float xscale,
                                 void* stream) {
  if (!spectral_gemm_args_ok("os2d_spectral_gemm_f16_quads", "", w16, X, Y, NB, C, Cout, nbins, xscale)) return -1;
  return os2d_launch_spectral_gemm_f16(w16, X, Y, NB, C, Cout, nbins, xscale, 1, os2d_dft_channel_stride(C), os2d_stream(stream));
}

float os2d_dft_xscale(int H, int W) {
  int t[6];
  if (H < 1 || W < 1 || !os2d_dft_plan(H, W, nullptr, nullptr, nullptr, t)) return 0.f;
  return os2d_spectral_xscale_for(t[4], t[5]);
}

int os2d_alignment_grids(const float* params, int NB, int H, int W, int P, int inverse, float* theta, float* grids,
                         void* stream) {
  if (!params || (!theta && !grids) || NB < 1 || H < 1 || W < 1 || bad_P(P)) return OS2D_REFUSE(-1, "os2d_alignment_grids: bad arguments");
  return os2d_launch_alignment_grids(params, NB, H, W, P, inverse, theta, grids, os2d_stream(stream));
}

int os2d_prof_event_create(void** ev) {
  hipEvent_t e;
  hipError_t rc = hipEventCreate(&e);
  if (rc != hipSuccess || !ev) return OS2D_REFUSE(-4, "hipEventCreate: %s", hipGetErrorString(rc));
  *ev = e;
  return 0;
}
int os2d_prof_event_destroy(void* ev) { return hipEventDestroy(reinterpret_cast<hipEvent_t>(ev)) == hipSuccess ? 0 : -4; }
int os2d_prof_event_elapsed_ms(void* a, void* b, float* ms) {
  hipError_t rc = hipEventElapsedTime(ms, reinterpret_cast<hipEvent_t>(a), reinterpret_cast<hipEvent_t>(b));
  if (rc != hipSuccess) return OS2D_REFUSE(-4, "hipEventElapsedTime: %s", hipGetErrorString(rc));
  return 0;
}

}  // extern "C"
