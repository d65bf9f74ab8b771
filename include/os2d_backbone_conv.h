/* C ABI of libos2d_backbone_conv.so: the 1x1 convolutions of a ResNet with frozen BatchNorms as strict fp32 GEMMs on the fp32-input
 * matrix instruction of gfx950, with the folded BatchNorm, the residual add and the ReLU as the GEMM's epilogue - the inference
 * route "fused_conv1x1" of the backbone (os2d_amd/modeling/backbone_fused.py).
 *
 * In NCHW a 1x1 convolution is, per image, Y[Cout][HW] = W[Cout][Cin] . X[Cin][HW] with all three operands row-major as they lie in
 * memory: nothing is transposed or copied.  s / t (and sr / tr) are a BatchNorm folded as include/os2d_backbone.h describes.
 *
 * All tensors are fp32, contiguous, NCHW and 4-byte aligned.  The arithmetic written at the entry point is the contract: fmaf is
 * ONE rounding, relu_nan(v) = (v < 0) ? 0 : v keeps a NaN as torch.relu does.
 *
 * `stream` is a hipStream_t, the call only enqueues work.  Return value: 0, or a negative code with the text in
 * os2d_backbone_conv_last_error() (-1 bad argument: nothing was launched and nothing written, -4 launch failure).
 * Sizes, for x AND y: every size >= 1, N * C < 2^31, H * W <= 2^30, N * C * H * W <= 2^40; Cin, Cout <= 2^20.
 */
#ifndef OS2D_BACKBONE_CONV_H
#define OS2D_BACKBONE_CONV_H
#include <stddef.h>

#define OS2D_BACKBONE_CONV_ABI_VERSION 1
/* The work-group's tile: TILE_M output channels x TILE_N pixels, TILE_K input channels per step.  A layer of at most
 * SMALL_TILE_M output channels runs in the second shape, SMALL_TILE_M x SMALL_TILE_N (same TILE_K, same arithmetic). */
#define OS2D_BACKBONE_CONV_TILE_M 128
#define OS2D_BACKBONE_CONV_TILE_N 128
#define OS2D_BACKBONE_CONV_TILE_K 16
#define OS2D_BACKBONE_CONV_SMALL_TILE_M 64
#define OS2D_BACKBONE_CONV_SMALL_TILE_N 256
#define OS2D_BACKBONE_CONV_MAX_GROUPS 2048 /* no launch has more work-groups: the kernel strides over the rest of the tiles */

#ifdef __cplusplus
extern "C" {
#endif

int os2d_backbone_conv_abi_version(void);
const char* os2d_backbone_conv_last_error(void);

/* x [N][Cin][H][W], w [Cout][Cin] (conv.weight as it is), y and r [N][Cout][Ho][Wo] with Ho = (H - 1) / stride + 1 and Wo likewise;
 * stride is 1 or 2, relu 0 or 1.
 *
 *   acc = sum over k of w[co][k] * x[n][k][stride * i][stride * j]
 * in fp32 on v_mfma_f32_32x32x2_f32, as ONE chain per output in ascending k:  acc = 0;  acc = fmaf(w[co][k], x[..k..], acc) for
 * k = 0, 1, ..., Kp - 1, where Kp is Cin rounded up to a multiple of TILE_K and the steps k >= Cin multiply 0 by 0 (both operands
 * are written as zeros: nothing from outside a tensor reaches an output).  The order is a function of Cin alone - not of n, the
 * position, N, H, W, the tile shape or the grid - so an output's bits depend only on its own input column, w[co], and the fold.
 * A NaN or an Inf * 0 in a column makes every output of that column NaN, as torch's convolution does, and touches no other.
 *
 *   v = fmaf(acc, s[co], t[co]);   d = r ? (sr ? fmaf(r, sr[co], tr[co]) : r) : none;   y = v + d  (a separately rounded add; y = v
 *   without r);   y = relu_nan(y) if relu.
 * sr and tr are both given or both NULL, and only together with r.  y overlaps none of x, w, r. */
int os2d_backbone_conv1x1(const float* x, const float* w, const float* s, const float* t, const float* r, const float* sr, const float* tr,
                          float* y, int N, int Cin, int Cout, int H, int W, int stride, int relu, void* stream);

#ifdef __cplusplus
}
#endif
#endif
