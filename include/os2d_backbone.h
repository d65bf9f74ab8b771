/* C ABI of libos2d_backbone.so: what runs between the convolutions of a ResNet with frozen BatchNorms on the device (gfx950) -
 * the inference route of the backbone (os2d_amd/modeling/backbone_fused.py).  The convolutions stay with
 * MIOpen; a BatchNorm arrives folded into one multiplier and one offset per channel,
 *   s = gamma / sqrt(running_var + eps),  t = beta - running_mean * s,
 * computed by the caller in float64 and rounded once to fp32.
 *
 * All tensors are fp32, contiguous, NCHW and 4-byte aligned; s / t (and sr / tr) are fp32 vectors of C entries.  The arithmetic
 * written at each entry point is the contract: fmaf is ONE rounding, relu_nan(v) = (v < 0) ? 0 : v keeps a NaN as torch.relu does.
 *
 * `stream` is a hipStream_t, the calls only enqueue work.  Return value: 0, or a negative code with the text in
 * os2d_backbone_last_error() (-1 bad argument: nothing was launched and nothing written, -4 launch failure).
 * Sizes: N, C, HW, H, W >= 1, N * C < 2^31, HW (H * W) <= 2^30, N * C * HW <= 2^40.
 */
#ifndef OS2D_BACKBONE_H
#define OS2D_BACKBONE_H
#include <stddef.h>

#define OS2D_BACKBONE_ABI_VERSION 1
#define OS2D_BACKBONE_MAX_GROUPS 2048 /* no launch has more work-groups: the kernels stride over the rest */

#ifdef __cplusplus
extern "C" {
#endif

int os2d_backbone_abi_version(void);
const char* os2d_backbone_last_error(void);

/* y[n][c][i] = relu_nan(fmaf(x[n][c][i], s[c], t[c])).  y may BE x (in place); any other overlap of the two is refused. */
int os2d_backbone_bn_relu(const float* x, const float* s, const float* t, float* y, int N, int C, int HW, void* stream);

/* The end of a bottleneck:  v = fmaf(x, s[c], t[c]);  d = sr ? fmaf(r, sr[c], tr[c]) : r  (the BatchNorm of the downsample branch, or
 * the block's input as it is);  y = relu_nan(v + d), the sum a separately rounded add.  sr and tr are both given or both NULL.
 * y may BE x; y must not overlap r. */
int os2d_backbone_bn_add_relu(const float* x, const float* s, const float* t, const float* r, const float* sr, const float* tr,
                              float* y, int N, int C, int HW, void* stream);

/* The end of the stem: MaxPool2d(kernel 3, stride 2, padding 1) over relu_nan(fmaf(x, s[c], t[c])).  x is [N][C][H][W], y is
 * [N][C][(H - 1) / 2 + 1][(W - 1) / 2 + 1].  A NaN anywhere in a window makes that output NaN, as torch's pooling does; the
 * padding never wins, every value being at least 0.  y must not overlap x. */
int os2d_backbone_bn_relu_maxpool(const float* x, const float* s, const float* t, float* y, int N, int C, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif
