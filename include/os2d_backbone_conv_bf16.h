/* C ABI of libos2d_backbone_conv_bf16.so: the 1x1 convolutions of include/os2d_backbone_conv.h in a second arithmetic, split bf16
 * ("bf16x3"): every fp32 operand is split exactly into three bf16 values, six of the nine products run on the bf16 matrix instruction
 * of gfx950 and are accumulated in fp32 - the setting conv1x1_precision = "bf16x3" of the backbone's inference route "fused_conv1x1"
 * (os2d_amd/modeling/backbone_fused.py).
 *
 * Tensors, the fold s / t (sr / tr), `stream`, the return codes (0, -1 bad argument: nothing was launched and nothing written, -4 launch
 * failure; the text in os2d_backbone_conv_bf16_last_error()) and the size limits are those of include/os2d_backbone_conv.h.
 *
 * The split of a value v (os2d_amd/csrc_backbone_conv_bf16/bf16x3_split.h), bf16() rounding to nearest even:
 *     v0 = bf16(v)   v1 = bf16(v - v0)   v2 = bf16(v - v0 - v1)       v == v0 + v1 + v2, |v1| <= 2^-8 |v|, |v2| <= 2^-16 |v|
 * A finite v has finite parts (where bf16(v) would be infinite, v0 is v truncated to bf16).  A non-finite v is ONE part, +-Inf or the quiet
 * NaN 0x7FC0, and the other two are 0: the leading part of a weight, the LAST part of an activation, which meets only the leading part of
 * the weight in the six products below - so that Inf * w is one product.  The parts of a value below 2^-109 in magnitude may lose what lies
 * below bf16's smallest subnormal.
 */
#ifndef OS2D_BACKBONE_CONV_BF16_H
#define OS2D_BACKBONE_CONV_BF16_H
#include <stddef.h>

#define OS2D_BACKBONE_CONV_BF16_ABI_VERSION 1
/* The work-group's tile, as in os2d_backbone_conv.h: TILE_M output channels x TILE_N pixels, or SMALL_TILE_M x SMALL_TILE_N for a layer
 * of at most SMALL_TILE_M output channels.  TILE_K input channels per step: Kp is Cin rounded up to a multiple of it. */
#define OS2D_BACKBONE_CONV_BF16_TILE_M 128
#define OS2D_BACKBONE_CONV_BF16_TILE_N 128
#define OS2D_BACKBONE_CONV_BF16_TILE_K 32
#define OS2D_BACKBONE_CONV_BF16_SMALL_TILE_M 64
#define OS2D_BACKBONE_CONV_BF16_SMALL_TILE_N 256
#define OS2D_BACKBONE_CONV_BF16_MAX_GROUPS 2048 /* no launch has more work-groups: the kernel strides over the rest of the tiles */

#ifdef __cplusplus
extern "C" {
#endif

int os2d_backbone_conv_bf16_abi_version(void);
const char* os2d_backbone_conv_bf16_last_error(void);

/* The size of the packed weights of a layer in 16-bit elements, 3 * Kp * Cout; 0 for a size outside 1 ... 2^20.
 *
 * The layout, wp[part][Kp / 8][Cout][8]: element (part p, output channel co, input channel k) is at
 *     ((p * (Kp / 8) + k / 8) * Cout + co) * 8 + k % 8
 * so the 8 consecutive k that a lane of the matrix instruction holds for its row of the A operand are one 16-byte unit, and the units of
 * consecutive output channels follow each other.  Part 0 is the leading one.  Elements with k >= Cin are zeros. */
size_t os2d_backbone_conv_bf16_packed_elems(int Cout, int Cin);

/* Splits w [Cout][Cin] (fp32, conv.weight as it is) into wp as laid out above.  wp is 16-byte aligned and apart from w. */
int os2d_backbone_conv_bf16_pack_weights(const float* w, unsigned short* wp, int Cout, int Cin, void* stream);

/* os2d_backbone_conv1x1 with wp, the packed weights of the layer, in place of w; x [N][Cin][H][W] is split inside the kernel, on its way
 * into LDS.
 *
 *   acc = sum over the blocks B = 0, 1, ..., Kp / 16 - 1 of 16 consecutive k, in this order, and within a block over the six products
 *         x2 w0,  x1 w1,  x0 w2,  x1 w0,  x0 w1,  x0 w0          (smallest first; the parts xi of x[n][k][stride * i][stride * j], wi of w[co][k])
 *   in this order, each of them one v_mfma_f32_32x32x16_bf16 that adds its 16 exact products to the one fp32 accumulator of the output.
 * Steps with k >= Cin multiply 0 by 0: both operands are written as zeros, nothing from outside a tensor reaches an output.  The order
 * is a function of Cin alone - not of n, the position, N, H, W, the tile shape, the grid or the load path - so an output's bits depend only
 * on its own input column, w[co] and the fold.  The three products left out are below (2^-23 + 2^-32) |w x|.  A NaN or an Inf * 0 in a
 * column makes every output of that column NaN and touches no other; Inf * w is +-Inf as in fp32 (for a finite w whose leading part is not
 * 0, |w| >= 2^-134).  A non-finite WEIGHT makes every output of its row non-finite, but NaN where fp32 may have an infinity.
 *
 *   v = fmaf(acc, s[co], t[co]);   d = r ? (sr ? fmaf(r, sr[co], tr[co]) : r) : none;   y = v + d  (a separately rounded add; y = v
 *   without r);   y = relu_nan(y) if relu.
 * sr and tr are both given or both NULL, and only together with r.  wp is 16-byte aligned; y overlaps none of x, wp, r. */
int os2d_backbone_conv1x1_bf16x3(const float* x, const unsigned short* wp, const float* s, const float* t, const float* r, const float* sr,
                                 const float* tr, float* y, int N, int Cin, int Cout, int H, int W, int stride, int relu, void* stream);

#ifdef __cplusplus
}
#endif
#endif
