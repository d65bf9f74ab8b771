/* C ABI of libos2d_augment.so: the training images from uint8 images on the device (gfx950) - what the dataloader's augmentation
 * adds to the image pyramid of libos2d_image.so (include/os2d_image.h): the resize of a window that may leave the image, and
 * PIL's colour operations.  A library of its own: libos2d_image.so keeps exactly its two kernels and its ABI.
 *
 * `stream` is a hipStream_t, the calls only enqueue work.  Return value: 0, or a negative code with the text in
 * os2d_augment_last_error() (-1 bad argument, -4 launch failure).
 */
#ifndef OS2D_AUGMENT_H
#define OS2D_AUGMENT_H
#include <stddef.h>

#define OS2D_AUGMENT_ABI_VERSION 1
#define OS2D_AUGMENT_MAX_RATIO 16 /* as OS2D_IMAGE_MAX_RATIO */

#ifdef __cplusplus
extern "C" {
#endif

int os2d_augment_abi_version(void);
const char* os2d_augment_last_error(void);

/* os2d_image_resample (same arguments, same kernel source, same tables) with a window that may extend beyond the image on any
 * side: a position outside the image is a pixel of value 0 that takes its filter weight (an image expanded by a border of
 * zeros, then cropped).  x0 / y0 may be negative and x0 + w / y0 + h may exceed the image; |x0|, |y0|, w, h <= 2^30.  A window
 * without a pixel inside the image is refused. */
int os2d_augment_resample_padded(const unsigned char* src, int A, int img_w, int img_h, long long row_pitch, long long image_stride,
                                 int x0, int y0, int w, int h, int hflip, int vflip, const int* xcoef, const int* xbounds,
                                 const int* xbounds_host, int kx, const int* ycoef, const int* ybounds, const int* ybounds_host,
                                 int ky, int ow, int oh, const float* lut, void* out, int out_u8, void* stream);

/* Colour distortion of one uint8 HWC image in the arithmetic of PIL's ImageEnhance (Image.blend with a degenerate image) and
 * of its RGB <-> HSV conversion: a chain of n_ops <= OS2D_AUGMENT_COLOR_MAX_OPS operations applied to every pixel in the order
 * given.  kinds / factors (HOST arrays of n_ops entries, read before the call returns):
 *   BRIGHTNESS f  blend with black;  SATURATION f  blend with the pixel's luma;  CONTRAST f  blend with the rounded mean luma
 *   of the image as it stands when the operation is reached (at most one per chain);  HUE f  H += (int)(f * 255) modulo 256
 *   in HSV;  TO_HSV / FROM_HSV (factor unused)  the two conversions of HUE on their own: the three bytes become (H, S, V) / are
 *   read as (H, S, V).  Factors are finite; a blend uses its factor rounded to float.
 * src (device): w x h, row y at + y * row_pitch (bytes), 3 bytes per pixel.
 * lut (device, float [3][256]): the value of every byte per channel; unused (may be NULL) when out_u8.
 * out (device): out_u8 == 0: float [3][h][w], 16-byte aligned; out_u8 != 0: uint8 [h][w][3]; not src.
 * sums (device, OS2D_AUGMENT_COLOR_SLOTS 64-bit words, 8-byte aligned): workspace of the mean, needed (and overwritten) only by
 *   a chain with a contrast operation - then the call enqueues two kernels, else one.  Nothing comes back to the host. */
#define OS2D_AUGMENT_COLOR_MAX_OPS 4
#define OS2D_AUGMENT_COLOR_SLOTS 256
#define OS2D_AUGMENT_COLOR_BRIGHTNESS 1
#define OS2D_AUGMENT_COLOR_CONTRAST 2
#define OS2D_AUGMENT_COLOR_SATURATION 3
#define OS2D_AUGMENT_COLOR_HUE 4
#define OS2D_AUGMENT_COLOR_TO_HSV 5
#define OS2D_AUGMENT_COLOR_FROM_HSV 6
int os2d_augment_color(const unsigned char* src, int w, int h, long long row_pitch, int n_ops, const int* kinds, const double* factors,
                       const float* lut, void* out, int out_u8, unsigned long long* sums, void* stream);

#ifdef __cplusplus
}
#endif
#endif
