/* C ABI of libos2d_image.so: the normalised image pyramid from uint8 images on the device (gfx950) - the resize of an 8-bit
 * RGB image in the integer arithmetic of Pillow's Resample.c (a horizontal pass rounded to uint8, then a vertical pass) followed
 * by a per-channel table lookup (ToTensor + Normalize of every byte value).
 *
 * `stream` is a hipStream_t, the call only enqueues work.  Return value: 0, or a negative code with the text in
 * os2d_image_last_error() (-1 bad argument, -4 launch failure).
 */
#ifndef OS2D_IMAGE_H
#define OS2D_IMAGE_H
#include <stddef.h>

#define OS2D_IMAGE_ABI_VERSION 1
#define OS2D_IMAGE_MAX_RATIO 16 /* in/out and out/in size ratio per axis beyond which a call is refused */

#ifdef __cplusplus
extern "C" {
#endif

int os2d_image_abi_version(void);
const char* os2d_image_last_error(void);

/* One level: resizes the window (x0, y0, w, h) of `A` uint8 HWC images to ow x oh.
 *
 * src (device): image a starts at src + a * image_stride, its row y at + y * row_pitch (bytes), 3 bytes per pixel; the images
 *   are img_w x img_h.  hflip / vflip: the window's pixel (x, y) is read at (w - 1 - x, h - 1 - y) - the flip follows the crop.
 * Tables of an axis with n source and m output positions (x: n = w, m = ow, k = kx; y: n = h, m = oh, k = ky):
 *   coef (device, int32 [m][k]): fixed-point weights (22 fractional bits) of the taps of every output position;
 *   bounds (device, int32 [m][2]): (first source position, number of taps); bounds_host: the same table in host memory, read
 *   before the launch: 0 <= first, 1 <= taps <= k, first + taps <= n are checked and the tile height is chosen from it.
 * lut (device, float [3][256]): the value of every byte per channel; unused (may be NULL) when out_u8.
 * out (device): out_u8 == 0: float [A][3][oh][ow], 16-byte aligned; out_u8 != 0: uint8 [A][oh][ow][3].
 */
int os2d_image_resample(const unsigned char* src, int A, int img_w, int img_h, long long row_pitch, long long image_stride, int x0,
                        int y0, int w, int h, int hflip, int vflip, const int* xcoef, const int* xbounds, const int* xbounds_host,
                        int kx, const int* ycoef, const int* ybounds, const int* ybounds_host, int ky, int ow, int oh,
                        const float* lut, void* out, int out_u8, void* stream);

#ifdef __cplusplus
}
#endif
#endif
