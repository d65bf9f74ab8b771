// libos2d_image.so: the resize of 8-bit RGB images in the arithmetic of Pillow's Resample.c and the normalised float planes
// of an image-pyramid level, in one kernel (include/os2d_image.h).
//
// A work-group owns an output tile of IMG_TW columns x th rows of one image.
//   Phase 1: the horizontal pass of the source rows the tile's vertical taps reach, for the tile's columns, rounded and clipped
//            to uint8 as ImagingResampleHorizontal_8bpc does, into LDS as three byte planes per row.
//   Phase 2: the vertical pass from LDS (ImagingResampleVertical_8bpc), then either the byte itself (uint8 HWC output) or the
//            table value of (channel, byte) stored as whole 16-byte units of the float plane's row; the units at the two ends of
//            a tile's row that the row only partly covers are stored element by element.
// Tap counts and positions come from the tables, nothing below knows the filter.  The kernel is a template in
// resample_kernel.h; this library instantiates it for windows inside the image (PADDED = false).  Every source index is clamped to the window
// and every LDS row to the staged range, so tables that differ from the checked host copy cannot make the kernel leave its
// buffers.  No atomics; every output element is written by exactly one thread from the inputs alone.
#include "resample_kernel.h"
#include "../../include/os2d_image.h"

static_assert(OS2D_RESAMPLE_MAX_RATIO == OS2D_IMAGE_MAX_RATIO, "the ratio the launch checks is the header's");

extern "C" {

int os2d_image_abi_version(void) { return OS2D_IMAGE_ABI_VERSION; }
const char* os2d_image_last_error(void) { return os2d_error_text; }

int os2d_image_resample(const unsigned char* src, int A, int img_w, int img_h, long long row_pitch, long long image_stride, int x0,
                        int y0, int w, int h, int hflip, int vflip, const int* xcoef, const int* xbounds, const int* xbounds_host,
                        int kx, const int* ycoef, const int* ybounds, const int* ybounds_host, int ky, int ow, int oh,
                        const float* lut, void* out, int out_u8, void* stream) {
  return resample<false>(src, A, img_w, img_h, row_pitch, image_stride, x0, y0, w, h, hflip, vflip, xcoef, xbounds, xbounds_host, kx,
                         ycoef, ybounds, ybounds_host, ky, ow, oh, lut, out, out_u8, stream);
}

}  // extern "C"
