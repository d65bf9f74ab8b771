// libos2d_augment.so: the resize of libos2d_image.so for a window that may leave the image (include/os2d_augment.h, DESIGN.md
// section 15) - the PADDED instantiations of the one kernel template (csrc_image/resample_kernel.h): a position outside the
// image is a pixel of value 0 that keeps its filter weight and is never read.
#include "../csrc_image/resample_kernel.h"
#include "../../include/os2d_augment.h"

static_assert(OS2D_RESAMPLE_MAX_RATIO == OS2D_AUGMENT_MAX_RATIO, "the ratio the launch checks is the header's");

extern "C" {

int os2d_augment_abi_version(void) { return OS2D_AUGMENT_ABI_VERSION; }
const char* os2d_augment_last_error(void) { return os2d_error_text; }

int os2d_augment_resample_padded(const unsigned char* src, int A, int img_w, int img_h, long long row_pitch, long long image_stride,
                                 int x0, int y0, int w, int h, int hflip, int vflip, const int* xcoef, const int* xbounds,
                                 const int* xbounds_host, int kx, const int* ycoef, const int* ybounds, const int* ybounds_host,
                                 int ky, int ow, int oh, const float* lut, void* out, int out_u8, void* stream) {
  return resample<true>(src, A, img_w, img_h, row_pitch, image_stride, x0, y0, w, h, hflip, vflip, xcoef, xbounds, xbounds_host, kx,
                        ycoef, ybounds, ybounds_host, ky, ow, oh, lut, out, out_u8, stream);
}

}  // extern "C"
