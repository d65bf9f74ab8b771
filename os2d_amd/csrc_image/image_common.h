// Shared by the translation units of libos2d_image.so: the tile geometry (error text, launch check and stream cast:
// csrc_shared/abi_common.h).
#ifndef OS2D_IMAGE_COMMON_H
#define OS2D_IMAGE_COMMON_H
#include "../csrc_shared/abi_common.h"

#define IMG_THREADS 256
#define IMG_TW 128                                   // output columns of a tile
#define IMG_TH_MAX 16                                // output rows of a tile: 16, 8, 4, 2 or 1 (chosen per level)
#define IMG_UNITS (IMG_TW / 4 + 1)                   // 16-byte units a tile's row of floats can touch (unaligned row start)
#define IMG_LUT_BYTES (3 * 256 * 4)
#define IMG_LDS_BYTES 65536
#define IMG_MAX_ROWS ((IMG_LDS_BYTES - IMG_LUT_BYTES) / (3 * IMG_TW))    // staged source rows that fit: 162
#define IMG_PRECISION_BITS 22                        // Pillow: 32 - 8 - 2

#endif
