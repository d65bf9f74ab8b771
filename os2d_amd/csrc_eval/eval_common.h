// Shared by the translation units of libos2d_eval.so: the tile geometry of the device-wide kernels (error text, launch check
// and stream cast: csrc_shared/abi_common.h).
#ifndef OS2D_EVAL_COMMON_H
#define OS2D_EVAL_COMMON_H
#include "../csrc_shared/abi_common.h"

#define EVAL_THREADS 256
#define EVAL_ITEMS 8
#define EVAL_TILE (EVAL_THREADS * EVAL_ITEMS)   // positions per work-group in the sort and the scans

typedef unsigned int u32;
typedef unsigned long long u64;

static inline int tiles(int D) { return (int)(((long long)D + EVAL_TILE - 1) / EVAL_TILE); }
static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

#endif
