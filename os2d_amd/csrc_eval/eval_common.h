// Shared by the translation units of libos2d_eval.so: the error store (it lives in match.hip; the library links against
// neither of the other two), launch plumbing and the tile geometry of the device-wide kernels.
#ifndef OS2D_EVAL_COMMON_H
#define OS2D_EVAL_COMMON_H
#include <hip/hip_runtime.h>
#include <stdio.h>

#define EVAL_THREADS 256
#define EVAL_ITEMS 8
#define EVAL_TILE (EVAL_THREADS * EVAL_ITEMS)   // positions per work-group in the sort and the scans

typedef unsigned int u32;
typedef unsigned long long u64;

// Stores `text` as the calling thread's last error (not exported).
__attribute__((visibility("hidden"))) void os2d_eval_store_error(const char* text);

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

static inline int refuse(const char* text) {
  os2d_eval_store_error(text);
  return -1;
}

// after a kernel launch: 0, or -4 with "<what>: <HIP error>" as the thread's last error
static inline int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    char buf[512];
    snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
    os2d_eval_store_error(buf);
    return -4;
  }
  return 0;
}

static inline int tiles(int D) { return (int)(((long long)D + EVAL_TILE - 1) / EVAL_TILE); }
static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

#endif
