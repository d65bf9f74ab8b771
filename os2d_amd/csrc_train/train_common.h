// Shared by the translation units of libos2d_train.so: the error text that os2d_train_last_error() returns lives in train.hip
// (the library has its own error store: it does not link against the forward's).
#ifndef OS2D_TRAIN_COMMON_H
#define OS2D_TRAIN_COMMON_H
#include <hip/hip_runtime.h>
#include <stdio.h>

// Stores `text` as the calling thread's last error (not exported).
__attribute__((visibility("hidden"))) void os2d_train_store_error(const char* text);

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

// after a kernel launch: 0, or -4 with "<what>: <HIP error>" as the thread's last error
static inline int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    char buf[512];
    snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
    os2d_train_store_error(buf);
    return -4;
  }
  return 0;
}

#endif
