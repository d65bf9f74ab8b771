// Host plumbing that every translation unit of every library shares: the calling thread's last error text, the refusal and
// launch checks that fill it, and the stream cast of the C ABIs.
//
// The text is an inline thread_local variable with hidden visibility: the units of ONE library share it (the linker merges the
// copies), two libraries loaded into one process each keep their own (nothing is exported, so none binds to another's), and no
// library has to link against another or carry a translation unit for it.  Each library's *_last_error returns it.
//
// Host-emulated builds (tests/host/*.cpp, -DOS2D_HOST_EMU, plain g++) get the text and its setters only: no HIP runtime.
#pragma once
#include <stdarg.h>
#include <stdio.h>

__attribute__((visibility("hidden"))) inline thread_local char os2d_error_text[512] = {0};

__attribute__((format(printf, 1, 2))) static inline void os2d_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(os2d_error_text, sizeof(os2d_error_text), fmt, ap);
  va_end(ap);
}
static inline void os2d_clear_error() { os2d_error_text[0] = 0; }
// an argument check failed: `text` becomes the thread's last error, the entry point returns -1
static inline int os2d_refuse(const char* text) {
  os2d_set_error("%s", text);
  return -1;
}
// a failed check in one statement: the formatted text becomes the thread's last error, the value is `rc`
#define OS2D_REFUSE(rc, ...) (os2d_set_error(__VA_ARGS__), (rc))

#ifndef OS2D_HOST_EMU
#include <hip/hip_runtime.h>

static inline hipStream_t os2d_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// after a kernel launch: 0, or -4 with "<what> launch: <HIP error>" as the thread's last error
static inline int os2d_launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    os2d_set_error("%s launch: %s", what, hipGetErrorString(e));
    return -4;
  }
  return 0;
}
#endif
