// Operand loaders and result stores of the backward GEMMs (train_gemm.hip: gemm16_kernel, fp32; gemm_f16x3_kernel, split-fp16),
// the workspace layouts of their entry points and the five launch sites.
//
// A loader answers two questions about the same matrix:
//   operator()(z, row, k)          one element (gemm16_kernel stages element by element);
//   load8(z, row, k, ke, v)        the 8 elements k .. k+7 of one row, zeros from ke on (k is a multiple of 8): the index
//                                  decomposition k -> (channel, tap) or (pair, position) is done once and then walked.
// "Row" is the operand's non-reduced index: m for an A operand, n for a B operand.
#pragma once
#include "../csrc/os2d_common.h"

namespace os2d_train_gemm {

// 8 consecutive floats at p (the first `valid` of them exist; `vec`: p is 16-byte aligned and all 8 exist)
__device__ __forceinline__ void ld8(const float* __restrict__ p, int valid, bool vec, float (&v)[8]) {
  if (vec) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = j < valid ? p[j] : 0.f;
  }
}

// tap offset of the zero-bordered plane layout: flat distance of tap t = (dy, dx) of a KS x KS kernel
struct Taps {
  int ks, r, ws, t2;
  __device__ __forceinline__ int off(int t) const {
    const int dy = t / ks, dx = t - dy * ks;
    return (dy - r) * ws + (dx - r);
  }
};

// A(m, k) = w[m][k], row-major K columns
struct LdRows {
  const float* w;
  int K;
  bool vec = false;     // w is 16-byte aligned and K a multiple of 4: load8 may read 16 bytes at a time
  __device__ __forceinline__ float operator()(int, int m, int k) const { return w[(size_t)m * K + k]; }
  __device__ __forceinline__ void load8(int, int m, int k, int ke, float (&v)[8]) const {
    ld8(w + (size_t)m * K + k, ke - k, vec && k + 8 <= ke, v);
  }
};
// B(k = (c, t), n) = x[z][c][n + off(t)] (zero outside the plane)
struct LdShifted {
  const float* x;
  size_t zstride;
  int PL;
  Taps tp;
  __device__ __forceinline__ float operator()(int z, int k, int n) const {
    const int c = k / tp.t2, t = k - c * tp.t2;
    const int idx = n + tp.off(t);
    return (idx >= 0 && idx < PL) ? x[z * zstride + (size_t)c * PL + idx] : 0.f;
  }
  __device__ __forceinline__ void load8(int z, int n, int k, int ke, float (&v)[8]) const {
    int c = k / tp.t2;
    const int t = k - c * tp.t2;
    int dy = t / tp.ks, dx = t - dy * tp.ks;
    const float* base = x + z * zstride;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int idx = n + (dy - tp.r) * tp.ws + (dx - tp.r);
      v[j] = (k + j < ke && idx >= 0 && idx < PL) ? base[(size_t)c * PL + idx] : 0.f;
      if (++dx == tp.ks) {
        dx = 0;
        if (++dy == tp.ks) {
          dy = 0;
          ++c;
        }
      }
    }
  }
};
// out[z][m][n] of a plane buffer, zero at the pad cells; `bias` (NULL: none) is a per-row constant added at the data cells - a
// forward convolution's bias (one functor for both, so that the data gradient and the forward convolution share a kernel)
struct StPlane {
  float* out;
  size_t zstride;
  int PL, H, W;
  const float* bias = nullptr;
  __device__ __forceinline__ void operator()(int z, int m, int n, float v) const {
    out[z * zstride + (size_t)m * PL + n] = os2d_interior(n, H, W) ? (bias ? v + bias[m] : v) : 0.f;
  }
};
// weight gradient: A(o, k = (pair, n)) = dy[pair][o][n]
struct LdPairRows {
  const float* dy;
  size_t zstride;
  int PL;
  bool vec = false;     // dy is 16-byte aligned
  __device__ __forceinline__ float operator()(int, int m, int k) const {
    const int nb = k / PL, n = k - nb * PL;
    return dy[nb * zstride + (size_t)m * PL + n];
  }
  // PLANE is a multiple of 64: 8 positions from a multiple of 8 stay inside one pair's plane
  __device__ __forceinline__ void load8(int, int m, int k, int ke, float (&v)[8]) const {
    const int nb = k / PL, n = k - nb * PL;
    ld8(dy + nb * zstride + (size_t)m * PL + n, ke - k, vec && k + 8 <= ke, v);
  }
};
// B(k = (pair, n), j = (c, t)) = x[pair][c][n + off(t)]
struct LdPairShifted {
  const float* x;
  size_t zstride;
  int PL;
  Taps tp;
  __device__ __forceinline__ float operator()(int, int k, int j) const {
    const int nb = k / PL, n = k - nb * PL;
    const int c = j / tp.t2, t = j - c * tp.t2;
    const int idx = n + tp.off(t);
    return (idx >= 0 && idx < PL) ? x[nb * zstride + (size_t)c * PL + idx] : 0.f;
  }
  __device__ __forceinline__ void load8(int, int j, int k, int ke, float (&v)[8]) const {
    const int c = j / tp.t2, t = j - c * tp.t2;        // of the row alone: the same in every k-step
    const int nb = k / PL, n = k - nb * PL;
    const int idx = n + tp.off(t);
    const float* p = x + nb * zstride + (size_t)c * PL;
    if (k + 8 <= ke && idx >= 0 && idx + 8 <= PL) {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = p[idx + i];
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = (k + i < ke && idx + i >= 0 && idx + i < PL) ? p[idx + i] : 0.f;
    }
  }
};
struct StSlice {
  float* part;
  int M, N;
  __device__ __forceinline__ void operator()(int z, int m, int n, float v) const {
    part[((size_t)z * M + m) * N + n] = v;
  }
};
// correlation backward, image side (z = image a): A(c, k = (b, p)) = qp[b][c][p], B(k, n) = dcorr[a*B*225 + k][n]
struct LdClassT {
  const float* qp;
  int C;
  __device__ __forceinline__ float operator()(int, int c, int k) const {
    const int b = k / OS2D_K, p = k - b * OS2D_K;
    return qp[((size_t)b * C + c) * OS2D_QROWS + p];
  }
  __device__ __forceinline__ void load8(int, int c, int k, int ke, float (&v)[8]) const {
    int b = k / OS2D_K, p = k - b * OS2D_K;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[j] = k + j < ke ? qp[((size_t)b * C + c) * OS2D_QROWS + p] : 0.f;
      if (++p == OS2D_K) {
        p = 0;
        ++b;
      }
    }
  }
};
struct LdCorrRows {
  const float* dcorr;
  int B, HW;
  __device__ __forceinline__ float operator()(int z, int k, int n) const {
    return dcorr[((size_t)z * B * OS2D_K + k) * HW + n];
  }
  __device__ __forceinline__ void load8(int z, int n, int k, int ke, float (&v)[8]) const {
    const float* p = dcorr + ((size_t)z * B * OS2D_K + k) * HW + n;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = k + j < ke ? p[(size_t)j * HW] : 0.f;
  }
};
struct StDense {
  float* out;
  int M, N;
  __device__ __forceinline__ void operator()(int z, int m, int n, float v) const { out[((size_t)z * M + m) * N + n] = v; }
};
// correlation backward, class side (z = class b): A(c, k = (a, n)) = fm[a][c][n] / (|fm[a][:,n]| + 1e-5),
// B(k = (a, n), p) = dcorr[a*B + b][p][n]
struct LdImageNorm {
  const float* fm;
  const float* rinv;
  int C, HW;
  __device__ __forceinline__ float operator()(int, int c, int k) const {
    const int a = k / HW, n = k - a * HW;
    return fm[((size_t)a * C + c) * HW + n] * rinv[(size_t)a * HW + n];
  }
  __device__ __forceinline__ void load8(int, int c, int k, int ke, float (&v)[8]) const {
    int a = k / HW, n = k - a * HW;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[j] = k + j < ke ? fm[((size_t)a * C + c) * HW + n] * rinv[(size_t)a * HW + n] : 0.f;
      if (++n == HW) {
        n = 0;
        ++a;
      }
    }
  }
};
struct LdCorrCols {
  const float* dcorr;
  int B, HW;
  __device__ __forceinline__ float operator()(int z, int k, int p) const {
    const int a = k / HW, n = k - a * HW;
    return dcorr[(((size_t)a * B + z) * OS2D_K + p) * HW + n];
  }
  __device__ __forceinline__ void load8(int z, int p, int k, int ke, float (&v)[8]) const {
    int a = k / HW, n = k - a * HW;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[j] = k + j < ke ? dcorr[(((size_t)a * B + z) * OS2D_K + p) * HW + n] : 0.f;
      if (++n == HW) {
        n = 0;
        ++a;
      }
    }
  }
};

// ---- k-step of either kernel: the split-K slices of the weight gradient are whole k-steps
constexpr int GEMM16_KSTEP = 16, F16X3_KSTEP = 32;
inline int kstep(int arith) { return arith ? F16X3_KSTEP : GEMM16_KSTEP; }

// ---- the float workspaces of the *_ex entry points, each defined once for its size function, its "workspace too small" check
// and its launch.  Maxima words exist at arith = 1 only; the sites clear (hipMemsetAsync) and fill them, nothing waits for the host.
// data gradient: the flipped filters, then conv_words; forward convolution: conv_words alone (fp32: one float nobody reads)
inline size_t conv_words(int arith, int NB) { return arith ? 1 + (size_t)NB : 0; }      // the filters', one per pair
inline size_t conv_forward_floats(int arith, int NB) { return arith ? conv_words(arith, NB) : 1; }
// weight gradient: weight_words_room floats (2 words: dy, x) in front of the split-K slices, and as many more per slice of room
constexpr size_t WEIGHT_WORDS = 2;
inline size_t weight_words_room(int arith) { return arith ? 16 : 0; }
// correlation backward: rinv [A,HW] | A*HW floats not used | dfh [A,C,HW] | words: qp, the normalised image map, dcorr per
// image (A), dcorr per class (B)
inline size_t corr_words(int arith, int A, int B) { return arith ? 2 + (size_t)A + B : 0; }
struct CorrWorkspace {
  size_t dfh, words, total;       // rinv starts at 0
};
inline CorrWorkspace corr_workspace(int arith, int A, int B, int C, size_t HW) {
  const size_t dfh = 2 * (size_t)A * HW, words = dfh + (size_t)A * C * HW;
  return {dfh, words, words + corr_words(arith, A, B)};
}

}  // namespace os2d_train_gemm

// ---- the five GEMM launch sites (train_gemm.hip), each for both arithmetics: arith 0 = gemm16_kernel (fp32), 1 = the maxima
// pass of the site's operands + gemm_f16x3_kernel.  `words`: the site's maxima words (not read at arith 0).  Calls between the
// units of the library, not exports of it: hidden.
#pragma GCC visibility push(hidden)
// conv data gradient: wt = the flipped filters [cin][cout*T2]
int os2d_gemm_conv_data(int arith, const float* wt, const float* dy, float* dx, int cout, int cin, int ks, int NB, int H, int W,
                        unsigned* words, hipStream_t stream);
// forward convolution z = conv(x) + bias (the training forward of a layer whose BatchNorm takes batch statistics): w = the raw
// filters [cout][cin*T2] - a forward convolution is the data gradient's shape with the channel counts swapped and unflipped
// filters -, xplanes = planes per pair of x
int os2d_gemm_conv_forward(int arith, const float* w, const float* bias, const float* x, int xplanes, float* z, int cout, int cin, int ks,
                           int NB, int H, int W, unsigned* words, hipStream_t stream);
// conv weight gradient into `splits` partial slices of ksplit positions (a multiple of kstep(arith)); xplanes = planes per pair of x
int os2d_gemm_conv_weight(int arith, const float* x, int xplanes, const float* dy, float* part, int cout, int cin, int ks, int NB, int H,
                          int W, int splits, int ksplit, unsigned* words, hipStream_t stream);
// correlation backward, image side (dfh = d of the normalised image map) and class side (dq).  At arith = 1
// os2d_gemm_corr_maxima goes first: it clears the 2 + A + B words and takes the maxima of dcorr both sides scale it by.
int os2d_gemm_corr_maxima(const float* dcorr, int A, int B, int HW, unsigned* words, hipStream_t stream);
int os2d_gemm_corr_image(int arith, const float* qp, const float* dcorr, int A, int B, int C, int HW, float* dfh, unsigned* words,
                         hipStream_t stream);
int os2d_gemm_corr_class(int arith, const float* fm, const float* rinv, const float* dcorr, int A, int B, int C, int HW, float* dq,
                         unsigned* words, hipStream_t stream);
#pragma GCC visibility pop
