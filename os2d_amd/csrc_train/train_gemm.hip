// The GEMMs of the training library in both arithmetics, and the five sites that launch them (train_gemm.h declares the sites;
// the entry points of train.hip call them with their `arith`).
//
// arith 0, fp32: ONE tiled kernel on v_mfma_f32_16x16x4_f32 (gemm16_kernel): 64 x 64 output tile per 256-thread work-group
// (4 waves, each 2 x 2 blocks of 16 x 16), k-steps of 16 staged in LDS element by element.  Operands are read through the small
// loader functors of train_gemm.h, so the same kernel runs the transposed convolutions (B = the output gradient read at the tap
// offsets of the zero-bordered plane layout), the forward convolution in front of a batch-statistics BatchNorm (the same launch
// with the raw filters and the bias added in the store), the weight gradients (an implicit GEMM over K = NB * PLANE positions,
// split-K, partial sums added in a fixed order) and the two correlation GEMMs (d F^ = Q^T d corr, d Q^ = d corr F^T).
// arith 1, split-fp16 ("f16x3") on v_mfma_f32_32x32x16_f16 (gemm_f16x3_kernel), same loaders, same stores:
//
// Arithmetic.  Every fp32 operand value x is multiplied by its operand's power-of-two scale 2^e, split into fp16 hi = rn16(x 2^e)
// and lo = rn16(x 2^e - hi) where it is staged into LDS, and a product of two fragments is lo*hi + hi*lo + hi*hi accumulated in
// fp32 (the lo*lo term, 2^-22 of the product, is dropped); the epilogue multiplies by 2^-ea 2^-eb.  Nothing but the scale is a
// rounding the fp32 route does not have: the split carries 22 bits of every value.
//
// Scales.  A maxima pass per operand (absmax_kernel) writes the largest |x| as its fp32 bit pattern with atomicMax - non-negative
// floats order as unsigned integers - into words the launcher has cleared; the GEMM reads the word and takes e = 141 - the
// biased exponent: the largest magnitude lands in [2^14, 2^15), one binade below the end of the fp16 range.  An operand a GEMM
// reduces over as a whole has one word; a batched operand one per slice of the GEMM's batch index (dy per pair, dcorr per image /
// per class), because a slice 2^-20 smaller than its neighbour would otherwise lose 20 of the 22 bits.  A zero maximum: e = 0
// (the products are exact zeros).  A non-finite maximum (word >= 0x7f800000): e = 0, and the NaN / Inf runs through the
// conversion (hi = Inf gives lo = NaN) and the MFMA into every output that depends on it.
//
// Shape.  256 threads = 4 waves as 2 x 2; a wave owns (32 MI) x 64 outputs = MI x 2 accumulator tiles of 32 x 32, so the
// work-group tile is 128 x 128 (MI = 2) or 64 x 128 (MI = 1: problems of up to 64 rows, and both correlation GEMMs, whose few
// batch slices leave the 128-row tile with fewer work-groups than the device has CUs).  K-steps of 32: two MFMA k-blocks of 16.
// LDS holds hi and lo of both operands k-contiguous, rows of 32 + 8 halves (80 bytes: the 16-byte fragment reads and the 16-byte
// staging writes of 16 consecutive rows fall into distinct banks).  Staging: a thread owns whole runs of 8 consecutive k of one
// row (train_gemm.h: load8 decomposes the index once per run); for an operand whose memory runs along its row index (the
// plane-shifted dy of the data gradient, the rows of dcorr) the lanes of a wave walk the rows and the run's k is the same for
// the whole wave - its (channel, tap) decomposition is scalar work; for one whose memory runs along k, 4 neighbouring lanes
// cover the 32 k of a row.  The global loads of step i+1 are issued into registers before the products of step i and converted
// after them (one LDS buffer, two barriers per step): their latency hides under the MFMAs, the conversion does not.
#include "train_gemm.h"
#include "../csrc/tile_common.h"

using namespace os2d_train_gemm;

namespace {

// ------------------------------------------------------------------------------------------------ fp32-MFMA GEMM
constexpr int GT = 64;   // output tile (M and N)
constexpr int GK = GEMM16_KSTEP;   // k-step staged in LDS

// C(z)[m][n] = sum_{k in [kb, ke)} A(z, m, k) * B(z, k, n).  ksplit > 0: z is a split-K slice, [kb, ke) = [z*ksplit, ...);
// ksplit == 0: z is a batch index and the whole K is reduced.  B_KFAST: B's fastest-varying address is k (else n).
template <class LA, class LB, class ST, bool B_KFAST>
__global__ __launch_bounds__(256) void gemm16_kernel(LA la, LB lb, ST st, int M, int N, int K, int ksplit) {
  __shared__ float As[GK][GT + 4];
  __shared__ float Bs[GK][GT + 4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wm = wv >> 1, wn = wv & 1;
  const int m0 = blockIdx.y * GT, n0 = blockIdx.x * GT, z = blockIdx.z;
  const int kb = ksplit > 0 ? z * ksplit : 0;
  const int ke = ksplit > 0 ? min(K, kb + ksplit) : K;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = kb; k0 < ke; k0 += GK) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int e = tid + r * 256;
      const int kk = e & (GK - 1), mm = e >> 4;
      const int m = m0 + mm, k = k0 + kk;
      As[kk][mm] = (m < M && k < ke) ? la(z, m, k) : 0.f;
      int bk, bn;
      if (B_KFAST) {
        bk = e & (GK - 1);
        bn = e >> 4;
      } else {
        bn = e & (GT - 1);
        bk = e >> 6;
      }
      const int n = n0 + bn, k2 = k0 + bk;
      Bs[bk][bn] = (n < N && k2 < ke) ? lb(z, k2, n) : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < GK / 4; ++s) {
      const int kr = s * 4 + (lane >> 4);
      const float a0 = As[kr][wm * 32 + (lane & 15)], a1 = As[kr][wm * 32 + 16 + (lane & 15)];
      const float b0 = Bs[kr][wn * 32 + (lane & 15)], b1 = Bs[kr][wn * 32 + 16 + (lane & 15)];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm * 32 + i * 16 + (lane >> 4) * 4 + r;   // C/D map of the 16x16 MFMA: row (lane>>4)*4+r, col lane&15
        const int n = n0 + wn * 32 + j * 16 + (lane & 15);
        if (m < M && n < N) st(z, m, n, acc[i][j][r]);
      }
}

template <bool B_KFAST, class LA, class LB, class ST>
int gemm(LA la, LB lb, ST st, int M, int N, int K, int Z, int ksplit, hipStream_t stream, const char* what) {
  const dim3 grid((N + GT - 1) / GT, (M + GT - 1) / GT, Z);
  hipLaunchKernelGGL((gemm16_kernel<LA, LB, ST, B_KFAST>), grid, dim3(256), 0, stream, la, lb, st, M, N, K, ksplit);
  return os2d_launched(what);
}
// ------------------------------------------------------------------------------------------------ split-fp16 GEMM
constexpr int FK = F16X3_KSTEP;    // k-step
constexpr int FROW = FK + 8;            // halves per LDS row
constexpr int FTN = 128;                // columns per work-group

// where an operand's maximum is: word (z / div) % mod
struct ScaleWord {
  const unsigned* w;
  int div, mod;
};
__device__ __forceinline__ int scale_exp(ScaleWord s, int z) {
  const unsigned bits = s.w[(z / s.div) % s.mod];
  if (bits == 0u || bits >= 0x7f800000u) return 0;
  return min(141 - (int)(bits >> 23), 126);      // a subnormal maximum: the largest scale a float holds
}
__device__ __forceinline__ float pow2i(int e) { return __uint_as_float((unsigned)(127 + e) << 23); }   // e in [-126, 127]

// 8 scaled values -> hi and lo halves, packed in k order
__device__ __forceinline__ void split8(const float (&v)[8], float s, u32x4& hi, u32x4& lo) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float x0 = v[2 * p] * s, x1 = v[2 * p + 1] * s;
    typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
    const half2_t h = {(_Float16)x0, (_Float16)x1};
    const unsigned hb = __builtin_bit_cast(unsigned, h);
    hi[p] = hb;
    lo[p] = os2d_split_lo_pair(x0, x1, hb);
  }
}

template <int MI, class LA, class LB, class ST, bool B_KFAST>
__global__ __launch_bounds__(256) void gemm_f16x3_kernel(LA la, LB lb, ST st, ScaleWord sa, ScaleWord sb, int M, int N, int K, int ksplit) {
  constexpr int TM = 64 * MI;
  __shared__ __attribute__((aligned(16))) _Float16 As[2][TM][FROW];      // [hi | lo][row][k]
  __shared__ __attribute__((aligned(16))) _Float16 Bs[2][FTN][FROW];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wv >> 1, wn = wv & 1;
  const int m0 = blockIdx.y * TM, n0 = blockIdx.x * FTN, z = blockIdx.z;
  const int kb = ksplit > 0 ? z * ksplit : 0;
  const int ke = ksplit > 0 ? min(K, kb + ksplit) : K;
  const int ea = scale_exp(sa, z), eb = scale_exp(sb, z);
  const float fa = pow2i(ea), fb = pow2i(eb);
  // staging runs of this thread: A (memory along k): 4 lanes per row; B: the same, or lanes along the rows with a wave-uniform k
  const int a_kg = tid & 3, a_row = tid >> 2;                    // + 64 i, i < MI
  const int b_kg = B_KFAST ? (tid & 3) : (wv >> 1);              // + 2 i for the row-walking form
  const int b_row = B_KFAST ? (tid >> 2) : (wv & 1) * 64 + lane; // + 64 i for the k-walking form
  float ra[MI][8], rb[2][8];
  f32x16 acc[MI][2];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  auto fetch = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int m = m0 + a_row + 64 * i;
      if (m < M) {
        la.load8(z, m, k0 + a_kg * 8, ke, ra[i]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) ra[i][j] = 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int n = n0 + b_row + (B_KFAST ? 64 * i : 0);
      const int k = k0 + (b_kg + (B_KFAST ? 0 : 2 * i)) * 8;
      if (n < N) {
        lb.load8(z, n, k, ke, rb[i]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) rb[i][j] = 0.f;
      }
    }
  };

  fetch(kb);
  for (int k0 = kb; k0 < ke; k0 += FK) {
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      u32x4 hi, lo;
      split8(ra[i], fa, hi, lo);
      *reinterpret_cast<u32x4*>(&As[0][a_row + 64 * i][a_kg * 8]) = hi;
      *reinterpret_cast<u32x4*>(&As[1][a_row + 64 * i][a_kg * 8]) = lo;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      u32x4 hi, lo;
      split8(rb[i], fb, hi, lo);
      const int row = b_row + (B_KFAST ? 64 * i : 0), kg = b_kg + (B_KFAST ? 0 : 2 * i);
      *reinterpret_cast<u32x4*>(&Bs[0][row][kg * 8]) = hi;
      *reinterpret_cast<u32x4*>(&Bs[1][row][kg * 8]) = lo;
    }
    __syncthreads();
    if (k0 + FK < ke) fetch(k0 + FK);       // in flight under the products below
#pragma unroll
    for (int s = 0; s < FK / 16; ++s) {
      const int kk = (s * 2 + (lane >> 5)) * 8;       // operand lane map of the 32x32x16 MFMA: row lane & 31, k = 8 (lane >> 5) + j
      half8 ah[MI], al[MI], bh[2], bl[2];
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        const int row = wm * 32 * MI + i * 32 + (lane & 31);
        ah[i] = *reinterpret_cast<const half8*>(&As[0][row][kk]);
        al[i] = *reinterpret_cast<const half8*>(&As[1][row][kk]);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int row = wn * 64 + j * 32 + (lane & 31);
        bh[j] = *reinterpret_cast<const half8*>(&Bs[0][row][kk]);
        bl[j] = *reinterpret_cast<const half8*>(&Bs[1][row][kk]);
      }
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[i], bh[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bl[j], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();
  }
  const float ia = pow2i(-ea), ib = pow2i(-eb);     // two factors: 2^-(ea+eb) alone may be below the smallest float
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        // C/D map of the 32x32 MFMA: column lane & 31, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
        const int m = m0 + wm * 32 * MI + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int n = n0 + wn * 64 + j * 32 + (lane & 31);
        if (m < M && n < N) st(z, m, n, acc[i][j][r] * ia * ib);
      }
}

// ROWS128: the 128-row tile for problems of more than 64 rows (else the 64-row tile whatever M)
template <bool B_KFAST, bool ROWS128, class LA, class LB, class ST>
int gemm_f16x3(LA la, LB lb, ST st, ScaleWord sa, ScaleWord sb, int M, int N, int K, int Z, int ksplit, hipStream_t stream, const char* what) {
  if constexpr (ROWS128) {
    if (M > 64) {
      const dim3 grid((N + FTN - 1) / FTN, (M + 127) / 128, Z);
      hipLaunchKernelGGL((gemm_f16x3_kernel<2, LA, LB, ST, B_KFAST>), grid, dim3(256), 0, stream, la, lb, st, sa, sb, M, N, K, ksplit);
      return os2d_launched(what);
    }
  }
  {
    const dim3 grid((N + FTN - 1) / FTN, (M + 63) / 64, Z);
    hipLaunchKernelGGL((gemm_f16x3_kernel<1, LA, LB, ST, B_KFAST>), grid, dim3(256), 0, stream, la, lb, st, sa, sb, M, N, K, ksplit);
  }
  return os2d_launched(what);
}

// ------------------------------------------------------------------------------------------------ maxima
struct MaxWord {
  unsigned* w;      // NULL: none
  int div, mod;
};
// element i of slice s of a strided tensor
struct SrcPlain {
  const float* p;
  size_t stride;
  __device__ __forceinline__ float operator()(size_t s, size_t i) const { return p[s * stride + i]; }
};
// the normalised image map: slice = image a, i = c * HW + n
struct SrcImageNorm {
  const float* fm;
  const float* rinv;
  size_t C, HW;
  __device__ __forceinline__ float operator()(size_t a, size_t i) const { return fm[a * C * HW + i] * rinv[a * HW + i % HW]; }
};
constexpr int MAX_CHUNK = 16384;     // elements per work-group: 64 per thread
__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }
// largest |x| of slice blockIdx.x, as the bits of a non-negative float (a NaN's are above every number's): work-group blockIdx.y
// reduces its chunk and makes ONE atomicMax per word - atomics to one address are served one after the other
__device__ __forceinline__ void absmax_finish(unsigned m, size_t slice, MaxWord w0, MaxWord w1) {
  __shared__ unsigned red[4];
  for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = max(max(red[0], red[1]), max(red[2], red[3]));
    if (m != 0u) {
      atomicMax(w0.w + (slice / w0.div) % w0.mod, m);
      if (w1.w) atomicMax(w1.w + (slice / w1.div) % w1.mod, m);
    }
  }
}
template <class SRC>
__global__ __launch_bounds__(256) void absmax_kernel(SRC src, size_t n, MaxWord w0, MaxWord w1) {
  const size_t slice = blockIdx.x;
  unsigned m = 0u;
  for (size_t i0 = (size_t)blockIdx.y * MAX_CHUNK; i0 < n; i0 += (size_t)gridDim.y * MAX_CHUNK) {
    const size_t i1 = i0 + MAX_CHUNK < n ? i0 + MAX_CHUNK : n;
#pragma unroll 4
    for (size_t i = i0 + threadIdx.x; i < i1; i += 256) m = max(m, abs_bits(src(slice, i)));
  }
  absmax_finish(m, slice, w0, w1);
}
// the same for a tensor whose slices are 16-byte aligned and a multiple of 4 floats long
__global__ __launch_bounds__(256) void absmax_vec_kernel(const float* __restrict__ p, size_t stride, size_t n, MaxWord w0, MaxWord w1) {
  const size_t slice = blockIdx.x, n4 = n / 4;
  const f32x4* q = reinterpret_cast<const f32x4*>(p + slice * stride);
  unsigned m = 0u;
  for (size_t i0 = (size_t)blockIdx.y * (MAX_CHUNK / 4); i0 < n4; i0 += (size_t)gridDim.y * (MAX_CHUNK / 4)) {
    const size_t i1 = i0 + MAX_CHUNK / 4 < n4 ? i0 + MAX_CHUNK / 4 : n4;
#pragma unroll 4
    for (size_t i = i0 + threadIdx.x; i < i1; i += 256) {
      const f32x4 v = q[i];
      m = max(max(m, max(abs_bits(v[0]), abs_bits(v[1]))), max(abs_bits(v[2]), abs_bits(v[3])));
    }
  }
  absmax_finish(m, slice, w0, w1);
}
dim3 absmax_grid(size_t slices, size_t n) {
  const size_t chunks = (n + MAX_CHUNK - 1) / MAX_CHUNK;       // beyond 4096 of them a work-group walks several
  return dim3((unsigned)slices, (unsigned)(chunks < 1 ? 1 : chunks > 4096 ? 4096 : chunks));
}
template <class SRC>
int absmax(SRC src, size_t slices, size_t n, MaxWord w0, MaxWord w1, hipStream_t stream) {
  hipLaunchKernelGGL((absmax_kernel<SRC>), absmax_grid(slices, n), dim3(256), 0, stream, src, n, w0, w1);
  return os2d_launched("absmax_kernel");
}
int absmax(SrcPlain src, size_t slices, size_t n, MaxWord w0, MaxWord w1, hipStream_t stream) {
  if (((uintptr_t)src.p & 15) == 0 && (src.stride & 3) == 0 && (n & 3) == 0) {
    hipLaunchKernelGGL(absmax_vec_kernel, absmax_grid(slices, n), dim3(256), 0, stream, src.p, src.stride, n, w0, w1);
    return os2d_launched("absmax_vec_kernel");
  }
  return absmax<SrcPlain>(src, slices, n, w0, w1, stream);
}
int clear_words(unsigned* words, size_t n, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(words, 0, n * sizeof(unsigned), stream);
  if (e != hipSuccess) {
    os2d_set_error("hipMemsetAsync of the maxima words: %s", hipGetErrorString(e));
    return -4;
  }
  return 0;
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// ================================================================================================ the five sites
// Each builds its operand loaders, its store and its dimensions ONCE and hands them to the kernel of the arithmetic asked for.
// The `vec` hints of LdRows / LdPairRows are load8's: gemm16_kernel does not read them.

// C(z)[m][n] = sum over (c < creduce, tap) of a[m][(c, tap)] * b[z][c][n + off(tap)] (+ bias[m]) on the plane layout: the data
// gradient and the forward convolution (bplanes = planes per pair of b, of which the first creduce are read)
static int conv_planes(int arith, const float* a, const float* bias, const float* b, int bplanes, float* out, int M, int creduce, int ks,
                       int NB, int H, int W, unsigned* words, hipStream_t stream, const char* what, const char* what_f16x3) {
  const int PL = os2d_plane(H, W), T2 = ks * ks, K = creduce * T2;
  const auto la = LdRows{a, K, aligned16(a) && (K & 3) == 0};
  const auto lb = LdShifted{b, (size_t)bplanes * PL, PL, Taps{ks, ks / 2, os2d_ws(W), T2}};
  const auto st = StPlane{out, (size_t)M * PL, PL, H, W, bias};
  if (!arith) return gemm<false>(la, lb, st, M, PL, K, NB, 0, stream, what);
  int rc = clear_words(words, conv_words(arith, NB), stream);
  if (rc) return rc;
  if ((rc = absmax(SrcPlain{a, 0}, 1, (size_t)M * K, MaxWord{words, 1, 1}, MaxWord{nullptr, 1, 1}, stream))) return rc;
  if ((rc = absmax(SrcPlain{b, (size_t)bplanes * PL}, NB, (size_t)creduce * PL, MaxWord{words + 1, 1, NB}, MaxWord{nullptr, 1, 1}, stream)))
    return rc;
  return gemm_f16x3<false, true>(la, lb, st, ScaleWord{words, 1, 1}, ScaleWord{words + 1, 1, NB}, M, PL, K, NB, 0, stream, what_f16x3);
}

int os2d_gemm_conv_data(int arith, const float* wt, const float* dy, float* dx, int cout, int cin, int ks, int NB, int H, int W,
                        unsigned* words, hipStream_t stream) {
  return conv_planes(arith, wt, nullptr, dy, cout, dx, cin, cout, ks, NB, H, W, words, stream, "conv data gradient",
                     "conv data gradient (f16x3)");
}

int os2d_gemm_conv_forward(int arith, const float* w, const float* bias, const float* x, int xplanes, float* z, int cout, int cin, int ks,
                           int NB, int H, int W, unsigned* words, hipStream_t stream) {
  return conv_planes(arith, w, bias, x, xplanes, z, cout, cin, ks, NB, H, W, words, stream, "conv forward", "conv forward (f16x3)");
}

int os2d_gemm_conv_weight(int arith, const float* x, int xplanes, const float* dy, float* part, int cout, int cin, int ks, int NB, int H,
                          int W, int splits, int ksplit, unsigned* words, hipStream_t stream) {
  const int PL = os2d_plane(H, W), T2 = ks * ks, N = cin * T2;
  const auto la = LdPairRows{dy, (size_t)cout * PL, PL, aligned16(dy)};
  const auto lb = LdPairShifted{x, (size_t)xplanes * PL, PL, Taps{ks, ks / 2, os2d_ws(W), T2}};
  const auto st = StSlice{part, cout, N};
  if (!arith) return gemm<true>(la, lb, st, cout, N, NB * PL, splits, ksplit, stream, "conv weight gradient");
  int rc = clear_words(words, WEIGHT_WORDS, stream);
  if (rc) return rc;
  // both operands are reduced over every pair: one word each (x: the cin planes the layer reads of the xplanes a pair has)
  if ((rc = absmax(SrcPlain{dy, (size_t)cout * PL}, NB, (size_t)cout * PL, MaxWord{words, 1, 1}, MaxWord{nullptr, 1, 1}, stream))) return rc;
  if ((rc = absmax(SrcPlain{x, (size_t)xplanes * PL}, NB, (size_t)cin * PL, MaxWord{words + 1, 1, 1}, MaxWord{nullptr, 1, 1}, stream))) return rc;
  return gemm_f16x3<true, true>(la, lb, st, ScaleWord{words, 1, 1}, ScaleWord{words + 1, 1, 1}, cout, N, NB * PL, splits, ksplit, stream,
                                "conv weight gradient (f16x3)");
}

// the words of the correlation backward: qp, the normalised image map, dcorr per image, dcorr per class
struct CorrWords {
  unsigned *qp, *fm, *img, *cls;
};
static CorrWords split_corr_words(unsigned* words, int A) { return {words, words + 1, words + 2, words + 2 + A}; }

int os2d_gemm_corr_maxima(const float* dcorr, int A, int B, int HW, unsigned* words, hipStream_t stream) {
  const CorrWords w = split_corr_words(words, A);
  const int rc = clear_words(words, corr_words(1, A, B), stream);
  if (rc) return rc;
  // one maximum per pair of dcorr, combined per image (pair / B) and per class (pair % B) by the atomics themselves
  return absmax(SrcPlain{dcorr, (size_t)OS2D_K * HW}, (size_t)A * B, (size_t)OS2D_K * HW, MaxWord{w.img, B, A}, MaxWord{w.cls, 1, B}, stream);
}

int os2d_gemm_corr_image(int arith, const float* qp, const float* dcorr, int A, int B, int C, int HW, float* dfh, unsigned* words,
                         hipStream_t stream) {
  const auto la = LdClassT{qp, C};
  const auto lb = LdCorrRows{dcorr, B, HW};
  const auto st = StDense{dfh, C, HW};
  if (!arith) return gemm<false>(la, lb, st, C, HW, B * OS2D_K, A, 0, stream, "correlation backward (image)");
  const CorrWords w = split_corr_words(words, A);
  // rows 225 .. 255 of a class operand row are zeros: reading them moves no maximum
  const int rc = absmax(SrcPlain{qp, (size_t)C * OS2D_QROWS}, B, (size_t)C * OS2D_QROWS, MaxWord{w.qp, 1, 1}, MaxWord{nullptr, 1, 1}, stream);
  if (rc) return rc;
  return gemm_f16x3<false, false>(la, lb, st, ScaleWord{w.qp, 1, 1}, ScaleWord{w.img, 1, A}, C, HW, B * OS2D_K, A, 0, stream,
                                  "correlation backward (image, f16x3)");
}

int os2d_gemm_corr_class(int arith, const float* fm, const float* rinv, const float* dcorr, int A, int B, int C, int HW, float* dq,
                         unsigned* words, hipStream_t stream) {
  const auto la = LdImageNorm{fm, rinv, C, HW};
  const auto lb = LdCorrCols{dcorr, B, HW};
  const auto st = StDense{dq, C, OS2D_K};
  if (!arith) return gemm<true>(la, lb, st, C, OS2D_K, A * HW, B, 0, stream, "correlation backward (class)");
  const CorrWords w = split_corr_words(words, A);
  const int rc = absmax(SrcImageNorm{fm, rinv, (size_t)C, (size_t)HW}, A, (size_t)C * HW, MaxWord{w.fm, 1, 1}, MaxWord{nullptr, 1, 1}, stream);
  if (rc) return rc;
  return gemm_f16x3<true, false>(la, lb, st, ScaleWord{w.fm, 1, 1}, ScaleWord{w.cls, 1, B}, C, OS2D_K, A * HW, B, 0, stream,
                                 "correlation backward (class, f16x3)");
}
