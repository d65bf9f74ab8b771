// libos2d_train.so (include/os2d_train.h): the backward pass of the OS2D head on gfx950, fp32 throughout (the *_ex entry points
// take the GEMMs to the split-fp16 kernel of gemm_f16x3.hip at arith = 1).
//
// Matrix-shaped work goes through ONE tiled GEMM kernel on v_mfma_f32_16x16x4_f32 (gemm16_kernel): 64 x 64 output tile per
// 256-thread work-group (4 waves, each 2 x 2 blocks of 16 x 16), k-steps of 16 staged in LDS.  Operands are read through small
// loader functors, so the same kernel runs
//   * the transposed convolutions (B = the output gradient read at the tap offsets of the zero-bordered plane layout),
//   * the weight gradients (an implicit GEMM over K = NB * PLANE positions, split-K, partial sums added in a fixed order),
//   * the two correlation GEMMs (d F^ = Q^T d corr per image, d Q^ = d corr F^T per class).
//   * the forward convolution of a layer whose BatchNorm takes batch statistics (os2d_train_conv_forward: the data gradient's
//     launch with the raw filters as the A operand and the bias added in the store; bn_live.hip has the BatchNorm itself).
// The rest is per-location work: resample / pool / box decode backward, BatchNorm + ReLU masks, the two L2 normalisations
// and the bilinear class-map resize.
#include <stdio.h>

#include "../../include/os2d_train.h"
#include "../csrc/os2d_common.h"
#include "../csrc/sample_decode.h"
#include "train_gemm.h"     // the operand loaders and result stores of the GEMMs; the launchers of gemm_f16x3.hip
#include "decode_det.h"     // the fixed-point grid of the order-independent d corr scatter

using namespace os2d_train_gemm;

namespace {

struct Layer {
  int cout, cin, ks;
};
bool layer_shape(int layer, int P, Layer* s) {
  switch (layer) {
    case 1: *s = {128, OS2D_K, 7}; return true;
    case 2: *s = {64, 128, 5}; return true;
    case 3:
      if (P != 6 && P != 4) return false;
      *s = {P, 64, 5};
      return true;
    default: return false;
  }
}
// channel count of the forward buffer that feeds a layer: rnorm keeps 226 planes per pair (OS2D_KP)
int input_planes(int layer) { return layer == 1 ? OS2D_KP : layer == 2 ? 128 : 64; }

bool shape_ok(int NB, int H, int W) { return NB >= 1 && H >= 1 && W >= 1 && W <= OS2D_MAX_W_DIRECT7 && H <= OS2D_MAX_H; }

// ------------------------------------------------------------------------------------------------ fp32-MFMA GEMM
constexpr int GT = 64;   // output tile (M and N)
constexpr int GK = 16;   // k-step staged in LDS

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

// ------------------------------------------------------------------------------------------------ small kernels
// Wt[c][o*T2 + t] = w[o][c][T2-1-t]: the filters of the transposed convolution
__global__ __launch_bounds__(256) void flip_weights_kernel(const float* __restrict__ w, int cout, int cin, int t2, float* __restrict__ wt) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t total = (size_t)cout * cin * t2;
  if (i >= total) return;
  const int t = (int)(i % t2);
  const size_t oc = i / t2;
  const int c = (int)(oc % cin), o = (int)(oc / cin);
  wt[((size_t)c * cout + o) * t2 + t] = w[i - t + (t2 - 1 - t)];
}

// out[i] = sum_s part[s][i], s in order: the split-K partial sums of a weight gradient
__global__ __launch_bounds__(256) void split_sum_kernel(const float* __restrict__ part, int splits, size_t n, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int k = 0; k < splits; ++k) s += part[(size_t)k * n + i];
  out[i] = s;
}

__device__ __forceinline__ float block_sum(float v, float* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- the order-independent d corr scatter (decode_det.h): where a pair's sums go and on which grid
struct DetSink {
  unsigned long long* acc;    // [NB,225,HW] fixed-point sums (two's complement: the wrap-around of unsigned addition is signed addition)
  const unsigned* words;      // [NB] the largest |dcls + dcls_det| of each pair, fp32 bits
  int L;                      // os2d_det_log2_addends(H, W)
};
__device__ __forceinline__ double det_pow2(int e) { return __longlong_as_double((long long)(1023 + e) << 52); }   // e in [-1022, 1023]
// one addend onto the grid: the product is exact, the rounding to the nearest integer is the route's only one
__device__ __forceinline__ void det_add(unsigned long long* cell, float a, double scale) {
  const long long q = __double2ll_rn((double)a * scale);
  if (q != 0) atomicAdd(cell, (unsigned long long)q);
}

// ---- (a) resample + pool + box decode backward: one thread per (pair, location).  DET = false adds the d corr taps into
// dcorr with fp32 atomics (os2d_train_decode_backward); DET = true rounds the same fp32 addends onto the pair's fixed-point
// grid and adds them into `sink` with 64-bit integer atomics (os2d_train_decode_backward_det: dcorr is not touched here).
// Everything else - theta, the coordinates, the clamps, dparams - is the same code on both routes.
template <bool DET>
__global__ __launch_bounds__(256) void decode_backward_kernel(const float* __restrict__ corr, const float* __restrict__ params,
                                                              const float* __restrict__ dcls, const float* __restrict__ dcls_det,
                                                              const float* __restrict__ dloc, int H, int W, int P, int inverse,
                                                              float stride, float half_box, float* __restrict__ dcorr,
                                                              float* __restrict__ dparams, DetSink sink) {
  const int HW = H * W;
  const int nb = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
  if (n >= HW) return;
  const int h = n / W, w = n - h * W;
  const float* pp = params + (size_t)nb * P * HW + n;
  float t00, t01, t02, t10, t11, t12;
  os2d_theta(pp, HW, P, inverse, t00, t01, t02, t10, t11, t12);     // the forward's own theta
  const size_t o = (size_t)nb * HW + n;
  const float gcls = dcls ? dcls[o] : 0.f;
  const float gsum = gcls + (dcls_det ? dcls_det[o] : 0.f);
  constexpr int NTAP = POOL_HI - POOL_LO;
  const float inv_pool = 1.0f / (NTAP * NTAP);
  const float wsc = gsum * inv_pool, wth = gcls * inv_pool;
  const float half_t = 0.5f * OS2D_T;
  const float cx = (float)w + 0.5f, cy = (float)h + 0.5f;
  const float wmax = (float)(W - 1), hmax = (float)(H - 1);
  const float* cbase = corr + (size_t)nb * OS2D_K * HW;
  float* dbase = DET ? nullptr : dcorr + (size_t)nb * OS2D_K * HW;
  unsigned long long* abase = nullptr;
  double scale = 0.0;
  bool scatter = true;
  if (DET) {                  // a zero maximum has nothing to add; a non-finite one is the convert pass's to report
    const int e = os2d_det_exponent(sink.words[nb], sink.L);
    scatter = e != OS2D_TRAIN_DET_ZERO && e != OS2D_TRAIN_DET_NONFINITE;
    scale = det_pow2(scatter ? e : 0);
    abase = sink.acc + (size_t)nb * OS2D_K * HW;
  }
  float d00 = 0.f, d01 = 0.f, d02 = 0.f, d10 = 0.f, d11 = 0.f, d12 = 0.f;
  if (wsc != 0.f || wth != 0.f) {
    for (int j = POOL_LO; j < POOL_HI; ++j) {
      const float xj = os2d_template_coord(j);
      for (int i = POOL_LO; i < POOL_HI; ++i) {
        const float yi = os2d_template_coord(i);
        const float gx = t00 * xj + t01 * yi + t02;
        const float gy = t10 * xj + t11 * yi + t12;
        const float Xr = gx * half_t + cx, Yr = gy * half_t + cy;
        const float X = fminf(fmaxf(Xr, 0.f), wmax);
        const float Y = fminf(fmaxf(Yr, 0.f), hmax);
        const float fx0 = floorf(X), fy0 = floorf(Y);
        const float ax = X - fx0, ay = Y - fy0;
        const int x0 = (int)fx0, y0 = (int)fy0;
        const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
        const size_t ch = (size_t)(j * OS2D_T + i) * HW;
        if (wsc != 0.f) {       // d corr: the pool weight over the 4 taps of the point's own channel
          const float a00 = wsc * (1.f - ax) * (1.f - ay), a01 = wsc * ax * (1.f - ay);
          const float a10 = wsc * (1.f - ax) * ay, a11 = wsc * ax * ay;
          if (DET) {
            if (scatter) {
              unsigned long long* d = abase + ch;
              det_add(d + y0 * W + x0, a00, scale);
              det_add(d + y0 * W + x1, a01, scale);
              det_add(d + y1 * W + x0, a10, scale);
              det_add(d + y1 * W + x1, a11, scale);
            }
          } else {
            float* d = dbase + ch;
            unsafeAtomicAdd(d + y0 * W + x0, a00);
            unsafeAtomicAdd(d + y0 * W + x1, a01);
            unsafeAtomicAdd(d + y1 * W + x0, a10);
            unsafeAtomicAdd(d + y1 * W + x1, a11);
          }
        }
        if (wth != 0.f) {       // d grid: derivative of the bilinear weights, zero where the coordinate was clamped
          const float* c = cbase + ch;
          const float v00 = c[y0 * W + x0], v01 = c[y0 * W + x1], v10 = c[y1 * W + x0], v11 = c[y1 * W + x1];
          const float dX = (Xr >= 0.f && Xr <= wmax) ? (1.f - ay) * (v01 - v00) + ay * (v11 - v10) : 0.f;
          const float dY = (Yr >= 0.f && Yr <= hmax) ? (1.f - ax) * (v10 - v00) + ax * (v11 - v01) : 0.f;
          const float dgx = dX * half_t * wth, dgy = dY * half_t * wth;
          d00 += dgx * xj;
          d01 += dgx * yi;
          d02 += dgx;
          d10 += dgy * xj;
          d11 += dgy * yi;
          d12 += dgy;
        }
      }
    }
  }
  if (dloc) {   // loc = encode(clip(min / max over the corners of the transformed template), anchor)
    const float l0 = dloc[((size_t)nb * 4 + 0) * HW + n], l1 = dloc[((size_t)nb * 4 + 1) * HW + n];
    const float l2 = dloc[((size_t)nb * 4 + 2) * HW + n], l3 = dloc[((size_t)nb * 4 + 3) * HW + n];
    const float ecx = stride * cx, ecy = stride * cy;
    float U[4], V[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float yi = (k & 2) ? 1.0f : -1.0f;
      const float xj = (k & 1) ? 1.0f : -1.0f;
      U[k] = (t00 * xj + t01 * yi + t02) * half_box + ecx;
      V[k] = (t10 * xj + t11 * yi + t12) * half_box + ecy;
    }
    // arg-min / arg-max: first occurrence in the reference's row-major point order (corners 0, 14, 210, 224 = k 0..3)
    int ux1 = 0, ux2 = 0, vy1 = 0, vy2 = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      if (U[k] < U[ux1]) ux1 = k;
      if (U[k] > U[ux2]) ux2 = k;
      if (V[k] < V[vy1]) vy1 = k;
      if (V[k] > V[vy2]) vy2 = k;
    }
    const float ax1 = ecx - half_box, ay1 = ecy - half_box;
    const float aw = (ecx + half_box) - ax1, ah = (ecy + half_box) - ay1;
    float dU[4] = {0.f, 0.f, 0.f, 0.f}, dV[4] = {0.f, 0.f, 0.f, 0.f};
    {
      float x1 = U[ux1], x2 = U[ux2];
      const bool clip = x1 + 1.0f > x2;
      if (clip) x2 = x1 + 1.0f;
      const float dg = 10.0f * l0 / aw, dw_ = 5.0f * l2 / (x2 - x1);
      float g1 = 0.5f * dg - dw_, g2 = 0.5f * dg + dw_;
      if (clip) {
        g1 += g2;
        g2 = 0.f;
      }
      dU[ux1] += g1;
      dU[ux2] += g2;
    }
    {
      float y1 = V[vy1], y2 = V[vy2];
      const bool clip = y1 + 1.0f > y2;
      if (clip) y2 = y1 + 1.0f;
      const float dg = 10.0f * l1 / ah, dh_ = 5.0f * l3 / (y2 - y1);
      float g1 = 0.5f * dg - dh_, g2 = 0.5f * dg + dh_;
      if (clip) {
        g1 += g2;
        g2 = 0.f;
      }
      dV[vy1] += g1;
      dV[vy2] += g2;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float yi = (k & 2) ? 1.0f : -1.0f;
      const float xj = (k & 1) ? 1.0f : -1.0f;
      const float gx = dU[k] * half_box, gy = dV[k] * half_box;
      d00 += gx * xj;
      d01 += gx * yi;
      d02 += gx;
      d10 += gy * xj;
      d11 += gy * yi;
      d12 += gy;
    }
  }
  double g[6] = {d00, d01, d02, d10, d11, d12};
  if (inverse) {   // theta = top rows of M^-1 (M = [[p],[0 0 1]], regularised as the forward did): dM = -N^T G N^T in fp64
    double a, b, c, d, tx, ty;
    if (P == 6) {
      a = pp[0]; b = pp[HW]; tx = pp[2 * (size_t)HW]; c = pp[3 * (size_t)HW]; d = pp[4 * (size_t)HW]; ty = pp[5 * (size_t)HW];
    } else {
      a = pp[0]; b = 0.0; tx = pp[HW]; c = 0.0; d = pp[2 * (size_t)HW]; ty = pp[3 * (size_t)HW];
    }
    double hom = 1.0;
    double det = a * d - b * c;
    if (det == 0.0) {
      a = (double)((float)a + 1e-5f);
      d = (double)((float)d + 1e-5f);
      hom = (double)(1.0f + 1e-5f);
      det = a * d - b * c;
    }
    const double r = 1.0 / det;
    const double i00 = d * r, i01 = -b * r, i10 = -c * r, i11 = a * r;
    const double N[3][3] = {{i00, i01, -(i00 * tx + i01 * ty) / hom}, {i10, i11, -(i10 * tx + i11 * ty) / hom}, {0.0, 0.0, 1.0 / hom}};
    const double G[3][3] = {{g[0], g[1], g[2]}, {g[3], g[4], g[5]}, {0.0, 0.0, 0.0}};
    double X[3][3];   // X = G N^T
    for (int u = 0; u < 3; ++u)
      for (int v = 0; v < 3; ++v) X[u][v] = G[u][0] * N[v][0] + G[u][1] * N[v][1] + G[u][2] * N[v][2];
    for (int u = 0; u < 2; ++u)     // dM[u][v] = -sum_s N[s][u] X[s][v]
      for (int v = 0; v < 3; ++v) g[u * 3 + v] = -(N[0][u] * X[0][v] + N[1][u] * X[1][v] + N[2][u] * X[2][v]);
  }
  float* dp = dparams + (size_t)nb * P * HW + n;
  if (P == 6) {
#pragma unroll
    for (int k = 0; k < 6; ++k) dp[(size_t)k * HW] = (float)g[k];
  } else {
    dp[0] = (float)g[0];
    dp[HW] = (float)g[2];
    dp[2 * (size_t)HW] = (float)g[4];
    dp[3 * (size_t)HW] = (float)g[5];
  }
}

// ---- the maxima of the order-independent route: words[nb] = max over the pair's locations of |dcls + dcls_det| (the fp32 sum
// decode_backward_kernel forms), as the bits of a non-negative float - they order as unsigned integers, a NaN's above every
// number's.  A work-group reduces DET_MAX_CHUNK locations and makes ONE atomicMax (the maxima pass of gemm_f16x3.hip).
constexpr int DET_MAX_CHUNK = 2048;
__global__ __launch_bounds__(256) void decode_det_max_kernel(const float* __restrict__ dcls, const float* __restrict__ dcls_det, int HW,
                                                             unsigned* __restrict__ words) {
  __shared__ unsigned red[4];
  const int nb = blockIdx.y;
  const int n0 = blockIdx.x * DET_MAX_CHUNK, n1 = min(HW, n0 + DET_MAX_CHUNK);
  unsigned m = 0u;
  for (int n = n0 + threadIdx.x; n < n1; n += 256) {
    const size_t o = (size_t)nb * HW + n;
    const float gcls = dcls ? dcls[o] : 0.f;
    const float gsum = gcls + (dcls_det ? dcls_det[o] : 0.f);
    m = max(m, __float_as_uint(gsum) & 0x7fffffffu);
  }
  for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = max(max(red[0], red[1]), max(red[2], red[3]));
    if (m != 0u) atomicMax(words + nb, m);
  }
}

// ---- the convert pass: dcorr[cell] += (float)(sum * 2^-e), one thread per cell of a pair.  A zero sum leaves the cell as it
// is (so does a pair whose maximum is zero); a pair with a non-finite maximum gets NaN in every cell.
__global__ __launch_bounds__(256) void decode_det_convert_kernel(DetSink sink, size_t cells, float* __restrict__ dcorr) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int nb = blockIdx.y;
  if (i >= cells) return;
  const int e = os2d_det_exponent(sink.words[nb], sink.L);
  if (e == OS2D_TRAIN_DET_ZERO) return;
  float* d = dcorr + (size_t)nb * cells + i;
  if (e == OS2D_TRAIN_DET_NONFINITE) {
    *d = __uint_as_float(0x7fc00000u);
    return;
  }
  const long long q = (long long)sink.acc[(size_t)nb * cells + i];
  if (q != 0) *d += (float)((double)q * det_pow2(-e));
}

// dparams [NB,P,HW] -> plane layout (zero pads)
__global__ __launch_bounds__(256) void compact_to_plane_kernel(const float* __restrict__ src, int C, int H, int W, int PL,
                                                               float* __restrict__ dst) {
  const int cell = blockIdx.x * 256 + threadIdx.x;
  const size_t plane = blockIdx.y;    // nb * C + c
  if (cell >= PL) return;
  float v = 0.f;
  if (os2d_interior(cell, H, W)) {
    const int r = cell - os2d_base(W), ws = os2d_ws(W);
    const int h = r / ws, w = r - h * ws;
    v = src[plane * H * W + h * W + w];
  }
  dst[plane * PL + cell] = v;
}

// sum over pairs and positions of channel c of a compact [NB,C,HW] tensor (one work-group per channel, fixed order)
__global__ __launch_bounds__(256) void channel_sum_kernel(const float* __restrict__ src, int NB, int C, int HW, float* __restrict__ out) {
  __shared__ float red[4];
  const int c = blockIdx.x;
  float s = 0.f;
  for (int nb = 0; nb < NB; ++nb)
    for (int n = threadIdx.x; n < HW; n += 256) s += src[((size_t)nb * C + c) * HW + n];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[c] = s;
}

// frozen BatchNorm + ReLU: dy = dh * (h > 0) * scale at data cells, 0 at pads
__global__ __launch_bounds__(256) void bn_relu_mask_kernel(const float* __restrict__ dh, const float* __restrict__ hh,
                                                           const float* __restrict__ gamma, const float* __restrict__ var, float eps,
                                                           int C, int H, int W, int PL, float* __restrict__ dy) {
  const int cell = blockIdx.x * 256 + threadIdx.x;
  const size_t plane = blockIdx.y;
  if (cell >= PL) return;
  const int c = (int)(plane % C);
  const size_t i = plane * PL + cell;
  const float scale = gamma[c] / sqrtf(var[c] + eps);
  dy[i] = (os2d_interior(cell, H, W) && hh[i] > 0.f) ? dh[i] * scale : 0.f;
}

__global__ __launch_bounds__(256) void bn_relu_sums_kernel(const float* __restrict__ dh, const float* __restrict__ hh,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ var, float eps, int NB, int C, int H, int W,
                                                           int PL, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                           float* __restrict__ dbias) {
  __shared__ float red[4];
  const int c = blockIdx.x;
  const float g = gamma[c], b = beta[c];
  const float scale = g / sqrtf(var[c] + eps);
  const float inv_g = g != 0.f ? 1.0f / g : 0.f;
  float sb = 0.f, sg = 0.f;
  for (int nb = 0; nb < NB; ++nb)
    for (int cell = threadIdx.x; cell < PL; cell += 256) {
      const size_t i = ((size_t)nb * C + c) * PL + cell;
      const float hv = hh[i];
      if (hv > 0.f && os2d_interior(cell, H, W)) {
        const float dz = dh[i];
        sb += dz;
        sg += dz * (hv - b);
      }
    }
  sb = block_sum(sb, red);
  sg = block_sum(sg, red);
  if (threadIdx.x == 0) {
    if (dbeta) dbeta[c] = sb;
    if (dgamma) dgamma[c] = sg * inv_g;
    if (dbias) dbias[c] = sb * scale;
  }
}

// relu + L2 over 225 channels (eps 1e-6) backward, one thread per (pair, position); adds into dcorr
__global__ __launch_bounds__(256) void norm225_backward_kernel(const float* __restrict__ corr, const float* __restrict__ dxn, int H,
                                                               int W, int PL, float* __restrict__ dcorr) {
  const int HW = H * W;
  const int nb = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
  if (n >= HW) return;
  const int h = n / W, w = n - h * W;
  const float* c = corr + (size_t)nb * OS2D_K * HW + n;
  const float* g = dxn + (size_t)nb * OS2D_K * PL + os2d_base(W) + h * os2d_ws(W) + w;
  float ss = 0.f, dot = 0.f;
  for (int k = 0; k < OS2D_K; ++k) {
    const float x = os2d_relu(c[(size_t)k * HW]);
    ss += x * x;
    dot += x * g[(size_t)k * PL];
  }
  const float r = sqrtf(ss), s = 1.0f / (r + 1e-6f);
  const float q = r > 0.f ? s * s * dot / r : 0.f;
  float* d = dcorr + (size_t)nb * OS2D_K * HW + n;
  for (int k = 0; k < OS2D_K; ++k) {
    const float v = c[(size_t)k * HW];
    if (v > 0.f) d[(size_t)k * HW] += s * g[(size_t)k * PL] - q * v;
  }
}

// image map L2 over C (eps 1e-5): the inverse norms (the class-side GEMM's operand), then the backward
__global__ __launch_bounds__(256) void image_norm_kernel(const float* __restrict__ fm, int C, int HW, float* __restrict__ rinv) {
  const int a = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
  if (n >= HW) return;
  const float* f = fm + (size_t)a * C * HW + n;
  float ss = 0.f;
  for (int c = 0; c < C; ++c) ss += f[(size_t)c * HW] * f[(size_t)c * HW];
  rinv[(size_t)a * HW + n] = 1.0f / (sqrtf(ss) + 1e-5f);
}

// d x = s g - s^2 (g.x / r) x, s = 1 / (r + eps), r = |x|.  The two terms cancel down to eps s^2 g where x is (nearly) parallel
// to g - always when C = 1 - so the two reductions and the combination are done in fp64: one rounding of the result.
__global__ __launch_bounds__(256) void image_norm_backward_kernel(const float* __restrict__ fm, const float* __restrict__ dfh, int C,
                                                                  int HW, float* __restrict__ dfm) {
  const int a = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
  if (n >= HW) return;
  const size_t base = (size_t)a * C * HW + n;
  double ss = 0.0, dot = 0.0;
  for (int c = 0; c < C; ++c) {
    const double f = fm[base + (size_t)c * HW];
    ss += f * f;
    dot += (double)dfh[base + (size_t)c * HW] * f;
  }
  const double r = sqrt(ss), s = 1.0 / (r + (double)1e-5f);
  const double q = r > 0.0 ? s * s * dot / r : 0.0;
  for (int c = 0; c < C; ++c) dfm[base + (size_t)c * HW] = (float)(s * (double)dfh[base + (size_t)c * HW] - q * (double)fm[base + (size_t)c * HW]);
}

// class maps: L2 over C (eps 1e-5) backward per (class, cell), in fp64 as above; dq in x-major channel order, q15 / out in cell order
__global__ __launch_bounds__(256) void class_norm_backward_kernel(const float* __restrict__ q15, const float* __restrict__ dq, int C,
                                                                  float* __restrict__ dq15) {
  const int b = blockIdx.y, cell = threadIdx.x;
  if (cell >= OS2D_K) return;
  const int i = cell / OS2D_T, j = cell - i * OS2D_T;
  const int m = j * OS2D_T + i;
  const float* q = q15 + (size_t)b * C * OS2D_K;
  const float* g = dq + (size_t)b * C * OS2D_K;
  double ss = 0.0, dot = 0.0;
  for (int c = 0; c < C; ++c) {
    const double v = q[(size_t)c * OS2D_K + cell];
    ss += v * v;
    dot += v * (double)g[(size_t)c * OS2D_K + m];
  }
  const double r = sqrt(ss), s = 1.0 / (r + (double)1e-5f);
  const double qf = r > 0.0 ? s * s * dot / r : 0.0;
  for (int c = 0; c < C; ++c)
    dq15[((size_t)b * C + c) * OS2D_K + cell] = (float)(s * (double)g[(size_t)c * OS2D_K + m] - qf * (double)q[(size_t)c * OS2D_K + cell]);
}

// bilinear resize backward, one thread per (class, channel): the thread owns the whole h x w plane of its channel (written
// in a fixed order: deterministic); the sampling positions are those of class_resize_sample (prep.hip)
__global__ __launch_bounds__(256) void class_resize_backward_kernel(const float* __restrict__ dq15, int C, float* const* __restrict__ dsrcs,
                                                                    const int* __restrict__ sizes) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const int h = sizes[2 * b], w = sizes[2 * b + 1];
  float* d = dsrcs[b] + (size_t)c * h * w;
  for (int k = 0; k < h * w; ++k) d[k] = 0.f;
  const float* g = dq15 + ((size_t)b * C + c) * OS2D_K;
  const float step = 2.0f / (OS2D_T - 1);
  for (int cell = 0; cell < OS2D_K; ++cell) {
    const int i = cell / OS2D_T, j = cell - i * OS2D_T;
    const float xu = (j < OS2D_T / 2) ? __fmaf_rn(step, (float)j, -1.0f) : __fmaf_rn(-step, (float)(OS2D_T - 1 - j), 1.0f);
    const float yu = (i < OS2D_T / 2) ? __fmaf_rn(step, (float)i, -1.0f) : __fmaf_rn(-step, (float)(OS2D_T - 1 - i), 1.0f);
    const float ix = ((xu + 1.0f) * 0.5f) * (float)(w - 1);
    const float iy = ((yu + 1.0f) * 0.5f) * (float)(h - 1);
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float ax = ix - fx0, ay = iy - fy0;
    const bool x0in = x0 >= 0 && x0 < w, x1in = x0 + 1 >= 0 && x0 + 1 < w;
    const bool y0in = y0 >= 0 && y0 < h, y1in = y0 + 1 >= 0 && y0 + 1 < h;
    const float v = g[cell];
    if (x0in && y0in) d[y0 * w + x0] += v * (1.f - ax) * (1.f - ay);
    if (x1in && y0in) d[y0 * w + x0 + 1] += v * ax * (1.f - ay);
    if (x0in && y1in) d[(y0 + 1) * w + x0] += v * (1.f - ax) * ay;
    if (x1in && y1in) d[(y0 + 1) * w + x0 + 1] += v * ax * ay;
  }
}

inline unsigned blocks(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

// ================================================================================================ C ABI
extern "C" {

int os2d_train_abi_version(void) { return OS2D_TRAIN_ABI_VERSION; }
const char* os2d_train_last_error(void) { return os2d_error_text; }

int os2d_train_decode_backward(const float* corr, const float* params, const float* dcls, const float* dcls_det, const float* dloc,
                               int NB, int H, int W, int P, int inverse, int stride, int rec_field, float* dcorr, float* dparams,
                               void* stream) {
  os2d_clear_error();
  if (!corr || !params || !dcorr || !dparams) {
    os2d_set_error("os2d_train_decode_backward: null pointer");
    return -1;
  }
  if (NB < 1 || H < 1 || W < 1 || (P != 6 && P != 4) || stride < 1 || rec_field < 1) {
    os2d_set_error("os2d_train_decode_backward: bad shape NB=%d H=%d W=%d P=%d stride=%d rec_field=%d", NB, H, W, P, stride, rec_field);
    return -1;
  }
  if (NB > 65535) {
    os2d_set_error("os2d_train_decode_backward: NB=%d > 65535", NB);
    return -3;
  }
  const float half_box = 0.5f * (float)(stride * (OS2D_T - 1) + rec_field);
  hipLaunchKernelGGL(decode_backward_kernel<false>, dim3(blocks((size_t)H * W), NB), dim3(256), 0, os2d_stream(stream), corr, params, dcls,
                     dcls_det, dloc, H, W, P, inverse ? 1 : 0, (float)stride, half_box, dcorr, dparams, DetSink{nullptr, nullptr, 0});
  return os2d_launched("decode_backward_kernel");
}

int os2d_train_decode_det_exponent(unsigned max_bits, int H, int W) {
  const int L = os2d_det_log2_addends(H, W);
  return L < 0 ? OS2D_TRAIN_DET_REFUSED : os2d_det_exponent(max_bits, L);
}

// the accumulator, then the pair words
static size_t det_acc_bytes(int NB, int H, int W) { return (size_t)NB * OS2D_K * H * W * sizeof(long long); }
size_t os2d_train_decode_backward_det_workspace_bytes(int NB, int H, int W) {
  if (NB < 1 || NB > 65535 || os2d_det_log2_addends(H, W) < 0) return 0;
  return (det_acc_bytes(NB, H, W) + (size_t)NB * sizeof(unsigned) + 255) / 256 * 256;
}

int os2d_train_decode_backward_det(const float* corr, const float* params, const float* dcls, const float* dcls_det, const float* dloc,
                                   int NB, int H, int W, int P, int inverse, int stride, int rec_field, float* dcorr, float* dparams,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  os2d_clear_error();
  if (!corr || !params || !dcorr || !dparams || !workspace) {
    os2d_set_error("os2d_train_decode_backward_det: null pointer");
    return -1;
  }
  if (NB < 1 || H < 1 || W < 1 || (P != 6 && P != 4) || stride < 1 || rec_field < 1) {
    os2d_set_error("os2d_train_decode_backward_det: bad shape NB=%d H=%d W=%d P=%d stride=%d rec_field=%d", NB, H, W, P, stride, rec_field);
    return -1;
  }
  if (NB > 65535) {
    os2d_set_error("os2d_train_decode_backward_det: NB=%d > 65535", NB);
    return -3;
  }
  const int L = os2d_det_log2_addends(H, W);
  if (L < 0) {
    os2d_set_error("os2d_train_decode_backward_det: H*W=%lld > 2^%d locations: the fixed-point step would exceed 2^-30 of a pair's largest addend",
                   (long long)H * W, OS2D_DET_MAX_LOG2 - 2);
    return -3;
  }
  if (((uintptr_t)workspace & 7) != 0) {
    os2d_set_error("os2d_train_decode_backward_det: workspace is not 8-byte aligned");
    return -1;
  }
  const size_t need = os2d_train_decode_backward_det_workspace_bytes(NB, H, W);
  if (workspace_bytes < need) {
    os2d_set_error("os2d_train_decode_backward_det: workspace %zu bytes < %zu", workspace_bytes, need);
    return -2;
  }
  const int HW = H * W;
  const size_t cells = (size_t)OS2D_K * HW;
  unsigned* words = reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + det_acc_bytes(NB, H, W));
  const DetSink sink{static_cast<unsigned long long*>(workspace), words, L};
  const hipError_t err = hipMemsetAsync(workspace, 0, need, os2d_stream(stream));
  if (err != hipSuccess) {
    os2d_set_error("os2d_train_decode_backward_det: hipMemsetAsync of the workspace: %s", hipGetErrorString(err));
    return -4;
  }
  int rc = 0;
  if (dcls || dcls_det) {       // without either the words stay zero: no pair adds anything
    hipLaunchKernelGGL(decode_det_max_kernel, dim3((HW + DET_MAX_CHUNK - 1) / DET_MAX_CHUNK, NB), dim3(256), 0, os2d_stream(stream), dcls,
                       dcls_det, HW, words);
    if ((rc = os2d_launched("decode_det_max_kernel"))) return rc;
  }
  const float half_box = 0.5f * (float)(stride * (OS2D_T - 1) + rec_field);
  hipLaunchKernelGGL(decode_backward_kernel<true>, dim3(blocks((size_t)HW), NB), dim3(256), 0, os2d_stream(stream), corr, params, dcls,
                     dcls_det, dloc, H, W, P, inverse ? 1 : 0, (float)stride, half_box, dcorr, dparams, sink);
  if ((rc = os2d_launched("decode_backward_kernel (deterministic)"))) return rc;
  if (!dcls && !dcls_det) return 0;
  hipLaunchKernelGGL(decode_det_convert_kernel, dim3(blocks(cells), NB), dim3(256), 0, os2d_stream(stream), sink, cells, dcorr);
  return os2d_launched("decode_det_convert_kernel");
}

int os2d_train_params_backward(const float* dparams, int NB, int P, int H, int W, float* dy, float* dbias, void* stream) {
  os2d_clear_error();
  if (!dparams || !dy) {
    os2d_set_error("os2d_train_params_backward: null pointer");
    return -1;
  }
  if ((P != 6 && P != 4) || !shape_ok(NB, H, W) || (size_t)NB * P > 65535) {
    os2d_set_error("os2d_train_params_backward: bad shape NB=%d P=%d H=%d W=%d", NB, P, H, W);
    return -1;
  }
  const int PL = os2d_plane(H, W);
  hipLaunchKernelGGL(compact_to_plane_kernel, dim3(blocks(PL), NB * P), dim3(256), 0, os2d_stream(stream), dparams, P, H, W, PL, dy);
  int rc = os2d_launched("compact_to_plane_kernel");
  if (rc || !dbias) return rc;
  hipLaunchKernelGGL(channel_sum_kernel, dim3(P), dim3(256), 0, os2d_stream(stream), dparams, NB, P, H * W, dbias);
  return os2d_launched("channel_sum_kernel");
}

int os2d_train_bn_relu_backward(int layer, const float* dh, const float* h, const float* gamma, const float* beta,
                                const float* running_var, float eps, int NB, int H, int W, float* dy, float* dgamma, float* dbeta,
                                float* dbias, void* stream) {
  os2d_clear_error();
  Layer L;
  if (layer != 1 && layer != 2) {
    os2d_set_error("os2d_train_bn_relu_backward: layer %d has no BatchNorm (1 or 2)", layer);
    return -1;
  }
  layer_shape(layer, 6, &L);
  if (!dh || !h || !gamma || !beta || !running_var || !dy) {
    os2d_set_error("os2d_train_bn_relu_backward: null pointer");
    return -1;
  }
  if (!shape_ok(NB, H, W) || (size_t)NB * L.cout > 65535 || !(eps >= 0.f)) {
    os2d_set_error("os2d_train_bn_relu_backward: bad shape NB=%d H=%d W=%d eps=%g", NB, H, W, (double)eps);
    return -1;
  }
  const int PL = os2d_plane(H, W);
  hipLaunchKernelGGL(bn_relu_mask_kernel, dim3(blocks(PL), NB * L.cout), dim3(256), 0, os2d_stream(stream), dh, h, gamma, running_var, eps,
                     L.cout, H, W, PL, dy);
  int rc = os2d_launched("bn_relu_mask_kernel");
  if (rc || (!dgamma && !dbeta && !dbias)) return rc;
  hipLaunchKernelGGL(bn_relu_sums_kernel, dim3(L.cout), dim3(256), 0, os2d_stream(stream), dh, h, gamma, beta, running_var, eps, NB, L.cout, H,
                     W, PL, dgamma, dbeta, dbias);
  return os2d_launched("bn_relu_sums_kernel");
}

size_t os2d_train_conv_data_workspace_floats(int layer, int P) {
  Layer L;
  if (!layer_shape(layer, P, &L)) return 0;
  return (size_t)L.cout * L.cin * L.ks * L.ks;
}

size_t os2d_train_conv_data_workspace_floats_ex(int arith, int layer, int P, int NB) {
  const size_t wf = os2d_train_conv_data_workspace_floats(layer, P);
  if (arith == 0 || wf == 0) return arith == 0 ? wf : 0;
  if (arith != 1 || NB < 1) return 0;
  return wf + 1 + (size_t)NB;                 // the flipped filters, then the maxima words: the filters', one per pair of dy
}

int os2d_train_conv_backward_data_ex(int arith, int layer, int P, const float* w, const float* dy, int NB, int H, int W, float* dx,
                                     float* workspace, size_t workspace_floats, void* stream) {
  os2d_clear_error();
  Layer L;
  if (arith != 0 && arith != 1) {
    os2d_set_error("os2d_train_conv_backward_data: bad arith %d (0 = fp32, 1 = f16x3)", arith);
    return -1;
  }
  if (!layer_shape(layer, P, &L)) {
    os2d_set_error("os2d_train_conv_backward_data: bad layer %d / P %d", layer, P);
    return -1;
  }
  if (!w || !dy || !dx || !workspace) {
    os2d_set_error("os2d_train_conv_backward_data: null pointer");
    return -1;
  }
  if (!shape_ok(NB, H, W) || NB > 65535) {
    os2d_set_error("os2d_train_conv_backward_data: bad shape NB=%d H=%d W=%d (W <= %d)", NB, H, W, OS2D_MAX_W_DIRECT7);
    return -1;
  }
  const int T2 = L.ks * L.ks;
  const size_t wf = (size_t)L.cout * L.cin * T2;
  const size_t need = arith ? wf + 1 + (size_t)NB : wf;
  if (workspace_floats < need) {
    os2d_set_error("os2d_train_conv_backward_data: workspace %zu floats < %zu", workspace_floats, need);
    return -2;
  }
  hipLaunchKernelGGL(flip_weights_kernel, dim3(blocks(wf)), dim3(256), 0, os2d_stream(stream), w, L.cout, L.cin, T2, workspace);
  int rc = os2d_launched("flip_weights_kernel");
  if (rc) return rc;
  if (arith)
    return os2d_f16x3_conv_data(workspace, dy, dx, L.cout, L.cin, L.ks, NB, H, W, reinterpret_cast<unsigned*>(workspace + wf),
                                os2d_stream(stream));
  const int PL = os2d_plane(H, W);
  const Taps tp{L.ks, L.ks / 2, os2d_ws(W), T2};
  const int K = L.cout * T2;
  return gemm<false>(LdRows{workspace, K}, LdShifted{dy, (size_t)L.cout * PL, PL, tp}, StPlane{dx, (size_t)L.cin * PL, PL, H, W}, L.cin,
                     PL, K, NB, 0, os2d_stream(stream), "conv data gradient");
}

int os2d_train_conv_backward_data(int layer, int P, const float* w, const float* dy, int NB, int H, int W, float* dx,
                                  float* workspace, size_t workspace_floats, void* stream) {
  return os2d_train_conv_backward_data_ex(0, layer, P, w, dy, NB, H, W, dx, workspace, workspace_floats, stream);
}

// the forward convolution of a layer whose BatchNorm takes batch statistics: the data gradient's GEMM with the roles of the
// channel counts swapped, the raw (unflipped) filters as the A operand and the bias added in the store
size_t os2d_train_conv_forward_workspace_floats(int arith, int layer, int P, int NB) {
  Layer L;
  if ((layer != 1 && layer != 2) || !layer_shape(layer, P, &L) || NB < 1) return 0;
  return arith == 0 ? 1 : arith == 1 ? 1 + (size_t)NB : 0;      // f16x3: the maxima words (the filters', one per pair of x)
}

int os2d_train_conv_forward(int arith, int layer, int P, const float* w, const float* bias, const float* x, int NB, int H, int W, float* z,
                            float* workspace, size_t workspace_floats, void* stream) {
  os2d_clear_error();
  Layer L;
  if (arith != 0 && arith != 1) {
    os2d_set_error("os2d_train_conv_forward: bad arith %d (0 = fp32, 1 = f16x3)", arith);
    return -1;
  }
  if ((layer != 1 && layer != 2) || !layer_shape(layer, P, &L)) {
    os2d_set_error("os2d_train_conv_forward: bad layer %d / P %d (the layers with a BatchNorm: 1 or 2)", layer, P);
    return -1;
  }
  if (!w || !bias || !x || !z || !workspace) {
    os2d_set_error("os2d_train_conv_forward: null pointer");
    return -1;
  }
  if (!shape_ok(NB, H, W) || (size_t)NB * L.cout > 65535) {
    os2d_set_error("os2d_train_conv_forward: bad shape NB=%d H=%d W=%d (W <= %d, NB * %d <= 65535)", NB, H, W, OS2D_MAX_W_DIRECT7, L.cout);
    return -1;
  }
  const size_t need = arith ? 1 + (size_t)NB : 1;
  if (workspace_floats < need) {
    os2d_set_error("os2d_train_conv_forward: workspace %zu floats < %zu", workspace_floats, need);
    return -2;
  }
  if (arith)
    return os2d_f16x3_conv_forward(w, bias, x, input_planes(layer), z, L.cout, L.cin, L.ks, NB, H, W, reinterpret_cast<unsigned*>(workspace),
                                   os2d_stream(stream));
  const int PL = os2d_plane(H, W), T2 = L.ks * L.ks;
  const Taps tp{L.ks, L.ks / 2, os2d_ws(W), T2};
  return gemm<false>(LdRows{w, L.cin * T2}, LdShifted{x, (size_t)input_planes(layer) * PL, PL, tp},
                     StPlane{z, (size_t)L.cout * PL, PL, H, W, bias}, L.cout, PL, L.cin * T2, NB, 0, os2d_stream(stream), "conv forward");
}

size_t os2d_train_conv_weight_slice_floats(int layer, int P) { return os2d_train_conv_data_workspace_floats(layer, P); }

// f16x3: every slice of room carries WEIGHT_WORDS floats more; the maxima words take the first WEIGHT_WORDS floats of the workspace
constexpr size_t WEIGHT_WORDS = 16;
size_t os2d_train_conv_weight_slice_floats_ex(int arith, int layer, int P) {
  const size_t slice = os2d_train_conv_weight_slice_floats(layer, P);
  if (arith == 0 || slice == 0) return arith == 0 ? slice : 0;
  return arith == 1 ? slice + WEIGHT_WORDS : 0;
}

int os2d_train_conv_backward_weight_ex(int arith, int layer, int P, const float* x, const float* dy, int NB, int H, int W, float* dw,
                                       float* workspace, size_t workspace_floats, void* stream) {
  os2d_clear_error();
  Layer L;
  if (arith != 0 && arith != 1) {
    os2d_set_error("os2d_train_conv_backward_weight: bad arith %d (0 = fp32, 1 = f16x3)", arith);
    return -1;
  }
  if (!layer_shape(layer, P, &L)) {
    os2d_set_error("os2d_train_conv_backward_weight: bad layer %d / P %d", layer, P);
    return -1;
  }
  if (!x || !dy || !dw || !workspace) {
    os2d_set_error("os2d_train_conv_backward_weight: null pointer");
    return -1;
  }
  if (!shape_ok(NB, H, W)) {
    os2d_set_error("os2d_train_conv_backward_weight: bad shape NB=%d H=%d W=%d (W <= %d)", NB, H, W, OS2D_MAX_W_DIRECT7);
    return -1;
  }
  const int T2 = L.ks * L.ks;
  const size_t slice = (size_t)L.cout * L.cin * T2;
  const int PL = os2d_plane(H, W);
  const long long K = (long long)NB * PL;
  if (K > 0x7fffffffLL) {
    os2d_set_error("os2d_train_conv_backward_weight: NB * PLANE = %lld positions exceed the 32-bit index", K);
    return -3;
  }
  const size_t room = arith ? slice + WEIGHT_WORDS : slice;
  const int kstep = arith ? OS2D_F16X3_KSTEP : GK;
  long long splits = (long long)(workspace_floats / room);
  if (splits < 1) {
    os2d_set_error("os2d_train_conv_backward_weight: workspace %zu floats < one slice of %zu", workspace_floats, room);
    return -2;
  }
  if (splits > 64) splits = 64;
  if (splits > (K + kstep - 1) / kstep) splits = (K + kstep - 1) / kstep;
  const int ksplit = (int)(((K + splits - 1) / splits + kstep - 1) / kstep * kstep);
  splits = (K + ksplit - 1) / ksplit;
  float* part = arith ? workspace + WEIGHT_WORDS : workspace;
  int rc;
  if (arith) {
    rc = os2d_f16x3_conv_weight(x, input_planes(layer), dy, part, L.cout, L.cin, L.ks, NB, H, W, (int)splits, ksplit,
                                reinterpret_cast<unsigned*>(workspace), os2d_stream(stream));
  } else {
    const Taps tp{L.ks, L.ks / 2, os2d_ws(W), T2};
    const int N = L.cin * T2;
    rc = gemm<true>(LdPairRows{dy, (size_t)L.cout * PL, PL}, LdPairShifted{x, (size_t)input_planes(layer) * PL, PL, tp},
                    StSlice{workspace, L.cout, N}, L.cout, N, (int)K, (int)splits, ksplit, os2d_stream(stream), "conv weight gradient");
  }
  if (rc) return rc;
  hipLaunchKernelGGL(split_sum_kernel, dim3(blocks(slice)), dim3(256), 0, os2d_stream(stream), part, (int)splits, slice, dw);
  return os2d_launched("split_sum_kernel");
}

int os2d_train_conv_backward_weight(int layer, int P, const float* x, const float* dy, int NB, int H, int W, float* dw,
                                    float* workspace, size_t workspace_floats, void* stream) {
  return os2d_train_conv_backward_weight_ex(0, layer, P, x, dy, NB, H, W, dw, workspace, workspace_floats, stream);
}

int os2d_train_norm225_backward(const float* corr, const float* dxn, int NB, int H, int W, float* dcorr, void* stream) {
  os2d_clear_error();
  if (!corr || !dxn || !dcorr) {
    os2d_set_error("os2d_train_norm225_backward: null pointer");
    return -1;
  }
  if (!shape_ok(NB, H, W) || NB > 65535) {
    os2d_set_error("os2d_train_norm225_backward: bad shape NB=%d H=%d W=%d", NB, H, W);
    return -1;
  }
  hipLaunchKernelGGL(norm225_backward_kernel, dim3(blocks((size_t)H * W), NB), dim3(256), 0, os2d_stream(stream), corr, dxn, H, W,
                     os2d_plane(H, W), dcorr);
  return os2d_launched("norm225_backward_kernel");
}

size_t os2d_train_corr_workspace_floats(int A, int C, int H, int W) {
  if (A < 1 || C < 1 || H < 1 || W < 1) return 0;
  const size_t HW = (size_t)H * W;
  return 2 * (size_t)A * HW + (size_t)A * C * HW;
}

size_t os2d_train_corr_workspace_floats_ex(int arith, int A, int B, int C, int H, int W) {
  const size_t base = os2d_train_corr_workspace_floats(A, C, H, W);
  if (arith == 0 || base == 0) return arith == 0 ? base : 0;
  if (arith != 1 || B < 1) return 0;
  return base + 2 + (size_t)A + B;            // the maxima words: qp, the normalised image map, dcorr per image, dcorr per class
}

int os2d_train_corr_backward_ex(int arith, const float* fm, const float* qp, const float* dcorr, int A, int B, int C, int H, int W,
                                float* dfm, float* dq, float* workspace, size_t workspace_floats, void* stream) {
  os2d_clear_error();
  if (arith != 0 && arith != 1) {
    os2d_set_error("os2d_train_corr_backward: bad arith %d (0 = fp32, 1 = f16x3)", arith);
    return -1;
  }
  if (!fm || !qp || !dcorr || !workspace) {
    os2d_set_error("os2d_train_corr_backward: null pointer");
    return -1;
  }
  if (A < 1 || B < 1 || C < 1 || H < 1 || W < 1 || A > 65535 || B > 65535) {
    os2d_set_error("os2d_train_corr_backward: bad shape A=%d B=%d C=%d H=%d W=%d", A, B, C, H, W);
    return -1;
  }
  const long long HW = (long long)H * W;
  if ((long long)B * OS2D_K > 0x7fffffffLL || (long long)A * HW > 0x7fffffffLL) {
    os2d_set_error("os2d_train_corr_backward: reduction length exceeds the 32-bit index");
    return -3;
  }
  const size_t base = os2d_train_corr_workspace_floats(A, C, H, W);
  const size_t need = arith ? base + 2 + (size_t)A + B : base;
  if (workspace_floats < need) {
    os2d_set_error("os2d_train_corr_backward: workspace %zu floats < %zu", workspace_floats, need);
    return -2;
  }
  if (!dfm && !dq) return 0;
  float* rinv = workspace;
  float* dfh = rinv + 2 * (size_t)A * HW;     // the second A * HW floats are not used
  hipLaunchKernelGGL(image_norm_kernel, dim3(blocks(HW), A), dim3(256), 0, os2d_stream(stream), fm, C, (int)HW, rinv);
  int rc = os2d_launched("image_norm_kernel");
  if (rc) return rc;
  if (arith) {
    rc = os2d_f16x3_corr(fm, rinv, qp, dcorr, A, B, C, (int)HW, dfm ? dfh : nullptr, dq, reinterpret_cast<unsigned*>(workspace + base),
                         os2d_stream(stream));
    if (rc || !dfm) return rc;
    hipLaunchKernelGGL(image_norm_backward_kernel, dim3(blocks(HW), A), dim3(256), 0, os2d_stream(stream), fm, dfh, C, (int)HW, dfm);
    return os2d_launched("image_norm_backward_kernel");
  }
  if (dfm) {
    rc = gemm<false>(LdClassT{qp, C}, LdCorrRows{dcorr, B, (int)HW}, StDense{dfh, C, (int)HW}, C, (int)HW, B * OS2D_K, A, 0, os2d_stream(stream),
                     "correlation backward (image)");
    if (rc) return rc;
    hipLaunchKernelGGL(image_norm_backward_kernel, dim3(blocks(HW), A), dim3(256), 0, os2d_stream(stream), fm, dfh, C, (int)HW, dfm);
    rc = os2d_launched("image_norm_backward_kernel");
    if (rc) return rc;
  }
  if (dq)
    rc = gemm<true>(LdImageNorm{fm, rinv, C, (int)HW}, LdCorrCols{dcorr, B, (int)HW}, StDense{dq, C, OS2D_K}, C, OS2D_K, A * (int)HW, B,
                    0, os2d_stream(stream), "correlation backward (class)");
  return rc;
}

int os2d_train_corr_backward(const float* fm, const float* qp, const float* dcorr, int A, int B, int C, int H, int W, float* dfm,
                             float* dq, float* workspace, size_t workspace_floats, void* stream) {
  return os2d_train_corr_backward_ex(0, fm, qp, dcorr, A, B, C, H, W, dfm, dq, workspace, workspace_floats, stream);
}

int os2d_train_class_backward(const float* q15, const float* dq, int B, int C, float* const* dsrcs, const int* sizes,
                              float* workspace, size_t workspace_floats, void* stream) {
  os2d_clear_error();
  if (!q15 || !dq || !dsrcs || !sizes || !workspace) {
    os2d_set_error("os2d_train_class_backward: null pointer");
    return -1;
  }
  if (B < 1 || C < 1 || B > 65535) {
    os2d_set_error("os2d_train_class_backward: bad shape B=%d C=%d", B, C);
    return -1;
  }
  const size_t need = (size_t)B * C * OS2D_K;
  if (workspace_floats < need) {
    os2d_set_error("os2d_train_class_backward: workspace %zu floats < %zu", workspace_floats, need);
    return -2;
  }
  hipLaunchKernelGGL(class_norm_backward_kernel, dim3(1, B), dim3(256), 0, os2d_stream(stream), q15, dq, C, workspace);
  int rc = os2d_launched("class_norm_backward_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(class_resize_backward_kernel, dim3(blocks(C), B), dim3(256), 0, os2d_stream(stream), workspace, C, dsrcs, sizes);
  return os2d_launched("class_resize_backward_kernel");
}

}  // extern "C"
