// The backward of resample + pool + box decode (os2d_train_decode_backward, os2d_train_decode_backward_det; decode_det.h
// declares the two launch functions the entry points of train.hip call after their checks): one kernel for both routes of the
// d corr scatter - fp32 atomics, or 64-bit integers on the fixed-point grid of decode_det.h with a maxima pass in front and a
// convert pass behind.
#include "../csrc/os2d_common.h"
#include "../csrc/sample_decode.h"
#include "train_common.h"
#include "decode_det.h"

using os2d_train::blocks;

namespace {

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
// number's.  A work-group reduces DET_MAX_CHUNK locations and makes ONE atomicMax (as the maxima pass of train_gemm.hip).
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

}  // namespace

static float decode_half_box(int stride, int rec_field) { return 0.5f * (float)(stride * (OS2D_T - 1) + rec_field); }

int os2d_decode_backward_launch(const float* corr, const float* params, const float* dcls, const float* dcls_det, const float* dloc, int NB,
                                int H, int W, int P, int inverse, int stride, int rec_field, float* dcorr, float* dparams,
                                hipStream_t stream) {
  hipLaunchKernelGGL(decode_backward_kernel<false>, dim3(blocks((size_t)H * W), NB), dim3(256), 0, stream, corr, params, dcls, dcls_det, dloc,
                     H, W, P, inverse ? 1 : 0, (float)stride, decode_half_box(stride, rec_field), dcorr, dparams, DetSink{nullptr, nullptr, 0});
  return os2d_launched("decode_backward_kernel");
}

int os2d_decode_backward_det_launch(const float* corr, const float* params, const float* dcls, const float* dcls_det, const float* dloc,
                                    int NB, int H, int W, int P, int inverse, int stride, int rec_field, float* dcorr, float* dparams,
                                    void* workspace, hipStream_t stream) {
  const int HW = H * W;
  const size_t cells = (size_t)OS2D_K * HW;
  unsigned* words = reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + os2d_det_acc_bytes(NB, H, W));
  const DetSink sink{static_cast<unsigned long long*>(workspace), words, os2d_det_log2_addends(H, W)};
  const hipError_t err = hipMemsetAsync(workspace, 0, os2d_det_workspace_bytes(NB, H, W), stream);
  if (err != hipSuccess) {
    os2d_set_error("os2d_train_decode_backward_det: hipMemsetAsync of the workspace: %s", hipGetErrorString(err));
    return -4;
  }
  int rc = 0;
  if (dcls || dcls_det) {       // without either the words stay zero: no pair adds anything
    hipLaunchKernelGGL(decode_det_max_kernel, dim3((HW + DET_MAX_CHUNK - 1) / DET_MAX_CHUNK, NB), dim3(256), 0, stream, dcls, dcls_det, HW,
                       words);
    if ((rc = os2d_launched("decode_det_max_kernel"))) return rc;
  }
  hipLaunchKernelGGL(decode_backward_kernel<true>, dim3(blocks((size_t)HW), NB), dim3(256), 0, stream, corr, params, dcls, dcls_det, dloc, H,
                     W, P, inverse ? 1 : 0, (float)stride, decode_half_box(stride, rec_field), dcorr, dparams, sink);
  if ((rc = os2d_launched("decode_backward_kernel (deterministic)"))) return rc;
  if (!dcls && !dcls_det) return 0;
  hipLaunchKernelGGL(decode_det_convert_kernel, dim3(blocks(cells), NB), dim3(256), 0, stream, sink, cells, dcorr);
  return os2d_launched("decode_det_convert_kernel");
}
