// Batch-statistics ("live") BatchNorm of the TransformNet layers 1 (128 channels) and 2 (64) for the training forward and
// backward (include/os2d_train.h): statistics, normalise + ReLU, and the backward through the statistics.  The raw
// convolution that feeds them is os2d_train_conv_forward (train.hip: it runs on the GEMMs of the backward pass, train_gemm.hip).
//
// All four kernels are memory-bound passes over z [NB,C,PLANE]: 16-byte loads and stores along the plane (PLANE is a multiple
// of 64 floats, every plane 16-byte aligned), pad cells told from data cells by index - what a pad cell holds is never used.
// Per-channel sums are reduced in fp64 in a fixed order: a thread walks its cells in order, a wave combines by butterfly, the
// four waves of a work-group are added as (0 + 1) + (2 + 3), and the work-groups of a channel - one per slice of `per`
// consecutive pairs - are combined in slice order.  Two runs on the same input give the same bits.
#include "../../include/os2d_train.h"
#include "train_common.h"    // layer_channels, shape_ok

using namespace os2d_train;

namespace {

constexpr int MAX_SLICES = 32;     // work-groups per channel

// pairs per slice, slices
void slices(int NB, int* per, int* S) {
  *per = (NB + MAX_SLICES - 1) / MAX_SLICES;
  *S = (NB + *per - 1) / *per;
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// which of the 4 cells cell .. cell+3 (cell a multiple of 4) are data cells; false when none is
__device__ __forceinline__ bool interior4(int cell, int H, int W, bool (&in)[4]) {
  const int ws = os2d_ws(W), end = H * ws;
  const int r = cell - os2d_base(W);       // a multiple of 4: the base is one
  if (r < 0 || r >= end) {
    in[0] = in[1] = in[2] = in[3] = false;
    return false;
  }
  int col = r - (r / ws) * ws;
  bool any = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    in[j] = col < W && r + j < end;
    any |= in[j];
    if (++col == ws) col = 0;
  }
  return any;
}

__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- statistics, first kernel: (mean, M2 = sum of squared distances to that mean) of channel blockIdx.x over the data cells
// of the pairs of slice blockIdx.y: two passes (the second finds the slice in L2).  part [C][S][2] doubles.
__global__ __launch_bounds__(256) void bn_stats_slice_kernel(const float* __restrict__ z, int NB, int C, int H, int W, int PL, int per,
                                                             double* __restrict__ part) {
  __shared__ double red[4];
  const int c = blockIdx.x, s = blockIdx.y;
  const int nb0 = s * per, nb1 = min(NB, nb0 + per);
  const double count = (double)(nb1 - nb0) * H * W;
  double mean = 0.0, acc = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    acc = 0.0;
    for (int nb = nb0; nb < nb1; ++nb) {
      const f32x4* p = reinterpret_cast<const f32x4*>(z + ((size_t)nb * C + c) * PL);
      for (int i = threadIdx.x; i < PL / 4; i += 256) {
        bool in[4];
        if (!interior4(4 * i, H, W, in)) continue;
        const f32x4 v = p[i];
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (in[j]) {
            const double d = (double)v[j] - mean;     // pass 0: mean = 0
            acc += pass ? d * d : d;
          }
      }
    }
    acc = block_sum_f64(acc, red);
    if (pass == 0) mean = acc / count;
  }
  if (threadIdx.x == 0) {
    part[((size_t)c * gridDim.y + s) * 2] = mean;
    part[((size_t)c * gridDim.y + s) * 2 + 1] = acc;
  }
}

// ---- statistics, second kernel: Chan's combination of the slices in slice order, one thread per channel
__global__ __launch_bounds__(64) void bn_stats_combine_kernel(const double* __restrict__ part, int NB, int C, int HW, int per, int S,
                                                              float eps, float* __restrict__ mean, float* __restrict__ var,
                                                              float* __restrict__ invstd) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  double n = 0.0, m = 0.0, m2 = 0.0;
  for (int s = 0; s < S; ++s) {
    const double ns = (double)(min(NB, (s + 1) * per) - s * per) * HW;
    const double ms = part[((size_t)c * S + s) * 2], m2s = part[((size_t)c * S + s) * 2 + 1];
    const double delta = ms - m, tot = n + ns;
    m += delta * (ns / tot);
    m2 += m2s + delta * delta * (n * ns / tot);
    n = tot;
  }
  const double v = m2 / n;
  mean[c] = (float)m;
  var[c] = (float)v;
  invstd[c] = (float)(1.0 / sqrt(v + (double)eps));
}

// ---- normalise + ReLU: h = relu(((z - mean) invstd) gamma + beta) at data cells, +0.0 elsewhere
__global__ __launch_bounds__(256) void bn_relu_apply_kernel(const float* __restrict__ z, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, int C, int H, int W, int PL,
                                                            float* __restrict__ h) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const size_t plane = blockIdx.y;
  if (i >= PL / 4) return;
  const int c = (int)(plane % C);
  f32x4 out = {0.f, 0.f, 0.f, 0.f};
  bool in[4];
  if (interior4(4 * i, H, W, in)) {
    const f32x4 v = reinterpret_cast<const f32x4*>(z + plane * PL)[i];
    const float m = mean[c], r = invstd[c], g = gamma[c], b = beta[c];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (in[j]) out[j] = os2d_relu(((v[j] - m) * r) * g + b);
  }
  reinterpret_cast<f32x4*>(h + plane * PL)[i] = out;
}

// ---- backward, first kernel: sum g and sum g xhat of channel blockIdx.x over slice blockIdx.y; g = dh where h > 0,
// xhat = (z - mean) invstd in fp32 as the forward formed it.  part [C][S][2] doubles.
__global__ __launch_bounds__(256) void bn_batch_sums_kernel(const float* __restrict__ dh, const float* __restrict__ z,
                                                            const float* __restrict__ hh, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, int NB, int C, int H, int W, int PL,
                                                            int per, double* __restrict__ part) {
  __shared__ double red[4];
  const int c = blockIdx.x, s = blockIdx.y;
  const int nb0 = s * per, nb1 = min(NB, nb0 + per);
  const float m = mean[c], r = invstd[c];
  double sb = 0.0, sg = 0.0;
  for (int nb = nb0; nb < nb1; ++nb) {
    const size_t o = ((size_t)nb * C + c) * PL;
    for (int i = threadIdx.x; i < PL / 4; i += 256) {
      bool in[4];
      if (!interior4(4 * i, H, W, in)) continue;
      const f32x4 hv = reinterpret_cast<const f32x4*>(hh + o)[i];
      const f32x4 dv = reinterpret_cast<const f32x4*>(dh + o)[i];
      const f32x4 zv = reinterpret_cast<const f32x4*>(z + o)[i];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (in[j] && hv[j] > 0.f) {
          sb += (double)dv[j];
          sg += (double)dv[j] * (double)((zv[j] - m) * r);
        }
    }
  }
  sb = block_sum_f64(sb, red);
  sg = block_sum_f64(sg, red);
  if (threadIdx.x == 0) {
    part[((size_t)c * gridDim.y + s) * 2] = sb;
    part[((size_t)c * gridDim.y + s) * 2 + 1] = sg;
  }
}

// ---- backward, second kernel: dy = gamma invstd (g - dbeta / n - xhat dgamma / n) at data cells, 0 elsewhere; the slices of
// the channel are added in slice order by every thread (at most 32 pairs of doubles); the first work-group of a channel
// writes dbeta / dgamma
__global__ __launch_bounds__(256) void bn_batch_apply_kernel(const float* __restrict__ dh, const float* __restrict__ z,
                                                             const float* __restrict__ hh, const float* __restrict__ gamma,
                                                             const float* __restrict__ mean, const float* __restrict__ invstd,
                                                             const double* __restrict__ part, int S, double inv_n, int C, int H, int W,
                                                             int PL, float* __restrict__ dy, float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const size_t plane = blockIdx.y;
  const int c = (int)(plane % C);
  double sb = 0.0, sg = 0.0;
  for (int s = 0; s < S; ++s) {
    sb += part[((size_t)c * S + s) * 2];
    sg += part[((size_t)c * S + s) * 2 + 1];
  }
  if (plane == (size_t)c && i == 0) {       // pair 0
    if (dbeta) dbeta[c] = (float)sb;
    if (dgamma) dgamma[c] = (float)sg;
  }
  if (i >= PL / 4) return;
  f32x4 out = {0.f, 0.f, 0.f, 0.f};
  bool in[4];
  if (interior4(4 * i, H, W, in)) {
    const size_t o = plane * PL;
    const f32x4 hv = reinterpret_cast<const f32x4*>(hh + o)[i];
    const f32x4 dv = reinterpret_cast<const f32x4*>(dh + o)[i];
    const f32x4 zv = reinterpret_cast<const f32x4*>(z + o)[i];
    const float m = mean[c], r = invstd[c], k = gamma[c] * r;
    const float mb = (float)(sb * inv_n), mg = (float)(sg * inv_n);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (in[j]) {
        const float g = hv[j] > 0.f ? dv[j] : 0.f;
        out[j] = k * ((g - mb) - ((zv[j] - m) * r) * mg);
      }
  }
  reinterpret_cast<f32x4*>(dy + plane * PL)[i] = out;
}

// the argument checks the three entry points share; C = the layer's channels on success
int check_common(const char* who, int layer, int NB, int H, int W, bool pointers, bool aligned, int* C) {
  *C = layer_channels(layer);
  if (*C == 0) {
    os2d_set_error("%s: layer %d has no BatchNorm (1 or 2)", who, layer);
    return -1;
  }
  if (!pointers) {
    os2d_set_error("%s: null pointer", who);
    return -1;
  }
  if (!shape_ok(NB, H, W) || (size_t)NB * *C > 65535) {
    os2d_set_error("%s: bad shape NB=%d H=%d W=%d (W <= %d, NB * %d <= 65535)", who, NB, H, W, OS2D_MAX_W_DIRECT7, *C);
    return -1;
  }
  if (!aligned) {
    os2d_set_error("%s: plane tensors must be 16-byte aligned", who);
    return -1;
  }
  return 0;
}

}  // namespace

extern "C" {

size_t os2d_train_bn_workspace_bytes(int layer, int NB) {
  const int C = layer_channels(layer);
  if (C == 0 || NB < 1 || (size_t)NB * C > 65535) return 0;
  int per, S;
  slices(NB, &per, &S);
  return (size_t)C * S * 2 * sizeof(double);
}

int os2d_train_bn_stats(int layer, const float* z, int NB, int H, int W, float eps, float* mean, float* var, float* invstd,
                        void* workspace, size_t workspace_bytes, void* stream) {
  os2d_clear_error();
  int C;
  int rc = check_common("os2d_train_bn_stats", layer, NB, H, W, z && mean && var && invstd && workspace, aligned16(z) && aligned16(workspace),
                        &C);
  if (rc) return rc;
  if ((long long)NB * H * W < 2 || !(eps >= 0.f)) {
    os2d_set_error("os2d_train_bn_stats: batch statistics need n = NB*H*W >= 2 values per channel and eps >= 0 (n = %lld, eps = %g)",
                   (long long)NB * H * W, (double)eps);
    return -1;
  }
  const size_t need = os2d_train_bn_workspace_bytes(layer, NB);
  if (workspace_bytes < need) {
    os2d_set_error("os2d_train_bn_stats: workspace %zu bytes < %zu", workspace_bytes, need);
    return -2;
  }
  int per, S;
  slices(NB, &per, &S);
  const int PL = os2d_plane(H, W);
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(bn_stats_slice_kernel, dim3(C, S), dim3(256), 0, os2d_stream(stream), z, NB, C, H, W, PL, per, part);
  if ((rc = os2d_launched("bn_stats_slice_kernel"))) return rc;
  hipLaunchKernelGGL(bn_stats_combine_kernel, dim3((C + 63) / 64), dim3(64), 0, os2d_stream(stream), part, NB, C, H * W, per, S, eps, mean, var,
                     invstd);
  return os2d_launched("bn_stats_combine_kernel");
}

int os2d_train_bn_relu_forward(int layer, const float* z, const float* gamma, const float* beta, const float* mean, const float* invstd,
                               int NB, int H, int W, float* h, void* stream) {
  os2d_clear_error();
  int C;
  const int rc = check_common("os2d_train_bn_relu_forward", layer, NB, H, W, z && gamma && beta && mean && invstd && h,
                              aligned16(z) && aligned16(h), &C);
  if (rc) return rc;
  const int PL = os2d_plane(H, W);
  hipLaunchKernelGGL(bn_relu_apply_kernel, dim3((PL / 4 + 255) / 256, NB * C), dim3(256), 0, os2d_stream(stream), z, gamma, beta, mean, invstd,
                     C, H, W, PL, h);
  return os2d_launched("bn_relu_apply_kernel");
}

int os2d_train_bn_relu_backward_batch(int layer, const float* dh, const float* z, const float* h, const float* gamma, const float* mean,
                                      const float* invstd, int NB, int H, int W, float* dy, float* dgamma, float* dbeta, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  os2d_clear_error();
  int C;
  int rc = check_common("os2d_train_bn_relu_backward_batch", layer, NB, H, W, dh && z && h && gamma && mean && invstd && dy && workspace,
                        aligned16(dh) && aligned16(z) && aligned16(h) && aligned16(dy) && aligned16(workspace), &C);
  if (rc) return rc;
  if ((long long)NB * H * W < 2) {
    os2d_set_error("os2d_train_bn_relu_backward_batch: batch statistics need n = NB*H*W >= 2 values per channel (n = %lld)",
                   (long long)NB * H * W);
    return -1;
  }
  const size_t need = os2d_train_bn_workspace_bytes(layer, NB);
  if (workspace_bytes < need) {
    os2d_set_error("os2d_train_bn_relu_backward_batch: workspace %zu bytes < %zu", workspace_bytes, need);
    return -2;
  }
  int per, S;
  slices(NB, &per, &S);
  const int PL = os2d_plane(H, W);
  double* part = static_cast<double*>(workspace);
  hipLaunchKernelGGL(bn_batch_sums_kernel, dim3(C, S), dim3(256), 0, os2d_stream(stream), dh, z, h, mean, invstd, NB, C, H, W, PL, per, part);
  if ((rc = os2d_launched("bn_batch_sums_kernel"))) return rc;
  hipLaunchKernelGGL(bn_batch_apply_kernel, dim3((PL / 4 + 255) / 256, NB * C), dim3(256), 0, os2d_stream(stream), dh, z, h, gamma, mean, invstd,
                     part, S, 1.0 / ((double)NB * H * W), C, H, W, PL, dy, dgamma, dbeta);
  return os2d_launched("bn_batch_apply_kernel");
}

}  // extern "C"
