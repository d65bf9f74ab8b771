// libos2d_train.so (include/os2d_train.h): the C ABI of the backward pass of the OS2D head on gfx950 - check, size, launch - and
// its per-location kernels: BatchNorm + ReLU masks, the two L2 normalisations, the bilinear class-map resize and the small
// passes around the GEMMs.  The matrix-shaped work is train_gemm.hip's (fp32, or split-fp16 at arith = 1 of the *_ex entry
// points), the resample / pool / box decode backward decode_backward.hip's.
#include <stdio.h>

#include "../../include/os2d_train.h"
#include "../csrc/os2d_common.h"
#include "train_common.h"   // the layer table, shape_ok, blocks
#include "train_gemm.h"     // the five GEMM sites and the layouts of their workspaces
#include "decode_det.h"     // the fixed-point grid of the order-independent d corr scatter; the launches of decode_backward.hip

using namespace os2d_train;
using namespace os2d_train_gemm;

namespace {

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

// ---- the argument checks the entry points share; `who` is the entry point's name in the error text (the *_ex entry points
// report under the name without _ex).  The bad_... ones return true after setting the text.
bool null_pointer(const char* who, bool pointers) { return !pointers && OS2D_REFUSE(true, "%s: null pointer", who); }
// 0, or the return code
int check_decode(const char* who, bool pointers, int NB, int H, int W, int P, int stride, int rec_field) {
  if (null_pointer(who, pointers)) return -1;
  if (NB < 1 || H < 1 || W < 1 || (P != 6 && P != 4) || stride < 1 || rec_field < 1)
    return OS2D_REFUSE(-1, "%s: bad shape NB=%d H=%d W=%d P=%d stride=%d rec_field=%d", who, NB, H, W, P, stride, rec_field);
  return NB > 65535 ? OS2D_REFUSE(-3, "%s: NB=%d > 65535", who, NB) : 0;
}
bool bad_arith(const char* who, int arith) {
  return arith != 0 && arith != 1 && OS2D_REFUSE(true, "%s: bad arith %d (0 = fp32, 1 = f16x3)", who, arith);
}
// bn_only: the entry point takes the layers with a BatchNorm alone
bool bad_layer(const char* who, int layer, int P, bool bn_only, Layer* L) {
  if ((!bn_only || layer_channels(layer)) && layer_shape(layer, P, L)) return false;
  return OS2D_REFUSE(true, "%s: bad layer %d / P %d%s", who, layer, P, bn_only ? " (the layers with a BatchNorm: 1 or 2)" : "");
}
// planes: the launch puts NB * planes on a grid axis (1: NB itself, 0: neither)
bool bad_conv_shape(const char* who, int NB, int H, int W, int planes) {
  if (shape_ok(NB, H, W) && (size_t)NB * planes <= 65535) return false;
  if (planes <= 1) return OS2D_REFUSE(true, "%s: bad shape NB=%d H=%d W=%d (W <= %d)", who, NB, H, W, OS2D_MAX_W_DIRECT7);
  return OS2D_REFUSE(true, "%s: bad shape NB=%d H=%d W=%d (W <= %d, NB * %d <= 65535)", who, NB, H, W, OS2D_MAX_W_DIRECT7, planes);
}
bool workspace_too_small(const char* who, size_t have, size_t need) {
  return have < need && OS2D_REFUSE(true, "%s: workspace %zu floats < %zu", who, have, need);
}

}  // namespace

// ================================================================================================ C ABI
extern "C" {

int os2d_train_abi_version(void) { return OS2D_TRAIN_ABI_VERSION; }
const char* os2d_train_last_error(void) { return os2d_error_text; }

int os2d_train_decode_backward(const float* corr, const float* params, const float* dcls, const float* dcls_det, const float* dloc,
                               int NB, int H, int W, int P, int inverse, int stride, int rec_field, float* dcorr, float* dparams,
                               void* stream) {
  os2d_clear_error();
  const int rc = check_decode("os2d_train_decode_backward", corr && params && dcorr && dparams, NB, H, W, P, stride, rec_field);
  if (rc) return rc;
  return os2d_decode_backward_launch(corr, params, dcls, dcls_det, dloc, NB, H, W, P, inverse, stride, rec_field, dcorr, dparams,
                                     os2d_stream(stream));
}

int os2d_train_decode_det_exponent(unsigned max_bits, int H, int W) {
  const int L = os2d_det_log2_addends(H, W);
  return L < 0 ? OS2D_TRAIN_DET_REFUSED : os2d_det_exponent(max_bits, L);
}

size_t os2d_train_decode_backward_det_workspace_bytes(int NB, int H, int W) {
  if (NB < 1 || NB > 65535 || os2d_det_log2_addends(H, W) < 0) return 0;
  return os2d_det_workspace_bytes(NB, H, W);
}

int os2d_train_decode_backward_det(const float* corr, const float* params, const float* dcls, const float* dcls_det, const float* dloc,
                                   int NB, int H, int W, int P, int inverse, int stride, int rec_field, float* dcorr, float* dparams,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  os2d_clear_error();
  const int rc = check_decode("os2d_train_decode_backward_det", corr && params && dcorr && dparams && workspace, NB, H, W, P, stride, rec_field);
  if (rc) return rc;
  if (os2d_det_log2_addends(H, W) < 0)
    return OS2D_REFUSE(-3, "os2d_train_decode_backward_det: H*W=%lld > 2^%d locations: the fixed-point step would exceed 2^-30 of a pair's "
                       "largest addend", (long long)H * W, OS2D_DET_MAX_LOG2 - 2);
  if (((uintptr_t)workspace & 7) != 0) return OS2D_REFUSE(-1, "os2d_train_decode_backward_det: workspace is not 8-byte aligned");
  const size_t need = os2d_det_workspace_bytes(NB, H, W);
  if (workspace_bytes < need) return OS2D_REFUSE(-2, "os2d_train_decode_backward_det: workspace %zu bytes < %zu", workspace_bytes, need);
  return os2d_decode_backward_det_launch(corr, params, dcls, dcls_det, dloc, NB, H, W, P, inverse, stride, rec_field, dcorr, dparams,
                                         workspace, os2d_stream(stream));
}

int os2d_train_params_backward(const float* dparams, int NB, int P, int H, int W, float* dy, float* dbias, void* stream) {
  os2d_clear_error();
  if (null_pointer("os2d_train_params_backward", dparams && dy)) return -1;
  if ((P != 6 && P != 4) || !shape_ok(NB, H, W) || (size_t)NB * P > 65535)
    return OS2D_REFUSE(-1, "os2d_train_params_backward: bad shape NB=%d P=%d H=%d W=%d", NB, P, H, W);
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
  const int C = layer_channels(layer);
  if (C == 0) return OS2D_REFUSE(-1, "os2d_train_bn_relu_backward: layer %d has no BatchNorm (1 or 2)", layer);
  if (null_pointer("os2d_train_bn_relu_backward", dh && h && gamma && beta && running_var && dy)) return -1;
  if (!shape_ok(NB, H, W) || (size_t)NB * C > 65535 || !(eps >= 0.f))
    return OS2D_REFUSE(-1, "os2d_train_bn_relu_backward: bad shape NB=%d H=%d W=%d eps=%g", NB, H, W, (double)eps);
  const int PL = os2d_plane(H, W);
  hipLaunchKernelGGL(bn_relu_mask_kernel, dim3(blocks(PL), NB * C), dim3(256), 0, os2d_stream(stream), dh, h, gamma, running_var, eps, C, H, W,
                     PL, dy);
  int rc = os2d_launched("bn_relu_mask_kernel");
  if (rc || (!dgamma && !dbeta && !dbias)) return rc;
  hipLaunchKernelGGL(bn_relu_sums_kernel, dim3(C), dim3(256), 0, os2d_stream(stream), dh, h, gamma, beta, running_var, eps, NB, C, H, W, PL,
                     dgamma, dbeta, dbias);
  return os2d_launched("bn_relu_sums_kernel");
}

size_t os2d_train_conv_data_workspace_floats(int layer, int P) {
  Layer L;
  if (!layer_shape(layer, P, &L)) return 0;
  return (size_t)L.cout * L.cin * L.ks * L.ks;
}

size_t os2d_train_conv_data_workspace_floats_ex(int arith, int layer, int P, int NB) {
  const size_t wf = os2d_train_conv_data_workspace_floats(layer, P);
  if ((arith != 0 && arith != 1) || wf == 0 || (arith && NB < 1)) return 0;
  return wf + conv_words(arith, NB);
}

int os2d_train_conv_backward_data_ex(int arith, int layer, int P, const float* w, const float* dy, int NB, int H, int W, float* dx,
                                     float* workspace, size_t workspace_floats, void* stream) {
  os2d_clear_error();
  const char* who = "os2d_train_conv_backward_data";
  Layer L;
  if (bad_arith(who, arith) || bad_layer(who, layer, P, false, &L) || null_pointer(who, w && dy && dx && workspace) ||
      bad_conv_shape(who, NB, H, W, 1))
    return -1;
  const size_t wf = (size_t)L.cout * L.cin * L.ks * L.ks;
  if (workspace_too_small(who, workspace_floats, wf + conv_words(arith, NB))) return -2;      // the flipped filters, then the words
  hipLaunchKernelGGL(flip_weights_kernel, dim3(blocks(wf)), dim3(256), 0, os2d_stream(stream), w, L.cout, L.cin, L.ks * L.ks, workspace);
  const int rc = os2d_launched("flip_weights_kernel");
  if (rc) return rc;
  return os2d_gemm_conv_data(arith, workspace, dy, dx, L.cout, L.cin, L.ks, NB, H, W, reinterpret_cast<unsigned*>(workspace + wf),
                             os2d_stream(stream));
}

int os2d_train_conv_backward_data(int layer, int P, const float* w, const float* dy, int NB, int H, int W, float* dx,
                                  float* workspace, size_t workspace_floats, void* stream) {
  return os2d_train_conv_backward_data_ex(0, layer, P, w, dy, NB, H, W, dx, workspace, workspace_floats, stream);
}

// the forward convolution of a layer whose BatchNorm takes batch statistics
size_t os2d_train_conv_forward_workspace_floats(int arith, int layer, int P, int NB) {
  Layer L;
  if ((arith != 0 && arith != 1) || layer_channels(layer) == 0 || !layer_shape(layer, P, &L) || NB < 1) return 0;
  return conv_forward_floats(arith, NB);
}

int os2d_train_conv_forward(int arith, int layer, int P, const float* w, const float* bias, const float* x, int NB, int H, int W, float* z,
                            float* workspace, size_t workspace_floats, void* stream) {
  os2d_clear_error();
  const char* who = "os2d_train_conv_forward";
  Layer L;
  if (bad_arith(who, arith) || bad_layer(who, layer, P, true, &L) || null_pointer(who, w && bias && x && z && workspace) ||
      bad_conv_shape(who, NB, H, W, L.cout))
    return -1;
  if (workspace_too_small(who, workspace_floats, conv_forward_floats(arith, NB))) return -2;
  return os2d_gemm_conv_forward(arith, w, bias, x, input_planes(layer), z, L.cout, L.cin, L.ks, NB, H, W,
                                reinterpret_cast<unsigned*>(workspace), os2d_stream(stream));
}

size_t os2d_train_conv_weight_slice_floats(int layer, int P) { return os2d_train_conv_data_workspace_floats(layer, P); }

size_t os2d_train_conv_weight_slice_floats_ex(int arith, int layer, int P) {
  const size_t slice = os2d_train_conv_weight_slice_floats(layer, P);
  if ((arith != 0 && arith != 1) || slice == 0) return 0;
  return slice + weight_words_room(arith);
}

int os2d_train_conv_backward_weight_ex(int arith, int layer, int P, const float* x, const float* dy, int NB, int H, int W, float* dw,
                                       float* workspace, size_t workspace_floats, void* stream) {
  os2d_clear_error();
  const char* who = "os2d_train_conv_backward_weight";
  Layer L;
  if (bad_arith(who, arith) || bad_layer(who, layer, P, false, &L) || null_pointer(who, x && dy && dw && workspace) ||
      bad_conv_shape(who, NB, H, W, 0))
    return -1;
  const size_t slice = (size_t)L.cout * L.cin * L.ks * L.ks;
  const long long K = (long long)NB * os2d_plane(H, W);
  if (K > 0x7fffffffLL) return OS2D_REFUSE(-3, "os2d_train_conv_backward_weight: NB * PLANE = %lld positions exceed the 32-bit index", K);
  const size_t room = slice + weight_words_room(arith);
  const int ks = kstep(arith);
  long long splits = (long long)(workspace_floats / room);
  if (splits < 1)
    return OS2D_REFUSE(-2, "os2d_train_conv_backward_weight: workspace %zu floats < one slice of %zu", workspace_floats, room);
  if (splits > 64) splits = 64;
  if (splits > (K + ks - 1) / ks) splits = (K + ks - 1) / ks;
  const int ksplit = (int)(((K + splits - 1) / splits + ks - 1) / ks * ks);
  splits = (K + ksplit - 1) / ksplit;
  float* part = workspace + weight_words_room(arith);
  const int rc = os2d_gemm_conv_weight(arith, x, input_planes(layer), dy, part, L.cout, L.cin, L.ks, NB, H, W, (int)splits, ksplit,
                                       reinterpret_cast<unsigned*>(workspace), os2d_stream(stream));
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
  if (null_pointer("os2d_train_norm225_backward", corr && dxn && dcorr)) return -1;
  if (!shape_ok(NB, H, W) || NB > 65535) return OS2D_REFUSE(-1, "os2d_train_norm225_backward: bad shape NB=%d H=%d W=%d", NB, H, W);
  hipLaunchKernelGGL(norm225_backward_kernel, dim3(blocks((size_t)H * W), NB), dim3(256), 0, os2d_stream(stream), corr, dxn, H, W,
                     os2d_plane(H, W), dcorr);
  return os2d_launched("norm225_backward_kernel");
}

size_t os2d_train_corr_workspace_floats(int A, int C, int H, int W) {
  if (A < 1 || C < 1 || H < 1 || W < 1) return 0;
  return corr_workspace(0, A, 0, C, (size_t)H * W).total;
}

size_t os2d_train_corr_workspace_floats_ex(int arith, int A, int B, int C, int H, int W) {
  if ((arith != 0 && arith != 1) || os2d_train_corr_workspace_floats(A, C, H, W) == 0 || (arith && B < 1)) return 0;
  return corr_workspace(arith, A, B, C, (size_t)H * W).total;
}

int os2d_train_corr_backward_ex(int arith, const float* fm, const float* qp, const float* dcorr, int A, int B, int C, int H, int W,
                                float* dfm, float* dq, float* workspace, size_t workspace_floats, void* stream) {
  os2d_clear_error();
  const char* who = "os2d_train_corr_backward";
  if (bad_arith(who, arith) || null_pointer(who, fm && qp && dcorr && workspace)) return -1;
  if (A < 1 || B < 1 || C < 1 || H < 1 || W < 1 || A > 65535 || B > 65535)
    return OS2D_REFUSE(-1, "os2d_train_corr_backward: bad shape A=%d B=%d C=%d H=%d W=%d", A, B, C, H, W);
  const long long HW = (long long)H * W;
  if ((long long)B * OS2D_K > 0x7fffffffLL || (long long)A * HW > 0x7fffffffLL)
    return OS2D_REFUSE(-3, "os2d_train_corr_backward: reduction length exceeds the 32-bit index");
  const CorrWorkspace ws = corr_workspace(arith, A, B, C, (size_t)HW);
  if (workspace_too_small(who, workspace_floats, ws.total)) return -2;
  if (!dfm && !dq) return 0;
  hipStream_t st = os2d_stream(stream);
  float* rinv = workspace;
  float* dfh = workspace + ws.dfh;
  unsigned* words = reinterpret_cast<unsigned*>(workspace + ws.words);
  hipLaunchKernelGGL(image_norm_kernel, dim3(blocks(HW), A), dim3(256), 0, st, fm, C, (int)HW, rinv);
  int rc = os2d_launched("image_norm_kernel");
  if (rc) return rc;
  if (arith && (rc = os2d_gemm_corr_maxima(dcorr, A, B, (int)HW, words, st))) return rc;
  if (dfm) {
    if ((rc = os2d_gemm_corr_image(arith, qp, dcorr, A, B, C, (int)HW, dfh, words, st))) return rc;
    hipLaunchKernelGGL(image_norm_backward_kernel, dim3(blocks(HW), A), dim3(256), 0, st, fm, dfh, C, (int)HW, dfm);
    if ((rc = os2d_launched("image_norm_backward_kernel"))) return rc;
  }
  if (dq) rc = os2d_gemm_corr_class(arith, fm, rinv, dcorr, A, B, C, (int)HW, dq, words, st);
  return rc;
}

int os2d_train_corr_backward(const float* fm, const float* qp, const float* dcorr, int A, int B, int C, int H, int W, float* dfm,
                             float* dq, float* workspace, size_t workspace_floats, void* stream) {
  return os2d_train_corr_backward_ex(0, fm, qp, dcorr, A, B, C, H, W, dfm, dq, workspace, workspace_floats, stream);
}

int os2d_train_class_backward(const float* q15, const float* dq, int B, int C, float* const* dsrcs, const int* sizes,
                              float* workspace, size_t workspace_floats, void* stream) {
  os2d_clear_error();
  if (null_pointer("os2d_train_class_backward", q15 && dq && dsrcs && sizes && workspace)) return -1;
  if (B < 1 || C < 1 || B > 65535) return OS2D_REFUSE(-1, "os2d_train_class_backward: bad shape B=%d C=%d", B, C);
  if (workspace_too_small("os2d_train_class_backward", workspace_floats, (size_t)B * C * OS2D_K)) return -2;
  hipLaunchKernelGGL(class_norm_backward_kernel, dim3(1, B), dim3(256), 0, os2d_stream(stream), q15, dq, C, workspace);
  int rc = os2d_launched("class_norm_backward_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(class_resize_backward_kernel, dim3(blocks(C), B), dim3(256), 0, os2d_stream(stream), workspace, C, dsrcs, sizes);
  return os2d_launched("class_resize_backward_kernel");
}

}  // extern "C"
