// The range plan of the split-fp16 ("f16x3") path on the device: eval-mode BatchNorm fold, the bounds of the layer outputs and
// the activation, unit and weight exponents of TransformationNet.range_plan (os2d_amd/modeling/head.py), from the raw fp32
// parameters, in float64 throughout.  Three launches, one per layer, because layer 2 needs every bound and exponent of layer 1
// and layer 3 the exponents of layer 2; no host wait, no atomics.
//
// One work-group per output row.  Every reduction of a row runs in a fixed order - per-lane partial sums, an exchange inside the
// wave, the waves' results through LDS - so two calls on the same parameters give the same bits, the float64 bounds included.
// The arithmetic restates the reference operation for operation (no fused multiply-adds); what differs is the order of the sums.
// The scalar rules and the layout of the two result buffers: range_plan_math.h.  The C ABI (include/os2d_train.h:
// os2d_train_range_plan*) is at the end of the unit.
#include "../../include/os2d_train.h"
#include "../csrc/os2d_common.h"   // the layer table, OS2D_RNORM_EXP
#include "range_plan_math.h"

namespace {
using namespace os2d_rp;

constexpr int RP_THR = 256, RP_WAVES = RP_THR / 64;
constexpr Os2dLayer L1 = os2d_layer(1), L2 = os2d_layer(2), L3 = os2d_layer(3);
static_assert(L1.cout == RP_C1 && L2.cout == RP_C2 && L3.cout <= RP_P3 && L2.cin <= RP_THR, "layout of range_plan_math.h");

// torch.amax: a NaN on either side stays
__device__ __forceinline__ double rp_nanmax(double a, double b) { return a != a ? a : (b > a || b != b) ? b : a; }

// Sum / maximum over the work-group, the same bits in every thread.  The butterfly adds lane pairs (commutative: both lanes of a
// pair get the same bits), then every thread combines the waves' results in wave order.  `lds`: RP_WAVES doubles, free again on return.
template <bool MAX>
__device__ __forceinline__ double rp_block_reduce(double v, double* lds) {
  for (int off = 32; off; off >>= 1) {
    const double o = __shfl_xor(v, off);
    v = MAX ? rp_nanmax(v, o) : v + o;
  }
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = lds[0];
  for (int w = 1; w < RP_WAVES; ++w) r = MAX ? rp_nanmax(r, lds[w]) : r + lds[w];
  __syncthreads();
  return r;
}

// scale and folded bias of output row o (head.py:619-629, as TransformationNet._folded): s = bn_w / sqrt(var + eps),
// b' = (b - mean) * s + bn_b; without BatchNorm 1 and b
__device__ __forceinline__ double rp_fold(const float* bn_w, const float* bn_b, const float* bn_mean, const float* bn_var, double eps,
                                          const float* b, int o, double* bias) {
#pragma clang fp contract(off)
  if (!bn_w) {
    *bias = (double)b[o];
    return 1.0;
  }
  const double s = (double)bn_w[o] / sqrt((double)bn_var[o] + eps);
  *bias = ((double)b[o] - (double)bn_mean[o]) * s + (double)bn_b[o];
  return s;
}

// layer 1: B1[o] = 7 * ||w1[o] * s||_2 + |b'|, e1 = out_exp(B1), wexp1 = weight_exp(max |w1[o] * s| * 2^-rnorm_exp)
__global__ __launch_bounds__(RP_THR) void range_plan_layer1_kernel(const float* __restrict__ w, const float* __restrict__ b,
                                                                   const float* __restrict__ bn_w, const float* __restrict__ bn_b,
                                                                   const float* __restrict__ bn_mean, const float* __restrict__ bn_var,
                                                                   double eps, int* __restrict__ exps, double* __restrict__ bounds) {
#pragma clang fp contract(off)
  __shared__ double lds[RP_WAVES];
  constexpr int N = L1.cin * L1.ks * L1.ks;
  const int o = blockIdx.x;
  double bias;
  const double s = rp_fold(bn_w, bn_b, bn_mean, bn_var, eps, b, o, &bias);
  const float* row = w + (size_t)o * N;
  double ss = 0.0, m = 0.0;
  for (int i = threadIdx.x; i < N; i += RP_THR) {
    const double wf = (double)row[i] * s;
    ss += wf * wf;
    m = rp_nanmax(m, fabs(wf));
  }
  ss = rp_block_reduce<false>(ss, lds);
  m = rp_block_reduce<true>(m, lds);
  if (threadIdx.x == 0) {
    const double bound = (double)L1.ks * sqrt(ss) + fabs(bias);
    const int e = out_exp(bound);
    bounds[RP_B1 + o] = bound;
    exps[RP_E1 + o] = e;
    exps[RP_UNIT + o] = e - 15;
    exps[RP_WEXP1 + o] = weight_exp(ldexp(m, -OS2D_RNORM_EXP));
  }
}

// layer 2: l1 = sum_c B1[c] * ||w2'[o,c]||_1, l2 = 5 * ||B1||_2 * ||w2'[o]||_2, B2[o] = min(l1, l2) + |b'|, e2 = out_exp(B2),
// wexp2 = weight_exp(max_c,tap |w2'[o,c]| * 2^-e1[c]).  Thread c owns input channel c (its 25 taps): the product with B1[c] is
// taken per channel, as the reference does (an infinite bound times an all-zero channel is NaN there too).
__global__ __launch_bounds__(RP_THR) void range_plan_layer2_kernel(const float* __restrict__ w, const float* __restrict__ b,
                                                                   const float* __restrict__ bn_w, const float* __restrict__ bn_b,
                                                                   const float* __restrict__ bn_mean, const float* __restrict__ bn_var,
                                                                   double eps, int* __restrict__ exps, double* __restrict__ bounds) {
#pragma clang fp contract(off)
  __shared__ double lds[RP_WAVES];
  constexpr int TAPS = L2.ks * L2.ks;
  const int o = blockIdx.x, c = threadIdx.x;
  double bias;
  const double s = rp_fold(bn_w, bn_b, bn_mean, bn_var, eps, b, o, &bias);
  double l1 = 0.0, ss = 0.0, bb = 0.0, m = 0.0;
  if (c < L2.cin) {
    const float* taps = w + ((size_t)o * L2.cin + c) * TAPS;
    double a1 = 0.0;
    for (int t = 0; t < TAPS; ++t) {
      const double wf = (double)taps[t] * s;
      a1 += fabs(wf);
      ss += wf * wf;
      m = rp_nanmax(m, fabs(wf));
    }
    const double b1 = bounds[RP_B1 + c];
    l1 = a1 * b1;
    bb = b1 * b1;
    m = ldexp(m, -exps[RP_E1 + c]);
  }
  l1 = rp_block_reduce<false>(l1, lds);
  ss = rp_block_reduce<false>(ss, lds);
  bb = rp_block_reduce<false>(bb, lds);
  m = rp_block_reduce<true>(m, lds);
  if (threadIdx.x == 0) {
    const double l2 = (double)L2.ks * sqrt(bb) * sqrt(ss);
    const double least = (l1 != l1 || l2 != l2) ? l1 + l2 : l1 < l2 ? l1 : l2;      // torch.minimum: a NaN stays
    const double bound = least + fabs(bias);
    bounds[RP_B2 + o] = bound;
    exps[RP_E2 + o] = out_exp(bound);
    exps[RP_WEXP2 + o] = weight_exp(m);
  }
}

// layer 3: wexp3 = weight_exp(max_c,tap |w3[o,c]| * 2^-e2[c]); the rows past P are zero
__global__ __launch_bounds__(RP_THR) void range_plan_layer3_kernel(const float* __restrict__ w, int P, int* __restrict__ exps) {
  __shared__ double lds[RP_WAVES];
  constexpr int TAPS = L3.ks * L3.ks, N = L3.cin * TAPS;
  const int o = blockIdx.x;
  double m = 0.0;
  if (o < P)
    for (int i = threadIdx.x; i < N; i += RP_THR) m = rp_nanmax(m, ldexp(fabs((double)w[(size_t)o * N + i]), -exps[RP_E2 + i / TAPS]));
  m = rp_block_reduce<true>(m, lds);
  if (threadIdx.x == 0) exps[RP_WEXP3 + o] = o < P ? weight_exp(m) : 0;
}
}  // namespace


extern "C" size_t os2d_train_range_plan_ints(void) { return os2d_rp::RP_INTS; }
extern "C" size_t os2d_train_range_plan_doubles(void) { return os2d_rp::RP_DOUBLES; }

extern "C" int os2d_train_range_plan(int P, const float* w1, const float* b1, const float* bn1_weight, const float* bn1_bias,
                                     const float* bn1_running_mean, const float* bn1_running_var, double bn1_eps, const float* w2,
                                     const float* b2, const float* bn2_weight, const float* bn2_bias, const float* bn2_running_mean,
                                     const float* bn2_running_var, double bn2_eps, const float* w3, int* exps, double* bounds, void* stream) {
  // BatchNorm folding takes all four of weight / bias / running_mean / running_var, or none
  const auto bn_all_or_none = [](const float* w, const float* b, const float* m, const float* v) { return (w && b && m && v) || !(w || b || m || v); };
  if (!w1 || !b1 || !w2 || !b2 || !w3 || !exps || !bounds) return OS2D_REFUSE(-1, "os2d_train_range_plan: null pointer");
  if (P != 6 && P != 4) return OS2D_REFUSE(-1, "os2d_train_range_plan: bad P %d (6 or 4)", P);
  if (!bn_all_or_none(bn1_weight, bn1_bias, bn1_running_mean, bn1_running_var))
    return OS2D_REFUSE(-1, "os2d_train_range_plan: BatchNorm of layer 1 needs all four of weight/bias/running_mean/running_var");
  if (!bn_all_or_none(bn2_weight, bn2_bias, bn2_running_mean, bn2_running_var))
    return OS2D_REFUSE(-1, "os2d_train_range_plan: BatchNorm of layer 2 needs all four of weight/bias/running_mean/running_var");
  if ((reinterpret_cast<uintptr_t>(bounds) & 7) || (reinterpret_cast<uintptr_t>(exps) & 3))
    return OS2D_REFUSE(-1, "os2d_train_range_plan: bounds must be 8-byte, exps 4-byte aligned");
  const hipStream_t st = os2d_stream(stream);
  hipLaunchKernelGGL(range_plan_layer1_kernel, dim3(RP_C1), dim3(RP_THR), 0, st, w1, b1, bn1_weight, bn1_bias, bn1_running_mean, bn1_running_var,
                     bn1_eps, exps, bounds);
  int rc = os2d_launched("range_plan_layer1");
  if (rc) return rc;
  hipLaunchKernelGGL(range_plan_layer2_kernel, dim3(RP_C2), dim3(RP_THR), 0, st, w2, b2, bn2_weight, bn2_bias, bn2_running_mean, bn2_running_var,
                     bn2_eps, exps, bounds);
  rc = os2d_launched("range_plan_layer2");
  if (rc) return rc;
  hipLaunchKernelGGL(range_plan_layer3_kernel, dim3(RP_P3), dim3(RP_THR), 0, st, w3, P, exps);
  return os2d_launched("range_plan_layer3");
}
