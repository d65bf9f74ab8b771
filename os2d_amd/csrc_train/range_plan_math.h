// The scalar rules of the split-fp16 range plan and the layout of its two result buffers, each written once for the kernels
// (range_plan.hip), the C ABI (os2d_train_range_plan) and a host program that includes this header on its own
// (tests/host/range_plan_math_check.cpp).  The float64 reference is TransformationNet.range_plan (os2d_amd/modeling/head.py),
// which takes floor(log2(x)); floor_log2 below reads the exponent field instead, so the two can differ only where the float64
// quotient lies within an ulp or two of a power of two.
#pragma once

#include <math.h>

#ifndef RP_HD
#ifdef __HIPCC__
#define RP_HD static inline __host__ __device__
#else
#define RP_HD static inline
#endif
#endif

namespace os2d_rp {

// ---- os2d_train_range_plan's int32 buffer: wexp1 [128] | e1 [128] | unit_exp [128] | wexp2 [64] | e2 [64] | wexp3 [8]
//   wexp<l>   weight_exp of layer l per output row (entries of wexp3 past P are zero)
//   e1, e2    out_exp of layers 1 and 2 = in_exp of layers 2 and 3
//   unit_exp  e1 - 15: the layer-1 output exponents in the "<= 1" convention
constexpr int RP_C1 = 128, RP_C2 = 64, RP_P3 = 8;      // rows of the three layers in the buffer (layer 3 padded to 8)
constexpr int RP_WEXP1 = 0, RP_E1 = RP_WEXP1 + RP_C1, RP_UNIT = RP_E1 + RP_C1, RP_WEXP2 = RP_UNIT + RP_C1, RP_E2 = RP_WEXP2 + RP_C2,
              RP_WEXP3 = RP_E2 + RP_C2, RP_INTS = RP_WEXP3 + RP_P3;
// ---- its float64 buffer: B1 [128] | B2 [64], the bounds of |conv1[o]| and |conv2[o]|
constexpr int RP_B1 = 0, RP_B2 = RP_B1 + RP_C1, RP_DOUBLES = RP_B2 + RP_C2;

constexpr int RP_EXP_CLAMP = 60;

// exact floor(log2(x)) of a finite x > 0, clamped to [-60, 60]; 0 for zero, negative, NaN and Inf
RP_HD int floor_log2(double x) {
  if (!(x > 0.0) || x > 1.7976931348623157e308) return 0;
  int e;
  frexp(x, &e);      // x = m * 2^e with m in [0.5, 1), subnormals included
  e -= 1;
  return e < -RP_EXP_CLAMP ? -RP_EXP_CLAMP : e > RP_EXP_CLAMP ? RP_EXP_CLAMP : e;
}
// exponent that puts an activation bound at <= 2^15 (both comparisons are false for NaN; 32768 / Inf = 0 gives 0)
RP_HD int out_exp(double bound) { return bound > 0.0 ? floor_log2(32768.0 / fmax(bound, 1e-300)) : 0; }
// largest exponent that keeps a weight row's maximum <= 16384
RP_HD int weight_exp(double amax) { return amax > 0.0 ? floor_log2(16384.0 / fmax(amax, 1e-300)) : 0; }

}  // namespace os2d_rp
