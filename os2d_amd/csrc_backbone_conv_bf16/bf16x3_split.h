// The split of one fp32 value into three bf16 values, x == b0 + b1 + b2 (include/os2d_backbone_conv_bf16.h).
// Plain C++: it compiles for the host (tests/host/bf16x3_split_check.cpp) as well as for the device, where the rounding is the
// conversion instruction v_cvt_pk_bf16_f32 and here the same round-to-nearest-even in integers.
//
//   b0 = bf16(x)   b1 = bf16(x - b0)   b2 = bf16(x - b0 - b1)        bf16() rounds to nearest, ties to even
// Both differences are exact in fp32 (b0 holds the leading 8 bits of x, b1 the leading 8 of what is left), and the last rounding has
// at most 8 significant bits to round: the split is exact for every finite x whose last part does not fall below bf16's smallest
// subnormal, 2^-133 (which needs |x| < 2^-109).
//   - A finite x never has a non-finite part: where bf16(x) would be infinite (|x| >= 0x7F7F8000 as bits), b0 is x TRUNCATED to bf16, the
//     largest finite bf16, and b1, b2 follow from it as above.
//   - A non-finite x has b1 = b2 = 0: b0 = +-Inf, or the one quiet NaN 0x7FC0 for every NaN.
// bf16x3_split_x is the split of an ACTIVATION: the same, but a non-finite x stands in the LAST part alone (0, 0, b0).  Of the six products
// x2 w0, x1 w1, x0 w2, x1 w0, x0 w1, x0 w0 the last part of x meets only the leading part of w, which has the sign of w and is 0 only for
// w = 0: Inf * w is ONE product, +-Inf of the right sign, and Inf * 0 is NaN, as in fp32.  In the leading part Inf would also meet w1 and
// w2, whose signs are their own (Inf - Inf) and which are 0 for a w that bf16 holds exactly (Inf * 0).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define BF16X3_FN __host__ __device__ inline
#else
#define BF16X3_FN inline
#endif

BF16X3_FN uint32_t bf16x3_bits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}

BF16X3_FN float bf16x3_float(uint32_t u) {
  float x;
  memcpy(&x, &u, 4);
  return x;
}

// a bf16 as the fp32 of the same value
BF16X3_FN float bf16x3_widen(uint16_t b) { return bf16x3_float((uint32_t)b << 16); }

#if defined(__HIPCC__)
typedef float bf16x3_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x3_bf16x2 __attribute__((ext_vector_type(2)));
// two roundings in one v_cvt_pk_bf16_f32: lo in bits 0 ... 15, hi in bits 16 ... 31
__device__ __forceinline__ uint32_t bf16x3_round_pair(float lo, float hi) {
  bf16x3_f32x2 v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x3_bf16x2));
}
#endif

// round to nearest even of a value that is neither a NaN nor rounds to infinity
BF16X3_FN uint16_t bf16x3_round(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint16_t)(bf16x3_round_pair(x, 0.0f) & 0xFFFFu);
#else
  const uint32_t u = bf16x3_bits(x);
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
#endif
}

// does x need the rules for the top of the range: a NaN, an infinity, or a finite value that rounds to bf16's infinity
BF16X3_FN bool bf16x3_special(float x) { return (bf16x3_bits(x) & 0x7FFFFFFFu) >= 0x7F7F8000u; }

BF16X3_FN void bf16x3_split(float x, uint16_t* b0, uint16_t* b1, uint16_t* b2) {
  const uint32_t u = bf16x3_bits(x), mag = u & 0x7FFFFFFFu;
  if (mag >= 0x7F800000u) {                 // Inf, NaN
    *b0 = mag > 0x7F800000u ? (uint16_t)0x7FC0u : (uint16_t)(u >> 16);
    *b1 = 0;
    *b2 = 0;
    return;
  }
  const uint16_t p0 = mag >= 0x7F7F8000u ? (uint16_t)(u >> 16) : bf16x3_round(x);
  const float r1 = x - bf16x3_widen(p0);
  const uint16_t p1 = bf16x3_round(r1);
  const float r2 = r1 - bf16x3_widen(p1);
  *b0 = p0;
  *b1 = p1;
  *b2 = bf16x3_round(r2);
}

BF16X3_FN void bf16x3_split_x(float x, uint16_t* b0, uint16_t* b1, uint16_t* b2) {
  bf16x3_split(x, b0, b1, b2);
  if ((bf16x3_bits(x) & 0x7FFFFFFFu) >= 0x7F800000u) {
    *b2 = *b0;
    *b0 = 0;
  }
}
