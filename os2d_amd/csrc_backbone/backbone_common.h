// libos2d_backbone.so: the arithmetic and the launch geometry that its kernels share (include/os2d_backbone.h).
#pragma once
#include "../csrc_shared/abi_common.h"
#include "../../include/os2d_backbone.h"

constexpr int BB_THREADS = 256;                       // threads of every work-group
constexpr int BB_MIN_LANES_LOG2 = 4;                  // a channel row is shared by 16 ... 256 lanes of a work-group
constexpr int BB_MAX_LANES_LOG2 = 8;
constexpr long long BB_MAX_ROWS = (1ll << 31) - 1;    // N * C
constexpr long long BB_MAX_PLANE = 1ll << 30;         // HW
constexpr long long BB_MAX_ELEMENTS = 1ll << 40;      // N * C * HW

// one folded BatchNorm: ONE rounding
__device__ __forceinline__ float bb_bn(float x, float s, float t) { return __builtin_fmaf(x, s, t); }

// torch.relu: a NaN is not below zero and stays
__device__ __forceinline__ float bb_relu_nan(float v) { return v < 0.0f ? 0.0f : v; }

// torch's pooling maximum: a NaN wins and then stays (no later value is above it)
__device__ __forceinline__ float bb_max_nan(float m, float v) { return (v > m || v != v) ? v : m; }

static inline bool bb_misaligned(const void* p, size_t a) { return (reinterpret_cast<size_t>(p) & (a - 1)) != 0; }

// do [a, a + na) and [b, b + nb) bytes meet?
static inline bool bb_bytes_meet(const void* a, size_t na, const void* b, size_t nb) {
  const size_t pa = reinterpret_cast<size_t>(a), pb = reinterpret_cast<size_t>(b);
  return pa < pb + nb && pb < pa + na;
}

// do [a, a + n) and [b, b + n) floats share a byte?
static inline bool bb_overlap(const float* a, const float* b, long long n) {
  return bb_bytes_meet(a, (size_t)n * sizeof(float), b, (size_t)n * sizeof(float));
}

// the work-groups of a launch over `tiles` tiles: every tile has one when there are few, else the kernel strides
static inline unsigned bb_groups(long long tiles) { return (unsigned)(tiles < OS2D_BACKBONE_MAX_GROUPS ? tiles : OS2D_BACKBONE_MAX_GROUPS); }
