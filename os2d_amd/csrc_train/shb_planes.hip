// The bridge from the split-fp16 ("f16x3") training forward to the backward pass (include/os2d_train.h:
// os2d_train_planes_from_shb), gfx950.
//
// The f16x3 convolutions of libos2d_hip.so leave their activations in the split-half blocked layout (SHB, csrc/conv_f16x3.hip):
// [NB][ceil(channels / 8)][hi | lo][PLANE] units of 16 bytes = 8 channels of one plane cell as fp16, channel c stored as
// x * 2^exp[c], hi = rn16(x 2^exp), lo = rn16(x 2^exp - hi).  The backward kernels read fp32 planes [NB][channels][PLANE] in the
// zero-bordered plane geometry of csrc/os2d_common.h.  This kernel unpacks the one into the other:
//   planes[nb][c][n] = (float(hi) + float(lo)) * 2^-exp[c]      at interior cells,
//                    = +0                                        at every other cell, whatever the SHB buffer holds there,
// and planes channels .. out_channels - 1 are written as zeros (rnorm is [NB][226][PLANE] with a zero plane 225).  The result
// is exact for the halves a split produces (hi + lo of a split fp32 value fits 24 bits; v_ldexp_f32 only moves the exponent),
// so the backward differentiates exactly the values the forward multiplied with.
//
// Pure streaming, no LDS: a lane takes a run of RUN = 4 consecutive plane cells of one 8-channel group - 4 x 16 bytes of hi
// and of lo (the wave's four load instructions cover 4 KB of consecutive addresses between them) - and stores 16 bytes
// (4 cells) to each of the 8 channel planes: every store instruction of a wave writes 1 KB of consecutive addresses.  PLANE is
// a multiple of 64 floats, so every run is 16-byte aligned in every plane and no run straddles two planes.
#include <stdint.h>
#include <stdio.h>

#include "../../include/os2d_train.h"
#include "../csrc/os2d_common.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
constexpr int RUN = 4;          // plane cells per lane
constexpr int THREADS = 256;

// grid: x = blocks of THREADS runs of a plane, y = pair * OG + group; OG = ceil(out_channels / 8) >= G = ceil(channels / 8)
__global__ __launch_bounds__(THREADS) void planes_from_shb_kernel(const uint4* __restrict__ shb, const int* __restrict__ exp,
                                                                  float* __restrict__ planes, int G, int OG, int channels,
                                                                  int out_channels, int H, int W, int PLANE) {
  const int n0 = (blockIdx.x * THREADS + threadIdx.x) * RUN;
  if (n0 >= PLANE) return;
  const int nb = blockIdx.y / OG, g = blockIdx.y - nb * OG;
  bool interior[RUN];
#pragma unroll
  for (int k = 0; k < RUN; ++k) interior[k] = os2d_interior(n0 + k, H, W);
  f32x4 v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (g < G) {                  // (a group of extra planes only has nothing to read)
    const uint4* hi = shb + ((size_t)nb * G + g) * 2 * PLANE + n0;
    const uint4* lo = hi + PLANE;
    int e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = g * 8 + j < channels ? exp[g * 8 + j] : 0;
#pragma unroll
    for (int k = 0; k < RUN; ++k) {
      const half8 h = __builtin_bit_cast(half8, hi[k]), l = __builtin_bit_cast(half8, lo[k]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // a select, not a product with a mask: a pad cell or a padded channel may hold any bits (NaN halves included)
        const float x = ldexpf((float)h[j] + (float)l[j], -e[j]);
        v[j][k] = (interior[k] && g * 8 + j < channels) ? x : 0.f;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = g * 8 + j;
    if (c < out_channels) *reinterpret_cast<f32x4*>(planes + ((size_t)nb * out_channels + c) * PLANE + n0) = v[j];
  }
}

}  // namespace

extern "C" int os2d_train_planes_from_shb(const void* shb, const int* exp, int NB, int channels, int out_channels, int H, int W,
                                          float* planes, void* stream) {
  if (!shb || !exp || !planes) return os2d_refuse("os2d_train_planes_from_shb: null pointer");
  if (NB < 1 || channels < 1 || out_channels < channels || H < 1 || W < 1 || H > OS2D_MAX_H || W > OS2D_MAX_W) {
    os2d_set_error("os2d_train_planes_from_shb: bad shape NB=%d channels=%d out_channels=%d H=%d W=%d (need NB, channels, H, W >= 1, "
                   "out_channels >= channels, H <= %d, W <= %d)", NB, channels, out_channels, H, W, OS2D_MAX_H, OS2D_MAX_W);
    return -1;
  }
  const int G = (channels + 7) / 8, OG = (out_channels + 7) / 8;
  if ((long long)NB * OG > 65535) {     // one grid row per (pair, group)
    os2d_set_error("os2d_train_planes_from_shb: NB=%d x %d channel groups > 65535 grid rows", NB, OG);
    return -1;
  }
  if ((reinterpret_cast<uintptr_t>(shb) | reinterpret_cast<uintptr_t>(planes)) & 15)
    return os2d_refuse("os2d_train_planes_from_shb: shb and planes must be 16-byte aligned");
  const int PLANE = os2d_plane(H, W);   // a multiple of 64: whole runs
  const int runs = PLANE / RUN;
  hipLaunchKernelGGL(planes_from_shb_kernel, dim3((runs + THREADS - 1) / THREADS, NB * OG), dim3(THREADS), 0, os2d_stream(stream),
                     static_cast<const uint4*>(shb), exp, planes, G, OG, channels, out_channels, H, W, PLANE);
  return os2d_launched("planes_from_shb_kernel");
}
