// The fixed-point grid of the order-independent d corr scatter (os2d_train_decode_backward_det, include/os2d_train.h): one
// rule, used by the host helper os2d_train_decode_det_exponent and by the scatter and convert kernels of decode_backward.hip.
//
// Per pair, m = the largest |dcls + dcls_det| over its locations (the fp32 sum the kernel forms), read from the pair's word
// as an fp32 bit pattern.  An addend of the scatter is wsc * (a bilinear weight in [0, 1]) with |wsc| = |gsum| / 121 (one
// fp32 rounding each), so |addend| <= m / 121 * (1 + 2^-21) < m / 64.  One cell of one channel receives at most 4 addends per
// location - the 4 taps of the channel's own sample point, which coincide under the clamp - hence at most 4 H W addends.
//
// Rule: L = ceil(log2(4 H W)), e = 60 - L - floor(log2 m), i.e. m 2^e lies in [2^(60-L), 2^(61-L)).  Headroom: a cell's exact
// integer sum is bounded by 4 H W * (m / 64 * 2^e + 1/2) < 2^L * (2^(55-L) + 1/2) = 2^55 + 2^(L-1) < 2^56: seven binades below
// the overflow of a signed 64-bit word; the weaker bound the interface states, 2^(floor(log2 m)+1) 2^e 4 H W <= 2^61 < 2^62,
// does not even use the 1/121.  Resolution: the grid step is 2^-e <= m 2^(L-60); against the pair's largest possible addend
// m / 121 that is 121 * 2^(L-60), which stays at or below 2^-30 exactly while L <= 23, i.e. H W <= 2^21.  Larger maps are
// refused (at the training shape 38 x 38: L = 13, step <= 2^-40 of the largest addend).
//
// The scaled addend (double)a * 2^e is exact (a has 24 significant bits, 2^e is a double for every e the rule gives:
// -90 <= e <= 207), and so is every partial sum: integers commute and associate.
#ifndef OS2D_TRAIN_DECODE_DET_H
#define OS2D_TRAIN_DECODE_DET_H

#include "../../include/os2d_train.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OS2D_DET_HD __host__ __device__
#else
#define OS2D_DET_HD
#endif

constexpr int OS2D_DET_MAX_LOG2 = 23;            // L at most: H W <= 2^21

// L = ceil(log2(4 H W)), or -1 for a shape the rule refuses
OS2D_DET_HD inline int os2d_det_log2_addends(int H, int W) {
  if (H < 1 || W < 1) return -1;
  const long long n = 4LL * H * W;
  int L = 2;
  while ((1LL << L) < n) ++L;
  return L <= OS2D_DET_MAX_LOG2 ? L : -1;
}

// e of a pair whose word is `bits`, L from os2d_det_log2_addends (>= 2); OS2D_TRAIN_DET_ZERO / _NONFINITE for the special words
OS2D_DET_HD inline int os2d_det_exponent(unsigned bits, int L) {
  if (bits == 0u) return OS2D_TRAIN_DET_ZERO;
  if (bits >= 0x7f800000u) return OS2D_TRAIN_DET_NONFINITE;
  int fl;                                        // floor(log2 m)
  if (bits >> 23) {
    fl = (int)(bits >> 23) - 127;
  } else {                                       // subnormal: m = bits * 2^-149
    int top = 22;
    while (!(bits >> top)) --top;
    fl = top - 149;
  }
  return 60 - L - fl;
}

// the workspace of the route (for a shape the rule accepts): the accumulator [NB,225,HW] of 64-bit sums, then the pair words
inline size_t os2d_det_acc_bytes(int NB, int H, int W) { return (size_t)NB * 225 * H * W * sizeof(long long); }
inline size_t os2d_det_workspace_bytes(int NB, int H, int W) {
  return (os2d_det_acc_bytes(NB, H, W) + (size_t)NB * sizeof(unsigned) + 255) / 256 * 256;
}

#if defined(__HIPCC__)
// ---- the launches of decode_backward.hip; the entry points of train.hip have checked the arguments.  The deterministic one
// clears `workspace` (os2d_det_workspace_bytes), takes the maxima, scatters and converts.  Not exports of the library: hidden.
#pragma GCC visibility push(hidden)
int os2d_decode_backward_launch(const float* corr, const float* params, const float* dcls, const float* dcls_det, const float* dloc, int NB,
                                int H, int W, int P, int inverse, int stride, int rec_field, float* dcorr, float* dparams,
                                hipStream_t stream);
int os2d_decode_backward_det_launch(const float* corr, const float* params, const float* dcls, const float* dcls_det, const float* dloc,
                                    int NB, int H, int W, int P, int inverse, int stride, int rec_field, float* dcorr, float* dparams,
                                    void* workspace, hipStream_t stream);
#pragma GCC visibility pop
#endif

#endif
