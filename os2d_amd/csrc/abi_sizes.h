// What abi.hip (the per-stage entry points) and head_call.hip (the head call) share: the shape check of a head call and the byte
// size of every buffer that one entry point reports and another carves or checks - each written once.  Host code, static: no
// symbol leaves a unit.
#pragma once
#include "os2d_common.h"

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline bool aligned_to(size_t a, const void* p, const void* q = nullptr, const void* r = nullptr) {
  return !((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(r)) & (a - 1));
}

static inline bool head_args_ok(int A, int B, int C, int H, int W, int P) {
  if (A < 1 || B < 1 || C < 1 || H < 1 || W < 1 || (P != 6 && P != 4))
    return OS2D_REFUSE(false, "bad head shape A=%d B=%d C=%d H=%d W=%d P=%d (need A,B,C,H,W>=1, P in {6,4})", A, B, C, H, W, P);
  if (W > OS2D_MAX_W)
    return OS2D_REFUSE(false, "feature map width %d > %d: beyond what the transform planner of the 7x7 layer tiles (images wider than %d px "
                       "at stride 16 are not supported)", W, OS2D_MAX_W, OS2D_MAX_W * 16);
  if (H > OS2D_MAX_H)
    return OS2D_REFUSE(false, "feature map height %d > %d: beyond what the transform planner of the 7x7 layer tiles (images taller than %d px "
                       "at stride 16 are not supported)", H, OS2D_MAX_H, OS2D_MAX_H * 16);
  return true;
}

// split class operand of ONE class (corr_f16x3.hip: qs [C/8 groups][hi|lo][256 rows] units of 16 B)
static inline size_t class_split_bytes(int C) { return (size_t)os2d_corr_groups(C) * 2 * OS2D_QROWS * 16; }
// split image features of A images: 16 B per (group, hi|lo, cell)
static inline size_t fm_split_bytes(int A, int C, size_t HW) { return (size_t)A * os2d_corr_groups(C) * 2 * HW * 16; }
// split-half blocked (SHB) activations of `channels` planes: [groups of 8][hi|lo][PLANE] units of 16 B
static inline size_t shb_bytes(int channels, int H, int W) { return (size_t)((channels + 7) / 8) * 2 * os2d_plane(H, W) * 16; }
// workspace of the stand-alone correlation entry points: sumsq | split image features, and with B > 0 (the packed form) | the 64-bit
// sums of A * B maps; byte offsets and the total
struct CorrWorkspace {
  size_t sumsq, fs, sumfx, total;
};
static inline CorrWorkspace corr_workspace(int A, int B, int C, int H, int W) {
  const size_t HW = (size_t)H * W;
  CorrWorkspace w = {0, align_up((size_t)A * HW * sizeof(float), 256), 0, 0};
  w.total = w.fs + fm_split_bytes(A, C, HW);
  if (B > 0) w.sumfx = align_up(w.total, 256), w.total = w.sumfx + (size_t)A * B * HW * sizeof(unsigned long long);
  return w;
}
static inline size_t nms_workspace_bytes(int NC, int N) { return (size_t)NC * N * 4 * sizeof(float); }
