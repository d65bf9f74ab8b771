// What the host checks of os2d_amd/csrc/dft_mfma.h share (dft_mfma_check.cpp, dft_radix2_check.cpp, dft_chain_check.cpp): the
// hardware hooks of the header on the SPMD emulator (spmd_emu.h) - the kernel source itself is compiled unchanged - and the
// helpers of their float64 references.  The includer sets DFT_EMU_POLICY (0: the smallest transform per map, 1: the canonical
// sizes) before the include where the default policy of the check is not 0.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "spmd_emu.h"

#define OS2D_HOST_EMU 1
#ifndef DFT_EMU_POLICY
#define DFT_EMU_POLICY 0
#endif
static int emu_dft_policy = DFT_EMU_POLICY;
#define DFT_DEV static inline
#define DFT_TID emu::tid()
#define DFT_BID emu::bid()
#define DFT_GRID emu::grid()
#define DFT_LDS emu::lds()
#define DFT_BARRIER() emu::group_barrier()
#define DFT_MFMA(a, b, c) emu::mfma_32x32x16_f16(a, b, c)
#define DFT_SHFL_XOR(v, m) emu::shfl_xor(v, m)
#define DFT_SHFL_XOR_U32(v, m) emu::shfl_xor_u32(v, m)
#define DFT_BALLOT(p) emu::ballot(p)
#define DFT_FLAG int*
#define DFT_FLAG_SET(f) ((f) != nullptr)
#define DFT_RAISE(p) (*(p) = 1)
#define DFT_UNIFORM(x) (x)
#include "dft_mfma.h"

// The spectra layouts, stated independently of the kernels' helper (include/os2d_hip.h): blocks of 64 pairs,
// [pair / 64][quad of bins][pair % 64 (last block: what is left)][channel][4 bins][re | im]
static inline size_t spec_index(int bin, int pair, int NBT, int nquads, int chans, int c) {
  const int blk = pair / 64, in_blk = pair % 64, held = std::min(64, NBT - 64 * blk);
  return ((((size_t)blk * 64 * nquads + (size_t)(bin / 4) * held + in_blk) * chans + c) * 4 + (bin & 3)) * 2;
}

// double [n][2] = (cos, sin) of -2 pi m / n
static inline std::vector<double> table(int n) {
  std::vector<double> t(2 * n);
  for (int m = 0; m < n; ++m) {
    t[2 * m] = std::cos(-2.0 * M_PI * m / n);
    t[2 * m + 1] = std::sin(-2.0 * M_PI * m / n);
  }
  return t;
}

static inline double frand(unsigned& s) {
  s = s * 1664525u + 1013904223u;
  return ((s >> 8) & 0xffffff) / double(1 << 24);
}

// the activation planes of the 5x5 layer (os2d_ws / os2d_base / os2d_plane of os2d_common.h, stated on their own): row pitch,
// first cell of the map, cells of a plane
static inline int ws_of(int W) { return W + 3; }
static inline int base_of(int W) { return os2d_dft::dft_round_up(3 * ws_of(W) + 3, 4); }
static inline int plane_of(int H, int W) { return os2d_dft::dft_round_up(base_of(W) + (H + 3) * ws_of(W) + 3, 64); }
