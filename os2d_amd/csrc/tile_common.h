// What the matrix-shaped kernel units share (gfx950): the 16-byte vector types, LDS-DMA, the XCD-aware work-group order, the
// column-strip geometry of the 5x5 convolutions and the host's launch plumbing - once each, for the units that include this
// header (os2d_common.h stays what EVERY unit needs).  The 5x5 kernels (conv_mfma.hip, conv_f16x3.hip, conv3_f16x3.hip) must
// agree on the strip geometry index for index; they do by construction when all of them call the functions below.
//
// The integer code is compiled for the host by tests/host/tile_check.cpp (-DOS2D_HOST_EMU): no HIP runtime then, only the types
// and the geometry.
#pragma once
#ifdef OS2D_HOST_EMU
#define OS2D_PAD 3
#define TILE_DEV static inline
#define TILE_HD static inline
typedef float f32x16 __attribute__((ext_vector_type(16)));     // (os2d_common.h's, for the headers that build on this one)
typedef float f32x4 __attribute__((ext_vector_type(4)));
#else
#include "os2d_common.h"
#define TILE_DEV __device__ __forceinline__
#define TILE_HD static inline __host__ __device__
#endif

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));   // 16-byte unit (8 halves); ext vector: stays in VGPRs
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// ---- XCD-aware work-group order.  The dispatcher places work-group L on XCD L % 8 and every XCD has its own L2, so XCD x is given
// the contiguous range [x * per, (x + 1) * per) of the kernel's LOGICAL order, per = grid / 8: work-groups that share cache
// lines (the ~40 tiles of one plane, whose input slabs overlap by 2/3, and both channel halves of a tile; the parts of a bin
// group of the spectral GEMMs) run on ONE XCD at about the same time and their operands are fetched into that L2 once instead
// of ~6 times (conv 7x7: FETCH_SIZE 2.0 -> 0.6 GB per launch at 64 classes).  The grid is a multiple of 8 (os2d_xcd_grid); the
// kernel drops logical indices past its work.
TILE_DEV int os2d_xcd_logical(unsigned block, unsigned grid) {
  const int per = grid >> 3;
  return (block & 7) * per + (block >> 3);
}

// ---- column strips of the 5x5 kernels (maps wider than OS2D_MAX_W_LINEAR5, whose linear slab 256 + 2 HALO would pass 1536
// units; the reference has no width limit, head.py:622-629).  The map is cut into NS strips of SW = ceil(Ws / NS) output
// columns (they cover the W data columns and the 3 pad columns of a row), at most 256 each.  A strip is treated as a
// zero-bordered plane of its own with row pitch SP = SW + 2 R: strip-plane cell (h, j) is map cell (h, c0 - R + j), zero outside
// the map - so the R columns either side of the strip's outputs hold the NEIGHBOURING strips' data instead of zeros - and the
// convolution is again a shift-and-accumulate over the flat strip-plane index n' = h * SP + j, exact for the output columns
// R <= j < SP - R.  The matrix loops are the linear ones with SP for the row pitch; only the slab loads and the epilogues
// translate n' into map cells.
static inline void os2d_conv_strips(int W, int R, int* NS, int* SP) {
  const int Ws = W + OS2D_PAD;
  *NS = (Ws + 255) / 256;
  *SP = (Ws + *NS - 1) / *NS + 2 * R;
}
// map column of strip-plane column 0 ("c0mR")
TILE_HD int os2d_strip_origin(int strip, int SP, int R) { return strip * (SP - 2 * R) - R; }
// the map-plane cell of strip-plane index np, or 0 - a border cell of every plane, zero by contract - when np lies outside the map
TILE_DEV int os2d_strip_cell(int np, int SP, int c0mR, int H, int W, int Ws, int BASE) {
  const int h = np / SP, c = c0mR + (np - h * SP);
  return (np >= 0 && h < H && c >= 0 && c < W) ? BASE + h * Ws + c : 0;
}
// The way back, for the epilogues: index n of a tile's output range (strip: strip-plane index, linear: map-plane index >= BASE)
// -> map row, column and plane cell.  own: this tile stores the cell - strip: the strip's own output columns of the H rows up
// to and including the map's pad columns; linear: whatever lies inside the plane.  valid (of a cell the tile owns): a data
// cell; the other cells a tile owns are pad cells (plane-layout outputs store exact zeros there).
// Returns own; *hr, *wc, *cell, *valid as above.
TILE_DEV bool os2d_tile_cell(bool strip, int n, int SP, int R, int c0mR, int H, int W, int Ws, int BASE, int PLANE, int* hr, int* wc,
                             int* cell, bool* valid) {
  bool own;
  if (strip) {
    *hr = n / SP;
    const int j = n - *hr * SP;
    *wc = c0mR + j;
    own = !(j < R || j >= SP - R || *hr >= H || *wc >= Ws);
    *cell = BASE + *hr * Ws + *wc;
  } else {
    const int r = n - BASE;
    *hr = r / Ws;
    *wc = r - *hr * Ws;
    own = n < PLANE;
    *cell = n;
  }
  *valid = *hr < H && *wc < W;
  return own;
}
// Host: the tiles of NT cells a map is cut into.  Linear: the H * Ws cells of the data rows, *SP = *TPS = 0.  Strips: NS strips of
// *TPS tiles each (tile -> strip = tile / TPS), *SP = the strip-plane pitch.
static inline int os2d_conv_tiles(bool strip, int H, int W, int R, int NT, int* SP, int* TPS) {
  *SP = *TPS = 0;
  if (!strip) return (H * (W + OS2D_PAD) + NT - 1) / NT;
  int NS;
  os2d_conv_strips(W, R, &NS, SP);
  *TPS = (H * *SP + NT - 1) / NT;
  return NS * *TPS;
}

#ifndef OS2D_HOST_EMU
// ---- LDS-DMA: 16 bytes per lane from global memory straight into LDS (global_load_lds_dwordx4; the wave's lanes land in 64
// consecutive units from lds_dst on, which is wave-uniform)
typedef const void __attribute__((address_space(1))) * gptr_t;
typedef void __attribute__((address_space(3))) * lptr_t;
__device__ __forceinline__ void os2d_lds_dma16(const void* src, void* lds_dst) {
  __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)lds_dst, 16, 0, 0);
}

// ---- launch plumbing (host)
// grid of a kernel that walks its work in os2d_xcd_logical order: `groups` rounded up to a multiple of 8, so that every XCD gets
// the same number of logical slots
static inline int os2d_xcd_grid(long long groups, const char* what, unsigned* grid) {
  if (groups + 7 > 0x7fffffffLL) {
    os2d_set_error("%s: too many work-groups (%lld)", what, groups);
    return -3;
  }
  *grid = (unsigned)((groups + 7) / 8 * 8);
  return 0;
}
template <class K>
int os2d_set_dynamic_lds(K kernel, size_t bytes, const char* what) {
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) {
    os2d_set_error("hipFuncSetAttribute(%s): %s", what, hipGetErrorString(e));
    return -4;
  }
  return 0;
}
#endif
