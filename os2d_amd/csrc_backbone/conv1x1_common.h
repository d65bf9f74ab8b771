// What the 1x1 GEMMs of libos2d_backbone_conv.so and libos2d_backbone_conv_bf16.so share whatever their arithmetic: the record of a
// call, the epilogue, the argument contract and the tile plan (DESIGN.md sections 18.6 and 18.7).  The tile sizes and the cap on
// work-groups are each library's own public macros and reach this header as a ConvTiles; it includes neither public header.
//
// A work-group of 4 waves owns a tile of output channels x pixels, pixels = N * Ho * Wo: the batch index is folded into the pixel
// dimension, a tile may span images.  A wave owns 64 x 64 of the tile as 2 x 2 MFMA accumulators of 32 x 32 with W as the A operand:
// register q of accumulator [a][b] is channel 32 * a + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5) at pixel 32 * b + (lane & 31), so every
// store of the epilogue is 32 consecutive floats of one output row.
#pragma once
#include "backbone_common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr long long CONV_MAX_CHANNELS = 1ll << 20;

// one call: the operands but the weights, the geometry and the tile walk.  Each kernel's parameter struct is this and its weights.
struct ConvCall {
  const float *x, *s, *t, *r, *sr, *tr;
  float* y;
  int Cin, Cout, W, Wo, HWo, HW, stride, relu;
  int ksteps;              // ceil(Cin / TILE_K)
  int mtiles;
  long long pixels;        // N * Ho * Wo
  long long tiles;
};

// a library's tile sizes (the large shape, the one for layers of at most small_m outputs, the k-step) and its cap on work-groups
struct ConvTiles {
  int m, n, small_m, small_n, k, max_groups;
};

// the weight operand of an entry point: the one argument that is not the same in both
struct ConvWeights {
  const void* p;
  const char* name;        // in the messages
  size_t align, bytes;
};

__device__ __forceinline__ void conv_clear(f32x16 (&acc)[2][2]) {
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[a][b][q] = 0.0f;
}

// Is `pix` a pixel of y?  off: where channel 0 of its source pixel is in x (0 when it is none), the stride-2 gather included.
__device__ __forceinline__ bool conv_source(const ConvCall& p, long long pix, long long& off) {
  const bool ok = pix < p.pixels;
  off = 0;
  if (ok) {
    const long long img = pix / p.HWo;
    const int i = (int)(pix - img * p.HWo);
    const int src = p.stride == 1 ? i : (i / p.Wo) * 2 * p.W + (i % p.Wo) * 2;
    off = img * p.Cin * (long long)p.HW + src;
  }
  return ok;
}

// MODE 0: the fold alone, 1: + r, 2: + the fold of r
template <int MODE>
__device__ __forceinline__ float conv_out(float acc, float s, float t, float r, float sr, float tr, bool relu) {
#pragma clang fp contract(off)
  float v = bb_bn(acc, s, t);
  if (MODE) {
    const float d = MODE == 2 ? bb_bn(r, sr, tr) : r;
    v = v + d;
  }
  return relu ? bb_relu_nan(v) : v;
}

// The epilogue of one wave's 64 x 64 outputs from its accumulators: register q of accumulator [a][b] is channel cbase + 32 * a +
// (q & 3) + 8 * (q >> 2) at pixel pbase + 32 * b.  Every load is from a clamped, always valid address and has no branch around it, so
// that the 16 loads of a group are in flight together; only the stores are predicated.
template <int MODE>
__device__ __forceinline__ void conv_epilogue(const ConvCall& p, const f32x16 (&acc)[2][2], int cbase, long long pbase) {
  const bool relu = p.relu != 0;
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    float s[16], t[16], sr[16], tr[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int co = cbase + a * 32 + (q & 3) + 8 * (q >> 2);
      const int cc = co < p.Cout ? co : p.Cout - 1;
      s[q] = p.s[cc];
      t[q] = p.t[cc];
      sr[q] = MODE == 2 ? p.sr[cc] : 0.0f;
      tr[q] = MODE == 2 ? p.tr[cc] : 0.0f;
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const long long pix = pbase + b * 32;
      const bool pix_ok = pix < p.pixels;
      const long long pc = pix_ok ? pix : p.pixels - 1;
      const long long img = pc / p.HWo;
      const long long at = img * p.Cout * p.HWo + (pc - img * p.HWo);
      float r[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int co = cbase + a * 32 + (q & 3) + 8 * (q >> 2);
        const int cc = co < p.Cout ? co : p.Cout - 1;
        r[q] = MODE ? p.r[at + (long long)cc * p.HWo] : 0.0f;
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int co = cbase + a * 32 + (q & 3) + 8 * (q >> 2);
        const float out = conv_out<MODE>(acc[a][b][q], s[q], t[q], r[q], sr[q], tr[q], relu);
        if (pix_ok && co < p.Cout) p.y[at + (long long)co * p.HWo] = out;
      }
    }
  }
}

// The end of a tile: the epilogue in the form the call's pointers name, for the wave whose 64 x 64 outputs start at channel m0 and
// pixel n0 (half = lane >> 5, l32 = lane & 31).
__device__ __forceinline__ void conv_finish(const ConvCall& p, const f32x16 (&acc)[2][2], int m0, long long n0, int half, int l32) {
  const int mode = p.r == nullptr ? 0 : (p.sr == nullptr ? 1 : 2);
  const int cbase = m0 + 4 * half;
  const long long pbase = n0 + l32;
  if (mode == 0)
    conv_epilogue<0>(p, acc, cbase, pbase);
  else if (mode == 1)
    conv_epilogue<1>(p, acc, cbase, pbase);
  else
    conv_epilogue<2>(p, acc, cbase, pbase);
}

// the limits of include/os2d_backbone.h on one tensor of N x C x plane
static inline bool conv_too_large(int N, int C, long long plane) {
  return (long long)N * C > BB_MAX_ROWS || plane > BB_MAX_PLANE || (long long)N * C * plane > BB_MAX_ELEMENTS;
}

static inline bool conv_channels_ok(int C) { return C >= 1 && C <= CONV_MAX_CHANNELS; }

// What both GEMM entry points check of their arguments, in this order, and the operands and geometry of the call -> 0, or -1 and the
// thread's last error.  A weight operand of 4-byte alignment is one of "the pointers"; another has a message of its own.
static inline int conv_check(const char* what, ConvCall& p, const ConvWeights& w, const float* x, const float* s, const float* t, const float* r,
                             const float* sr, const float* tr, float* y, int N, int Cin, int Cout, int H, int W, int stride, int relu) {
  if (!x || !w.p || !s || !t || !y) return OS2D_REFUSE(-1, "%s: null pointer", what);
  if ((sr == nullptr) != (tr == nullptr)) return OS2D_REFUSE(-1, "%s: sr and tr are both given or both NULL", what);
  if (sr && !r) return OS2D_REFUSE(-1, "%s: sr and tr come only together with r", what);
  if (bb_misaligned(x, 4) || (w.align == 4 && bb_misaligned(w.p, 4)) || bb_misaligned(s, 4) || bb_misaligned(t, 4) || bb_misaligned(r, 4) ||
      bb_misaligned(sr, 4) || bb_misaligned(tr, 4) || bb_misaligned(y, 4))
    return OS2D_REFUSE(-1, "%s: pointer not aligned (4 bytes)", what);
  if (bb_misaligned(w.p, w.align)) return OS2D_REFUSE(-1, "%s: %s not aligned (%zu bytes)", what, w.name, w.align);
  if (N < 1 || Cin < 1 || Cout < 1 || H < 1 || W < 1) return OS2D_REFUSE(-1, "%s: bad shape (every size >= 1)", what);
  if (stride != 1 && stride != 2) return OS2D_REFUSE(-1, "%s: stride is 1 or 2", what);
  if (relu != 0 && relu != 1) return OS2D_REFUSE(-1, "%s: relu is 0 or 1", what);
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const long long HW = (long long)H * W, HWo = (long long)Ho * Wo;
  if (!conv_channels_ok(Cin) || !conv_channels_ok(Cout) || conv_too_large(N, Cin, HW) || conv_too_large(N, Cout, HWo))
    return OS2D_REFUSE(-1, "%s: too large (Cin, Cout <= 2^20; for x and y: N * C < 2^31, H * W <= 2^30, N * C * H * W <= 2^40)", what);
  const long long ny = (long long)N * Cout * HWo;
  if (bb_bytes_meet(y, (size_t)ny * sizeof(float), x, (size_t)N * Cin * HW * sizeof(float))) return OS2D_REFUSE(-1, "%s: y overlaps x", what);
  if (bb_bytes_meet(y, (size_t)ny * sizeof(float), w.p, w.bytes)) return OS2D_REFUSE(-1, "%s: y overlaps %s", what, w.name);
  if (r && bb_overlap(r, y, ny)) return OS2D_REFUSE(-1, "%s: y overlaps r", what);
  p.x = x; p.s = s; p.t = t; p.r = r; p.sr = sr; p.tr = tr; p.y = y;
  p.Cin = Cin; p.Cout = Cout; p.W = W; p.Wo = Wo; p.HWo = (int)HWo; p.HW = (int)HW; p.stride = stride; p.relu = relu;
  p.pixels = (long long)N * HWo;
  return 0;
}

// The tile walk of a checked call: the small shape for a layer of at most small_m outputs, output-channel tiles of one pixel tile next
// to each other so that its slice of x is read from HBM once -> the work-groups, which stride over the tiles when there are more.
static inline unsigned conv_plan(ConvCall& p, const ConvTiles& tiles, bool& small) {
  small = p.Cout <= tiles.small_m;
  const int tm = small ? tiles.small_m : tiles.m, tn = small ? tiles.small_n : tiles.n;
  p.ksteps = (p.Cin + tiles.k - 1) / tiles.k;
  p.mtiles = (p.Cout + tm - 1) / tm;
  p.tiles = p.mtiles * ((p.pixels + tn - 1) / tn);
  return (unsigned)(p.tiles < tiles.max_groups ? p.tiles : tiles.max_groups);
}
